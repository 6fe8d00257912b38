#!/usr/bin/env python3
"""Times the site overview (SemanticMapping.site_overview; scroll.py, csrc/seg_overview.hip) on the default 2000 x 2000 x 5 float64
window of 0.1 m cells with 10 m tiles (T = 100, 20 x 20 tiles, 160 MB):

    a site of 3 x 3 windows, every tile full (3600 tiles, 1.44 GB), at k = 1 and k = 10 cells per pixel, and
    a sparse site: a diagonal corridor of 20 windows through a rectangle of 20 x 20 windows (8000 tiles, 3.2 GB, in a rectangle of
    160 000 tile places) at k = 10 -- each arm in ONE process, alternating, `rounds` times over (every other round in reverse order):
        copy       dst.copy_(src) of as many bytes as the kernel reads, between two device events: the yardstick of the kernel;
        kernel     avl_site_overview alone (its zero fill included) on a ready-made, uploaded table, picture only, between two events;
        kernel_R   the same with the reduced grid written too;
        overview   SemanticMapping.site_overview(k), wall clock per call with one synchronisation behind `reps` calls: the window's
                   emptiness reduction, the table, its validation and upload, the launch;
        parent     the parent commit's route to the same picture, render_bev_map(site_map()[1]), wall clock (k = 1 is its only
                   resolution).  On the sparse site it is not run: its byte count is reported.

    python tools/bench_site_overview.py [--reps 20] [--warmup 2] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd import SemanticMapping, _lib, get_cfg_defaults, scroll as S, synthetic as syn  # noqa: E402
from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET  # noqa: E402
from vision_semantic_segmentation_amd.renderer import render_bev_map  # noqa: E402
from vision_semantic_segmentation_amd.utils.logger import MyLogger  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda", 0)
RES, TILE_M, HALF = 0.1, 10.0, 100.0
ANCHOR = (PCD_ORIGIN_OFFSET[0] - HALF, PCD_ORIGIN_OFFSET[1] - HALF)


def make_sm():
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], HALF)
    cfg.MAPPING.RESOLUTION = RES
    cfg.MAPPING.DEPTH_METHOD = "points_raw"
    cfg.MAPPING.SCROLL.ENABLED = True
    cfg.MAPPING.SCROLL.TILE_M = TILE_M
    cfg.MAPPING.SCROLL.HYSTERESIS_TILES = 0
    return SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))


def pose_at(ti, tj):
    """the vehicle in the middle of tile (ti, tj), heading along x"""
    return np.array([ANCHOR[0] - PCD_ORIGIN_OFFSET[0] + (ti + 0.5) * TILE_M, ANCHOR[1] - PCD_ORIGIN_OFFSET[1] + (tj + 0.5) * TILE_M, 0.0, 0.0, 0.0, 0.0, 1.0])


def stats(samples):
    return {"median_us": round(statistics.median(samples), 1), "min_us": round(min(samples), 1), "max_us": round(max(samples), 1)}


def event_time(fn, reps):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def wall_time(fn, reps):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def alternate(arms):
    samples = {name: [] for name, _, _ in arms}
    for r in range(args.rounds):
        for name, fn, timer in (arms if r % 2 == 0 else arms[::-1]):
            samples[name].append(timer(fn, args.reps))
    return {name: stats(v) for name, v in samples.items()}


def drive(sm, windows):
    """every window of ``windows`` (in windows of 20 x 20 tiles) filled with the same random log-odds pattern"""
    pattern = torch.randn((sm.map_height, sm.map_width, sm.map_depth), dtype=torch.float64, device=dev)
    for a, b in windows:
        sm.scroll_to(pose_at(10 + 20 * a, 10 + 20 * b))
        sm.map_dev.copy_(pattern)


def kernel_arms(sm, k):
    """avl_site_overview alone: the table of the whole site, built, validated and uploaded once -> (run(picture only), run(with R),
    bytes read, rect)"""
    store = sm._scroll
    rect, table, buffers = store.overview_table()
    nh, nw = rect[1] - rect[0] + 1, rect[3] - rect[2] + 1
    T, Cn = store.T, store.C
    S.validate_sources(table, buffers, T, Cn * 8, nh, nw)
    rec = np.zeros(len(table), dtype=S.SRC_DTYPE)
    S.encode_sources(table, buffers, rec)
    tiles = torch.from_numpy(rec.view(np.uint8)).to(dev)
    P = T // k
    picture = torch.empty((nh * P, nw * P, 3), dtype=torch.uint8, device=dev)
    reduced = torch.empty((nh * P, nw * P, Cn), dtype=torch.float64, device=dev)
    colors = np.ascontiguousarray(np.asarray(sm.label_colors), dtype=np.uint8)
    col = (C.c_uint8 * colors.size)(*colors.ravel().tolist())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(red):
        rc = _lib.lib().avl_site_overview(C.c_void_p(tiles.data_ptr()), len(table), nh, nw, T, Cn, _lib.AVL_F64, k, col, None, None,
                                          C.c_void_p(picture.data_ptr()), red, stream)
        if rc:
            raise RuntimeError(_lib.last_error())
    return (lambda: run(None)), (lambda: run(C.c_void_p(reduced.data_ptr()))), len(table) * T * T * Cn * 8, rect, picture


def bench_dense():
    sm = make_sm()
    drive(sm, [(a, b) for a in range(3) for b in range(3)])
    (i0, j0), full = sm.site_map()
    assert len(sm.site_tiles()) == 3600 and tuple(full.shape) == (6000, 6000, 5)
    other = torch.empty_like(full)
    rows = []
    for k in (1, 10):
        kernel, kernel_R, nbytes, rect, picture = kernel_arms(sm, k)
        assert nbytes == full.numel() * 8
        kernel()
        assert torch.equal(picture, sm.site_overview(k)[1])
        if k == 1:
            assert torch.equal(picture, render_bev_map(full, sm.label_colors))
        row = {"what": "3 x 3 windows, k = %d" % k, "tiles": 3600, "read_mb": round(nbytes / 1e6, 1), "picture": list(picture.shape[:2])}
        row.update(alternate([("copy", lambda: other.copy_(full), event_time), ("kernel", kernel, event_time), ("kernel_R", kernel_R, event_time),
                              ("overview", lambda: sm.site_overview(k), wall_time),
                              ("parent", lambda: render_bev_map(sm.site_map()[1], sm.label_colors), wall_time)]))
        row["kernel_over_copy"] = round(row["kernel"]["median_us"] / row["copy"]["median_us"], 3)
        row["host_share_us"] = round(row["overview"]["median_us"] - row["kernel"]["median_us"], 1)
        row["parent_over_overview"] = round(row["parent"]["median_us"] / row["overview"]["median_us"], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_sparse():
    sm = make_sm()
    drive(sm, [(a, a) for a in range(20)])
    k = 10
    kernel, kernel_R, nbytes, rect, picture = kernel_arms(sm, k)
    nh, nw = rect[1] - rect[0] + 1, rect[3] - rect[2] + 1
    assert (nh, nw) == (400, 400) and nbytes == 8000 * 100 * 100 * 40
    kernel()
    assert torch.equal(picture, sm.site_overview(k)[1]) and bool(picture[:1000, :1000].any()) and not bool(picture[:1000, 1000:].any())
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    row = {"what": "corridor of 20 windows in 20 x 20, k = %d" % k, "tiles": 8000, "tile_places": nh * nw, "read_mb": round(nbytes / 1e6, 1),
           "picture": list(picture.shape[:2]), "parent_route_bytes": nh * 100 * nw * 100 * 40}
    row.update(alternate([("copy", lambda: dst.copy_(src), event_time), ("kernel", kernel, event_time), ("kernel_R", kernel_R, event_time),
                          ("overview", lambda: sm.site_overview(k), wall_time)]))
    row["kernel_over_copy"] = round(row["kernel"]["median_us"] / row["copy"]["median_us"], 3)
    row["host_share_us"] = round(row["overview"]["median_us"] - row["kernel"]["median_us"], 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = bench_dense() + [bench_sparse()]
    print("\n%-42s %6s %8s | %-27s | %-27s | %-27s | %-27s | %s" % ("site", "tiles", "read MB", "copy_ us (min..max)", "kernel us (min..max)",
                                                                    "kernel + R us (min..max)", "site_overview wall us", "site_map + render_bev_map wall us"))
    for r in rows:
        cells = ["%9.1f (%7.1f..%8.1f)" % (r[n]["median_us"], r[n]["min_us"], r[n]["max_us"]) for n in ("copy", "kernel", "kernel_R", "overview")]
        parent = "%9.1f (%7.1f..%8.1f)" % (r["parent"]["median_us"], r["parent"]["min_us"], r["parent"]["max_us"]) if "parent" in r else \
            "infeasible: %.1f GB assembled" % (r["parent_route_bytes"] / 1e9)
        print("%-42s %6d %8.1f | %s | %s | %s | %s | %s" % (r["what"], r["tiles"], r["read_mb"], cells[0], cells[1], cells[2], cells[3], parent))
    for r in rows:
        print("%-42s kernel / copy %.3f, host share of site_overview %.1f us%s" % (
            r["what"], r["kernel_over_copy"], r["host_share_us"],
            ", parent route / site_overview %.2f" % r["parent_over_overview"] if "parent" in r else ""))


if __name__ == "__main__":
    main()
