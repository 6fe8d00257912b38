#!/usr/bin/env python3
"""Times the site finish (SemanticMapping.site_finish; scroll.py, csrc/seg_sitefinish.hip) on the default 2000 x 2000 x 5 float64
window of 0.1 m cells with 10 m tiles (T = 100, 20 x 20 tiles, 160 MB), on the two sites of tools/bench_site_overview.py:

    a site of 3 x 3 windows, every tile full (3600 tiles, 1.44 GB), and
    a sparse site: a diagonal corridor of 20 windows through a rectangle of 20 x 20 windows (8000 tiles, 3.2 GB, in a rectangle of
    160 000 tile places, 1.6e9 cells) -- each arm in ONE process, alternating, `rounds` times over (every other round in reverse order):
        copy        dst.copy_(src) of as many bytes as the listed tiles hold, between two device events: the yardstick of the kernel;
        k_picture   avl_site_finish alone (its zero fills included) on a ready-made, uploaded table, picture only, between two events;
        k_counts    the same, counts only (nothing of the rectangle's size is written);
        k_both      picture and counts;
        finish      SemanticMapping.site_finish(truth=...), wall clock per call: the window's emptiness reduction, the table, its
                    validation and upload, the launch, the counts' way back and the host's share of them (on the corridor: counts only,
                    and `finish_pic` the picture only);
        route       3 x 3 site only: the existing route to the same result, site_map() -> apply_filter -> render_bev_map ->
                    evaluation._run on a truth window that is already binned and on the device (Test.test_single_map's kernel without
                    its host-side binning), wall clock.  On the corridor it cannot run: its byte count is reported.

    python tools/bench_site_finish.py [--reps 10] [--warmup 2] [--rounds 5]
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
from vision_semantic_segmentation_amd import SemanticMapping, _lib, evaluation, get_cfg_defaults, scroll as S, synthetic as syn  # noqa: E402
from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET  # noqa: E402
from vision_semantic_segmentation_amd.renderer import apply_filter, render_bev_map  # noqa: E402
from vision_semantic_segmentation_amd.utils.logger import MyLogger  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
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


def site_truth(origin, T):
    """labels 0 .. 6 over the first 6000 x 6000 cells of the site's rectangle, shifted off the tile grid by (30, 70) cells"""
    g = torch.randint(0, 7, (6000, 6000), dtype=torch.uint8, device=dev)
    return evaluation.SiteTruth(g, (origin[0] + 30, origin[1] + 70), tile_cells=T)


def kernel_arms(sm, truth, with_picture=True):
    """avl_site_finish alone: the table of the whole site, built, validated and uploaded once -> ({arm: run}, bytes read, rect,
    picture, counts)"""
    store = sm._scroll
    rect, table, buffers = store.overview_table(None, S.finish_sources)
    nh, nw = rect[1] - rect[0] + 1, rect[3] - rect[2] + 1
    T, Cn = store.T, store.C
    S.validate_finish(table, buffers, T, Cn * 8, nh, nw)
    rec = np.zeros(len(table), dtype=S.FIN_DTYPE)
    S.encode_finish(table, buffers, rec)
    tiles = torch.from_numpy(rec.view(np.uint8)).to(dev)
    picture = torch.empty((nh * T, nw * T, 3), dtype=torch.uint8, device=dev) if with_picture else None
    counts = torch.empty(64, dtype=torch.int64, device=dev)
    gt, _ = truth.on(dev)
    r0, c0 = truth.origin_cell[0] - rect[0] * T, truth.origin_cell[1] - rect[2] * T
    colors = np.ascontiguousarray(np.asarray(sm.label_colors), dtype=np.uint8)
    col = (C.c_uint8 * colors.size)(*colors.ravel().tolist())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(pic, cnt):
        rc = _lib.lib().avl_site_finish(C.c_void_p(tiles.data_ptr()), len(table), nh, nw, T, Cn, _lib.AVL_F64, _lib.AVL_LIVE_FILTER, col, None,
                                        None, C.c_void_p(gt.data_ptr()) if cnt else None, int(gt.shape[0]), int(gt.shape[1]), int(gt.shape[1]),
                                        r0, c0, None, 0, C.c_void_p(picture.data_ptr()) if pic else None, None,
                                        C.c_void_p(counts.data_ptr()) if cnt else None, stream)
        if rc:
            raise RuntimeError(_lib.last_error())
    arms = {"k_counts": lambda: run(False, True)}
    if with_picture:
        arms["k_picture"] = lambda: run(True, False)
        arms["k_both"] = lambda: run(True, True)
    n_src = int((table["buf"] >= 0).sum())
    return arms, n_src * T * T * Cn * 8, rect, picture, counts, (n_src, len(table) - n_src)


def bench_dense():
    sm = make_sm()
    drive(sm, [(a, b) for a in range(3) for b in range(3)])
    origin, full = sm.site_map()
    T = sm._scroll.T
    assert len(sm.site_tiles()) == 3600 and tuple(full.shape) == (6000, 6000, 5)
    truth = site_truth(origin, T)
    truth_window = torch.zeros((6000, 6000), dtype=torch.uint8, device=dev)
    truth_window[30:, 70:] = truth.on(dev)[0][:6000 - 30, :6000 - 70]
    other = torch.empty_like(full)
    arms, nbytes, rect, picture, counts, n_rec = kernel_arms(sm, truth)
    assert nbytes == full.numel() * 8

    def route():
        pic = render_bev_map(apply_filter(sm.site_map()[1]).to(full.dtype), sm.label_colors)
        return pic, evaluation.stats_from_counts(evaluation._run(pic, None, truth_window)[1])
    arms["k_both"]()
    want_pic, _ = route()
    want_counts = evaluation._run(want_pic, None, truth_window)[1]
    res = sm.site_finish(truth=truth)
    assert torch.equal(picture, want_pic) and torch.equal(res.picture, want_pic)
    assert np.array_equal(counts.cpu().numpy().reshape(8, 8), want_counts) and np.array_equal(res.counts, want_counts)
    del want_pic, res
    row = {"what": "3 x 3 windows", "tiles": 3600, "records": list(n_rec), "read_mb": round(nbytes / 1e6, 1), "picture": list(picture.shape[:2])}
    row.update(alternate([("copy", lambda: other.copy_(full), event_time), ("k_picture", arms["k_picture"], event_time),
                          ("k_counts", arms["k_counts"], event_time), ("k_both", arms["k_both"], event_time),
                          ("finish", lambda: sm.site_finish(truth=truth), wall_time), ("route", route, wall_time)]))
    row["k_both_over_copy"] = round(row["k_both"]["median_us"] / row["copy"]["median_us"], 3)
    row["host_share_us"] = round(row["finish"]["median_us"] - row["k_both"]["median_us"], 1)
    row["route_over_finish"] = round(row["route"]["median_us"] / row["finish"]["median_us"], 2)
    print(json.dumps(row), flush=True)
    return row


def bench_sparse():
    sm = make_sm()
    drive(sm, [(a, a) for a in range(20)])
    T = sm._scroll.T
    tiles = sm.site_tiles()
    origin = (min(t[0] for t in tiles) * T, min(t[1] for t in tiles) * T)
    truth = site_truth(origin, T)
    arms, nbytes, rect, picture, counts, n_rec = kernel_arms(sm, truth)
    nh, nw = rect[1] - rect[0] + 1, rect[3] - rect[2] + 1
    assert (nh, nw) == (400, 400) and nbytes == 8000 * 100 * 100 * 40
    arms["k_both"]()
    first = counts.cpu().numpy().reshape(8, 8).copy()
    arms["k_counts"]()
    assert np.array_equal(first, counts.cpu().numpy().reshape(8, 8)) and first.sum() == sum(n_rec) * T * T
    assert bool(picture[:1000, :1000].any()) and not bool(picture[:1000, 3000:].any())
    res = sm.site_finish(truth=truth, picture=False)
    assert res.picture is None and res.counts.sum() == nh * T * nw * T and np.array_equal(res.counts[:, 1:], first[:, 1:])
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    row = {"what": "corridor of 20 windows in 20 x 20", "tiles": 8000, "records": list(n_rec), "tile_places": nh * nw, "read_mb": round(nbytes / 1e6, 1),
           "picture": list(picture.shape[:2]), "route_bytes": nh * T * nw * T * 40}
    del picture
    row.update(alternate([("copy", lambda: dst.copy_(src), event_time), ("k_picture", arms["k_picture"], event_time),
                          ("k_counts", arms["k_counts"], event_time), ("k_both", arms["k_both"], event_time),
                          ("finish", lambda: sm.site_finish(truth=truth, picture=False), wall_time),
                          ("finish_pic", lambda: sm.site_finish(), wall_time)]))
    row["k_counts_over_copy"] = round(row["k_counts"]["median_us"] / row["copy"]["median_us"], 3)
    row["host_share_us"] = round(row["finish"]["median_us"] - row["k_counts"]["median_us"], 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = [bench_dense(), bench_sparse()]
    names = ("copy", "k_picture", "k_counts", "k_both", "finish")
    print("\n%-36s %6s %8s | " % ("site", "tiles", "read MB") + " | ".join("%-27s" % (n + " us (min..max)") for n in names) + " | existing route wall us")
    for r in rows:
        cells = ["%9.1f (%7.1f..%8.1f)" % (r[n]["median_us"], r[n]["min_us"], r[n]["max_us"]) for n in names]
        route = "%9.1f (%7.1f..%8.1f)" % (r["route"]["median_us"], r["route"]["min_us"], r["route"]["max_us"]) if "route" in r else \
            "infeasible: %.1f GB assembled" % (r["route_bytes"] / 1e9)
        print("%-36s %6d %8.1f | %s | %s" % (r["what"], r["tiles"], r["read_mb"], " | ".join(cells), route))
    d, s = rows
    print("%-36s k_both / copy %.3f, host share of site_finish %.1f us, existing route / site_finish %.2f" % (
        d["what"], d["k_both_over_copy"], d["host_share_us"], d["route_over_finish"]))
    print("%-36s k_counts / copy %.3f, host share of site_finish(picture=False) %.1f us, site_finish() picture only %.1f us" % (
        s["what"], s["k_counts_over_copy"], s["host_share_us"], s["finish_pic"]["median_us"]))


if __name__ == "__main__":
    main()
