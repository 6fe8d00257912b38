#!/usr/bin/env python3
"""Times the scrolling grid (MAPPING.SCROLL; scroll.py, csrc/seg_scroll.hip) on the default 2000 x 2000 x 5 float64 grid of 0.1 m cells
with 10 m tiles (T = 100, a window of 20 x 20 tiles, 160 MB):

    a one-tile-row scroll (20 tiles leave, 20 enter, 380 move: 420 jobs), a diagonal one-tile scroll, a jump further than the window
    (400 leave, 400 enter), each three ways in ONE process, alternating, `rounds` times over (every other round in reverse order):
        copy     dst.copy_(src) of the same grid tensor on the same stream: the same bytes once each way, the yardstick;
        kernel   avl_tile_copy alone on the scroll's ready-made, uploaded job table, between two device events;
        scroll   SemanticMapping.scroll_to, wall clock per call with one synchronisation behind `reps` calls: the host's planning,
                 validation and encoding of the table, its upload, the launch, the flag copy and the buffer swap.
    HYSTERESIS_TILES is 0 here so that a move of one tile scrolls; the vehicle goes back and forth, and the window is full on both
    sides, so every scroll stores 20 (or 39, or 400) non-empty tiles and reloads as many.
    site_map() of a site of 3 x 3 windows (3600 tiles, 1.44 GB assembled), wall clock, against copy_ of a tensor of that size.
    One frame of mapping() (120 k points, one 1080 x 1920 colour image) with scrolling enabled and no scroll due, against the same
    frame on an instance with SCROLL.ENABLED = False and that window as its BOUNDARY (the parent commit's path), wall clock per
    frame, `rounds` alternating samples each: nothing may be launched, so the two must agree within their spread.  A third arm is
    the scrolling instance itself with its store detached for the call: the same buffers and boundary without the scroll_to call.

    python tools/bench_scroll.py [--reps 20] [--frame-reps 200] [--warmup 3] [--rounds 5]
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
from vision_semantic_segmentation_amd.camera import camera_setup_1  # noqa: E402
from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET, velodyne_to_baselink  # noqa: E402
from vision_semantic_segmentation_amd.utils.logger import MyLogger  # noqa: E402
from vision_semantic_segmentation_amd.utils.utils_ros import get_transform_from_pose  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--frame-reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda", 0)
RES, TILE_M, HALF = 0.1, 10.0, 100.0
ANCHOR = (PCD_ORIGIN_OFFSET[0] - HALF, PCD_ORIGIN_OFFSET[1] - HALF)


def make_sm(scroll=True, hysteresis=0, boundary=None):
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], HALF) if boundary is None else boundary
    cfg.MAPPING.RESOLUTION = RES
    cfg.MAPPING.DEPTH_METHOD = "points_raw"
    cfg.MAPPING.SCROLL.ENABLED = scroll
    cfg.MAPPING.SCROLL.TILE_M = TILE_M
    cfg.MAPPING.SCROLL.HYSTERESIS_TILES = hysteresis
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    return sm


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


def alternate(arms, reps_of):
    samples = {name: [] for name, _, _ in arms}
    for r in range(args.rounds):
        for name, fn, timer in (arms if r % 2 == 0 else arms[::-1]):
            samples[name].append(timer(fn, reps_of))
    return {name: stats(v) for name, v in samples.items()}


def bench_scroll(name, shift):
    sm = make_sm()
    store = sm._scroll
    home = (10, 10)
    sm.scroll_to(pose_at(*home))
    sm.map_dev.fill_(1.0)                                   # every tile holds something: it is stored when it leaves, reloaded when it returns
    away = (home[0] + shift[0], home[1] + shift[1])
    state = {"at": home}

    def scroll():
        state["at"] = away if state["at"] == home else home
        assert sm.scroll_to(pose_at(*state["at"]))
    scroll()
    sm.map_dev.fill_(1.0)                                   # the tiles that entered on the far side as well: both directions store and reload
    scroll(), scroll()                                      # the pool has its chunks, the second buffer exists
    other = torch.empty_like(sm.map_dev)

    def copy():
        other.copy_(sm.map_dev)
    # the kernel alone: the table of the scroll home -> away, built, validated and uploaded once
    T, L = store.T, store._layers()[0]
    o = (store.origin[0] // T, store.origin[1] // T)
    plan = S.plan_scroll(o, (o[0] + shift[0], o[1] + shift[1]), store.Ht, store.Wt, {})
    scratch = torch.empty(len(plan["leaving"]) * T * T * L.bpc + 16, dtype=torch.uint8, device=dev)
    jobs = S.scroll_jobs(plan, o, (o[0] + shift[0], o[1] + shift[1]), T, store.Wm, L.bpc, 1 << 30, list(range(len(plan["leaving"]))), {})
    buffers = {"old": store._extent(sm.map_dev), "new": store._extent(other), ("chunk", 0): store._extent(scratch)}
    S.validate_jobs(jobs, buffers, T, L.bpc, len(plan["leaving"]))
    rec = np.zeros(len(jobs), dtype=S.JOB_DTYPE)
    S.encode_jobs(jobs, buffers, rec)
    table = torch.from_numpy(rec.view(np.uint8)).to(dev)
    flags = torch.zeros(max(len(plan["leaving"]), 1), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def kernel():
        rc = _lib.lib().avl_tile_copy(C.c_void_p(table.data_ptr()), len(jobs), T, L.bpc, 0, C.c_void_p(flags.data_ptr()), len(plan["leaving"]), stream)
        if rc:
            raise RuntimeError(_lib.last_error())
    row = {"what": name, "shift_tiles": shift, "jobs": len(jobs), "leaving": len(plan["leaving"]),
           "grid_mb": round(sm.map_dev.numel() * 8 / 1e6, 1), "last_scroll": None}
    row.update(alternate([("copy", copy, event_time), ("kernel", kernel, event_time), ("scroll", scroll, wall_time)], args.reps))
    row["last_scroll"] = sm.last_scroll
    row["kernel_over_copy"] = round(row["kernel"]["median_us"] / row["copy"]["median_us"], 3)
    row["scroll_over_copy"] = round(row["scroll"]["median_us"] / row["copy"]["median_us"], 3)
    print(json.dumps(row), flush=True)
    return row


def bench_site_map():
    sm = make_sm()
    for a in range(3):                                      # nine windows side by side, each full
        for b in range(3):
            sm.scroll_to(pose_at(10 + 20 * a, 10 + 20 * b))
            sm.map_dev.fill_(1.0)
    tiles = sm.site_tiles()
    (i0, j0), out = sm.site_map()
    assert len(tiles) == 3600 and tuple(out.shape) == (6000, 6000, 5) and bool((out == 1.0).all())
    other = torch.empty_like(out)
    row = {"what": "site_map of 3 x 3 windows", "tiles": len(tiles), "out_mb": round(out.numel() * 8 / 1e6, 1)}
    row.update(alternate([("copy", lambda: other.copy_(out), wall_time), ("site_map", lambda: sm.site_map(), wall_time)], max(args.reps // 4, 2)))
    print(json.dumps(row), flush=True)
    return row


def bench_frame():
    H, W, n = 1080, 1920, 120000
    rng = np.random.default_rng(2)
    cam = camera_setup_1().scaled(1.0, H / 1440.0)
    pose = pose_at(13, 7)
    velo = syn.make_cloud(rng, n, cam.K, cam.R, cam.t, W, H)
    M = np.matmul(get_transform_from_pose(pose), velodyne_to_baselink())
    with np.errstate(all="ignore"):
        world = np.matmul(M, np.vstack([velo[0:3], np.ones((1, n))]))
    cloud = torch.from_numpy(np.ascontiguousarray(np.vstack([world[0:3], velo[3:4]]).T.astype(np.float32))).to(dev)
    image = torch.from_numpy(syn.colorize(syn.make_label_map(rng, H, W))).to(dev)
    on = make_sm(hysteresis=1)
    on.scroll_to(pose)
    (x0, _), (y0, _) = S.window_boundary(on._scroll.anchor, on.scroll_origin, on.map_height, on.map_width, RES)
    off = make_sm(scroll=False, boundary=[[x0, x0 + 2 * HALF + RES / 2], [y0, y0 + 2 * HALF + RES / 2]])      # the kernels read the minima only
    assert (off.map_height, off.map_width) == (on.map_height, on.map_width)
    for sm in (on, off):
        sm.pcd, sm.pcd_frame_id = cloud, "world"
    for sm in (on, off):
        sm.mapping(image, pose, cam)
    assert torch.equal(on.map_dev, off.map_dev) and int((on.map_dev != 0).sum()) > 0      # the two instances map the same frame alike
    count = on.scroll_count
    row = {"what": "mapping() frame, no scroll due", "points": n}
    store = on._scroll

    def detached():                                         # the scrolling instance, its buffers and its boundary, without the scroll_to call
        on._scroll = None
        on.mapping(image, pose, cam)
        on._scroll = store
    row.update(alternate([("scroll_off", lambda: off.mapping(image, pose, cam), wall_time), ("scroll_on", lambda: on.mapping(image, pose, cam), wall_time),
                          ("scroll_on_detached", detached, wall_time)], args.frame_reps))
    assert on.scroll_count == count
    row["on_minus_off_us"] = round(row["scroll_on"]["median_us"] - row["scroll_off"]["median_us"], 1)
    row["on_minus_detached_us"] = round(row["scroll_on"]["median_us"] - row["scroll_on_detached"]["median_us"], 1)
    t0 = time.perf_counter()
    for _ in range(10000):
        on._scroll.scroll_to(pose)
    row["scroll_to_host_us"] = round((time.perf_counter() - t0) * 1e6 / 10000, 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = [bench_scroll("one tile row", (1, 0)), bench_scroll("diagonal, one tile", (1, 1)), bench_scroll("jump", (30, 30))]
    print("\n%-20s %5s | copy_ us (min..max)         | kernel us (min..max)        | scroll_to wall us (min..max) | kernel/copy | scroll/copy" % ("scroll", "jobs"))
    for r in rows:
        a, b, c = r["copy"], r["kernel"], r["scroll"]
        print("%-20s %5d | %8.1f (%7.1f..%7.1f) | %8.1f (%7.1f..%7.1f) | %8.1f (%7.1f..%7.1f)  | %6.3f      | %6.3f" % (
            r["what"], r["jobs"], a["median_us"], a["min_us"], a["max_us"], b["median_us"], b["min_us"], b["max_us"], c["median_us"], c["min_us"],
            c["max_us"], r["kernel_over_copy"], r["scroll_over_copy"]))
    f = bench_frame()
    d = f["scroll_on_detached"]
    print("\nframe, no scroll due: SCROLL off %.1f us (%.1f..%.1f), on %.1f us (%.1f..%.1f), on - off %.1f us; the scrolling instance without the "
          "scroll_to call %.1f us (%.1f..%.1f), on - that %.1f us; scroll_to alone %.2f us of host time" % (
              f["scroll_off"]["median_us"], f["scroll_off"]["min_us"], f["scroll_off"]["max_us"], f["scroll_on"]["median_us"], f["scroll_on"]["min_us"],
              f["scroll_on"]["max_us"], f["on_minus_off_us"], d["median_us"], d["min_us"], d["max_us"], f["on_minus_detached_us"], f["scroll_to_host_us"]))
    s = bench_site_map()
    print("\nsite_map, 3600 tiles, %.0f MB: %.1f us (%.1f..%.1f); copy_ of as many bytes %.1f us (%.1f..%.1f)" % (
        s["out_mb"], s["site_map"]["median_us"], s["site_map"]["min_us"], s["site_map"]["max_us"], s["copy"]["median_us"], s["copy"]["min_us"],
        s["copy"]["max_us"]))


if __name__ == "__main__":
    main()
