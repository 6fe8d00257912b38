#!/usr/bin/env python3
"""Times the points-map mode's own index (points_map.py; avl_points_map_gather, one kernel: k_points_map_gather) on a site it is
meant for: a synthetic prior map of 5 M float32 points over 600 m x 600 m (13.9 points per square metre, z within 3 m of the ground),
the 2000 x 2000 x 5 float64 grid of 0.1 m cells around the vehicle, cameras at 1080 x 1920 with a 266 x 476 class map, the cloud's
RANGE_MAX of 100 m, MARGIN_M 1, the exact window (RADIUS_M 0).  TILE_M is swept over 5, 10 and 20 m.

    gather_frame    (a) the gather, then the frame on the gathered cloud
    whole           (b) the frame on the whole map
    cropped         (c) the frame on a cloud that already holds the same tiles: the floor, (a) - (c) is what the copy costs
    gather          the gather alone; its rate is 32 M algorithmic bytes (16 read, 16 written per point) over its time
    reuse_host      (d) reduced_map_device when the rectangle has not changed: no kernel; HOST microseconds per call (perf_counter)

The grids of (a), (b) and (c) are compared bit for bit once, before timing.  One-time costs: the index build (host clock around the
build and a synchronise) and the device memory it holds.  The GPU arms are called through ctypes with ready-made arguments in ONE
process: `warmup` calls, then `reps` calls between two device events; the arms alternate, `rounds` times over (every other round in
reverse order).

    python tools/bench_points_map.py [--reps 50] [--warmup 5] [--rounds 5] [--views 1,3] [--tiles 5,10,20] [--points 5000000]
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
from vision_semantic_segmentation_amd import SemanticMapping, _lib, get_cfg_defaults, points_map as pm, synthetic as syn  # noqa: E402
from vision_semantic_segmentation_amd.camera import Camera, camera_setup_1, camera_setup_6  # noqa: E402
from vision_semantic_segmentation_amd.labels import PALETTE_19  # noqa: E402
from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET, _dbl  # noqa: E402
from vision_semantic_segmentation_amd.utils.logger import MyLogger  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--views", default="1,3")
ap.add_argument("--tiles", default="5,10,20")
ap.add_argument("--points", type=int, default=5000000)
ap.add_argument("--extent", type=float, default=600.0)
args = ap.parse_args()

dev = torch.device("cuda", 0)
H, W, LH, LW = 1080, 1920, 266, 476
L = _lib.lib()
POSE = np.array([-PCD_ORIGIN_OFFSET[0] + 3.0, -PCD_ORIGIN_OFFSET[1] - 2.0, 0.0, 0.0, 0.0, np.sin(0.35), np.cos(0.35)])   # the grid's centre, yaw 0.7


def cameras(V):
    c1, c6 = camera_setup_1().scaled(1.0, H / 1440.0), camera_setup_6().scaled(1.0, H / 1440.0)
    K3 = c1.K.copy()
    K3[0, 2] += 171.0
    K3[1, 2] -= 52.0
    return [c1, c6, Camera(K3, c1.R, c1.t)][:V]


def site():
    """the prior map: uniform over extent x extent around the vehicle, float32 [N, 4] in the world frame"""
    rng = np.random.default_rng(7)
    n, e = args.points, args.extent
    p = np.empty((n, 4), dtype=np.float32)
    p[:, 0] = rng.uniform(POSE[0] - e / 2, POSE[0] + e / 2, n)
    p[:, 1] = rng.uniform(POSE[1] - e / 2, POSE[1] + e / 2, n)
    p[:, 2] = rng.uniform(-0.3, 2.7, n)
    p[:, 3] = rng.uniform(0.0, 255.0, n)
    return p


def gpu_time(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / args.reps


def check(rc):
    if rc:
        raise RuntimeError(_lib.last_error())


def run(cloud, tile_m, V):
    cams = cameras(V)
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary((3.0, -2.0), 100.0)           # POSE sits at the grid's centre
    cfg.MAPPING.RESOLUTION = 0.1
    cfg.MAPPING.PCD.USE_INTENSITY = False
    cfg.MAPPING.POINTS_MAP.SOURCE = "index"
    cfg.MAPPING.POINTS_MAP.TILE_M = tile_m
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    g = sm.grid
    assert (g.Hm, g.Wm, g.C) == (2000, 2000, 5) and g.map.dtype == torch.float64

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = sm.load_points_map(cloud, tile_m)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3

    rect = pm.window(index, POSE, cams, (H, W), float(sm.pcd_range_max), 0.0, float(cfg.MAPPING.POINTS_MAP.MARGIN_M))
    M, runs = pm.window_count(index.offsets_host, index.rows, index.cols, rect)
    box = pm.window_box(POSE, cams, (H, W), float(sm.pcd_range_max), 0.0, float(cfg.MAPPING.POINTS_MAP.MARGIN_M))
    dst = torch.empty((M, 4), dtype=torch.float32, device=dev)
    pm.gather(index, rect, dst)
    cropped = dst.clone()

    gen = torch.Generator().manual_seed(1)
    small = torch.randint(0, 19, (V, LH, LW), generator=gen, dtype=torch.uint8).to(dev)
    src = (C.c_void_p * V)(*[small[v].data_ptr() for v in range(V)])
    g.ensure_capacity(len(index))
    gs = g.struct()
    Pall = _dbl(np.stack([np.asarray(cam.P, dtype=np.float64) for cam in cams]))
    T = _dbl(sm._origin_to_velodyne(POSE))
    cm, colors, lut = _dbl(sm.confusion_matrix), sm._colors_host(), sm._lut_host(PALETTE_19)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def view(t):
        v = _lib.points_view(t, dev)
        return (C.c_void_p(v[0].data_ptr()),) + tuple(v[1:])
    views = {"whole": view(index.points), "cropped": view(cropped), "gathered": view(dst)}
    gargs = (C.c_void_p(index.points.data_ptr()), C.c_void_p(index.offsets.data_ptr()), index.offsets_host.ctypes.data_as(C.c_void_p), index.rows,
             index.cols, rect[0], rect[1], rect[2], rect[3], C.c_void_p(dst.data_ptr()), M, stream)

    def frame(which):
        check(L.avl_fused_frame_views(C.byref(gs), *views[which], V, Pall, T, float(sm.pcd_range_max), _lib.AVL_SRC_CLASSMAP, src, LW, LH, W, H,
                                      lut, colors, cm, 0, stream))

    def gather():
        check(L.avl_points_map_gather(*gargs))

    def gather_frame():
        gather()
        frame("gathered")

    arms = [("gather_frame", gather_frame), ("whole", lambda: frame("whole")), ("cropped", lambda: frame("cropped")), ("gather", gather)]
    grids = {}
    for name, fn in arms[:3]:
        g.map.zero_()
        fn()
        grids[name] = g.map.clone()
    equal = bool(torch.equal(grids["gather_frame"], grids["whole"]) and torch.equal(grids["cropped"], grids["whole"]))
    cells = int((grids["whole"] != 0).any(dim=2).sum().item())
    if not equal:
        raise RuntimeError("the grids of the gathered, the cropped and the whole cloud differ")

    samples = {name: [] for name, _ in arms}
    for r in range(args.rounds):
        for name, fn in (arms if r % 2 == 0 else arms[::-1]):
            samples[name].append(gpu_time(fn))
    # (d): the rectangle has not changed -- no kernel, the host's work per call
    sm.reduced_map_device(POSE, cams, (H, W))
    assert sm.last_reduced["reused"] is False and sm.last_reduced["points"] == M
    t0 = time.perf_counter()
    for _ in range(200):
        sm.reduced_map_device(POSE, cams, (H, W))
    reuse_host_us = (time.perf_counter() - t0) * 1e6 / 200
    assert sm.last_reduced["reused"] is True

    row = {"tile_m": tile_m, "n_views": V, "site_points": len(index), "site_extent_m": args.extent,
           "density_per_m2": round(len(index) / args.extent ** 2, 2), "tiles": [index.rows, index.cols], "rect": list(rect),
           "box_m": [round(b, 2) for b in box], "box_share_of_radius_square": round((box[1] - box[0]) * (box[3] - box[2]) / (2 * float(sm.pcd_range_max)) ** 2, 3),
           "gathered_points": M, "runs": runs, "share_of_site": round(M / len(index), 4), "cells_touched": cells, "grids_bit_equal": equal,
           "index_build_ms": round(build_ms, 1), "index_device_mb": round(index.device_bytes() / 1e6, 1), "reuse_host_us": round(reuse_host_us, 1)}
    for name in samples:
        row[name] = {"median_us": round(statistics.median(samples[name]), 2), "min_us": round(min(samples[name]), 2),
                     "max_us": round(max(samples[name]), 2)}
    row["copy_cost_us"] = round(row["gather_frame"]["median_us"] - row["cropped"]["median_us"], 2)
    row["gather_gb_per_s"] = round(32.0 * M / (row["gather"]["median_us"] * 1e-6) / 1e9, 1)
    print(json.dumps(row), flush=True)
    sm.points_map_index = None
    return row


def main():
    cloud = torch.from_numpy(site()).to(dev)
    print("site: %d points over %g m x %g m (%.1f per m2), z -0.3 .. 2.7 m; grid 2000 x 2000 x 5 f64; %d x %d images, class maps %d x %d"
          % (args.points, args.extent, args.extent, args.points / args.extent ** 2, H, W, LH, LW), flush=True)
    rows = [run(cloud, float(t), int(v)) for t in args.tiles.split(",") for v in args.views.split(",")]
    names = ("gather_frame", "whole", "cropped", "gather")
    print("\ntile V |        M | " + " | ".join("%-24s" % (n + " us (min..max)") for n in names) + " | copy us | GB/s | reuse host us | build ms |  MB")
    for r in rows:
        print("%4g %d | %8d | " % (r["tile_m"], r["n_views"], r["gathered_points"])
              + " | ".join("%8.1f (%6.1f..%7.1f)" % (r[n]["median_us"], r[n]["min_us"], r[n]["max_us"]) for n in names)
              + " | %7.1f | %4.0f | %13.1f | %8.1f | %4.0f" % (r["copy_cost_us"], r["gather_gb_per_s"], r["reuse_host_us"], r["index_build_ms"], r["index_device_mb"]))


if __name__ == "__main__":
    main()
