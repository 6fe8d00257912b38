#!/usr/bin/env python3
"""Times the fused frame with occlusion culling off and on, on the mapping configurations of tools/bench_mapping.py:

    C   120 k points on 2000 x 2000 cells (sparse: the partitioned lists)      E   1 M points on 4000 x 4000 cells (dense: the sweep)

for one view (avl_fused_frame / avl_fused_frame_occl) and three views (avl_fused_frame_views / avl_fused_frame_views_occl), class-map
sources 266 x 476 sampled as 1080 x 1920 images, float32-AoS clouds (the layout the node feeds), MAPPING.OCCLUSION's defaults.  The two
arms are called through ctypes with ready-made arguments in ONE process: `warmup` calls, then `reps` calls between two device events;
the arms alternate, `rounds` times over (every other round in reverse order).  The culling-off arm runs the kernels that were there
before culling existed, unchanged (profiles/occlusion/device_code_diff.txt); the figure to read is the extra time per frame of the
culling-on arm over it, which is the memsets of the depth buffer and the counts, the depth pass and the dearer vote kernel.

    python tools/bench_occlusion.py [--reps 200] [--warmup 10] [--rounds 5] [--views 1,3] [--configs C,E]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd import SemanticMapping, _lib, get_cfg_defaults, synthetic as syn  # noqa: E402
from vision_semantic_segmentation_amd.camera import Camera, camera_setup_1, camera_setup_6  # noqa: E402
from vision_semantic_segmentation_amd.labels import PALETTE_19  # noqa: E402
from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET, _dbl  # noqa: E402
from vision_semantic_segmentation_amd.utils.logger import MyLogger  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--views", default="1,3")
ap.add_argument("--configs", default="C,E")
args = ap.parse_args()

dev = torch.device("cuda", 0)
H, W = 1080, 1920
CONFIGS = {"C": (120000, 0.2, 200.0), "E": (1000000, 0.05, 100.0)}      # n, resolution, half extent (tools/bench_mapping.py)
L = _lib.lib()


def cameras(V):
    c1, c6 = camera_setup_1().scaled(1.0, H / 1440.0), camera_setup_6().scaled(1.0, H / 1440.0)
    K3 = c1.K.copy()
    K3[0, 2] += 171.0
    K3[1, 2] -= 52.0
    return [c1, c6, Camera(K3, c1.R, c1.t)][:V]


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


def run(config, V):
    n, res, half = CONFIGS[config]
    rng = np.random.default_rng(1)
    cams = cameras(V)
    pcd = np.concatenate([syn.make_cloud(rng, n // V, cam.K, cam.R, cam.t, W, H) for cam in cams], axis=1)
    pcd = np.ascontiguousarray(pcd[:, rng.permutation(pcd.shape[1])])
    n = pcd.shape[1]
    small = torch.from_numpy(np.stack([syn.make_label_map(rng, 266, 476, tile=8) for _ in range(V)])).to(dev)
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], half)
    cfg.MAPPING.RESOLUTION = res
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    pts_t = torch.from_numpy(np.ascontiguousarray(pcd.T.astype(np.float32))).to(dev)
    pts, n_, dtype, pstride, cstride = sm._points_view(pts_t)
    g = sm.grid
    g.ensure_capacity(n)
    gs = g.struct()
    Pall = _dbl(np.stack([np.asarray(cam.P, dtype=np.float64) for cam in cams]))
    src = (C.c_void_p * V)(*[small[v].data_ptr() for v in range(V)])
    cm, colors, lut, bonus = _dbl(sm.confusion_matrix), sm._colors_host(), sm._lut_host(PALETTE_19), sm._bonus_classes()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rmax = float(sm.pcd_range_max)
    occ = sm._occlusion(V, H, W)
    head = (C.byref(gs), pts, n, dtype, pstride, cstride, V, Pall, None, rmax, _lib.AVL_SRC_CLASSMAP, src, 476, 266, W, H, lut, colors, cm, bonus)

    def check(rc):
        if rc:
            raise RuntimeError(_lib.last_error())

    def off():
        check(L.avl_fused_frame_views(*head, stream))

    def on():
        check(L.avl_fused_frame_views_occl(*head, C.byref(occ), stream))

    g.map.zero_()
    off()
    touched_off = int((g.map != 0).any(dim=2).sum().item())
    g.map.zero_()
    on()
    touched_on = int((g.map != 0).any(dim=2).sum().item())
    counts = sm.last_culled                                # occ points into it: keep it alive while visibility_device makes its own
    culled = counts.cpu().tolist()
    state = sm.visibility_device(pts_t, "velodyne", None, cams, (H, W))
    candidates = [int((state[v] != 0).sum().item()) for v in range(V)]
    assert culled == [int((state[v] == 2).sum().item()) for v in range(V)]

    variants = [("off", off), ("on", on)]
    samples = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            samples[name].append(gpu_time(fn))
    row = {"config": config, "n": n, "cells": g.Hm * g.Wm, "n_views": V, "path": int(L.avl_fused_frame_views_path(C.byref(gs), n, V, bonus)),
           "depth_words": int(occ.depth_words), "candidates": candidates, "culled": culled, "touched_cells_off": touched_off,
           "touched_cells_on": touched_on}
    for name in samples:
        row[name] = {"median_us": round(statistics.median(samples[name]), 2), "min_us": round(min(samples[name]), 2),
                     "max_us": round(max(samples[name]), 2), "samples_us": [round(s, 2) for s in samples[name]]}
    row["extra_us"] = round(row["on"]["median_us"] - row["off"]["median_us"], 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = [run(config, V) for config in args.configs.split(",") for V in [int(v) for v in args.views.split(",")]]
    print("\nconfig  V path | culling off us (min..max) | culling on us (min..max) | extra us | candidates -> culled")
    for r in rows:
        a, b = r["off"], r["on"]
        print("%-6s %2d %4d | %7.1f (%6.1f..%6.1f)      | %7.1f (%6.1f..%6.1f)     | %7.1f  | %d -> %d"
              % (r["config"], r["n_views"], r["path"], a["median_us"], a["min_us"], a["max_us"], b["median_us"], b["min_us"], b["max_us"],
                 r["extra_us"], sum(r["candidates"]), sum(r["culled"])))


if __name__ == "__main__":
    main()
