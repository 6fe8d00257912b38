#!/usr/bin/env python3
"""Times the three ways a frame's LiDAR points can get their labels, on the mapping configurations of tools/bench_mapping.py

    C   120 k points on 2000 x 2000 cells (sparse: the partitioned lists)      E   1 M points on 4000 x 4000 cells (dense: the sweep)

for one view and three, fp32 logits 266 x 476 x 19 (what the default plan writes for a 1080 x 1920 camera), float32-AoS clouds:

    (a) classmap   avl_fused_frame(_views) on the plan's 266 x 476 label map, nearest-sampled as the 1080 x 1920 image
    (b) full_res   avl_seg_eval_full_res(_batch) writes the 1080 x 1920 arg-max of the interpolated logits, then (a) on that map
    (c) logits     avl_fused_frame(_views)_logits: the same labels as (b), interpolated only where a point lands (MIN_MARGIN 0)

All arms are called through ctypes with ready-made arguments in ONE process: `warmup` calls, then `reps` calls between two device
events; the arms alternate, `rounds` times over (every other round in reverse order).  (a) runs the kernels that were there before
the logits source existed, unchanged (profiles/point_logits/device_code_diff.txt).  The grids of (b) and (c) are compared once, before
the timing: they may differ only where the full-resolution kernel and the point kernel break a near tie differently.

With --robustness the tool also runs the bench frame (bench.py's seeded 1080 x 1920 image and 120 k point cloud) through the "mixed"
and the "f32" plan and reports, for a few MIN_MARGIN values, the share of candidates that abstain under either and the number of
grid cells whose values differ between the two precisions' grids after one frame -- what the gate is meant to buy.

    python tools/bench_point_logits.py [--reps 200] [--warmup 10] [--rounds 5] [--views 1,3] [--configs C,E] [--robustness]
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
from vision_semantic_segmentation_amd import SemanticMapping, _lib, get_cfg_defaults, seg_head, synthetic as syn  # noqa: E402
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
ap.add_argument("--robustness", action="store_true")
ap.add_argument("--margins", default="0,0.05,0.1,0.25,0.5,1.0")
args = ap.parse_args()

dev = torch.device("cuda", 0)
H, W = 1080, 1920
LH, LW, K = 266, 476, 19
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


def mapper(res, half):
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], half)
    cfg.MAPPING.RESOLUTION = res
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    return sm


def check(rc):
    if rc:
        raise RuntimeError(_lib.last_error())


def run(config, V):
    n, res, half = CONFIGS[config]
    rng = np.random.default_rng(1)
    cams = cameras(V)
    pcd = np.concatenate([syn.make_cloud(rng, n // V, cam.K, cam.R, cam.t, W, H) for cam in cams], axis=1)
    pcd = np.ascontiguousarray(pcd[:, rng.permutation(pcd.shape[1])])
    n = pcd.shape[1]
    gen = torch.Generator(device="cpu").manual_seed(3)
    logits = torch.randn((V, LH, LW, K), generator=gen).to(dev)
    small = logits.argmax(3).to(torch.uint8).contiguous()                 # what the plan's fused arg-max writes
    full = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    sm = mapper(res, half)
    pts_t = torch.from_numpy(np.ascontiguousarray(pcd.T.astype(np.float32))).to(dev)
    pts, n_, dtype, pstride, cstride = sm._points_view(pts_t)
    g = sm.grid
    g.ensure_capacity(n)
    gs = g.struct()
    Pall = _dbl(np.stack([np.asarray(cam.P, dtype=np.float64) for cam in cams]))
    src_small = (C.c_void_p * V)(*[small[v].data_ptr() for v in range(V)])
    src_full = (C.c_void_p * V)(*[full[v].data_ptr() for v in range(V)])
    cm, colors, lut, bonus = _dbl(sm.confusion_matrix), sm._colors_host(), sm._lut_host(PALETTE_19), sm._bonus_classes()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rmax = float(sm.pcd_range_max)
    sm.min_margin = 0.0
    abstained = torch.zeros(V, dtype=torch.int32, device=dev)
    pl, _, _ = sm._point_logits([logits[v] for v in range(V)], (H, W), (H, W), (abstained, 0))
    head = (C.byref(gs), pts, n, dtype, pstride, cstride, V, Pall, None, rmax)

    def classmap():
        check(L.avl_fused_frame_views(*head, _lib.AVL_SRC_CLASSMAP, src_small, LW, LH, W, H, lut, colors, cm, bonus, stream))

    def full_res():
        seg_head.full_res_eval(logits if V > 1 else logits[0], H, W, labels_out=full if V > 1 else full[0])
        check(L.avl_fused_frame_views(*head, _lib.AVL_SRC_CLASSMAP, src_full, W, H, W, H, lut, colors, cm, bonus, stream))

    def from_logits():
        check(L.avl_fused_frame_views_logits(*head, C.byref(pl), W, H, lut, cm, bonus, None, stream))

    grids = {}
    for name, fn in (("classmap", classmap), ("full_res", full_res), ("logits", from_logits)):
        g.map.zero_()
        fn()
        grids[name] = g.map.clone()
    touched = int((grids["logits"] != 0).any(dim=2).sum().item())
    differ_b = int((grids["logits"] != grids["full_res"]).any(dim=2).sum().item())
    differ_a = int((grids["logits"] != grids["classmap"]).any(dim=2).sum().item())

    variants = [("classmap", classmap), ("full_res", full_res), ("logits", from_logits)]
    samples = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            samples[name].append(gpu_time(fn))
    row = {"config": config, "n": n, "cells": g.Hm * g.Wm, "n_views": V, "path": int(L.avl_fused_frame_views_path(C.byref(gs), n, V, bonus)),
           "touched_cells": touched, "cells_differ_logits_vs_full_res": differ_b, "cells_differ_logits_vs_classmap": differ_a}
    for name in samples:
        row[name] = {"median_us": round(statistics.median(samples[name]), 2), "min_us": round(min(samples[name]), 2),
                     "max_us": round(max(samples[name]), 2), "samples_us": [round(s, 2) for s in samples[name]]}
    print(json.dumps(row), flush=True)
    return row


def robustness():
    """the bench frame through the mixed and the f32 plan: abstentions and grid differences per MIN_MARGIN"""
    from vision_semantic_segmentation_amd.network import SegNet, random_state_dict
    rng = np.random.default_rng(1)
    cam = camera_setup_1().scaled(1.0, H / 1440.0, imSize=[W, H])
    image = torch.from_numpy(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
    cloud = syn.make_cloud(rng, 120000, cam.K, cam.R, cam.t, W, H)
    points = torch.from_numpy(np.ascontiguousarray(cloud.T.astype(np.float32))).to(dev)
    state = random_state_dict(0)
    logits = {}
    for precision in ("mixed", "f32"):
        net = SegNet(state, H, W, precision=precision, device=dev)
        net.forward(image)
        logits[precision] = net.logits.clone()
        del net
    rows = []
    for gate in [float(m) for m in args.margins.split(",")]:
        row = {"min_margin": gate}
        grids = {}
        for precision in ("mixed", "f32"):
            sm = mapper(0.2, 200.0)
            sm.min_margin = gate
            st, _ = sm.point_labels_device(points, "velodyne", None, cam, logits[precision], (H, W))
            cand = int((st[0] != 255).sum().item())
            row["candidates"] = cand
            row["abstained_share_" + precision] = round(int((st[0] == 254).sum().item()) / max(cand, 1), 5)
            row["state_" + precision] = st[0]
            sm.frame_device(points, "velodyne", logits[precision], None, cam, src_kind="logits", image_size=(H, W))
            grids[precision] = sm.map_dev.clone()
        a, b = row.pop("state_mixed"), row.pop("state_f32")
        row["points_labelled_differently"] = int(((a != b) & (a < 254) & (b < 254)).sum().item())
        row["points_one_abstains"] = int(((a == 254) != (b == 254)).sum().item())
        row["cells_touched_f32"] = int((grids["f32"] != 0).any(dim=2).sum().item())
        row["cells_differ_mixed_vs_f32"] = int((grids["mixed"] != grids["f32"]).any(dim=2).sum().item())
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    rows = [run(config, V) for config in args.configs.split(",") for V in [int(v) for v in args.views.split(",")]]
    print("\nconfig  V path | (a) classmap us | (b) full_res + classmap us | (c) logits us | (c) - (a) | (b) - (c) | cells (c) != (b)")
    for r in rows:
        a, b, c = r["classmap"]["median_us"], r["full_res"]["median_us"], r["logits"]["median_us"]
        print("%-6s %2d %4d | %15.1f | %26.1f | %13.1f | %9.1f | %9.1f | %d of %d"
              % (r["config"], r["n_views"], r["path"], a, b, c, c - a, b - c, r["cells_differ_logits_vs_full_res"], r["touched_cells"]))
    if args.robustness:
        print("\nbench frame, mixed against f32 (120 k points, 2000 x 2000 cells):")
        robustness()


if __name__ == "__main__":
    main()
