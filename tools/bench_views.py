#!/usr/bin/env python3
"""Times avl_fused_frame_views (V cameras, one cloud, one fused pass) against V sequential avl_fused_frame calls, on the mapping
configurations of tools/bench_mapping.py:

    C   120 k points on 2000 x 2000 cells (sparse: the partitioned lists)      E   1 M points on 4000 x 4000 cells (dense: the sweep)

for V = 1, 2, 4 views (camera1, camera6, a shifted camera1, a zoomed-out camera6; class-map sources 266 x 476 sampled as
1080 x 1920 images) and float64-SoA / float32-AoS clouds.  The cloud is the union of synthetic.make_cloud draws through every
view's camera.  Every variant is called through ctypes with ready-made arguments: `warmup` calls, then `reps` calls between two
device events on the current stream.  The variants of one cell are timed in turn, `rounds` times over (every other round in
reverse order); the table gives the median of the rounds and their range.  --base PATH loads a second build of the library (e.g.
the parent commit's libavl_hip.so) and times V calls of ITS avl_fused_frame in the same rounds: the spread of those repeated runs
is the noise band a comparison has to clear.

    python tools/bench_views.py [--reps 200] [--warmup 10] [--rounds 5] [--base PATH] [--views 1,2,4] [--configs C,E]
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
ap.add_argument("--base", default=None, help="another build of libavl_hip.so whose avl_fused_frame is timed alongside (V calls)")
ap.add_argument("--views", default="1,2,4")
ap.add_argument("--configs", default="C,E")
args = ap.parse_args()

dev = torch.device("cuda", 0)
H, W = 1080, 1920
CONFIGS = {"C": (120000, 0.2, 200.0), "E": (1000000, 0.05, 100.0)}      # n, resolution, half extent (tools/bench_mapping.py)
L = _lib.lib()
BASE = None
if args.base:
    BASE = C.CDLL(os.path.abspath(args.base))
    BASE.avl_fused_frame.restype = C.c_int
    BASE.avl_fused_frame.argtypes = L.avl_fused_frame.argtypes


def cameras(V):
    c1, c6 = camera_setup_1().scaled(1.0, H / 1440.0), camera_setup_6().scaled(1.0, H / 1440.0)
    K3, K4 = c1.K.copy(), c6.K.copy()
    K3[0, 2] += 171.0
    K3[1, 2] -= 52.0
    K4[0, 0] *= 0.8
    K4[1, 1] *= 0.8
    return [c1, c6, Camera(K3, c1.R, c1.t), Camera(K4, c6.R, c6.t)][:V]


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


def summarise(samples):
    return {"median_us": round(statistics.median(samples), 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2)}


def run(config, V, layout):
    n, res, half = CONFIGS[config]
    rng = np.random.default_rng(1)
    cams = cameras(V)
    per = n // V
    pcd = np.concatenate([syn.make_cloud(rng, per, cam.K, cam.R, cam.t, W, H) for cam in cams], axis=1)
    pcd = np.ascontiguousarray(pcd[:, rng.permutation(pcd.shape[1])])
    n = pcd.shape[1]
    small = torch.from_numpy(np.stack([syn.make_label_map(rng, 266, 476, tile=8) for _ in range(V)])).to(dev)
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], half)
    cfg.MAPPING.RESOLUTION = res
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    if layout == "f32aos":
        pts_t = torch.from_numpy(np.ascontiguousarray(pcd.T.astype(np.float32))).to(dev)
    else:
        pts_t = torch.from_numpy(pcd).to(dev)
    pts, n_, dtype, pstride, cstride = sm._points_view(pts_t)
    g = sm.grid
    g.ensure_capacity(n)
    gs = g.struct()
    Ps = [_dbl(cam.P) for cam in cams]
    Pall = _dbl(np.stack([np.asarray(cam.P, dtype=np.float64) for cam in cams]))
    src = (C.c_void_p * V)(*[small[v].data_ptr() for v in range(V)])
    cm, colors, lut, bonus = _dbl(sm.confusion_matrix), sm._colors_host(), sm._lut_host(PALETTE_19), sm._bonus_classes()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rmax = float(sm.pcd_range_max)

    def check(rc):
        if rc:
            raise RuntimeError(_lib.last_error())

    def views():
        check(L.avl_fused_frame_views(C.byref(gs), pts, n, dtype, pstride, cstride, V, Pall, None, rmax, _lib.AVL_SRC_CLASSMAP, src, 476, 266,
                                      W, H, lut, colors, cm, bonus, stream))

    def sequential(lib):
        def fn():
            for v in range(V):
                check(lib.avl_fused_frame(C.byref(gs), pts, n, dtype, pstride, cstride, Ps[v], None, rmax, _lib.AVL_SRC_CLASSMAP,
                                          C.c_void_p(small[v].data_ptr()), 476, 266, W, H, lut, colors, cm, bonus, stream))
        return fn

    variants = [("views", views), ("sequential", sequential(L))]
    if BASE is not None:
        variants.append(("base_sequential", sequential(BASE)))

    # the two routes agree bit for bit, and the touched cells of the call (of each view for the sequential bytes)
    g.map.zero_()
    views()
    fused_map = g.map.clone()
    g.map.zero_()
    u_views = []
    prev = torch.zeros_like(g.map)
    for v in range(V):
        check(L.avl_fused_frame(C.byref(gs), pts, n, dtype, pstride, cstride, Ps[v], None, rmax, _lib.AVL_SRC_CLASSMAP,
                                C.c_void_p(small[v].data_ptr()), 476, 266, W, H, lut, colors, cm, bonus, stream))
        u_views.append(int((g.map != prev).any(dim=2).sum().item()))
        prev = g.map.clone()
    assert torch.equal(fused_map, g.map), "the fused views differ from the sequential frames"
    u = int((g.map != 0).any(dim=2).sum().item())
    del prev, fused_map

    samples = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            samples[name].append(gpu_time(fn))
    bpp = 16 if layout == "f32aos" else 32
    row_bytes = 2 * 5 * 8
    alg_views = n * bpp + n * V + u * (row_bytes + 8)
    alg_seq = V * (n * bpp + n) + sum(u_views) * (row_bytes + 2)
    row = {"config": config, "n": n, "cells": g.Hm * g.Wm, "n_views": V, "layout": layout,
           "path": int(L.avl_fused_frame_views_path(C.byref(gs), n, V, bonus)), "touched_cells": u, "touched_per_view": u_views,
           "algorithmic_MB_views": round(alg_views / 1e6, 2), "algorithmic_MB_sequential": round(alg_seq / 1e6, 2)}
    for name in samples:
        row[name] = summarise(samples[name])
        row[name]["samples_us"] = [round(s, 2) for s in samples[name]]
    ref = row.get("base_sequential", row["sequential"])
    row["ratio_views_over_reference"] = round(row["views"]["median_us"] / ref["median_us"], 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = []
    for config in args.configs.split(","):
        for layout in ("f64soa", "f32aos"):
            for V in [int(v) for v in args.views.split(",")]:
                rows.append(run(config, V, layout))
    ref_name = "base_sequential" if BASE is not None else "sequential"
    print("\nconfig layout  V path | views us (min..max) | %s us (min..max) | ratio | touched cells | MB views / sequential" % ref_name)
    for r in rows:
        a, b = r["views"], r[ref_name]
        print("%-6s %-7s %d %4d | %7.1f (%6.1f..%6.1f) | %7.1f (%6.1f..%6.1f) | %5.3f | %9d | %6.2f / %6.2f"
              % (r["config"], r["layout"], r["n_views"], r["path"], a["median_us"], a["min_us"], a["max_us"], b["median_us"], b["min_us"],
                 b["max_us"], r["ratio_views_over_reference"], r["touched_cells"], r["algorithmic_MB_views"], r["algorithmic_MB_sequential"]))


if __name__ == "__main__":
    main()
