#!/usr/bin/env python3
"""Times the fused frame plain, with the height gate (with and without its count), and with the gate and the elevation layer
(include/avl_hip.h, struct avl_height):

    120 k and 1 M points on the 2000 x 2000 x 5 float64 grid (0.2 m cells), class-map sources 266 x 476 sampled as 1080 x 1920 images,
    float32-AoS clouds (the layout the node feeds), one view (the single-view kernels) and three views (the views kernels).

The cloud is a ground sheet with +-0.2 m of noise (60 %), a canopy 2 to 5 m above it (30 %) and points up to 1.5 m below and above the
band (10 %) under the pixels of tools/bench_occlusion.py's cloud, the plane z = -2 of the velodyne frame, MAPPING.HEIGHT_GATE's and
MAPPING.ELEVATION's defaults.  The four arms are called through ctypes with ready-made arguments in ONE process: `warmup` calls, then
`reps` calls between two device events; the arms alternate, `rounds` times over (every other round in reverse order).  The plain arm
runs the kernels that were there before, unchanged (profiles/height/device_code_diff.txt); the figures to read are the extra time per
frame of the gated arm over it (the memset of the counts, the dearer vote kernel, and one atomic on gated[v] per wave that gated a
point), of the same without the count (gated = NULL: the gate's arithmetic alone) and of the layer over the gated arm (up to four
integer atomics per voting point).

    python tools/bench_height.py [--reps 200] [--warmup 10] [--rounds 5] [--views 1,3] [--points 120000,1000000]
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
ap.add_argument("--points", default="120000,1000000")
args = ap.parse_args()

dev = torch.device("cuda", 0)
H, W = 1080, 1920
RES, HALF = 0.2, 200.0                                         # 2000 x 2000 cells
GROUND = (0.0, 0.0, 1.0, 2.0)
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


def run(n, V):
    rng = np.random.default_rng(1)
    cams = cameras(V)
    pcd = np.concatenate([syn.make_cloud(rng, n // V, cam.K, cam.R, cam.t, W, H) for cam in cams], axis=1)
    pcd = np.ascontiguousarray(pcd[:, rng.permutation(pcd.shape[1])])
    n = pcd.shape[1]
    kind, u = rng.choice(3, size=n, p=[0.6, 0.3, 0.1]), rng.random(n)
    pcd[2] = -2.0 + np.select([kind == 0, kind == 1], [-0.2 + 0.4 * u, 2.0 + 3.0 * u], -1.5 + 3.0 * u)
    small = torch.from_numpy(np.stack([syn.make_label_map(rng, 266, 476, tile=8) for _ in range(V)])).to(dev)
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], HALF)
    cfg.MAPPING.RESOLUTION = RES
    cfg.MAPPING.HEIGHT_GATE.ENABLED = True
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    sm.set_ground_plane(GROUND)
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
    gated_only = sm._height(V, None, "velodyne")
    cfg.MAPPING.ELEVATION.ENABLED = True
    with_layer = sm._height(V, None, "velodyne")
    uncounted = _lib.AvlHeight.from_buffer_copy(gated_only)
    uncounted.gated = None
    head = (C.byref(gs), pts, n, dtype, pstride, cstride, V, Pall, None, rmax, _lib.AVL_SRC_CLASSMAP, src, 476, 266, W, H, lut, colors, cm, bonus)

    def check(rc):
        if rc:
            raise RuntimeError(_lib.last_error())

    def plain():
        check(L.avl_fused_frame_views(*head, stream))

    def gated():
        check(L.avl_fused_frame_views_height(*head, None, None, C.byref(gated_only), stream))

    def nocount():
        check(L.avl_fused_frame_views_height(*head, None, None, C.byref(uncounted), stream))

    def layer():
        check(L.avl_fused_frame_views_height(*head, None, None, C.byref(with_layer), stream))

    g.map.zero_()
    plain()
    touched_plain = int((g.map != 0).any(dim=2).sum().item())
    g.map.zero_()
    gated()
    touched_gated = int((g.map != 0).any(dim=2).sum().item())
    withheld = sm.last_gated.cpu().tolist()
    sm.reset_elevation()
    layer()
    cnt = sm.elevation_layer()[1]
    layer_points, layer_cells = int(cnt.sum().item()), int((cnt > 0).sum().item())

    variants = [("plain", plain), ("gated", gated), ("nocount", nocount), ("layer", layer)]
    samples = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            samples[name].append(gpu_time(fn))
    row = {"n": n, "cells": g.Hm * g.Wm, "n_views": V, "path": int(L.avl_fused_frame_views_path(C.byref(gs), n, V, bonus)),
           "gated_votes": withheld, "touched_cells_plain": touched_plain, "touched_cells_gated": touched_gated, "layer_points": layer_points,
           "layer_cells": layer_cells}
    for name in samples:
        row[name] = {"median_us": round(statistics.median(samples[name]), 2), "min_us": round(min(samples[name]), 2),
                     "max_us": round(max(samples[name]), 2), "samples_us": [round(s, 2) for s in samples[name]]}
    row["gate_extra_us"] = round(row["gated"]["median_us"] - row["plain"]["median_us"], 2)
    row["nocount_extra_us"] = round(row["nocount"]["median_us"] - row["plain"]["median_us"], 2)
    row["layer_extra_us"] = round(row["layer"]["median_us"] - row["gated"]["median_us"], 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = [run(int(n), V) for n in args.points.split(",") for V in [int(v) for v in args.views.split(",")]]
    print("\n      n  V path | plain us (min..max)       | gated us (min..max)       | gate + layer us (min..max) | gate extra | same, no count | layer extra | gated votes, layer points")
    for r in rows:
        a, b, c = r["plain"], r["gated"], r["layer"]
        print("%7d %2d %4d | %7.1f (%6.1f..%6.1f) | %7.1f (%6.1f..%6.1f) | %7.1f (%6.1f..%6.1f)  | %7.1f    | %7.1f        | %7.1f     | %d, %d"
              % (r["n"], r["n_views"], r["path"], a["median_us"], a["min_us"], a["max_us"], b["median_us"], b["min_us"], b["max_us"],
                 c["median_us"], c["min_us"], c["max_us"], r["gate_extra_us"], r["nocount_extra_us"], r["layer_extra_us"], sum(r["gated_votes"]), r["layer_points"]))


if __name__ == "__main__":
    main()
