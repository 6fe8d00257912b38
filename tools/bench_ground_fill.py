#!/usr/bin/env python3
"""Times the dense ground fill (avl_ground_fill_views / _logits, one kernel: k_ground_fill) on the scene it is meant for: a
600 x 600 window of the 2000 x 2000 x 5 float64 grid (0.1 m cells, velodyne frame) around the vehicle, cameras at 1080 x 1920 with
the 266 x 476 class map or the 266 x 476 x 19 logits, the ground plane of the vehicle's base link, GROUND_FILL's default range.

    fill_classmap     the fill from class maps
    fill_nocount      the same without the optional `filled` count (gf.filled NULL): no memset, no atomics
    fill_logits       the fill from logits (MIN_MARGIN 0)
    fill_occl         avl_occlusion_depth over a 120 k-point cloud, then the fill from class maps with the cull test
    virtual_cloud     the same cells as a float64 cloud of 360 k points through avl_fused_frame_views: the vote kernels that were
                      there before the fill existed, unchanged (profiles/ground_fill/device_code_diff.txt), and the only route to
                      the same grid without it (full class mask, the fill's range; the grids are compared once, before timing)
    frame_120k        the plain frame of the 120 k-point float32 cloud, for scale

The arms are called through ctypes with ready-made arguments in ONE process: `warmup` calls, then `reps` calls between two device
events; the arms alternate, `rounds` times over (every other round in reverse order).

    python tools/bench_ground_fill.py [--reps 200] [--warmup 10] [--rounds 5] [--views 1,3]
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
from vision_semantic_segmentation_amd.ground_plane import plane_to_frame  # noqa: E402
from vision_semantic_segmentation_amd.labels import PALETTE_19  # noqa: E402
from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET, _dbl  # noqa: E402
from vision_semantic_segmentation_amd.utils.logger import MyLogger  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--views", default="1,3")
args = ap.parse_args()

dev = torch.device("cuda", 0)
H, W, LH, LW, K = 1080, 1920, 266, 476, 19
N_CLOUD, WINDOW = 120000, 600
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


def check(rc):
    if rc:
        raise RuntimeError(_lib.last_error())


def run(V):
    rng = np.random.default_rng(1)
    cams = cameras(V)
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], 100.0)
    cfg.MAPPING.RESOLUTION = 0.1
    cfg.MAPPING.PCD.USE_INTENSITY = False
    cfg.MAPPING.OCCLUSION.ENABLED = True
    cfg.MAPPING.GROUND_FILL.CLASSES = list(cfg.LABELS_NAMES)              # a full class mask: the virtual cloud has none
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    g = sm.grid
    assert (g.Hm, g.Wm, g.C) == (2000, 2000, 5) and g.map.dtype == torch.float64
    plane = plane_to_frame([0.0, 0.0, 1.0, 0.0], sm.T_velodyne_to_basklink)       # the base link's z = 0, in the velodyne frame
    (x0, y0), (h, w), _ = sm.live_map_window(np.zeros(7), (WINDOW, WINDOW))
    fill_range = float(cfg.MAPPING.GROUND_FILL.RANGE_MAX)

    gen = torch.Generator().manual_seed(1)
    logits = torch.randn((V, LH, LW, K), generator=gen).to(dev)
    small = logits.argmax(3).to(torch.uint8).contiguous()
    src = (C.c_void_p * V)(*[small[v].data_ptr() for v in range(V)])
    abstained = torch.zeros(V, dtype=torch.int32, device=dev)
    pl, _, _ = sm._point_logits([logits[v] for v in range(V)], (H, W), (H, W), (abstained, 0))
    filled = torch.zeros(V, dtype=torch.int32, device=dev)
    gf = _lib.AvlGroundFill()
    gf.x0, gf.y0, gf.h, gf.w = x0, y0, h, w
    gf.plane[:] = [float(v) for v in plane]
    gf.range_max, gf.class_mask, gf.filled = fill_range, sm._ground_fill_class_mask(), filled.data_ptr()

    # the real cloud (float32 AoS, what the node feeds) and the window's cell centres on the plane (float64 SoA: exact)
    cloud = np.concatenate([syn.make_cloud(rng, N_CLOUD // V, cam.K, cam.R, cam.t, W, H) for cam in cams], axis=1)
    cloud_t = torch.from_numpy(np.ascontiguousarray(cloud[:, rng.permutation(cloud.shape[1])].T.astype(np.float32))).to(dev)
    i, j = np.meshgrid(np.arange(x0, x0 + h, dtype=np.float64), np.arange(y0, y0 + w, dtype=np.float64), indexing="ij")
    x = (float(sm.map_boundary[0][0]) + (i.ravel() + 0.5) * 0.1) - PCD_ORIGIN_OFFSET[0]
    y = (float(sm.map_boundary[1][0]) + (j.ravel() + 0.5) * 0.1) - PCD_ORIGIN_OFFSET[1]
    t = plane[0] * x
    t = t + plane[1] * y
    t = t + plane[3]
    virtual_t = torch.from_numpy(np.stack([x, y, (-t) / plane[2], np.zeros_like(x)])).to(dev)

    g.ensure_capacity(max(virtual_t.shape[1], cloud_t.shape[0]))
    gs = g.struct()
    Pall = _dbl(np.stack([np.asarray(cam.P, dtype=np.float64) for cam in cams]))
    cm, colors, lut = _dbl(sm.confusion_matrix), sm._colors_host(), sm._lut_host(PALETTE_19)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    occ = sm._occlusion(V, H, W)
    culled = sm.last_culled
    cpts = _lib.points_view(cloud_t, dev)
    vpts = _lib.points_view(virtual_t, dev)
    cview = (C.c_void_p(cpts[0].data_ptr()),) + tuple(cpts[1:])
    vview = (C.c_void_p(vpts[0].data_ptr()),) + tuple(vpts[1:])
    fill_head = (C.byref(gs), C.byref(gf), V, Pall, None)

    def fill_classmap():
        check(L.avl_ground_fill_views(*fill_head, _lib.AVL_SRC_CLASSMAP, src, LW, LH, W, H, lut, colors, cm, None, stream))

    gf_nocount = _lib.AvlGroundFill.from_buffer_copy(gf)
    gf_nocount.filled = None

    def fill_nocount():
        check(L.avl_ground_fill_views(C.byref(gs), C.byref(gf_nocount), V, Pall, None, _lib.AVL_SRC_CLASSMAP, src, LW, LH, W, H, lut, colors,
                                      cm, None, stream))

    def fill_logits():
        check(L.avl_ground_fill_views_logits(*fill_head, C.byref(pl), W, H, lut, cm, None, stream))

    def fill_occl():
        check(L.avl_occlusion_depth(*cview, V, Pall, None, float(sm.pcd_range_max), W, H, C.byref(occ), stream))
        check(L.avl_ground_fill_views(*fill_head, _lib.AVL_SRC_CLASSMAP, src, LW, LH, W, H, lut, colors, cm, C.byref(occ), stream))

    def virtual_cloud():
        check(L.avl_fused_frame_views(C.byref(gs), *vview, V, Pall, None, fill_range, _lib.AVL_SRC_CLASSMAP, src, LW, LH, W, H, lut, colors,
                                      cm, 0, stream))

    def frame_120k():
        check(L.avl_fused_frame_views(C.byref(gs), *cview, V, Pall, None, float(sm.pcd_range_max), _lib.AVL_SRC_CLASSMAP, src, LW, LH, W, H,
                                      lut, colors, cm, 0, stream))

    grids = {}
    for name, fn in (("fill_classmap", fill_classmap), ("virtual_cloud", virtual_cloud), ("fill_occl", fill_occl)):
        g.map.zero_()
        fn()
        grids[name] = g.map.clone()
        if name == "fill_classmap":
            n_filled = filled.cpu().tolist()
    differ = int((grids["fill_classmap"] != grids["virtual_cloud"]).any(dim=2).sum().item())
    cells ={name: int((m != 0).any(dim=2).sum().item()) for name, m in grids.items()}

    variants = [("fill_classmap", fill_classmap), ("fill_nocount", fill_nocount), ("fill_logits", fill_logits), ("fill_occl", fill_occl), ("virtual_cloud", virtual_cloud),
                ("frame_120k", frame_120k)]
    samples = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            samples[name].append(gpu_time(fn))
    row = {"n_views": V, "window": [h, w], "cells": h * w, "cloud_points": int(cloud_t.shape[0]), "filled": n_filled,
           "culled_with_occl": culled.cpu().tolist(), "cells_fill": cells["fill_classmap"], "cells_fill_occl": cells["fill_occl"], "cells_differ_fill_vs_virtual_cloud": differ,
           "virtual_cloud_path": int(L.avl_fused_frame_views_path(C.byref(gs), int(virtual_t.shape[1]), V, 0))}
    for name in samples:
        row[name] = {"median_us": round(statistics.median(samples[name]), 2), "min_us": round(min(samples[name]), 2),
                     "max_us": round(max(samples[name]), 2), "samples_us": [round(s, 2) for s in samples[name]]}
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = [run(int(v)) for v in args.views.split(",")]
    names = ("fill_classmap", "fill_nocount", "fill_logits", "fill_occl", "virtual_cloud", "frame_120k")
    print("\n V | " + " | ".join("%-22s" % (n + " us (min..max)") for n in names))
    for r in rows:
        print("%2d | " % r["n_views"] + " | ".join("%6.1f (%6.1f..%6.1f)" % (r[n]["median_us"], r[n]["min_us"], r[n]["max_us"]) for n in names))


if __name__ == "__main__":
    main()
