#!/usr/bin/env python3
"""Frames/s of every MODEL.BACKBONE at 1080 x 1920 (output stride 8) and the dense 3x3 kernel (AVL_OP_GCONV w_layout 2) per layer
shape.  Frames/s: device events around 20 graph replays after warm-up.  Kernel: per-op HIP events (avl_seg_plan_profile, best of
--reps), grouped by shape; the events bracket each launch, so for kernel-only times run it once more under
`rocprofv3 --kernel-trace --stats -- python tools/bench_backbones.py --no-profile` (k_conv3x3 rows).

    python tools/bench_backbones.py                                   # all backbones, mixed and split16
    python tools/bench_backbones.py --backbones resnet50 --precisions f16,split16"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd.network import BACKBONES, OP_GCONV, SegNet, random_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--h", type=int, default=1080)
ap.add_argument("--w", type=int, default=1920)
ap.add_argument("--backbones", default=",".join(sorted(BACKBONES)))
ap.add_argument("--precisions", default="mixed,split16", help="comma list of mixed, split16, f16, bf16, f32")
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-profile", action="store_true", help="frames/s only (for a run under rocprofv3)")
a = ap.parse_args()

img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=(a.h, a.w, 3), dtype=np.uint8)).cuda()
for bb in a.backbones.split(","):
    st = random_state_dict(0, backbone=bb)
    for prec in a.precisions.split(","):
        kw = dict(precision="mixed", full_split=True) if prec == "split16" else dict(precision=prec)
        net = SegNet(st, a.h, a.w, device="cuda:0", backbone=bb, **kw)
        net.forward(img)
        net.capture_graph()
        for _ in range(3):
            net.forward()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.frames):
            net.forward()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.frames
        print("%-18s %-8s %7.2f ms/frame  %7.1f frames/s" % (bb, prec, ms, 1e3 / ms), flush=True)
        if a.no_profile:
            del net
            continue
        best = None
        for _ in range(a.reps):
            prof = net.profile()
            if best is None:
                best = prof
            else:
                for b, p in zip(best, prof):
                    b["ms"] = min(b["ms"], p["ms"])
        shapes = {}
        for op, p in zip(net.ops, best):
            if op.kind == OP_GCONV and op.w_layout == 2:
                cg = op.in_c // op.groups
                key = (op.out_h * op.out_w, op.out_c, 9 * cg, op.groups, op.stride, op.dil)
                s = shapes.setdefault(key, [0, 0.0, 0.0])
                s[0] += 1; s[1] += p["ms"]; s[2] += p["flops"]
        for (m, n, k, g, s_, d), (cnt, tms, fl) in sorted(shapes.items(), key=lambda kv: -kv[1][1]):
            print("    dense 3x3  M %7d  N %5d  K %5d  groups %2d  stride %d  dil %d  x%-3d %8.3f ms/op  %6.1f TF/s"
                  % (m, n, k, g, s_, d, cnt, tms / cnt, fl / tms / 1e9), flush=True)
        del net
        torch.cuda.empty_cache()
