#!/usr/bin/env python3
"""Cost of MODEL.DECODER.REFINE_KERNEL_SIZE: the k x k depthwise op alone (AVL_OP_DWCONV, seg_dwconv_k.hip; k = 3 is the shipped
k_dwconv / k_dwconv_split for comparison) at the 1080p decoder shape, and whole-plan frames/s with k x k refine blocks.

Op alone: a one-op plan on 270 x 480 pixels x 512 channels (the first refine block's input at 1080 x 1920), for each form (f32, f16,
bf16, split = hi + lo f16 planes) and k; device events around --iters runs after warm-up, the median of --repeats such batches.  Bytes
= the input and output planes once each; the share is of --copy-tbs (the copy bandwidth measured on MI355X, about 6.3 TB/s).
Whole plan: SemanticSegmentation at 1080 x 1920 (captured graph), seeded weights drawn for each kernel-size list, --frames forwards.

    python tools/bench_refine_kernel.py
    python tools/bench_refine_kernel.py --ks 5 --forms split --plans "" --json out.json"""
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
from vision_semantic_segmentation_amd import SemanticSegmentation, _lib  # noqa: E402
from vision_semantic_segmentation_amd.config import get_network_cfg_defaults  # noqa: E402
from vision_semantic_segmentation_amd.network import AvlSegOp, OP_DWCONV, random_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", default="1,3,5,7", help="comma list of depthwise kernel sizes for the op alone")
ap.add_argument("--forms", default="f32,f16,bf16,split")
ap.add_argument("--shape", default="270x480x512", help="HxWxC of the op's input")
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--copy-tbs", type=float, default=6.3, help="measured copy bandwidth (TB/s) the op's bytes are compared with")
ap.add_argument("--plans", default="3-3,5-5,7-7", help="comma list of refine kernel-size lists for the whole plan ('' = none)")
ap.add_argument("--precisions", default="mixed,split16,f32")
ap.add_argument("--size", default="1080x1920")
ap.add_argument("--frames", type=int, default=30)
ap.add_argument("--json", default=None)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_refine_kernel.py measures on the GPU; none is visible")
dev = torch.device("cuda", 0)
stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
results = {"op": [], "plan": []}


def op_case(form, ks, h, w, c):
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}.get(form, torch.float16)
    oh, ow = h - (ks - 1), w - (ks - 1)
    g = torch.Generator().manual_seed(ks)
    keep = [torch.randn(h * w, c, generator=g).to(dt).to(dev), torch.empty(oh * ow, c, dtype=dt, device=dev),
            (0.2 * torch.randn(ks * ks, c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev),
            torch.zeros(64, dtype=torch.uint8, device=dev)]
    op = AvlSegOp()
    op.kind, op.dtype = OP_DWCONV, {"f32": _lib.AVL_F32, "bf16": _lib.AVL_BF16}.get(form, _lib.AVL_F16)
    op.in_, op.out, op.weight, op.bias = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr()
    if form == "split":
        keep += [torch.randn(h * w, c, generator=g).to(dt).to(dev) * 1e-3, torch.empty(oh * ow, c, dtype=dt, device=dev)]
        op.in_lo, op.out_lo = keep[5].data_ptr(), keep[6].data_ptr()
    if ks == 3:
        op.in2 = keep[4].data_ptr()             # the 3x3 op's zero page
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = h, w, c, c, h * w
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = oh, ow, c, c, oh * ow
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu = ks, 1, 0, 1, c, 1     # the decoder's geometry
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan)), "avl_seg_plan_create")
    try:
        for _ in range(5):
            _lib.check(_lib.lib().avl_seg_plan_run(plan, stream()), "avl_seg_plan_run")
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                _lib.lib().avl_seg_plan_run(plan, stream())
            e1.record()
            torch.cuda.synchronize(dev)
            times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    finally:
        _lib.lib().avl_seg_plan_destroy(plan)
    us = statistics.median(times)
    planes = 2 if form == "split" else 1
    nbytes = planes * keep[0].element_size() * c * (h * w + oh * ow)
    share = nbytes / (us * 1e-6) / (a.copy_tbs * 1e12)
    r = dict(form=form, k=ks, shape=[h, w, c], us=us, gbytes=nbytes / 1e9, share_of_copy=share)
    results["op"].append(r)
    print("op  k=%d %-5s %dx%dx%d: %8.1f us  %.3f GB  %5.1f %% of %.1f TB/s%s" % (ks, form, h, w, c, us, nbytes / 1e9, 100 * share, a.copy_tbs,
                                                                              "  (shipped 3x3 kernel)" if ks == 3 else ""), flush=True)


def plan_case(ks, precision, h, w):
    cfg = get_network_cfg_defaults()
    cfg.MODEL.PRECISION = "mixed" if precision == "split16" else precision
    cfg.MODEL.DECODER.REFINE_KERNEL_SIZE = list(ks)
    cfg.MODEL.MIXED_SELF_CHECK = False
    seg = SemanticSegmentation(cfg, device=dev, state_dict=random_state_dict(seed=0, refine_kernel_size=ks))
    if precision == "split16":
        seg._rung = "split16"
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(h, w, 3), dtype=np.uint8)).to(dev)
    net = seg.net_for(h, w)
    for _ in range(5):
        net.forward(img)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(a.frames):
        net.forward(img)
    torch.cuda.synchronize(dev)
    fps = a.frames / (time.perf_counter() - t0)
    prof = net.profile()
    dec_ms = sum(r["ms"] for r in prof if r["name"].startswith("decoder.refine_layers"))
    dw_ms = sum(r["ms"] for r in prof if r["name"].startswith("decoder.refine_layers") and r["kind"] == "dwconv")
    r = dict(refine_kernel_size=list(ks), precision=precision, size=[h, w], fps=fps, refine_blocks_ms=dec_ms, kxk_dwconv_ms=dw_ms)
    results["plan"].append(r)
    print("plan %s %-7s %dx%d: %6.1f frames/s  (refine blocks %.3f ms, of which depthwise ops %.3f ms, one profiled run)"
          % (list(ks), precision, h, w, fps, dec_ms, dw_ms), flush=True)
    del net, seg
    torch.cuda.empty_cache()


h, w, c = (int(v) for v in a.shape.split("x"))
for ks in [int(k) for k in a.ks.split(",") if k]:
    for form in [f for f in a.forms.split(",") if f]:
        op_case(form, ks, h, w, c)
H, W = (int(v) for v in a.size.split("x"))
for spec in [s for s in a.plans.split(",") if s]:
    ks = tuple(int(k) for k in spec.split("-"))
    for precision in [p for p in a.precisions.split(",") if p]:
        plan_case(ks, precision, H, W)
if a.json:
    with open(a.json, "w") as f:
        json.dump(results, f, indent=1)
