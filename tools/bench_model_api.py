#!/usr/bin/env python3
"""Cost of the reference's model API (models.DeepLabV3Plus: normalised fp32 N x 3 x H x W in, fp32 logits out, each call a new tensor)
against the uint8 path (SemanticSegmentation.logits on uint8 frames, a view of the plan's buffer), and of the stem alone per input format.

For every size, batch and precision: device events around --iters calls of model(x, upsample_pred=False), model(x, upsample_pred=True)
and seg.logits(u8) after warm-up, with x and the frames already on the device; then the stem's time from net.profile() (HIP events
around each op) of the u8 plan and of the fp32-input plan, the median of --profiles runs.  One line per case, then a markdown table
(DESIGN section 3.7).

    python tools/bench_model_api.py
    python tools/bench_model_api.py --cases 480x640x4 --precisions mixed --json out.json"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd import DeepLabV3Plus  # noqa: E402
from vision_semantic_segmentation_amd.config import get_network_cfg_defaults  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="1080x1920x1,480x640x4", help="comma list of HxWxN")
ap.add_argument("--precisions", default="mixed,split16,f32")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--profiles", type=int, default=10, help="net.profile() runs per plan for the stem's median time")
ap.add_argument("--json", default=None)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_model_api.py measures on the GPU; none is visible")
dev = torch.device("cuda", 0)
MEAN = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stem_ms(net, runs):
    return statistics.median(net.profile()[0]["ms"] for _ in range(runs))


cfg = get_network_cfg_defaults()
m = cfg.MODEL
rows = []
for case in a.cases.split(","):
    h, w, n = (int(v) for v in case.lower().split("x"))
    frames = torch.from_numpy(np.random.default_rng(h + n).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)).to(dev)
    x = ((frames.permute(0, 3, 1, 2).float() / 255 - MEAN) / STD).contiguous()
    u8 = frames[0] if n == 1 else frames
    for prec in a.precisions.split(","):
        model = DeepLabV3Plus(3, cfg.DATASET.NUM_CLASSES, m.BACKBONE, m.ASPP, m.DECODER, m.OUTPUT_STRIDE, precision=prec, device=dev,
                              self_check=False).eval()
        seg = model.segmentation()
        with torch.no_grad():
            r = dict(h=h, w=w, batch=n, precision=prec,
                     model_ms=timed(lambda: model(x, upsample_pred=False), a.iters, a.warmup),
                     model_upsample_ms=timed(lambda: model(x, upsample_pred=True), a.iters, a.warmup),
                     u8_logits_ms=timed(lambda: seg.logits(u8), a.iters, a.warmup),
                     u8_logits_upsample_ms=timed(lambda: seg.logits(u8, upsample_pred=True), a.iters, a.warmup))
        r["stem_u8_ms"] = stem_ms(seg.net_for(h, w, batch=n), a.profiles)
        r["stem_f32_ms"] = stem_ms(seg.net_for(h, w, batch=n, input_format="f32_nchw"), a.profiles)
        r["model_vs_u8"] = r["model_ms"] / r["u8_logits_ms"]
        r["stem_f32_vs_u8"] = r["stem_f32_ms"] / r["stem_u8_ms"]
        rows.append(r)
        print("%4dx%-4d N=%d %-7s model %7.3f ms (upsample %7.3f) | u8 logits %7.3f ms (upsample %7.3f) | x%.3f | stem u8 %.4f ms, f32 %.4f ms (x%.2f)"
              % (h, w, n, prec, r["model_ms"], r["model_upsample_ms"], r["u8_logits_ms"], r["u8_logits_upsample_ms"], r["model_vs_u8"],
                 r["stem_u8_ms"], r["stem_f32_ms"], r["stem_f32_vs_u8"]), flush=True)
        del model, seg
        torch.cuda.empty_cache()

print("\n| size x N | precision | model(x, False) ms | seg.logits(u8) ms | ratio | model(x) ms | seg.logits(u8, True) ms | stem u8 ms | stem f32 ms |")
print("|---|---|---|---|---|---|---|---|---|")
for r in rows:
    print("| %d x %d x %d | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.4f | %.4f |" % (r["h"], r["w"], r["batch"], r["precision"], r["model_ms"],
          r["u8_logits_ms"], r["model_vs_u8"], r["model_upsample_ms"], r["u8_logits_upsample_ms"], r["stem_u8_ms"], r["stem_f32_ms"]))
if a.json:
    with open(a.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(dev), rows=rows), f, indent=1)
