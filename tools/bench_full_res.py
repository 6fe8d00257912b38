#!/usr/bin/env python3
"""Times the full-resolution head (csrc/seg_head.hip) at the bench frame's shapes: logits 266 x 476 x 19 (what the plan leaves for a
1080 x 1920 input) -> 1080 x 1920, against the torch route it replaces.  Per case: `warmup` calls, then `reps` calls between two
hipEvents on the current stream; microseconds per call.

    upsample            avl_upsample_logits -> fp32 [19][1080][1920] (158 MB written)
    labels              avl_seg_eval_full_res, arg-max only
    labels+loss+cm      avl_seg_eval_full_res with labels, confusion matrix and loss (+ its one-workgroup finalize)
    torch route         GPU F.interpolate -> argmax -> cross_entropy(ignore_index=255) -> labels to the host -> np.bincount
                        (timed by wall clock around a synchronise: its last step runs on the CPU)

    python tools/bench_full_res.py [reps] [warmup]
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd import seg_head  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda", 0)
K, h, w, H, W = 19, 266, 476, 1080, 1920

g = torch.Generator().manual_seed(1)
logits = (4.0 * torch.randn((h, w, K), generator=g)).to(dev)
gt_cpu = torch.randint(0, K, (H, W), generator=g, dtype=torch.int64)
gt_cpu[torch.rand((H, W), generator=g) < 0.1] = 255
gt = gt_cpu.to(torch.uint8).to(dev)
gt64 = gt_cpu.to(dev)
up = torch.empty((K, H, W), dtype=torch.float32, device=dev)
lab = torch.empty((H, W), dtype=torch.uint8, device=dev)
cm = torch.zeros((K, K), dtype=torch.int64, device=dev)
ws = seg_head.EvalWorkspace(H, W, dev)


def gpu_time(fn):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def torch_route():
    preds = F.interpolate(logits.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=True)
    labels = torch.argmax(preds, dim=1)
    loss = F.cross_entropy(preds, gt64[None], ignore_index=255)
    p, l_ = labels.cpu().numpy()[0], gt_cpu.numpy()
    mask = l_ < K
    counts = np.bincount(K * l_[mask] + p[mask], minlength=K * K).reshape(K, K)
    return float(loss), counts


def wall_time(fn):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


res = {
    "upsample": gpu_time(lambda: seg_head.upsample_logits(logits, H, W, out=up)),
    "labels": gpu_time(lambda: seg_head.full_res_eval(logits, H, W, labels_out=lab)),
    "labels+loss+cm": gpu_time(lambda: seg_head.full_res_eval(logits, H, W, gt=gt, labels_out=lab, confusion=cm, workspace=ws)),
    "torch route": wall_time(torch_route),
}
# the fused result against the torch route, once (a timing tool that times wrong answers is no use)
cm.zero_()
seg_head.full_res_eval(logits, H, W, gt=gt, labels_out=lab, confusion=cm, workspace=ws)
loss_t, counts_t = torch_route()
r = ws.result()
agree = float((lab.long() == torch.argmax(F.interpolate(logits.permute(2, 0, 1)[None], size=(H, W), mode="bilinear",
                                                        align_corners=True), dim=1)[0]).float().mean())
for name, us in res.items():
    print("%-16s %9.1f us" % (name, us))
print("upsample write rate %.2f TB/s; loss fused %.9f torch %.9f; label agreement %.6f; confusion |d| sum %d"
      % (K * H * W * 4 / (res["upsample"] * 1e-6) / 1e12, r["loss"], loss_t, agree, int(np.abs(cm.cpu().numpy() - counts_t).sum())))
print(json.dumps({"shape": [K, h, w, H, W], "reps": reps, "warmup": warmup, "us_per_call": {k: round(v, 2) for k, v in res.items()},
                  "device": torch.cuda.get_device_name(0)}))
