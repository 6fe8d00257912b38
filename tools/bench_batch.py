#!/usr/bin/env python3
"""Time per image of batched plans: SegNet(batch=N) for N = 1, 2, 4 at 480 x 640, 720 x 960 and 1080 x 1920, "mixed" and "split16".
Device events around --frames graph replays of each plan after warm-up; the time of one replay divided by N is the time per image.
Every image of a batch is a different seeded noise frame.  One line per plan, then a markdown table.

    python tools/bench_batch.py                                   # the full table
    python tools/bench_batch.py --sizes 480x640 --batches 1,4 --precisions mixed
    python tools/bench_batch.py --json out.json                   # also write the rows as JSON"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd.network import SegNet, random_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="480x640,720x960,1080x1920")
ap.add_argument("--batches", default="1,2,4")
ap.add_argument("--precisions", default="mixed,split16", help="comma list of mixed, split16, f16, bf16, f32")
ap.add_argument("--frames", type=int, default=30, help="graph replays timed per plan")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--json", default=None, help="write the rows to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_batch.py measures on the GPU; none is visible")
dev = torch.device("cuda", 0)
state = random_state_dict(0)
rows = []
for size in a.sizes.split(","):
    h, w = (int(v) for v in size.lower().split("x"))
    for prec in a.precisions.split(","):
        kw = dict(precision="mixed", full_split=True) if prec == "split16" else dict(precision=prec)
        for n in (int(v) for v in a.batches.split(",")):
            rng = np.random.default_rng(h + w + n)
            img = rng.integers(0, 256, size=((n,) if n > 1 else ()) + (h, w, 3), dtype=np.uint8)
            net = SegNet(state, h, w, device=dev, batch=n, **kw)
            net.forward(torch.from_numpy(img).to(dev))
            net.capture_graph()
            for _ in range(a.warmup):
                net.forward()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.frames):
                net.forward()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.frames
            r = dict(h=h, w=w, precision=prec, batch=n, ms_per_replay=ms, ms_per_image=ms / n, images_per_s=1e3 * n / ms)
            rows.append(r)
            print("%4dx%-4d %-8s N=%d  %8.3f ms/replay  %7.3f ms/image  %7.1f images/s" % (h, w, prec, n, ms, ms / n, r["images_per_s"]), flush=True)
            del net
            torch.cuda.empty_cache()

print("\n| size | precision | " + " | ".join("N = %s ms/image" % n for n in a.batches.split(",")) + " | best gain vs N = 1 |")
print("|---|---|" + "---|" * len(a.batches.split(",")) + "---|")
for size in a.sizes.split(","):
    h, w = (int(v) for v in size.lower().split("x"))
    for prec in a.precisions.split(","):
        sel = [r for r in rows if (r["h"], r["w"], r["precision"]) == (h, w, prec)]
        base = [r for r in sel if r["batch"] == 1]
        gain = ("%.2fx" % (base[0]["ms_per_image"] / min(r["ms_per_image"] for r in sel))) if base else "-"
        print("| %d x %d | %s | %s | %s |" % (h, w, prec, " | ".join("%.3f" % r["ms_per_image"] for r in sel), gain))
if a.json:
    with open(a.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(dev), rows=rows), f, indent=1)
