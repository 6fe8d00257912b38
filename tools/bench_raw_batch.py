#!/usr/bin/env python3
"""Times one multi-camera trigger (V raw BGR frames, each with its own camera model) through the segmentation network, three ways on
one build of the library:

    (a) raw_batch     SemanticSegmentation.segmentation_device_raw_batch: the frames are copied into the batched raw-frame plan, whose
                      stem pre-processes each image with its own camera block (what image_callback_views runs now)
    (b) pair          what image_callback_views ran before, restated from public calls: preprocess_device per view -> torch.empty
                      [V, h, w, 3] -> copy_ per view -> segmentation_device (the plain batch = V plan, which copies the batch again)
    (c) sequential    V calls of segmentation_device_raw (the one-frame raw plan)

for V = 2 and 4 frames of 1440 x 1920 at IMAGE_SCALE 0.5 and 1.0 and of 480 x 640 at 1.0, "mixed" and "split16" plans (seeded weights,
camera1 / camera6 alternating, structured frames already on the device).  Every variant: `warmup` calls, then `reps` calls between two
device events; the variants of a row are timed in turn, `rounds` times over (every other round in reverse order).  A row also gives
the stem op's own time (SegNet.profile, best of 5) in the batched raw plan and in the plain batched plan, and checks that the three
routes give the same labels.  One JSON line per row, then a table.

    python tools/bench_raw_batch.py [--reps 20] [--warmup 3] [--rounds 3] [--views 2,4] [--kinds mixed,split16] [--sizes 1440x1920@0.5,...]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd import SemanticSegmentation  # noqa: E402
from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6  # noqa: E402
from vision_semantic_segmentation_amd.config import get_network_cfg_defaults  # noqa: E402
from vision_semantic_segmentation_amd.network import random_state_dict  # noqa: E402
from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--views", default="2,4")
ap.add_argument("--kinds", default="mixed,split16")
ap.add_argument("--sizes", default="1440x1920@0.5,1440x1920@1.0,480x640@1.0", help="HxW@IMAGE_SCALE, comma separated")
args = ap.parse_args()

dev = torch.device("cuda", 0)


def structured(rng, h, w, cell=32):
    coarse = rng.integers(0, 256, size=((h + cell - 1) // cell, (w + cell - 1) // cell, 3), dtype=np.uint8)
    bgr = np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:h, :w]
    return (bgr.astype(np.int32) + rng.integers(-8, 9, size=bgr.shape)).clip(0, 255).astype(np.uint8)


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
    return a.elapsed_time(b) / args.reps


def summarise(samples):
    return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4),
            "samples_ms": [round(s, 4) for s in samples]}


class Split16(SemanticSegmentation):
    """the complete hi + lo pipeline as the plan "mixed" means (the rung the self-check's ladder calls split16)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._rung = "split16"


def stem_ms(net):
    return min([r["ms"] for r in net.profile() if r["kind"] == "stem"][0] for _ in range(5))


def run(state, kind, H, W, scale, V):
    factor = int(round(1.0 / scale))
    h, w = H // factor, W // factor
    cfg = get_network_cfg_defaults()
    seg = (Split16 if kind == "split16" else SemanticSegmentation)(cfg, device=dev, state_dict=state)
    rng = np.random.default_rng(3)
    s = (W / 1920.0, H / 1440.0)
    cams = [(camera_setup_1 if v % 2 == 0 else camera_setup_6)().scaled(*s) for v in range(V)]
    frames = [torch.from_numpy(structured(rng, H, W)).to(dev) for _ in range(V)]
    Ks, dists = [c.K for c in cams], [c.dist for c in cams]

    def raw_batch():
        return seg.segmentation_device_raw_batch(frames, Ks, dists, factor)

    def pair():
        batch = None
        for v in range(V):
            rgb = preprocess_device(frames[v], cams[v], factor)
            if batch is None:
                batch = torch.empty((V,) + tuple(rgb.shape), dtype=torch.uint8, device=rgb.device)
            batch[v].copy_(rgb)
        return seg.segmentation_device(batch)

    def sequential():
        return [seg.segmentation_device_raw(frames[v], Ks[v], dists[v], factor) for v in range(V)]

    la = raw_batch().clone()
    lb = pair().clone()
    lc = torch.stack([x.clone() for x in [seg.segmentation_device_raw(frames[v], Ks[v], dists[v], factor).clone() for v in range(V)]])
    assert torch.equal(la, lb) and torch.equal(la, lc), "the three routes disagree"
    variants = [("raw_batch", raw_batch), ("pair", pair), ("sequential", sequential)]
    samples = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            samples[name].append(gpu_time(fn))
    row = {"kind": kind, "raw": [H, W], "image_scale": scale, "net_input": [h, w], "n_views": V, "reps": args.reps, "rounds": args.rounds}
    for name in samples:
        row[name] = summarise(samples[name])
    row["stem_ms_raw_batch_plan"] = round(stem_ms(seg.net_for(h, w, raw_frame=(H, W), batch=V, raw_batch=True)), 4)
    row["stem_ms_plain_batch_plan"] = round(stem_ms(seg.net_for(h, w, batch=V)), 4)
    row["ratio_raw_batch_over_pair"] = round(row["raw_batch"]["median_ms"] / row["pair"]["median_ms"], 4)
    row["pair_spread"] = round((row["pair"]["max_ms"] - row["pair"]["min_ms"]) / row["pair"]["median_ms"], 4)
    print(json.dumps(row), flush=True)
    seg._nets.clear()
    del seg
    torch.cuda.empty_cache()
    return row


def main():
    state = random_state_dict(0)
    rows = []
    for size in args.sizes.split(","):
        hw, scale = size.split("@")
        H, W = [int(x) for x in hw.split("x")]
        for kind in args.kinds.split(","):
            for V in [int(v) for v in args.views.split(",")]:
                rows.append(run(state, kind, H, W, float(scale), V))
    print("\nkind    raw        scale V | (a) raw_batch ms (min..max) | (b) pair ms (min..max) | (c) sequential ms | a/b    | (b) spread | stem: raw batch / plain batch ms")
    for r in rows:
        a, b, c = r["raw_batch"], r["pair"], r["sequential"]
        print("%-7s %4dx%-4d  %.1f  %d | %8.3f (%7.3f..%7.3f) | %8.3f (%7.3f..%7.3f) | %8.3f | %.4f | %.4f | %.3f / %.3f"
              % (r["kind"], r["raw"][0], r["raw"][1], r["image_scale"], r["n_views"], a["median_ms"], a["min_ms"], a["max_ms"],
                 b["median_ms"], b["min_ms"], b["max_ms"], c["median_ms"], r["ratio_raw_batch_over_pair"], r["pair_spread"],
                 r["stem_ms_raw_batch_plan"], r["stem_ms_plain_batch_plan"]))


if __name__ == "__main__":
    main()
