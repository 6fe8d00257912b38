#!/usr/bin/env python3
"""The fp32 plan's pre-processing stem (k_stem_pre_f32, seg_stem_f32.hip) against the stand-alone pair it replaces: k_preprocess (the
RGB network input written to memory) followed by the plain fp32 k_stem (which reads it back).  At the camera's 1440 x 1920 with
camera1's distortion model, for each INTER_AREA factor (--factors):

* stem: the fused stem's row of SegNet.profile() on the raw-frame plan, against k_preprocess (device events around one call) plus the
  stem row of the plain plan of the same size; after warm-up, the median of --reps repetitions each;
* node: VisionSemanticSegmentationNode.image_callback frames/s with PRECISION f32 (camera frame in, colour image out, --frames frames
  after warm-up), next to the same chain through the stand-alone pre-processing kernel (what the node ran before).

Seeded weights (no trained checkpoint offline).  One JSON line at the end (--json also writes it to a file).

    python tools/bench_raw_frame_f32.py
    python tools/bench_raw_frame_f32.py --factors 2 --reps 50 --frames 100"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd import SemanticSegmentation, VisionSemanticSegmentationNode, get_cfg_defaults  # noqa: E402
from vision_semantic_segmentation_amd.config import get_network_cfg_defaults  # noqa: E402
from vision_semantic_segmentation_amd.network import random_state_dict  # noqa: E402
from vision_semantic_segmentation_amd.utils import Header, Message  # noqa: E402
from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import colorize_labels_device, preprocess_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1440x1920", help="HxW of the raw camera frame")
ap.add_argument("--factors", default="1,2", help="comma list of integer INTER_AREA factors (IMAGE_SCALE = 1 / factor)")
ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each stem measurement (>= 20)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--frames", type=int, default=40, help="timed image_callback frames per factor")
ap.add_argument("--json", default=None)
a = ap.parse_args()
assert a.reps >= 20, "--reps: at least 20 repetitions"

if not torch.cuda.is_available():
    sys.exit("bench_raw_frame_f32.py measures on the GPU; none is visible")
dev = torch.device("cuda", 0)
H, W = (int(v) for v in a.size.split("x"))
rng = np.random.default_rng(0)
coarse = rng.integers(0, 256, size=((H + 31) // 32, (W + 31) // 32, 3), dtype=np.uint8)
bgr = np.repeat(np.repeat(coarse, 32, axis=0), 32, axis=1)[:H, :W]
bgr = (bgr.astype(np.int32) + rng.integers(-8, 9, size=bgr.shape)).clip(0, 255).astype(np.uint8)
bgr_dev = torch.from_numpy(bgr).to(dev)

cfg = get_cfg_defaults()
net_cfg = get_network_cfg_defaults()
net_cfg.MODEL.PRECISION = "f32"
state = random_state_dict(0)
seg = SemanticSegmentation(net_cfg, device=dev, state_dict=state)
node_probe = VisionSemanticSegmentationNode(cfg, seg=seg)
cam1 = node_probe.cam1


def stem_ms(net):
    return [r["ms"] for r in net.profile() if r["kind"] == "stem"][0]


def median_of(fn):
    for _ in range(a.warmup):
        fn()
    return statistics.median(fn() for _ in range(a.reps))


def preprocess_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    preprocess_device(bgr_dev, cam1, f)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def frames_per_s(step):
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(a.frames):
        step()
    torch.cuda.synchronize(dev)
    return a.frames / (time.perf_counter() - t0)


results = []
for f in (int(v) for v in a.factors.split(",")):
    h, w = H // f, W // f
    raw = seg.net_for(h, w, raw_frame=(H, W))
    raw.set_camera(cam1.K, cam1.dist)
    raw.forward(bgr_dev)
    plain = seg.net_for(h, w)
    plain.forward(preprocess_device(bgr_dev, cam1, f))
    torch.cuda.synchronize(dev)
    fused = median_of(lambda: stem_ms(raw))
    pre = median_of(lambda: preprocess_ms(f))
    stem = median_of(lambda: stem_ms(plain))

    cfg.VISION_SEM_SEG.IMAGE_SCALE = 1.0 / f
    node = VisionSemanticSegmentationNode(cfg, seg=seg)
    msg = Message(Header(frame_id="camera1"), data=bgr)
    fps_node = frames_per_s(lambda: node.image_callback(msg))

    def detour():            # the former f32 route: stand-alone pre-processing, the plain plan, colour image to the host
        labels = seg.segmentation_device(preprocess_device(bgr, cam1, f))
        colorize_labels_device(labels, H, W, node.seg_color_ref).cpu()
    fps_detour = frames_per_s(detour)
    r = dict(factor=f, net_input=[h, w], k_preprocess_ms=round(pre, 4), k_stem_f32_ms=round(stem, 4), pair_ms=round(pre + stem, 4),
             fused_stem_ms=round(fused, 4), speedup=round((pre + stem) / fused, 3), node_fps=round(fps_node, 2),
             detour_fps=round(fps_detour, 2))
    results.append(r)
    print("%dx%d camera1, factor %d -> %dx%d: k_preprocess %.3f ms + k_stem f32 %.3f ms = %.3f ms  vs  k_stem_pre_f32 %.3f ms (x%.2f); "
          "image_callback f32 %.1f frames/s (stand-alone pre-processing route %.1f)"
          % (H, W, f, h, w, pre, stem, pre + stem, fused, r["speedup"], fps_node, fps_detour))
    seg._nets.clear()
    del raw, plain, node
    torch.cuda.empty_cache()

line = json.dumps(dict(tool="bench_raw_frame_f32", frame=[H, W], device=torch.cuda.get_device_name(dev), reps=a.reps, results=results))
print(line)
if a.json:
    with open(a.json, "w") as fh:
        fh.write(line + "\n")
