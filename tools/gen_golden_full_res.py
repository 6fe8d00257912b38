#!/usr/bin/env python3
"""Generate tests/golden/full_res_eval.npz by running the REFERENCE's own validation arithmetic on seeded logits.

TEST INFRASTRUCTURE ONLY (CPU, no GPU), run where a checkout of the reference exists:

    python tools/gen_golden_full_res.py --reference <path to the reference checkout>

What is imported from the reference:
  * src/network/deeplab_v3_plus/models/metrics.py -> MeanIOU (its np.bincount(x.astype(np.int)) needs `np.int`, which NumPy 2
    removed: shimmed here, in this script only);
  * src/network/deeplab_v3_plus/models/loss.py    -> CrossEntropyLoss, built with ignore_index=255 as models/build.py:20 does.
The upsampling is the reference's own call (deeplab_v3_plus.py:67-69): F.interpolate(feature, size=input_size, mode='bilinear',
align_corners=True).

Per frame: logits [19, 34, 60] (float32, seeded) upsampled to 152 x 256; a ground truth holding the 19 classes, blocks of 255 and a few
other values >= 19 (MeanIOU skips every value >= 19; torch's cross_entropy would raise on the non-255 ones, so the stored loss is the
reference loss with those pixels set to 255 -- what the fused kernel sums while it counts them as invalid).
Stored: the low-res logits, the ground truths, the expected labels (argmax of the upsampled logits), a near-tie mask (top-2 margin of
the upsampled logits <= 4e-6 * max|x|), the number of invalid labels, each frame's loss, the confusion matrix accumulated over both
frames and its mIoU.  Data only -- no reference source text.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OUT = os.path.join(REPO, "tests", "golden", "full_res_eval.npz")
K, h, w, H, W = 19, 34, 60, 152, 256
N_FRAMES, SEED = 2, 20261015


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_frame(rng):
    # smooth class scores plus noise, so that the upsampled arg-max forms regions as a network's does
    base = rng.normal(0.0, 1.0, size=(K, h // 4 + 2, w // 4 + 2)).astype(np.float32)
    smooth = F.interpolate(torch.from_numpy(base)[None], size=(h, w), mode="bilinear", align_corners=True)[0].numpy()
    logits = (3.0 * smooth + 0.5 * rng.normal(0.0, 1.0, size=(K, h, w))).astype(np.float32)
    return logits


def make_gt(rng, labels):
    # the prediction on about 70 % of the pixels, a random class elsewhere
    gt = np.where(rng.random((H, W)) < 0.7, labels, rng.integers(0, K, size=(H, W))).astype(np.uint8)
    for _ in range(6):                                   # ignored blocks
        y, x = int(rng.integers(0, H - 20)), int(rng.integers(0, W - 30))
        gt[y:y + int(rng.integers(4, 20)), x:x + int(rng.integers(4, 30))] = 255
    idx = rng.choice(H * W, size=40, replace=False)      # a few out-of-range values MeanIOU skips
    gt.reshape(-1)[idx] = rng.choice(np.array([19, 20, 64, 128, 254], dtype=np.uint8), size=40)
    return gt


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    net_dir = os.path.join(args.reference, "src", "network")
    sys.path.insert(0, net_dir)                          # metrics.py imports core.utils.metric
    if not hasattr(np, "int"):
        np.int = int                                     # NumPy 2 removed the alias metrics.py uses
    models = os.path.join(net_dir, "deeplab_v3_plus", "models")
    ref_metrics = load_module("ref_metrics", os.path.join(models, "metrics.py"))
    ref_loss = load_module("ref_loss", os.path.join(models, "loss.py"))

    rng = np.random.default_rng(SEED)
    metric = ref_metrics.MeanIOU(K)
    loss_fn = ref_loss.CrossEntropyLoss(ignore_index=255)
    out = {}
    for f in range(N_FRAMES):
        logits = make_frame(rng)
        preds = F.interpolate(torch.from_numpy(logits)[None], size=(H, W), mode="bilinear", align_corners=True)
        labels = torch.argmax(preds, dim=1)[0].numpy().astype(np.uint8)
        gt = make_gt(rng, labels)
        label = torch.from_numpy(gt.astype(np.int64))[None]
        invalid = (label >= K) & (label != 255)
        loss = float(loss_fn(preds, torch.where(invalid, torch.full_like(label, 255), label)))
        metric.evaluate(preds, label)
        top2 = torch.topk(preds[0], 2, dim=0).values
        near_tie = (top2[0] - top2[1]) <= 4e-6 * float(preds.abs().max())
        out["logits_%d" % f] = logits
        out["gt_%d" % f] = gt
        out["labels_%d" % f] = labels
        out["near_tie_%d" % f] = near_tie.numpy()
        out["invalid_%d" % f] = np.int64(int(invalid.sum()))
        out["loss_%d" % f] = np.float64(loss)
        print("frame %d: loss %.6f, %d invalid labels, %d near ties" % (f, loss, int(invalid.sum()), int(near_tie.sum())))
    out["confusion"] = metric.confusion_matrix.astype(np.int64)
    out["miou"] = np.float64(metric.global_avg)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes): mIoU %.6f" % (args.out, os.path.getsize(args.out), out["miou"]))


if __name__ == "__main__":
    main()
