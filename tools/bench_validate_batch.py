#!/usr/bin/env python3
"""Times the batched full-resolution head (csrc/seg_head.hip: avl_seg_eval_full_res_batch, avl_upsample_logits_batch) for N = 1, 2, 4, 8
against N calls of the single-image entry points, at the logits sizes of three inputs (K = 19, seeded logits and labels):

    1080 x 1920   logits 266 x 476      720 x 960   logits 176 x 236      480 x 640   logits 116 x 156

    eval       labels + confusion matrix + loss (+ the one-workgroup finalize): one batched call / N single-image calls
    upsample   fp32 [N][19][H][W]: one batched call / N single-image calls

Every variant is called through ctypes with ready-made arguments (so N single calls pay N host calls, as a Python loop over the images
does): `warmup` calls, then `reps` calls between two device events on the current stream.  The variants of one (size, N) are timed in
turn, `rounds` times over (every other round in reverse order), and the table gives the median of the rounds and their spread
((max - min) / median): compare two columns only beyond that spread.  --base PATH loads a second build of the library (e.g. the parent
commit's libavl_hip.so) and times ITS single-image entry points in the same rounds, alternating with this build's.

Then, unless --no-e2e: validate_step on a batch against N single calls, and the torch route through the drop-in module
(DeepLabV3Plus.forward -> CrossEntropyLoss -> MeanIOU.evaluate: N x K x H x W logits written out), by wall clock around calls that end
in a synchronise, on seeded weights and frames.

    python tools/bench_validate_batch.py [--reps 50] [--warmup 5] [--rounds 5] [--base PATH] [--batches 1,2,4,8] [--sizes 1080x1920,...] [--no-e2e]
"""
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
from vision_semantic_segmentation_amd import _lib, seg_head  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--base", default=None, help="another build of libavl_hip.so whose single-image entry points are timed alongside")
ap.add_argument("--batches", default="1,2,4,8")
ap.add_argument("--sizes", default="1080x1920,720x960,480x640", help="which input sizes the kernel part times")
ap.add_argument("--e2e-batch", type=int, default=4)
ap.add_argument("--e2e-sizes", default="480x640,720x960")
ap.add_argument("--e2e-reps", type=int, default=10)
ap.add_argument("--no-e2e", action="store_true")
ap.add_argument("--no-kernels", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda", 0)
K = 19
SIZES = [("1080x1920", (266, 476), (1080, 1920)), ("720x960", (176, 236), (720, 960)), ("480x640", (116, 156), (480, 640))]
SIZES = [s for s in SIZES if s[0] in args.sizes.split(",")]
BATCHES = [int(b) for b in args.batches.split(",")]
L = _lib.lib()
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
BASE = None
if args.base:
    BASE = C.CDLL(os.path.abspath(args.base))
    BASE.avl_upsample_logits.restype = _i
    BASE.avl_upsample_logits.argtypes = [_vp, _i, _i, _i, _i64, _vp, _i, _i, _vp]
    BASE.avl_seg_eval_full_res.restype = _i
    BASE.avl_seg_eval_full_res.argtypes = [_vp, _i, _i, _i, _i64, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]


def p(t):
    return C.c_void_p(t.data_ptr())


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


def wall_time(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def summarise(samples):
    med = statistics.median(samples)
    return {"median_us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2),
            "spread": round((max(samples) - min(samples)) / med, 4)}


def kernels():
    rows = []
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for name, (h, w), (H, W) in SIZES:
        for N in BATCHES:
            g = torch.Generator().manual_seed(1000 * N + h)
            logits = (4.0 * torch.randn((N, h, w, K), generator=g)).to(dev)
            gt_cpu = torch.randint(0, K, (N, H, W), generator=g, dtype=torch.int64)
            gt_cpu[torch.rand((N, H, W), generator=g) < 0.1] = 255
            gt = gt_cpu.to(torch.uint8).to(dev)
            up = torch.empty((N, K, H, W), dtype=torch.float32, device=dev)
            lab = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            cm = torch.zeros((K, K), dtype=torch.int64, device=dev)
            ws = seg_head.EvalWorkspace(H, W, dev, batch=N)
            ws1 = seg_head.EvalWorkspace(H, W, dev)

            def check(rc):
                if rc:
                    raise RuntimeError(_lib.last_error())

            def eval_batched():
                check(L.avl_seg_eval_full_res_batch(p(logits), N, h * w, h, w, K, K, H, W, p(gt), 255, p(lab), p(cm), p(ws.loss), p(ws.counts),
                                                    p(ws.image_loss), p(ws.image_counts), p(ws.scratch), stream))

            def up_batched():
                check(L.avl_upsample_logits_batch(p(logits), N, h * w, h, w, K, K, p(up), H, W, stream))

            ev_args = [(p(logits[i]), h, w, K, K, H, W, p(gt[i]), 255, p(lab[i]), p(cm), p(ws1.loss), p(ws1.counts), p(ws1.scratch), stream)
                       for i in range(N)]
            up_args = [(p(logits[i]), h, w, K, K, p(up[i]), H, W, stream) for i in range(N)]

            def singles(fn, arglist):
                def run():
                    for a in arglist:
                        if fn(*a):
                            raise RuntimeError("single-image call failed")
                return run

            variants = [("eval batched", eval_batched), ("eval N singles", singles(L.avl_seg_eval_full_res, ev_args)),
                        ("upsample batched", up_batched), ("upsample N singles", singles(L.avl_upsample_logits, up_args))]
            if BASE is not None:
                variants += [("eval N singles (base)", singles(BASE.avl_seg_eval_full_res, ev_args)),
                             ("upsample N singles (base)", singles(BASE.avl_upsample_logits, up_args))]
            samples = {v: [] for v, _ in variants}
            for r in range(args.rounds):
                for v, fn in (variants if r % 2 == 0 else variants[::-1]):          # (no variant always runs first or last)
                    samples[v].append(gpu_time(fn))
            # a timing tool that times wrong answers is no use: the batch against the single-image calls, once
            cm.zero_()
            eval_batched()
            res, cm_b, lab_b = ws.result(), cm.clone(), lab.clone()
            cm.zero_()
            sums = []
            for a in ev_args:
                L.avl_seg_eval_full_res(*a)
                sums.append(ws1.result()["loss_sum"])
            total = sums[0]
            for s in sums[1:]:
                total += s
            ok = bool(torch.equal(cm, cm_b)) and bool(torch.equal(lab, lab_b)) and res["loss_sum"] == total and res["image_loss_sum"] == sums
            row = {"size": name, "N": N, "same_results": ok}
            row.update({v: summarise(s) for v, s in samples.items()})
            rows.append(row)
            line = "%-9s N=%d" % (name, N)
            for v, _ in variants:
                line += " | %s %.1f us (%.1f / image, spread %.1f %%)" % (v, row[v]["median_us"], row[v]["median_us"] / N, 100 * row[v]["spread"])
            print(line + " | same results: %s" % ok, flush=True)
            del logits, gt, up, lab
    return rows


def end_to_end():
    from vision_semantic_segmentation_amd import build_model
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    cfg = get_network_cfg_defaults()
    cfg.MODEL.MIXED_SELF_CHECK = False
    cfg.MODEL.VALIDATE_BATCH = True
    net, loss_fn, _, _ = build_model(cfg)
    model = net.to(dev).eval()
    seg = model.segmentation()
    N = args.e2e_batch
    mean, std = np.array([0.485, 0.456, 0.406], dtype=np.float32), np.array([0.229, 0.224, 0.225], dtype=np.float32)
    rows = []
    for size in args.e2e_sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(h)
        frames = rng.integers(0, 256, size=(N, h, w, 3), dtype=np.uint8)
        label = rng.integers(0, K, size=(N, h, w)).astype(np.uint8)
        label[rng.random((N, h, w)) < 0.1] = 255
        frames_d, label_d = torch.from_numpy(frames).to(dev), torch.from_numpy(label).to(dev)
        x = torch.from_numpy(np.ascontiguousarray(((frames.astype(np.float32) / np.float32(255) - mean) / std).transpose(0, 3, 1, 2))).to(dev)
        metric = MeanIOU(K, device=dev)

        def batch_step():
            return seg.validate_step(frames_d, label_d, metric)

        def single_steps():
            return [seg.validate_step(frames_d[i], label_d[i], metric) for i in range(N)]

        def drop_in_step():
            return model.validate_step(x, label_d, metric)

        def torch_route():
            with torch.no_grad():
                preds = model(x)
                loss = float(loss_fn(preds, label_d))
            metric.evaluate(preds, label_d)
            return loss

        variants = [("validate_step batch", batch_step), ("validate_step N singles", single_steps),
                    ("DeepLabV3Plus.validate_step", drop_in_step), ("torch route", torch_route)]
        samples = {v: [] for v, _ in variants}
        for r in range(args.rounds):
            for v, fn in (variants if r % 2 == 0 else variants[::-1]):
                samples[v].append(wall_time(fn, args.e2e_reps))
        row = {"size": size, "N": N, "loss": {"batch": batch_step(), "drop_in": drop_in_step(), "torch": torch_route()}}
        row.update({v: summarise(s) for v, s in samples.items()})
        rows.append(row)
        print("%-9s N=%d" % (size, N) + "".join(" | %s %.0f us (%.0f / image, spread %.1f %%)" % (
            v, row[v]["median_us"], row[v]["median_us"] / N, 100 * row[v]["spread"]) for v, _ in variants) + " | losses %s" % row["loss"], flush=True)
    return rows


out = {"K": K, "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "base": args.base, "device": torch.cuda.get_device_name(0)}
if not args.no_kernels:
    out["kernels"] = kernels()
if not args.no_e2e:
    out["end_to_end"] = end_to_end()
print(json.dumps(out))
