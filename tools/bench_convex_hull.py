#!/usr/bin/env python3
"""Time the per-frame semantic extraction (two classes, the node's defaults) on label maps that are already on the GPU.

device route: class_hulls_device on the resident labels + ONE device-to-host copy of the packed vertices (HIP events around both);
host route:   the label map copied to the host + the scipy restatement of src/semantic_convex_hull.py (tests/_hull_reference.py) for
              the two classes (wall clock; it is the stand-in for the reference's cv2 / skimage / Counter chain, which is slower).
Sizes: 266 x 476 and 356 x 476 (the network's output for 1080p / 1440 x 1920 frames at output stride 8 .. 4) and 1080 x 1920
(upsample_pred=True).  Inputs: a blobby label map and a near-percolation random map: classes 1 and 2 at density 0.5 each on a grid of
3 x 3 pixel cells.  The erosion leaves every cell's centre and the bridge to a 4-neighbour cell of the same class, and cuts the diagonal
ones, so what is labelled is 4-connected site percolation at 0.5 (threshold 0.593): about a thousand ragged components at 266 x 476 and
sixteen times as many at 1080 x 1920, the largest across many tiles.
The yardstick is the reference's own limit: the extraction has to fit well inside one 0.1 s update period of the ground plane.

    python tools/bench_convex_hull.py [--iters 50] [--warmup 10] [--out profiles/hull/bench_convex_hull.log]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(266, 476), (356, 476), (1080, 1920)]
CLASSES = [2, 1]


def blobby(rng, h, w):
    grid = rng.integers(0, 3, size=(h // 24 + 1, w // 24 + 1), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(grid, np.ones((24, 24), dtype=np.uint8))[:h, :w])


def percolation(rng, h, w):
    grid = rng.integers(1, 3, size=(h // 3 + 1, w // 3 + 1), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(grid, np.ones((3, 3), dtype=np.uint8))[:h, :w])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import _hull_reference as ref
    from vision_semantic_segmentation_amd.semantic_convex_hull import class_hulls_device, hull_workspace_bytes
    dev = torch.device("cuda", 0)
    lines = ["# %s, torch %s; device route = class_hulls_device(2 classes) + one D2H of the vertices, median of %d after %d warm-up calls"
             % (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup)]
    for h, w in SIZES:
        for name, make in (("blobby", blobby), ("percolation", percolation)):
            lm = make(np.random.default_rng(7), h, w)
            t = torch.from_numpy(lm).to(dev)
            ws = torch.empty(hull_workspace_bytes(h, w, len(CLASSES), 1), dtype=torch.uint8, device=dev)
            for _ in range(args.warmup):
                res = class_hulls_device(t, CLASSES, workspace=ws).host()
            times = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = class_hulls_device(t, CLASSES, workspace=ws).host()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            dev_ms = float(np.median(times))
            host = []
            for _ in range(args.host_iters):
                t0 = time.perf_counter()
                lm_host = t.cpu().numpy()
                want = [ref.class_hulls(lm_host, c) for c in CLASSES]
                host.append((time.perf_counter() - t0) * 1e3)
            host_ms = float(np.median(host))
            for k, c in enumerate(CLASSES):                                  # the timed result is the right one
                got = [res.vertices[k, 0, :res.n_vertices[k, 0]]] if res.n_vertices[k, 0] else []
                assert len(got) == len(want[k]) and all(np.array_equal(g, wv[2]) for g, wv in zip(got, want[k])), (h, w, name, c)
            lines.append("%4d x %4d %-11s device %8.3f ms (min %.3f, max %.3f)   host %9.2f ms   host / device %7.1f x   areas %s, vertices %s"
                         % (h, w, name, dev_ms, min(times), max(times), host_ms, host_ms / dev_ms, res.areas[:, 0].tolist(), res.n_vertices[:, 0].tolist()))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
