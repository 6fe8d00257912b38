#!/usr/bin/env python3
"""Time one ground-plane estimate (ground_plane.estimate_ground_plane_device) on a cloud that is already on the GPU.

device route: the whole avl_plane_ransac call -- prepare, fit, score, select, moments -- between two HIP events, cloud, triples and
              workspace resident (median of --iters calls after --warmup); a second figure adds the copy of the 24 result words
              to the host and the refit there (wall clock around .host());
host route:   the NumPy restatement of the same steps (tests/_plane_reference.py, the reference's Plane3D line by line) on the same
              machine's CPU, wall clock.
Default size: 120 000 points x 256 hypotheses, the reference's weight ("x norm", x0 = 0, norm 1), float32 [N, 4] points; 20 000 x 256
is the size at which the reference's own NumPy eval takes about 0.3 s.  The scene is the tests' synthetic ground (tilted plane,
35 % outliers).  The timed result is checked against the restatement (counts and winner).

    python tools/bench_ground_plane.py [--iters 50] [--warmup 10] [--out profiles/plane/bench_ground_plane.log]
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

SIZES = [(20000, 256), (120000, 256), (120000, 1024)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import _plane_reference as ref
    from vision_semantic_segmentation_amd.ground_plane import GroundPlaneWorkspace, estimate_ground_plane_device, sample_triples
    dev = torch.device("cuda", 0)
    lines = ["# %s, torch %s; device = one avl_plane_ransac call between HIP events, median of %d after %d warm-up calls; "
             "+host() = wall clock of the call, the 24-word copy and the refit; host = NumPy restatement, wall clock"
             % (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup)]
    for n, n_hyp in SIZES:
        cloud = ref.scene(np.random.default_rng(12), n)
        triples = sample_triples(n, n_hyp, 0)
        pts, tri = torch.from_numpy(cloud).to(dev), torch.from_numpy(triples).to(dev)
        ws = GroundPlaneWorkspace(n, n_hyp, dev)
        run = lambda: estimate_ground_plane_device(pts, triples=tri, workspace=ws)  # noqa: E731
        for _ in range(args.warmup):
            res = run().host()
        times, walls = [], []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = run()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = run().host()
            walls.append((time.perf_counter() - t0) * 1e3)
        dev_ms, wall_ms = float(np.median(times)), float(np.median(walls))
        host = []
        for _ in range(args.host_iters):
            t0 = time.perf_counter()
            want = ref.ransac(cloud[:, :3], triples)
            host.append((time.perf_counter() - t0) * 1e3)
        host_ms = float(np.median(host))
        margin = want.margin[np.isfinite(want.margin)].min()
        same = np.array_equal(res.counts.cpu().numpy(), want.counts)
        assert same or margin <= ref.MARGIN, (n, n_hyp, margin)                # the timed result is the right one
        assert (res.hypothesis, res.inliers) == (want.best, want.inliers) or not same
        lines.append("%6d points x %4d hypotheses  device %7.3f ms (min %.3f, max %.3f)  +host() %7.3f ms   host %9.1f ms   host / device %7.0f x"
                     "   winner %d with %d inliers of %d used, plane %s, counts equal: %s (smallest margin %.2g)"
                     % (n, n_hyp, dev_ms, min(times), max(times), wall_ms, host_ms, host_ms / dev_ms, res.hypothesis, res.inliers, res.used,
                        np.array2string(res.plane.param.ravel(), precision=5), same, margin))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
