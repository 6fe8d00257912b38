#!/usr/bin/env python3
"""Time the live map's window against what the end-of-run functions offer for the same picture.

live route:  renderer.render_window (one avl_live_map launch: filter + arg-max renderer over the window) + the copy of the window into
             pinned host memory;
whole route: renderer.apply_filter over the whole grid (a second grid is allocated and written) + renderer.render_bev_map over the
             whole grid + the crop of the window + the same copy -- what a caller had before render_window existed.
Both end in a stream synchronise and are timed by a host clock around a batch of calls; the two routes alternate, batch by batch, in
one process, so that whatever else the machine does hits both.  The outputs are compared for equality before anything is timed.
The live route is also timed with the hole fill and with the thresholds renderer (no whole-grid counterpart is timed for those).

Grid 2000 x 2000 x 5 float64 (the reference's 200 m x 200 m at 0.1 m), a seeded fill of --density of the cells, window 600 x 600
(60 m x 60 m) in the middle.  Bytes the algorithm needs, from the shapes: the live route reads (600 + 2)^2 cells x 5 x 8 B = 14.5 MB
and writes 1.08 MB; the whole route reads 160 MB, writes 160 MB, reads 160 MB and writes 12 MB.

    python tools/bench_live_map.py [--rounds 30] [--out profiles/live_map/bench_live_map.log]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grid", type=int, nargs=3, default=[2000, 2000, 5])
    ap.add_argument("--window", type=int, nargs=2, default=[600, 600])
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--live-batch", type=int, default=20)
    ap.add_argument("--whole-batch", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from vision_semantic_segmentation_amd import renderer as rr
    from vision_semantic_segmentation_amd.labels import LABEL_COLORS
    assert torch.cuda.is_available(), "bench_live_map needs a GPU"
    dev = torch.device("cuda", 0)
    hm, wm, c = args.grid
    h, w = args.window
    colors = [[(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256] for i in range(c)] if c != 5 else LABEL_COLORS
    gen = torch.Generator(device=dev).manual_seed(7)
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    grid = torch.randn((hm, wm, c), generator=gen, device=dev, dtype=dt) * 4
    grid *= (torch.rand((hm, wm, 1), generator=gen, device=dev) < args.density).to(dt)
    origin = ((hm - h) // 2, (wm - w) // 2)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    host = torch.empty((h, w, 3), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream(dev)
    car = rr.car_block(hm / 2 + 0.3, wm / 2 + 0.6, np.cos(0.7), np.sin(0.7), 0.1)

    def live(**kw):
        rr.render_window(grid, colors, origin, (h, w), out=out, **kw)
        host.copy_(out, non_blocking=True)

    def whole():
        smooth = rr.apply_filter(grid).to(grid.dtype)
        crop = rr.render_bev_map(smooth, colors)[origin[0]:origin[0] + h, origin[1]:origin[1] + w].contiguous()
        host.copy_(crop, non_blocking=True)

    routes = [("live: filter + argmax", lambda: live(), args.live_batch),
              ("whole grid: apply_filter + render_bev_map + crop", whole, args.whole_batch),
              ("live: filter + argmax + car", lambda: live(car=car), args.live_batch),
              ("live: filter + argmax + fill_black", lambda: live(fill=True), args.live_batch),
              ("live: filter + thresholds", lambda: live(thresholds=[0.01] * c), args.live_batch),
              ("live: no filter, argmax", lambda: live(filter=False), args.live_batch)]
    live()
    stream.synchronize()
    a = host.clone()
    whole()
    stream.synchronize()
    assert torch.equal(a, host), "the two routes give different pictures"
    painted = float((a != 0).any(dim=2).float().mean())
    for _, fn, _ in routes:                                   # warm up every shape the timed window uses
        for _ in range(3):
            fn()
    stream.synchronize()
    times = {name: [] for name, _, _ in routes}
    for _ in range(args.rounds):
        for name, fn, batch in routes:                        # alternating, batch by batch
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            stream.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / batch)
    lines = ["# %s, torch %s; grid %d x %d x %d %s, %.0f %% of the cells filled, window %d x %d at %s (%.0f %% of its pixels coloured)"
             % (torch.cuda.get_device_name(0), torch.__version__, hm, wm, c, args.dtype, 100 * args.density, h, w, origin, 100 * painted),
             "# ms per call incl. the copy of the window into pinned memory and the synchronise; host clock around batches; %d rounds, "
             "routes alternating" % args.rounds]
    for name, _, batch in routes:
        t = np.array(times[name])
        lines.append("%-50s median %8.3f ms   min %8.3f   max %8.3f   (batches of %d)" % (name, np.median(t), t.min(), t.max(), batch))
    base = float(np.median(times[routes[1][0]]))
    lines.append("whole grid / live (filter + argmax): %.1f x" % (base / float(np.median(times[routes[0][0]]))))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
