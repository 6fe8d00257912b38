#!/usr/bin/env python3
"""Time the live cost map against the live map of the same window and against the route a user had before it existed.

cost route:  renderer.cost_window (avl_cost_map: k_cost_base + k_cost_inflate) + the copy of the int8 window into pinned host memory,
             at R = 0, 15 and 32 cells, in both orders, with and without the clearance (d2_out);
live route:  renderer.render_window of the same window with fill and car off + the copy of its picture: the same class evaluation,
             which is what the parent offers;
today:       that picture on the host -> colours matched back to classes -> class costs -> the NumPy twin's brute-force distance
             (tests/_cost_map_reference.py) -> table and max / unknown rule.  The window's ring is taken from a picture that is 2R
             larger, so the result is the cost route's, and the two are compared for equality before anything is timed.
Every GPU route ends in a stream synchronise and is timed by a host clock around a batch of calls; the routes alternate, batch by
batch, in one process.  `today` is timed once per radius: it takes seconds.

The two kernels alone are not visible to a host clock.  --kernels R only launches (the cost map at radius R in the yx order, then the
live map, --rounds times) and is meant to run under `rocprofv3 --kernel-trace --stats`, in a run of its own per radius;
k_cost_base, k_cost_inflate and k_live_map are the kernels' names in its table.

Grid 2000 x 2000 x 5 float64, a seeded fill of --density of the cells, window 600 x 600 in the middle.  Bytes the algorithm needs, from
the shapes, at R = 15: k_cost_base reads (630 + 2)^2 cells x 5 x 8 B = 16.0 MB and writes a 0.4 MB plane, k_cost_inflate reads it
and writes 0.36 MB (1.08 MB with d2); the live map reads (600 + 2)^2 x 40 B = 14.5 MB and writes 1.08 MB.  (h + 2R)(w + 2R) / hw is
1.10 at R = 15 and 1.22 at R = 32: what k_cost_base should cost over k_live_map.

    python tools/bench_cost_map.py [--rounds 30] [--out profiles/cost_map/bench_cost_map.log]
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

RADII = (0, 15, 32)
CLASS_COST = [0, 0, 0, 100, 100]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grid", type=int, nargs=3, default=[2000, 2000, 5])
    ap.add_argument("--window", type=int, nargs=2, default=[600, 600])
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--kernels", type=int, default=-1, metavar="R", help="launch only, at radius R (0, 15 or 32), for a kernel trace")
    ap.add_argument("--no-today", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import _cost_map_reference as cr
    from vision_semantic_segmentation_amd import renderer as rr
    from vision_semantic_segmentation_amd.labels import LABEL_COLORS
    assert torch.cuda.is_available(), "bench_cost_map needs a GPU"
    dev = torch.device("cuda", 0)
    hm, wm, c = args.grid
    h, w = args.window
    assert c == 5, "the class costs are the five map classes'"
    gen = torch.Generator(device=dev).manual_seed(7)
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    grid = torch.randn((hm, wm, c), generator=gen, device=dev, dtype=dt) * 4
    grid *= (torch.rand((hm, wm, 1), generator=gen, device=dev) < args.density).to(dt)
    origin = ((hm - h) // 2, (wm - w) // 2)
    stream = torch.cuda.current_stream(dev)
    tables = {r: rr.inflation_table(r, 0.1, 0.9, 3.0) for r in RADII}
    outs = {"xy": torch.empty((h, w), dtype=torch.int8, device=dev), "yx": torch.empty((w, h), dtype=torch.int8, device=dev)}
    d2s = {"xy": torch.empty((h, w), dtype=torch.uint16, device=dev), "yx": torch.empty((w, h), dtype=torch.uint16, device=dev)}
    hosts = {k: torch.empty(tuple(v.shape), dtype=torch.int8).pin_memory() for k, v in outs.items()}
    picture = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    picture_host = torch.empty((h, w, 3), dtype=torch.uint8).pin_memory()

    def cost(r, order="yx", d2=False, copy=True):
        rr.cost_window(grid, origin, (h, w), CLASS_COST, -1, r, tables[r], order=order, out=outs[order], d2_out=d2s[order] if d2 else None)
        if copy:
            hosts[order].copy_(outs[order], non_blocking=True)

    def live():
        rr.render_window(grid, LABEL_COLORS, origin, (h, w), out=picture)
        picture_host.copy_(picture, non_blocking=True)

    def today(r):
        """-> int8 [h, w]: what a user computed on the host, from a live map that is 2R larger"""
        big = rr.render_window(grid, LABEL_COLORS, (origin[0] - r, origin[1] - r), (h + 2 * r, w + 2 * r)).cpu().numpy()
        cls = np.full(big.shape[:2], c, dtype=np.int64)
        for k, col in enumerate(np.asarray(LABEL_COLORS, dtype=np.uint8)):
            cls[(big == col).all(axis=2)] = k
        return cr.finish(cr.base_plane(cls, origin, r, CLASS_COST, -1), r, tables[r])

    if args.kernels >= 0:
        for _ in range(args.rounds):
            cost(args.kernels, "yx", copy=False)
            rr.render_window(grid, LABEL_COLORS, origin, (h, w), out=picture)
        stream.synchronize()
        return

    lines = ["# %s, torch %s; grid %d x %d x %d %s, %.0f %% of the cells filled, window %d x %d at %s; class costs %s, unknown -1"
             % (torch.cuda.get_device_name(0), torch.__version__, hm, wm, c, args.dtype, 100 * args.density, h, w, origin, CLASS_COST),
             "# ms per call incl. the copy of the window into pinned memory and the synchronise; host clock around batches of %d; %d "
             "rounds, routes alternating" % (args.batch, args.rounds)]
    today_s = {}
    for r in RADII:                                            # equality first, and the host route's time
        if args.no_today:
            break
        t0 = time.perf_counter()
        want, want_d2 = today(r)
        today_s[r] = time.perf_counter() - t0
        cost(r, "xy", d2=True)
        stream.synchronize()
        assert np.array_equal(outs["xy"].cpu().numpy(), want) and np.array_equal(d2s["xy"].cpu().numpy(), want_d2), "R = %d differs" % r
        cost(r, "yx", d2=True)
        stream.synchronize()
        assert np.array_equal(outs["yx"].cpu().numpy(), want.T) and np.array_equal(d2s["yx"].cpu().numpy(), want_d2.T), "R = %d yx differs" % r
        lines.append("# R = %2d: equal to the host route; %4.1f %% of the window lethal, %4.1f %% inflated, %4.1f %% unknown"
                     % (r, 100 * float((want == 100).mean()), 100 * float(((want > 0) & (want < 100)).mean()), 100 * float((want == -1).mean())))
    routes = [("live map: filter + argmax, no fill, no car", live)]
    for r in RADII:
        routes += [("cost map R = %2d, yx" % r, lambda r=r: cost(r, "yx")), ("cost map R = %2d, xy" % r, lambda r=r: cost(r, "xy")),
                   ("cost map R = %2d, yx, with d2" % r, lambda r=r: cost(r, "yx", d2=True)),
                   ("cost map R = %2d, xy, with d2" % r, lambda r=r: cost(r, "xy", d2=True))]
    for _, fn in routes:                                       # warm up every shape the timed window uses
        for _ in range(3):
            fn()
    stream.synchronize()
    times = {name: [] for name, _ in routes}
    for _ in range(args.rounds):
        for name, fn in routes:                                # alternating, batch by batch
            t0 = time.perf_counter()
            for _ in range(args.batch):
                fn()
            stream.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.batch)
    for name, _ in routes:
        t = np.array(times[name])
        lines.append("%-46s median %8.3f ms   min %8.3f   max %8.3f" % (name, np.median(t), t.min(), t.max()))
    live_ms = float(np.median(times[routes[0][0]]))
    for r in RADII:
        ms = float(np.median(times["cost map R = %2d, yx" % r]))
        line = "R = %2d: cost map / live map %.2f x" % (r, ms / live_ms)
        if r in today_s:
            line += "; host route (live map of %d x %d -> host -> colour match -> NumPy inflation) %.2f s once, %.0f x the cost map" % (
                h + 2 * r, w + 2 * r, today_s[r], today_s[r] * 1e3 / ms)
        lines.append(line)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
