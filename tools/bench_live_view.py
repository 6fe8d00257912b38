#!/usr/bin/env python3
"""Time the heading-up live view against the only way to get that picture on the device without it.

fused route:    renderer.render_view (one avl_live_view launch: filter + arg-max renderer [+ fill_black] sampled through the matrix) + the
                copy of the picture into pinned host memory;
two-pass route: renderer.render_window of the axis-aligned bounding square of the rotated picture, side ceil(size * sqrt 2) + 2 cells
                (an intermediate image is written), + a torch advanced-index gather with index tensors computed once, outside the
                timed region, + the same copy.
Both end in a stream synchronise and are timed by a host clock around a batch of calls; the routes alternate, batch by batch, in one
process, so that whatever else the machine does hits all of them.  Before anything is timed the two routes' pictures are compared
for equality (without the car: the window paints it on cell centres, the view on the pixel's own coordinates).  The axis-aligned
renderer.render_window of the same output size is timed alongside, for the ratio rotated / axis-aligned.

Grid 2000 x 2000 x 5 float64, a seeded fill of --density of the cells, picture 600 x 600 at one cell per pixel about the grid's
middle, headings 30 and 45 degrees, fill off and on.

    python tools/bench_live_view.py [--rounds 30] [--out profiles/live_view/bench_live_view.log]
"""
import argparse
import functools
import math
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
    ap.add_argument("--size", type=int, nargs=2, default=[600, 600])
    ap.add_argument("--cells-per-pixel", type=float, default=1.0)
    ap.add_argument("--headings", type=float, nargs="+", default=[30.0, 45.0])
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from vision_semantic_segmentation_amd import renderer as rr
    from vision_semantic_segmentation_amd.labels import LABEL_COLORS
    assert torch.cuda.is_available(), "bench_live_view needs a GPU"
    dev = torch.device("cuda", 0)
    hm, wm, c = args.grid
    h, w = args.size
    k = args.cells_per_pixel
    colors = [[(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256] for i in range(c)] if c != 5 else LABEL_COLORS
    gen = torch.Generator(device=dev).manual_seed(7)
    dt = torch.float64 if args.dtype == "f64" else torch.float32
    grid = torch.randn((hm, wm, c), generator=gen, device=dev, dtype=dt) * 4
    grid *= (torch.rand((hm, wm, 1), generator=gen, device=dev) < args.density).to(dt)
    centre = (hm / 2 + 0.3, wm / 2 + 0.6)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    host = torch.empty((h, w, 3), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream(dev)
    side = int(math.ceil(max(h, w) * k * math.sqrt(2.0))) + 2
    origin = (int(centre[0]) - side // 2, int(centre[1]) - side // 2)
    window = torch.empty((side, side, 3), dtype=torch.uint8, device=dev)

    def indices(m):
        a = (np.arange(h, dtype=np.float64) + 0.5)[:, None]
        b = (np.arange(w, dtype=np.float64) + 0.5)[None, :]
        gx = np.floor((m[0, 0] * a + m[0, 1] * b) + m[0, 2]).astype(np.int64) - origin[0]
        gy = np.floor((m[1, 0] * a + m[1, 1] * b) + m[1, 2]).astype(np.int64) - origin[1]
        assert gx.min() >= 0 and gx.max() < side and gy.min() >= 0 and gy.max() < side, "the bounding square is too small"
        return torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev)

    def fused(m, fill):
        rr.render_view(grid, colors, m, (h, w), fill=fill, out=out)
        host.copy_(out, non_blocking=True)

    def two_pass(ix, iy, fill):
        rr.render_window(grid, colors, origin, (side, side), fill=fill, out=window)
        host.copy_(window[ix, iy], non_blocking=True)

    def aligned(fill):
        rr.render_window(grid, colors, (int(centre[0]) - h // 2, int(centre[1]) - w // 2), (h, w), fill=fill, out=out)
        host.copy_(out, non_blocking=True)

    routes, painted = [], []
    for fill in (False, True):
        tag = "fill_black" if fill else "no fill"
        routes.append(("axis-aligned render_window, %s" % tag, functools.partial(aligned, fill)))
        for deg in args.headings:
            m = rr.view_matrix(centre, (math.cos(math.radians(deg)), math.sin(math.radians(deg))), k, (h, w))
            ix, iy = indices(m)
            routes.append(("fused render_view %g deg, %s" % (deg, tag), functools.partial(fused, m, fill)))
            routes.append(("render_window %d^2 + gather %g deg, %s" % (side, deg, tag), functools.partial(two_pass, ix, iy, fill)))
            routes[-2][1]()
            stream.synchronize()
            a = host.clone()
            routes[-1][1]()
            stream.synchronize()
            assert torch.equal(a, host), "the two routes give different pictures at %g degrees, %s" % (deg, tag)
            painted.append(float((a != 0).any(dim=2).float().mean()))
    for _, fn in routes:                                      # warm up every shape the timed region uses
        for _ in range(3):
            fn()
    stream.synchronize()
    times = {name: [] for name, _ in routes}
    for _ in range(args.rounds):
        for name, fn in routes:                               # alternating, batch by batch
            t0 = time.perf_counter()
            for _ in range(args.batch):
                fn()
            stream.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.batch)
    lines = ["# %s, torch %s; grid %d x %d x %d %s, %.0f %% of the cells filled, picture %d x %d at %g cells per pixel about %s "
             "(%.0f %% of its pixels coloured); the two routes' pictures are equal"
             % (torch.cuda.get_device_name(0), torch.__version__, hm, wm, c, args.dtype, 100 * args.density, h, w, k, centre,
                100 * min(painted)),
             "# ms per call incl. the copy of the picture into pinned memory and the synchronise; host clock around batches of %d; "
             "%d rounds, routes alternating; median of the batches" % (args.batch, args.rounds)]
    med = {}
    for name, _ in routes:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        lines.append("%-50s median %8.3f ms   min %8.3f   max %8.3f" % (name, med[name], t.min(), t.max()))
    for i in range(0, len(routes), 1 + 2 * len(args.headings)):
        base = med[routes[i][0]]
        for j in range(i + 1, i + 1 + 2 * len(args.headings), 2):
            lines.append("%-40s two-pass / fused %.2f x   fused / axis-aligned %.2f x"
                         % (routes[j][0], med[routes[j + 1][0]] / med[routes[j][0]], med[routes[j][0]] / base))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
