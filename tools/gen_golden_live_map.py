#!/usr/bin/env python3
"""Generate tests/golden/fill_black.npz by running the REFERENCE's own fill_black and fill_edge on seeded colour images.

TEST INFRASTRUCTURE ONLY (CPU, no GPU), run where a checkout of the reference exists:

    python tools/gen_golden_live_map.py --reference <path to the reference checkout>

What is imported from the reference: src/renderer.py, which needs only numpy and scipy.

Two seeded 40 x 36 x 3 uint8 images.  Each holds blocks of the five palette colours of renderer.py:19-25 with black runs between
them, isolated single pixels of every label on black ground, black single pixels inside coloured blocks and a few pixels whose
colour is not in the palette (one with a palette R value and other G, B: fill_black matches on R only).  Recorded: img_a, img_b, the
reference's fill_black of each (38 x 34 x 3) and its fill_edge of a copy of img_a.  Data only -- no reference source text.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OUT = os.path.join(REPO, "tests", "golden", "fill_black.npz")
SEED, SHAPE = 20261019, (40, 36)


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_image(rng, palette):
    h, w = SHAPE
    img = np.zeros((h, w, 3), dtype=np.uint8)
    for _ in range(45):                                              # coloured blocks; later ones overlap earlier ones
        x, y = int(rng.integers(0, h - 3)), int(rng.integers(0, w - 3))
        img[x:x + int(rng.integers(2, 9)), y:y + int(rng.integers(2, 9))] = palette[int(rng.integers(0, len(palette)))]
    for _ in range(6):                                               # black runs
        x, y = int(rng.integers(0, h)), int(rng.integers(0, w - 6))
        img[x, y:y + int(rng.integers(3, 12))] = 0
        x, y = int(rng.integers(0, h - 6)), int(rng.integers(0, w))
        img[x:x + int(rng.integers(3, 12)), y] = 0
    img[30:40, 0:14] = 0                                             # black ground for the isolated pixels
    for i in range(len(palette)):
        img[32 + 3 * (i % 2), 2 + 2 * i] = palette[i]                # one isolated pixel of every label
    holes = np.argwhere(img[:, :, 0] != 0)
    for x, y in holes[rng.choice(len(holes), size=12, replace=False)]:
        img[x, y] = 0                                                # black single pixels inside blocks
    for k, col in enumerate([[1, 2, 3], [200, 10, 10], [128, 0, 0], [255, 0, 0], [17, 140, 200]]):
        img[int(rng.integers(0, 28)), int(rng.integers(0, w))] = col  # not in the palette; two carry a palette R value
    return img


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    ref = load_module("ref_renderer", os.path.join(args.reference, "src", "renderer.py"))
    palette = np.asarray(ref.label_colors, dtype=np.uint8)
    rng = np.random.default_rng(SEED)
    out = {"label_colors": palette}
    for name in ("a", "b"):
        img = make_image(rng, palette)
        out["img_" + name] = img
        out["fill_black_" + name] = np.asarray(ref.fill_black(img.copy()), dtype=np.uint8)
    out["fill_edge_a"] = np.asarray(ref.fill_edge(out["img_a"].copy()), dtype=np.uint8)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes, %d arrays)" % (args.out, os.path.getsize(args.out), len(out)))


if __name__ == "__main__":
    main()
