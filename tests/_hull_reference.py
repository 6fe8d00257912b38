"""CPU restatement of src/semantic_convex_hull.py:17-91 for the tests (shared by test_hull_cpu.py and test_gpu_hull.py).

cv2 and skimage are not available, so three library behaviours are ASSUMED here exactly as csrc/seg_hull.hip assumes them:
  * cv2.erode(img, ones((3, 3))) -- scipy.ndimage.binary_erosion(border_value=1): pixels outside the image do not erode;
  * skimage.measure.label(connectivity=2) -- scipy.ndimage.label(structure=ones((3, 3))): both number components in raster order of
    their first pixel; the labels are canonicalised to (smallest linear index of the component) + 1, which keeps that order;
  * cv2.convexHull -- a pure-Python monotone chain: strict vertices, starting at the smallest (x, then y), lower chain first, cross
    products on (x, y) as stored.
"""
from collections import Counter

import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=bool)


def erode(mask):
    return ndimage.binary_erosion(mask, structure=EIGHT, border_value=1)


def canonical_labels(mask):
    """int32 [h, w]: 0 background, else 1 + min linear index of the pixel's 8-connected component"""
    lab, n = ndimage.label(mask, structure=EIGHT)
    out = np.zeros(mask.shape, dtype=np.int32)
    if n:
        flat = lab.ravel()
        idx = np.flatnonzero(flat)
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat[idx], idx)
        out.ravel()[idx] = (first[flat[idx]] + 1).astype(np.int32)
    return out


def label_components(label_map, index, do_erode=True):
    mask = np.asarray(label_map) == index
    return canonical_labels(erode(mask) if do_erode else mask)


def monotone_chain(points):
    """points: iterable of (x, y) ints -> list of strict hull vertices, lower chain first from the smallest (x, y)"""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 1:
        return pts

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def class_hulls(label_map, index, top_number=1, area_threshold=30, drop_first=True, do_erode=True):
    """-> list of (label, area, vertices [n, 2] int32 (x, y)) for the components the reference would draw a hull for, in its order;
    a component without points after the drop is left out."""
    labels = label_components(label_map, index, do_erode)
    if not labels.any():
        return []
    count = Counter(labels[labels != 0].reshape(-1).tolist()).most_common(top_number)     # raster order: ties keep the smaller label first
    out = []
    for lab, area in count:
        if not area > area_threshold:
            continue
        ys, xs = np.where(labels == lab)                                                  # raster order
        pts = list(zip(xs.tolist(), ys.tolist()))
        if drop_first:
            pts = pts[1:]
        if not pts:
            continue
        out.append((int(lab), int(area), np.array(monotone_chain(pts), dtype=np.int32).reshape(-1, 2)))
    return out


def generate_convex_hull(label_map, index_care_about=1, top_number=1, area_threshold=30, drop_first=True):
    """the reference's return value: list of int32 [2, n + 1], each hull closed by its first vertex"""
    return [np.concatenate([v, v[:1]], axis=0).T.astype(np.int32)
            for _, _, v in class_hulls(label_map, index_care_about, top_number, area_threshold, drop_first)]


# ---------------------------------------------------------------------------------------------- inputs shared by the tests
def blob_map(rng, cells=(9, 12), cell=5, n_classes=3):
    """a random class grid, each cell enlarged to cell x cell pixels: blobs of every class, some touching every border"""
    grid = rng.integers(0, n_classes, size=cells, dtype=np.uint8)
    return np.kron(grid, np.ones((cell, cell), dtype=np.uint8))


def spiral(h, w, pitch=2, inset=0):
    """a 1-pixel-wide rectangular spiral walked inwards from (inset, inset) inside the box inset .. h-1-inset x inset .. w-1-inset,
    its turns `pitch` pixels apart: ONE 8-connected chain."""
    m = np.zeros((h, w), dtype=np.uint8)
    y, x, dy, dx = inset, inset, 0, 1
    if y >= h - inset or x >= w - inset:
        return m

    def blocked(y, x, dy, dx):
        for k in range(1, pitch + 1):
            yy, xx = y + k * dy, x + k * dx
            if not (inset <= yy < h - inset and inset <= xx < w - inset):
                return k == 1
            if m[yy, xx]:
                return True
        return False
    while True:
        m[y, x] = 1
        if blocked(y, x, dy, dx):
            dy, dx = dx, -dy                              # turn clockwise (y down): right -> down -> left -> up
            if blocked(y, x, dy, dx):
                return m
        y, x = y + dy, x + dx


def two_spirals(h, w):
    """a spiral of pitch 4 and, interleaved with it, the pixels exactly 2 away from it (the mid-line between its turns): the two never
    touch, not even diagonally"""
    a = spiral(h, w, 4).astype(bool)
    b = ndimage.binary_dilation(a, structure=np.ones((5, 5), dtype=bool)) & ~ndimage.binary_dilation(a, structure=EIGHT)
    return (a | b).astype(np.uint8)


def mask_patterns(h, w):
    """name -> uint8 [h, w] mask: the labelling cases of the GPU test"""
    yy, xx = np.mgrid[0:h, 0:w]
    single = np.zeros((h, w), dtype=np.uint8)
    single[h // 2, w // 2] = 1
    comb = ((xx % 2 == 0) | (yy == h - 1)).astype(np.uint8)
    out = {
        "zeros": np.zeros((h, w), dtype=np.uint8),
        "ones": np.ones((h, w), dtype=np.uint8),
        "single": single,
        "spiral": spiral(h, w, 2),
        "two_spirals": two_spirals(h, w),
        "checkerboard": ((yy + xx) % 2 == 0).astype(np.uint8),
        "anti_diagonal": (yy + xx == max(h, w) - 1).astype(np.uint8),
        "comb": comb,
    }
    for density in (0.40, 0.50, 0.60):
        for seed in range(3):
            rng = np.random.default_rng(1000 * seed + int(100 * density))
            out["bernoulli_%.2f_%d" % (density, seed)] = (rng.random((h, w)) < density).astype(np.uint8)
    return out
