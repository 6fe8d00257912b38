"""NumPy twin of avl_cost_map (include/avl_hip.h, the live cost map's rule).  TEST INFRASTRUCTURE ONLY (CPU).

The class of a cell is not restated here: it is read back from a picture of the whole grid that the existing renderers (or their
oracle) drew with distinct colours, through the crop of _live_map_reference.compose, which is black off the grid.  From there on
everything is stated in full: base cost, the ego footprint in float64 element by element (_live_map_reference.car_mask), the
distance by brute force over every offset of the (2R + 1)^2 square, the table and the max / unknown rule."""
import numpy as np

import _live_map_reference as lr

LETHAL, FAR = 100, 65535


def class_plane(rendered, palette, origin, size, radius):
    """-> int64 [h + 2R, w + 2R]: the class of every cell of the window and its ring of R cells, C = len(palette) for a cell with no
    class (black: empty, or off the grid).  `rendered` is the renderer's picture of the WHOLE grid in `palette`'s colours, which
    must be distinct and not black."""
    palette = np.asarray(palette, dtype=np.uint8)
    assert len({tuple(p) for p in palette.tolist()} | {(0, 0, 0)}) == len(palette) + 1
    r = int(radius)
    pic = lr.compose(rendered, (origin[0] - r, origin[1] - r), (size[0] + 2 * r, size[1] + 2 * r))
    cls = np.full(pic.shape[:2], len(palette), dtype=np.int64)
    for k, col in enumerate(palette):
        cls[(pic == col).all(axis=2)] = k
    assert ((cls < len(palette)) == (pic != 0).any(axis=2)).all(), "a colour of the picture is not in the palette"
    return cls


def base_plane(cls, origin, radius, class_cost, unknown_cost, car=None):
    """-> int64 plane of base costs; cost[C] = unknown_cost; 0 under the ego rectangle"""
    cost = np.array(list(class_cost) + [unknown_cost], dtype=np.int64)
    b = cost[cls]
    if car is not None:
        b = b.copy()
        b[lr.car_mask((origin[0] - radius, origin[1] - radius), cls.shape, car)] = 0
    return b


def distance2(lethal, radius):
    """lethal: bool plane of the window plus its ring of R cells -> int64 [h, w]: min dx^2 + dy^2 over the lethal cells of the
    (2R + 1)^2 square where that is <= R^2, else FAR.  Brute force: one shifted mask per offset and a running minimum."""
    r = int(radius)
    h, w = lethal.shape[0] - 2 * r, lethal.shape[1] - 2 * r
    d2 = np.full((h, w), FAR, dtype=np.int64)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            q = dx * dx + dy * dy
            if q > r * r:
                continue
            shifted = lethal[r + dx:r + dx + h, r + dy:r + dy + w]
            d2 = np.where(shifted & (q < d2), q, d2)
    return d2


def distance2_scalar(lethal, radius):
    """the same by a scalar triple loop, for the twin's own test"""
    r = int(radius)
    h, w = lethal.shape[0] - 2 * r, lethal.shape[1] - 2 * r
    d2 = np.full((h, w), FAR, dtype=np.int64)
    for i in range(h):
        for j in range(w):
            best = FAR
            for dx in range(-r, r + 1):
                for dy in range(-r, r + 1):
                    if lethal[r + i + dx, r + j + dy] and dx * dx + dy * dy <= r * r:
                        best = min(best, dx * dx + dy * dy)
            d2[i, j] = best
    return d2


def finish(base, radius, table):
    """base: int64 plane with its ring -> (cost int8 [h, w], d2 uint16 [h, w])"""
    r = int(radius)
    table = np.asarray(table, dtype=np.int64)
    assert table.shape == (r * r + 1,)
    d2 = distance2(base == LETHAL, r)
    b = base[r:base.shape[0] - r, r:base.shape[1] - r]
    v = np.where(d2 <= r * r, table[np.minimum(d2, r * r)], 0)
    out = np.where(b >= 0, np.maximum(b, v), np.where(v > 0, v, -1))
    return out.astype(np.int8), d2.astype(np.uint16)


def cost_map(rendered, palette, origin, size, class_cost, unknown_cost=-1, radius=0, table=(100,), car=None):
    """-> (cost int8 [h, w], d2 uint16 [h, w]) for the window, from the whole grid's picture"""
    cls = class_plane(rendered, palette, origin, size, radius)
    return finish(base_plane(cls, origin, radius, class_cost, unknown_cost, car), radius, table)
