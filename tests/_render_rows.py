"""Rows of a class map on which the render rule is easy to get wrong, shared by the renderer tests: cancellations whose sum is zero in
NumPy's summation order and not in a plain left fold (and the other way round), shares that equal their threshold after rounding to
the map's type, ties, NaN and infinite rows, all-zero rows; and the colours and thresholds that go with them."""
import numpy as np


def colors(c):
    return [[(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256] for i in range(c)]


def pad(row, c):
    row = list(row)[:c]
    return row + [0.0] * (c - len(row))


def constructed_rows(c, dtype):
    """rows whose zero test or share depends on the order and type of the channel sum (the ones named in the issue first)"""
    big = 1e8 if dtype == np.float32 else 1e16
    rows = [
        [1e8, 1, -1e8, 0, 0],                       # f32: NumPy's sum is 0, a float64 sum is 1
        [0, 1e16, 1, 0, -1e16, 0, -1, 0],           # f64, C = 8: NumPy's pairwise sum is 0, a left fold -1
        [1, 0, 1e8, 0, -1e8, 0, 0, -1],             # f32, C = 8: pairwise 0, a left fold not
        [big, 1, -big, -1, 0, 0, 0, 0, 1, -1],
        [1, big, 0, 0, 0, -big, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
        [big, 0, 0, 0, 0, 0, 0, 0, -big, 1, 0, 0, 0, 0, 0, 0],
        [1, 99],                                    # share of class 0: exactly float32(0.01) / 0.01
        [99, 1, 0, 0, 0, 0, 0, 0, 0],
        [1, 2], [2, 1, 0, 0, 0, 0, 0, 3],           # shares of exactly 1/3 and 1/2 in the map's type
        [3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3],   # ties everywhere: the first channel wins
        [-1, 5, 5, -9],
    ]
    return [pad(r, c) for r in rows]


def special_rows(c, rng):
    rows = [[0.0] * c, [-0.0] * c]
    for k in {0, c // 2, c - 1}:
        r = list(rng.normal(size=c))
        r[k] = np.nan
        rows.append(r)
        r = list(rng.normal(size=c))
        r[k] = np.inf
        rows.append(r)
        r = [0.0] * c
        r[k] = -np.inf
        rows.append(r)
    rows.append([np.nan] * c)
    rows.append([np.inf if i % 2 else -np.inf for i in range(c)])
    return rows


def cancellation_rows(c, dtype, rng, n=3000):
    """random rows of 0, +-1, +-2, +-big: many have sums that differ between summation orders"""
    big = 1e8 if dtype == np.float32 else 1e16
    vals = np.array([0.0, 0.0, 1.0, -1.0, 2.0, -2.0, big, -big, big / 2, -big / 2])
    return vals[rng.integers(0, vals.size, size=(n, c))].tolist()


def thresholds_for(c):
    base = [0.01, 1.0 / 3.0, 0.5, 0.01, 0.25, 0.1, 0.01, 0.75, 1.0 / 3.0, 0.01, 0.2, 0.5, 0.01, 0.3, 0.05, 0.01]
    return base[:c]
