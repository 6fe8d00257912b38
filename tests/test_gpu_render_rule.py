"""One render rule, many entry points: the hard rows of _render_rows.py -- cancellation sums on both sides of NumPy's 8-accumulator
order, NaN and infinite rows, ties, shares equal to their threshold -- give the picture of oracle/renderer_oracle.py, byte for byte,
through every entry point that calls the rule of csrc/avl_render.h: render_bev_map and render_bev_map_with_thresholds, render_window
and render_view without the filter, the site overview at one cell per pixel and the site finish with the filter off (the map cut into
tiles of T = 8 cells: a tile row is a multiple of 16 bytes at every C here).  The finish's labels are the oracle's convert_labels of
that picture.  The expectation is computed once per (C, dtype) and never comes from the library."""
import numpy as np
import pytest

import _site_overview_reference as ov
from _render_rows import cancellation_rows, constructed_rows, special_rows, thresholds_for
from _site_finish_reference import run_finish
from _site_overview_reference import run_kernel

pytestmark = pytest.mark.gpu

CLASS_COUNTS = [1, 5, 8, 9, 16]
DTYPES = [np.float32, np.float64]
WIDTH, T = 16, 8

_CASES = {}


def priority_for(c):
    """a priority that is not the identity (for c = 1 there is only one)"""
    return list(range(1, c)) + [0]


def case(c, dtype):
    """(map [H, 16, c], colours, thresholds, priority, expected arg-max picture, expected thresholds picture)"""
    key = (c, np.dtype(dtype).name)
    if key not in _CASES:
        from oracle import renderer_oracle as ro
        rng = np.random.default_rng(1000 + c)
        rows = constructed_rows(c, dtype) + special_rows(c, rng) + cancellation_rows(c, dtype, rng, n=200)
        h = -(-len(rows) // WIDTH)
        h += -h % T
        rows += [[0.0] * c] * (h * WIDTH - len(rows))
        m = np.array(rows, dtype=dtype).reshape(h, WIDTH, c)
        col = ov.COLORS[:c]                                   # for c = 5 the five map colours: the finish's labels are not all 0
        th, pr = thresholds_for(c), priority_for(c)
        with np.errstate(all="ignore"):
            want = ro.render_bev_map(m, col), ro.render_bev_map_with_thresholds(m, col, pr, th)
        assert c == 1 or (len(np.unique(want[0].reshape(-1, 3), axis=0)) >= 3 and (want[0] != want[1]).any())
        _CASES[key] = (m, col, th, pr) + want
    return _CASES[key]


def tile_table(sources, m):
    """the table of ``sources`` (scroll.overview_sources or finish_sources) for the map as one window of T x T tiles, all present"""
    nh, nw = m.shape[0] // T, m.shape[1] // T
    table = sources((0, nh - 1, 0, nw - 1), T, m.shape[2] * m.dtype.itemsize, m.shape[1], (0, 0), np.ones((nh, nw), dtype=bool),
                    np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64), 1)
    assert len(table) == nh * nw and nh >= 2 and nw == 2
    return table, [m.reshape(-1).view(np.uint8)], nh, nw


def _ids(v):
    return v.__name__ if isinstance(v, type) else str(v)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("c", CLASS_COUNTS)
def test_every_entry_point_draws_the_oracles_picture(c, dtype, cuda_device):
    from oracle import evaluation_oracle as eo
    from vision_semantic_segmentation_amd import renderer as rr, scroll
    m, col, th, pr, want_argmax, want_thresholds = case(c, dtype)
    grid = m.shape[:2]
    identity = [[1, 0, 0], [0, 1, 0]]
    src_table, bufs, nh, nw = tile_table(scroll.overview_sources, m)
    fin_table = tile_table(scroll.finish_sources, m)[0]
    for what, want, kw in (("arg-max", want_argmax, {}), ("thresholds", want_thresholds, dict(thresholds=th, priority=pr))):
        got = {
            "render_bev_map": rr.render_bev_map_with_thresholds(m, col, pr, th) if kw else rr.render_bev_map(m, col),
            "render_window": rr.render_window(m, col, origin=(0, 0), size=grid, filter=False, **kw),
            "render_view": rr.render_view(m, col, identity, size=grid, filter=False, **kw),
            "site overview": run_kernel(src_table, bufs, T, c, dtype, nh, nw, 1, cuda_device, **kw)[0],
        }
        got["site finish"], labels, _ = run_finish(fin_table, bufs, T, c, dtype, nh, nw, cuda_device, filter=False, **kw)
        for name, pic in got.items():
            assert pic.shape == want.shape and np.array_equal(pic, want), \
                "%s, %s: %d of %d cells differ" % (name, what, int((pic != want).any(axis=2).sum()), grid[0] * grid[1])
        want_labels = eo.convert_labels(want)
        assert np.array_equal(labels, want_labels.astype(np.uint8)), "%s: %d labels differ" % (what, int((labels != want_labels).sum()))
        assert c != 5 or len(np.unique(want_labels)) >= 4
