"""The site overview (SemanticMapping.site_overview, avl_site_overview) without a GPU: what makes the GPU tests mean something.

* the fold's order matters: on the f32 log-confusion-matrix site of the drive and on a random payload, the column-outer fold and
  NumPy's pairwise sum of each pixel's cells differ from the rule in bits.  (reshape(...).sum(axis=(1, 3)) does NOT: NumPy reduces
  the two strided axes in the rule's own order, so that expression is a second statement of the rule, and is asserted equal.)
* averaging matters: pixels whose colour is neither their block's first cell's nor its centre cell's;
* the twin at k = 1 is the oracle's renderer on the site array;
* scroll.validate_sources' refusals, scroll.overview_sources on a hand-made window and directory, the choice of k;
* avl_site_overview's argument errors through the real library."""
import ctypes as C

import numpy as np
import pytest

import _scroll_reference as ref
import _site_overview_reference as ov
from oracle import renderer_oracle as ro


def scroll():
    from vision_semantic_segmentation_amd import scroll as s
    return s


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


_SITE = {}


def drive_site():
    """the f32 log-confusion-matrix site of the main drive at full resolution"""
    if "a" not in _SITE:
        from vision_semantic_segmentation_amd import synthetic as syn
        d = ref.main_drive()
        site = d.numpy_site(syn.log_confusion(5), np.float32)
        _SITE["a"] = site.region(site.nonempty_tiles())[1]
        _SITE["T"] = d.T
    return _SITE["a"], _SITE["T"]


def test_config_defaults():
    from vision_semantic_segmentation_amd import get_cfg_defaults
    oc = get_cfg_defaults().MAPPING.SITE_OVERVIEW
    assert (oc.ENABLED, oc.CELLS_PER_PIXEL, oc.MAX_SIDE_PX, list(oc.THRESHOLDS)) == (False, 0, 4096, [])


# ------------------------------------------------------------------------------------------------ the rule is not vacuous
@pytest.mark.parametrize("what", ["drive", "random"])
def test_fold_order_matters(what):
    if what == "drive":
        a, T = drive_site()
        assert T % 4 == 0 and a.dtype == np.float32
    else:
        a = ov.payload(np.random.default_rng(11), (64, 48, 5), np.float32)
    k = 4
    R = ov.reduce_grid(a, k)
    assert R.dtype == np.float32 and R.shape == (a.shape[0] // k, a.shape[1] // k, 5)
    other = ov.reduce_grid_column_outer(a, k)
    block = ov.reduce_grid_numpy_block(a, k)
    assert int((bits(R) != bits(other)).sum()) > 0, "the column-outer fold gives the same bits: the order would not be tested"
    assert int((bits(R) != bits(block)).sum()) > 0, "NumPy's pairwise sum gives the same bits: the order would not be tested"
    assert np.allclose(R, other, rtol=1e-4, atol=1e-5) and np.allclose(R, block, rtol=1e-4, atol=1e-5)     # the same sum all the same
    assert np.array_equal(bits(R), bits(ov.reduce_grid_numpy_axes(a, k)))                   # NumPy's strided reduction is the rule's order


def test_averaging_matters():
    a, _ = drive_site()
    k = 4
    colors = ov.COLORS[:5]
    R, pic = ov.overview(a, k, colors)
    first = ro.render_bev_map(a[0::k, 0::k], colors)
    centre = ro.render_bev_map(a[k // 2::k, k // 2::k], colors)
    neither = (pic != first).any(axis=2) & (pic != centre).any(axis=2)
    assert int(neither.sum()) > 0, "a kernel that sub-samples a block instead of summing it would pass"
    assert len(np.unique(pic.reshape(-1, 3), axis=0)) >= 3 and (pic == 0).all(axis=2).any()


def test_twin_at_k_1_is_the_oracle_renderer():
    a, _ = drive_site()
    a = a.copy()
    a[3, 5] = -0.0
    R, pic = ov.overview(a, 1, ov.COLORS[:5])
    assert np.array_equal(R, a) and not np.signbit(R[3, 5]).any()                            # +0 + -0.0 = +0
    assert np.array_equal(pic, ro.render_bev_map(a, ov.COLORS[:5]))
    th, pr = [0.3, 0.01, 0.2, 0.05, 0.6], [3, 0, 4, 2, 1]
    with np.errstate(all="ignore"):
        want = ro.render_bev_map_with_thresholds(a, ov.COLORS[:5], np.array(pr), th)
    assert np.array_equal(ov.overview(a, 1, ov.COLORS[:5], th, pr)[1], want)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) >= 3


# ------------------------------------------------------------------------------------------------ the table
def test_overview_sources_on_a_hand_made_directory():
    s = scroll()
    T, bpc, Wm, chunk = 8, 40, 32, 4
    origin_tile = (2, -1)
    mask = np.array([[1, 0, 1, 1], [0, 0, 1, 0], [1, 1, 0, 0]], dtype=bool)                 # a window of 3 x 4 tiles
    stored = {(-3, 5): 9, (1, -1): 0, (7, 7): 2, (5, 0): 6}                                  # (5, 0) and (7, 7) lie outside the rectangle below
    rect = (-3, 3, -2, 5)                                                                    # the window's last tile row lies outside too
    table = s.overview_sources(rect, T, bpc, Wm, origin_tile, mask, list(stored), list(stored.values()), chunk)
    want = {}
    for i in range(3):
        for j in range(4):
            if mask[i, j] and rect[0] <= 2 + i <= rect[1] and rect[2] <= -1 + j <= rect[3]:
                off, pitch = s.window_ref((2 + i, -1 + j), origin_tile, T, Wm, bpc)
                want[(2 + i - rect[0], -1 + j - rect[2])] = (0, off, pitch)
    for t, slab in stored.items():
        if rect[0] <= t[0] <= rect[1] and rect[2] <= t[1] <= rect[3]:
            (_, c), off, pitch = s.slab_ref(slab, chunk, T, bpc)
            want[(t[0] - rect[0], t[1] - rect[2])] = (1 + c, off, pitch)
    got = {(int(r["row"]), int(r["col"])): (int(r["buf"]), int(r["off"]), int(r["pitch"])) for r in table}
    assert len(table) == len(got) == 6 and got == want
    assert {v[2] for v in got.values()} == {Wm * bpc, T * bpc}                                # the window's pitch and the slab's
    assert [(int(r["row"]), int(r["col"])) for r in table] == sorted(got)
    # the window holds nothing (after load_site): only the store
    table = s.overview_sources(rect, T, bpc, Wm, origin_tile, None, list(stored), list(stored.values()), chunk)
    assert sorted((int(r["row"]), int(r["col"])) for r in table) == [(0, 7), (4, 1)]
    # nothing anywhere
    assert len(s.overview_sources((0, -1, 0, -1), T, bpc, Wm, origin_tile, None, [], [], chunk)) == 0
    # it passes the validator with buffers of the right size, and encodes to device addresses
    buffers = [(4096, 3 * T * Wm * bpc)] + [(1 << 20 | k << 16, chunk * T * T * bpc) for k in range(3)]
    table = s.overview_sources(rect, T, bpc, Wm, origin_tile, mask, list(stored), list(stored.values()), chunk)
    s.validate_sources(table, buffers, T, bpc, 7, 8)
    rec = np.zeros(len(table), dtype=s.SRC_DTYPE)
    assert s.encode_sources(table, buffers, rec) == 6 and s.SRC_DTYPE.itemsize == 24
    assert all(int(rec["src"][n]) == buffers[int(r["buf"])][0] + int(r["off"]) and int(rec["src_pitch"][n]) == int(r["pitch"])
               for n, r in enumerate(table))


def test_table_case_assembles_to_its_rectangle():
    for dtype in (np.float32, np.float64):
        case = ov.TableCase(8, 5, dtype)
        assert len(case.table) == 10 and {int(p) for p in case.table["pitch"]} == {case.WT * 8 * case.bpc, 8 * case.bpc}
        got = ov.assemble_sources(case.table, case.bufs, 8, 5, dtype, 3, 4)
        assert np.array_equal(bits(got), bits(case.full)) and np.signbit(got).any()
        for r, c in case.absent:
            assert not got[r * 8:(r + 1) * 8, c * 8:(c + 1) * 8].any()


def good_table():
    s = scroll()
    T, bpc = 8, 40
    table = np.zeros(3, dtype=s.SOURCE_DTYPE)
    table["buf"] = [0, 1, 1]
    table["row"], table["col"] = [0, 1, 2], [0, 3, 1]
    table["off"] = [(T * 4 * T + 3 * T) * bpc, 0, T * T * bpc]                               # the window's and the pool's last tiles
    table["pitch"] = [4 * T * bpc, T * bpc, T * bpc]
    buffers = [(1 << 20, 2 * T * 4 * T * bpc), (1 << 24, 2 * T * T * bpc)]
    return s, table, buffers, T, bpc


def test_validate_sources_refuses():
    s, table, buffers, T, bpc = good_table()
    s.validate_sources(table, buffers, T, bpc, 3, 4)
    s.validate_sources(table[:0], buffers, T, bpc, 3, 4)

    def refused(match, nh=3, nw=4, bufs=None, **change):
        t = table.copy()
        for name, (k, v) in change.items():
            t[name][k] = v
        with pytest.raises(ValueError, match=match):
            s.validate_sources(t, buffers if bufs is None else bufs, T, bpc, nh, nw)
    refused("leaves its buffer", bufs=[buffers[0], (buffers[1][0], buffers[1][1] - 1)])       # the last tile ends one byte past the buffer
    refused("leaves its buffer", bufs=[(buffers[0][0], buffers[0][1] - 1), buffers[1]])       # the window tile too
    refused("leaves its buffer", off=(1, -16))
    refused("pitch", pitch=(0, 4 * T * bpc + 8))                                               # misaligned
    refused("pitch", pitch=(1, T * bpc - 16))                                                  # shorter than a row
    refused("16-byte aligned", off=(2, T * T * bpc - 8))
    refused("16-byte aligned", bufs=[(buffers[0][0] + 4, buffers[0][1]), buffers[1]])
    refused("an earlier record names", row=(2, 1), col=(2, 3))                                 # a duplicate (row, col)
    refused("outside the rectangle", row=(0, 3))
    refused("outside the rectangle", col=(1, -1))
    refused("outside the rectangle", nh=2)
    refused("names a buffer", buf=(1, 2))
    with pytest.raises(ValueError, match="bytes_per_cell"):
        s.validate_sources(table, buffers, 6, 12, 3, 4)


def test_cells_per_pixel_choice():
    s = scroll()
    assert s.overview_cells_per_pixel(100, 60, 60, 4096) == 2                                  # 6000 cells: 3000 pixels
    assert s.overview_cells_per_pixel(100, 3, 60, 4096) == 2
    assert s.overview_cells_per_pixel(100, 20, 30, 4096) == 1
    assert s.overview_cells_per_pixel(100, 400, 400, 4096) == 10
    assert s.overview_cells_per_pixel(8, 3, 3, 4) == 8 and s.overview_cells_per_pixel(8, 5, 5, 4) == 8     # one pixel per tile at the most
    assert s.overview_cells_per_pixel(12, 4, 2, 16) == 3


# ------------------------------------------------------------------------------------------------ the ABI
def test_site_overview_argument_errors_do_not_need_a_gpu():
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.AvlTileSrc) == 24 == scroll().SRC_DTYPE.itemsize
    tiles = (_lib.AvlTileSrc * 12)()
    out = (C.c_uint8 * 4096)()
    colors = (C.c_uint8 * 48)()
    bad_priority = (C.c_int32 * 5)(0, 1, 5, 3, 4)
    th = (C.c_double * 5)()
    p, o, col = C.cast(tiles, C.c_void_p), C.cast(out, C.c_void_p), C.cast(colors, C.c_void_p)
    o16 = C.c_void_p(o.value + (-o.value) % 16)

    def args(n_tiles=2, nh=3, nw=4, T=8, Cn=5, dt=_lib.AVL_F64, k=2, colors=col, priority=None, thresholds=None, picture=o, reduced=o16,
             tiles_dev=p):
        return (tiles_dev, n_tiles, nh, nw, T, Cn, dt, k, colors, priority, thresholds, picture, reduced, None)
    for a, word in [(args(k=0), "does not divide"), (args(k=-2), "does not divide"), (args(k=3), "does not divide"), (args(k=16), "does not divide"),
                    (args(Cn=0), "C = 0"), (args(Cn=17), "C = 17"),
                    (args(dt=_lib.AVL_BF16), "map dtype"), (args(dt=7), "map dtype"),
                    (args(T=0, k=1), "tile_cells"), (args(T=1 << 15, k=1), "tile_cells"),
                    (args(T=6, k=1, Cn=1, dt=_lib.AVL_F32), "multiple of 16"),
                    (args(nh=0), "rectangle"), (args(nw=-1), "rectangle"),
                    (args(n_tiles=-1), "n_tiles"), (args(n_tiles=13), "n_tiles"),
                    (args(nh=1 << 14, nw=1 << 14, T=8, k=1), "below 2^31"), (args(nh=1 << 30, nw=1, T=8, k=1), "below 2^31"),
                    (args(picture=None), "is NULL"), (args(colors=None), "is NULL"), (args(tiles_dev=None), "tiles_dev is NULL"),
                    (args(tiles_dev=C.c_void_p(p.value + 4)), "misaligned"), (args(reduced=C.c_void_p(o16.value + 4)), "misaligned"),
                    (args(dt=_lib.AVL_F32, reduced=C.c_void_p(o16.value + 2)), "misaligned"),
                    (args(priority=bad_priority, thresholds=th), "priority[2] = 5")]:
        assert L.avl_site_overview(*a) == -1, word
        assert word in _lib.last_error(), (word, _lib.last_error())
