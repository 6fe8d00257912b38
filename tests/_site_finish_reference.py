"""NumPy twin of the site finish's rule (THE RULE above struct avl_tile_fin in include/avl_hip.h), shared by test_site_finish_cpu.py and
test_gpu_site_finish.py, built on _site_overview_reference.assemble_sources / TableCase.

* the filter: a reflect-101 pad of the assembled rectangle, the nine products by float(float32(1) / float32(9)) accumulated in double
  from +0 with dy outer and dx inner, rounded to the map's dtype -- and two deliberate mistakes (dx outer, every tile alone),
  which the CPU test shows to differ;
* the picture: the oracle's renderers (oracle/renderer_oracle.py) on the filtered rectangle;
* the labels: oracle.evaluation_oracle.convert_labels' table; the counts: a plain np.add.at histogram over the cells of the tiles that
  have a record, the truth looked up in a raster laid over the rectangle at (gt_r0, gt_c0).
"""
import numpy as np

from oracle import evaluation_oracle as eo

import _site_overview_reference as ov

NINTH = float(np.float32(1.0) / np.float32(9.0))


# ------------------------------------------------------------------------------------------------ the rule
def box_filter(a, dx_outer=False):
    """F of the rule.  ``dx_outer``: the same nine products summed with dx as the outer loop -- NOT the rule."""
    h, w = a.shape[:2]
    p = np.pad(np.asarray(a, dtype=np.float64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    acc = np.zeros(a.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        taps = [(dy, dx) for dx in range(3) for dy in range(3)] if dx_outer else [(dy, dx) for dy in range(3) for dx in range(3)]
        for dy, dx in taps:
            acc = acc + NINTH * p[dy:dy + h, dx:dx + w]
        return acc.astype(a.dtype)


def box_filter_per_tile(a, T):
    """every tile filtered alone, the reflection at the TILE's edge -- NOT the rule"""
    out = np.empty_like(a)
    for i in range(0, a.shape[0], T):
        for j in range(0, a.shape[1], T):
            out[i:i + T, j:j + T] = box_filter(a[i:i + T, j:j + T])
    return out


def labels_of(picture, mask=None):
    """uint8 [H, W]: convert_labels' table; 0 where ``mask`` (same shape, or None) is 0"""
    lab = np.zeros(picture.shape[:2], dtype=np.uint8)
    for colour, l in eo.COLOR_TO_LABEL:
        lab[np.all(picture == np.array(colour, dtype=np.uint8), axis=-1)] = l
    if mask is not None:
        lab[np.asarray(mask) == 0] = 0
    return lab


def lay_over(raster, shape, r0, c0, fill):
    """``raster``, whose element [0, 0] lies at cell (r0, c0) of a rectangle of ``shape``, as an array of that shape; ``fill`` outside"""
    out = np.full(shape, fill, dtype=np.uint8)
    H, W = shape
    a0, a1, b0, b1 = max(r0, 0), min(r0 + raster.shape[0], H), max(c0, 0), min(c0 + raster.shape[1], W)
    if a0 < a1 and b0 < b1:
        out[a0:a1, b0:b1] = raster[a0 - r0:a1 - r0, b0 - c0:b1 - c0]
    return out


def histogram(truth, labels, cells=None):
    """int64 [8, 8]: counts[g][l] over the cells where ``cells`` (bool, or None = everywhere) holds; truth above 7 counts as 7"""
    counts = np.zeros((8, 8), dtype=np.int64)
    g = np.minimum(truth, 7).astype(np.int64)
    sel = np.ones(truth.shape, dtype=bool) if cells is None else cells
    np.add.at(counts, (g[sel], labels[sel].astype(np.int64)), 1)
    return counts


def record_cells(rows, cols, T, nh, nw):
    """bool [nh * T, nw * T]: the cells of the tiles at (rows[k], cols[k])"""
    tiles = np.zeros((nh, nw), dtype=bool)
    tiles[np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)] = True
    return np.repeat(np.repeat(tiles, T, axis=0), T, axis=1)


def finish(a, colors, filter=True, thresholds=None, priority=None, gt=None, gt_r0=0, gt_c0=0, mask=None, cells=None):
    """-> (picture, labels, counts or None) of the assembled rectangle ``a`` [H, W, C]; ``cells``: where the counts run (the tiles
    with a record), None = everywhere"""
    F = box_filter(a) if filter else a
    picture = ov.picture_of(F, colors, thresholds, priority)
    m = None if mask is None else lay_over(mask, a.shape[:2], gt_r0, gt_c0, 1)
    labels = labels_of(picture, m)
    counts = None if gt is None else histogram(lay_over(gt, a.shape[:2], gt_r0, gt_c0, 0), labels, cells)
    return picture, labels, counts


# ------------------------------------------------------------------------------------------------ the case's table
def finish_table(case):
    """finish_sources on a TableCase: the same arguments its overview table was built from"""
    from vision_semantic_segmentation_amd import scroll as s
    return s.finish_sources(case.RECT, case.T, case.bpc, case.WT * case.T, case.ORIGIN_TILE, case.mask, [t for t, _ in case.STORED],
                            [slab for _, slab in case.STORED], case.CHUNK)


def truth_raster(rng, shape):
    """labels 0 .. 6, a few of 7 and of 200 (counted as 7)"""
    g = rng.integers(0, 7, size=shape).astype(np.uint8)
    g[rng.random(shape) < 0.05] = 7
    g[rng.random(shape) < 0.02] = 200
    return g


# ------------------------------------------------------------------------------------------------ the kernel through the C ABI
def run_finish(table, bufs, T, Cn, dtype, nh, nw, device, filter=True, thresholds=None, priority=None, gt=None, gt_r0=0, gt_c0=0, mask=None,
               picture=True, labels=True):
    """-> (picture, labels, counts), None for what was not asked for: ``table`` through validate_finish, encode_finish and
    avl_site_finish; asserts that the guard strips around picture and labels survive"""
    import ctypes as C
    import torch
    from vision_semantic_segmentation_amd import _lib, scroll as s
    dtype = np.dtype(dtype)
    dev_bufs = [torch.from_numpy(b).to(device) for b in bufs]
    extents = [(t.data_ptr(), int(t.numel())) for t in dev_bufs]
    s.validate_finish(table, extents, T, Cn * dtype.itemsize, nh, nw)
    rec = np.zeros(max(len(table), 1), dtype=s.FIN_DTYPE)
    s.encode_finish(table, extents, rec)
    tiles = torch.from_numpy(rec.view(np.uint8)).to(device)
    ncell = nh * T * nw * T
    pic = torch.full((ov.GUARD + 3 * ncell + ov.GUARD,), 0xAB, dtype=torch.uint8, device=device)
    lab = torch.full((ov.GUARD + ncell + ov.GUARD,), 0xAB, dtype=torch.uint8, device=device)
    cnt = torch.full((64,), -1, dtype=torch.int64, device=device)
    gt_t = torch.from_numpy(np.ascontiguousarray(gt)).to(device) if gt is not None else None
    mask_t = torch.from_numpy(np.ascontiguousarray(mask)).to(device) if mask is not None else None
    Hg, Wg = (gt if gt is not None else mask).shape if (gt is not None or mask is not None) else (0, 0)
    colors = np.ascontiguousarray(ov.COLORS[:Cn])
    col = (C.c_uint8 * colors.size)(*colors.ravel().tolist())
    th = (C.c_double * Cn)(*thresholds) if thresholds is not None else None
    pr = (C.c_int32 * Cn)(*priority) if priority is not None else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = _lib.lib().avl_site_finish(C.c_void_p(tiles.data_ptr()), len(table), nh, nw, T, Cn, _lib.AVL_F64 if dtype == np.float64 else _lib.AVL_F32,
                                    _lib.AVL_LIVE_FILTER if filter else 0, col, pr, th, p(gt_t), Hg, Wg, Wg, gt_r0, gt_c0, p(mask_t), Wg,
                                    C.c_void_p(pic.data_ptr() + ov.GUARD) if picture else None, C.c_void_p(lab.data_ptr() + ov.GUARD) if labels else None,
                                    p(cnt) if gt is not None else None, C.c_void_p(stream))
    _lib.check(rc, "avl_site_finish")
    torch.cuda.synchronize(device)
    pic, lab, cnt = pic.cpu().numpy(), lab.cpu().numpy(), cnt.cpu().numpy()
    for name, a, asked in (("picture", pic, picture), ("labels", lab, labels)):
        assert (a[:ov.GUARD] == 0xAB).all() and (a[-ov.GUARD:] == 0xAB).all(), "guard strip of %s written" % name
        assert asked or (a == 0xAB).all(), "%s written although not asked for" % name
    assert gt is not None or (cnt == -1).all()
    return (pic[ov.GUARD:-ov.GUARD].reshape(nh * T, nw * T, 3) if picture else None, lab[ov.GUARD:-ov.GUARD].reshape(nh * T, nw * T) if labels else None,
            cnt.reshape(8, 8) if gt is not None else None)
