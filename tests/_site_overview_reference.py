"""NumPy twin of the site overview's rule (struct avl_tile_src in include/avl_hip.h), shared by test_site_overview_cpu.py and
test_gpu_site_overview.py.

* the reduction: acc = zeros; for di: for dj: acc = acc + a[di::k, dj::k], in the map's dtype -- and two other orders of the same sum,
  which the CPU test shows to differ;
* the picture: the oracle's renderers (oracle/renderer_oracle.py) applied to the reduced grid;
* an executor that applies a source table (scroll.SOURCE_DTYPE) to NumPy byte buffers: the rectangle at full resolution, absent tiles
  zero, then the two steps above;
* TableCase: a rectangle of tiles spread over a window buffer and the chunks of a pool, with absent tiles, for the kernel's tests.
"""
import numpy as np

from oracle import renderer_oracle as ro

COLORS = np.array([[128, 64, 128], [140, 140, 200], [255, 255, 255], [107, 142, 35], [244, 35, 232], [70, 70, 70], [190, 153, 153],
                   [220, 220, 0], [250, 170, 30], [0, 0, 142], [220, 20, 60], [152, 251, 152], [70, 130, 180], [119, 11, 32],
                   [0, 80, 100], [81, 0, 81]], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the rule
def reduce_grid(a, k):
    """R of the rule: di outer, dj inner, a left fold from +0 in a's dtype"""
    acc = np.zeros((a.shape[0] // k, a.shape[1] // k, a.shape[2]), dtype=a.dtype)
    for di in range(k):
        for dj in range(k):
            acc = acc + a[di::k, dj::k]
    return acc


def reduce_grid_column_outer(a, k):
    """the same sum with dj as the outer loop: NOT the rule"""
    acc = np.zeros((a.shape[0] // k, a.shape[1] // k, a.shape[2]), dtype=a.dtype)
    for dj in range(k):
        for di in range(k):
            acc = acc + a[di::k, dj::k]
    return acc


def reduce_grid_numpy_axes(a, k):
    """reshape(...).sum(axis=(1, 3)): NumPy reduces the two strided axes by plain element-wise additions, axis 1 outer and axis 3 inner
    -- which IS the rule's order (NumPy 2.2; test_site_overview_cpu.py asserts the equality), so it is a second statement of the
    rule, not a different order"""
    return a.reshape(a.shape[0] // k, k, a.shape[1] // k, k, a.shape[2]).sum(axis=(1, 3), dtype=a.dtype)


def reduce_grid_numpy_block(a, k):
    """the same sum in NumPy's own order for a contiguous run, each pixel's k * k cells laid out side by side: pairwise summation
    with eight accumulators from eight values on.  NOT the rule"""
    h, w, C = a.shape[0] // k, a.shape[1] // k, a.shape[2]
    blocks = np.ascontiguousarray(a.reshape(h, k, w, k, C).transpose(0, 2, 4, 1, 3)).reshape(h, w, C, k * k)
    return blocks.sum(axis=-1, dtype=a.dtype)


def picture_of(R, colors, thresholds=None, priority=None):
    if R.shape[0] == 0 or R.shape[1] == 0:
        return np.zeros(R.shape[:2] + (3,), dtype=np.uint8)
    with np.errstate(all="ignore"):
        if thresholds is None:
            return ro.render_bev_map(R, np.asarray(colors))
        return ro.render_bev_map_with_thresholds(R, np.asarray(colors), None if priority is None else np.asarray(priority), thresholds)


def overview(a, k, colors, thresholds=None, priority=None):
    """-> (R, picture) of the full-resolution rectangle ``a`` [H, W, C]"""
    R = reduce_grid(a, k)
    return R, picture_of(R, colors, thresholds, priority)


# ------------------------------------------------------------------------------------------------ the executor
def assemble_sources(table, buffers, T, C, dtype, nh, nw):
    """The rectangle of nh x nw tiles at full resolution from the source table: ``buffers`` is a list of np.uint8 arrays indexed by
    the records' ``buf``; a tile without a record is zero."""
    es = np.dtype(dtype).itemsize
    row = T * C * es
    out = np.zeros((nh * T, nw * T, C), dtype=dtype)
    for rec in table:
        buf = buffers[int(rec["buf"])]
        for r in range(T):
            s0 = int(rec["off"]) + r * int(rec["pitch"])
            assert 0 <= s0 and s0 + row <= buf.size
            out[int(rec["row"]) * T + r, int(rec["col"]) * T:(int(rec["col"]) + 1) * T] = buf[s0:s0 + row].view(dtype).reshape(T, C)
    return out


def execute_sources(table, buffers, T, C, dtype, nh, nw, k, colors, thresholds=None, priority=None):
    return overview(assemble_sources(table, buffers, T, C, dtype, nh, nw), k, colors, thresholds, priority)


# ------------------------------------------------------------------------------------------------ a rectangle over a window and a pool
def payload(rng, shape, dtype):
    """values of both signs and several magnitudes, as a log confusion matrix leaves them, some cells exactly zero"""
    v = rng.normal(0.0, 1.0, size=shape) * np.exp(rng.normal(0.0, 2.0, size=shape))
    v[rng.random(shape[:2]) < 0.15] = 0.0
    return v.astype(dtype)


class TableCase(object):
    """A rectangle of 3 x 4 tiles (rows -1 .. 1, columns 2 .. 5): six places lie in a window of 2 x 3 tiles whose first tile is (-1, 3)
    -- one of them masked out as empty although the buffer holds garbage there -- five tiles sit in slabs of a pool of chunks of four,
    one place, (1, 3), is nowhere.  ``full``: what the rectangle holds at full resolution."""

    RECT = (-1, 1, 2, 5)
    ORIGIN_TILE, HT, WT, CHUNK = (-1, 3), 2, 3, 4
    STORED = [((1, 2), 3), ((1, 4), 0), ((0, 2), 6), ((-1, 2), 1), ((1, 5), 4)]

    def __init__(self, T, C, dtype, seed=0):
        from vision_semantic_segmentation_amd import scroll as s
        rng = np.random.default_rng(seed + 7 * T + 131 * C + np.dtype(dtype).itemsize)
        self.T, self.C, self.dtype = T, C, np.dtype(dtype)
        self.bpc = C * self.dtype.itemsize
        self.nh, self.nw = 3, 4
        ti0, _, tj0, _ = self.RECT
        self.full = payload(rng, (self.nh * T, self.nw * T, C), dtype)
        self.full[1, 2, 0] = -0.0
        self.full[T:T + 2, T:T + 2] = -0.0                                         # whole pixels of -0.0: R is +0 and the pixel black
        Hm, Wm = self.HT * T, self.WT * T
        a, b = (self.ORIGIN_TILE[0] - ti0) * T, (self.ORIGIN_TILE[1] - tj0) * T
        window = self.full[a:a + Hm, b:b + Wm].copy()
        self.mask = np.ones((self.HT, self.WT), dtype=bool)
        self.mask[1, 1] = False                                                    # tile (0, 4): the window's bytes there are not read
        self.absent = [(0 - ti0, 4 - tj0), (1 - ti0, 3 - tj0)]
        n_chunks = -(-(max(slab for _, slab in self.STORED) + 1) // self.CHUNK)
        slab_bytes = T * T * self.bpc
        self.bufs = [np.ascontiguousarray(window).reshape(-1).view(np.uint8).copy()]
        self.bufs += [np.full(self.CHUNK * slab_bytes, 0x3F, dtype=np.uint8) for _ in range(n_chunks)]
        for (ti, tj), slab in self.STORED:
            tile = self.full[(ti - ti0) * T:(ti - ti0 + 1) * T, (tj - tj0) * T:(tj - tj0 + 1) * T]
            off = (slab % self.CHUNK) * slab_bytes
            self.bufs[1 + slab // self.CHUNK][off:off + slab_bytes] = np.ascontiguousarray(tile).reshape(-1).view(np.uint8)
        for r, c in self.absent:
            self.full[r * T:(r + 1) * T, c * T:(c + 1) * T] = 0.0
        self.table = s.overview_sources(self.RECT, T, self.bpc, Wm, self.ORIGIN_TILE, self.mask, [t for t, _ in self.STORED],
                                        [slab for _, slab in self.STORED], self.CHUNK)


# ------------------------------------------------------------------------------------------------ the kernel through the C ABI
GUARD = 256


def run_kernel(table, bufs, T, Cn, dtype, nh, nw, k, device, thresholds=None, priority=None, reduced=True, n_tiles=None):
    """-> (picture, R or None): ``table`` through validate_sources, encode_sources and avl_site_overview; asserts that the guard
    strips around both outputs survive"""
    import ctypes as C
    import torch
    from vision_semantic_segmentation_amd import _lib, scroll as s
    dtype = np.dtype(dtype)
    dev_bufs = [torch.from_numpy(b).to(device) for b in bufs]
    extents = [(t.data_ptr(), int(t.numel())) for t in dev_bufs]
    s.validate_sources(table, extents, T, Cn * dtype.itemsize, nh, nw)
    rec = np.zeros(max(len(table), 1), dtype=s.SRC_DTYPE)
    s.encode_sources(table, extents, rec)
    tiles = torch.from_numpy(rec.view(np.uint8)).to(device)
    P = T // k
    npx = nh * P * nw * P
    pic = torch.full((GUARD + 3 * npx + GUARD,), 0xAB, dtype=torch.uint8, device=device)
    red = torch.full((GUARD + npx * Cn * dtype.itemsize + GUARD,), 0xAB, dtype=torch.uint8, device=device)
    colors = np.ascontiguousarray(COLORS[:Cn])
    col = (C.c_uint8 * colors.size)(*colors.ravel().tolist())
    th = (C.c_double * Cn)(*thresholds) if thresholds is not None else None
    pr = (C.c_int32 * Cn)(*priority) if priority is not None else None
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = _lib.lib().avl_site_overview(C.c_void_p(tiles.data_ptr()), len(table) if n_tiles is None else n_tiles, nh, nw, T, Cn,
                                      _lib.AVL_F64 if dtype == np.float64 else _lib.AVL_F32, k, col, pr, th, C.c_void_p(pic.data_ptr() + GUARD),
                                      C.c_void_p(red.data_ptr() + GUARD) if reduced else None, C.c_void_p(stream))
    _lib.check(rc, "avl_site_overview")
    torch.cuda.synchronize(device)
    pic, red = pic.cpu().numpy(), red.cpu().numpy()
    for name, a in (("picture", pic), ("reduced", red)):
        assert (a[:GUARD] == 0xAB).all() and (a[-GUARD:] == 0xAB).all(), "guard strip of %s written" % name
    if not reduced:
        assert (red == 0xAB).all()
    return pic[GUARD:-GUARD].reshape(nh * P, nw * P, 3), (red[GUARD:-GUARD].view(dtype).reshape(nh * P, nw * P, Cn) if reduced else None)
