"""Exactly computable cases for the ring GEMM's EXT forms (strided input rows, a second destination, both in one op), shared by
test_exact_operands_cpu.py (operand conditions and teeth, without a GPU) and test_gpu_ring_ext_exact.py (which runs the ops).

Operands are the integers of _exact_operands.py, K = 256 (four 64-wide K blocks: the ring wraps).  The split modes are DECOUPLED
as in test_gpu_gemm_exact.py: weight rows [n][K/64][W1 64 | W2 64 (| W3 64)] from independent matrices, and an independent integer
in_lo plane:
    v = x . W1^T (+ x . W2^T) (+ x_lo . W3^T) + bias, then the ReLU            x, x_lo = the input planes' rows THROUGH THE PIXEL MAP
Every term is of one size, so a pass that pairs the lo plane with the wrong block, or reads it through the wrong row map, moves
outputs by hundreds of ulps.  36 * K * passes + max|bias| < 2^24: fp32 accumulation is exact in any order (asserted).

Expected, with v exact: out = type(v) rounded once, out_lo = f16(v - out) where a lo plane is written, columns [0, n_split) in the
first destination (at column COL of a buffer 128 columns wider than its slice), the rest in the second (64 columns wider); every
other element of both buffers' two planes keeps FILL.  stored() builds the WHOLE buffers, so one torch.equal covers rows past M,
neighbouring columns and planes that are not written.  The device input (device_input) holds NaN in every row and column the op
must not read: pixels a strided read skips, columns past K, rows past the last image.

Which kernel a case reaches is asked of the library (route(): avl_seg_gemm_route on the case's op, whose header comment states the
rule): k_gemm_ring<H, WM, WN, MI, STAGES, NSUB, IO, AST, EXT = true> with the arguments INSTANTIATION names for the case's mode and
tile variant; tests/test_exact_operands_cpu.py checks every case's route against that table."""
import collections
import functools

import torch

import _exact_operands as X

K = 256
FILL = 7.0
COL = 64                # the first destination starts at this column of its buffer
PAD1, PAD2 = 128, 64    # columns the two buffers are wider than the slice written
MODES = {"f16": ("f16", 1), "bf16": ("bf16", 1), "w2": ("f16", 2), "split": ("f16", 3)}      # mode -> (type, passes per K block)
INSTANTIATION = {       # (mode, tile variant) -> template arguments <H, WM, WN, MI, STAGES, NSUB, IO, AST, EXT>
    ("f16", 2): "f16, 4, 2, 4, 3, 1, 0, 3, true", ("bf16", 2): "bf16, 4, 2, 4, 3, 1, 0, 3, true",
    ("f16", 3): "f16, 2, 4, 8, 2, 1, 0, 2, true", ("bf16", 3): "bf16, 2, 4, 8, 2, 1, 0, 2, true",
    ("w2", 2): "f16, 4, 2, 4, 3, 2, 1, 3, true", ("w2", 3): "f16, 2, 4, 8, 3, 2, 1, 2, true",
    ("split", 2): "f16, 4, 2, 4, 3, 3, 1, 3, true", ("split", 3): "f16, 2, 4, 8, 2, 3, 1, 2, true",
}

# mode, w_layout, batch, input image (ih, iw) read with stride s (s = 1: ih = 1, iw = M), extra = in_ld - K, N, n_split (0 = one
# destination), lo1 / lo2 = out_lo / out2_lo set, relu
Case = collections.namedtuple("Case", "mode wl B ih iw s extra N n_split lo1 lo2 relu")


def case_id(c):
    return "%s-wl%d-b%d-%dx%d-s%d-ld%d-N%d-ns%d-lo%d%d-relu%d" % (c.mode, c.wl, c.B, c.ih, c.iw, c.s, K + c.extra, c.N, c.n_split, c.lo1, c.lo2, c.relu)


def _up(n, m):
    return (n + m - 1) // m * m


def geometry(c):
    oh, ow = (c.ih - 1) // c.s + 1, (c.iw - 1) // c.s + 1
    M = c.B * oh * ow
    n1 = c.n_split or c.N
    return dict(oh=oh, ow=ow, M=M, in_pix=c.B * c.ih * c.iw, in_rows=_up(max(M, c.B * c.ih * c.iw), 256), out_rows=_up(M, 256),
                w_rows=_up(c.N, 256), n1=n1, n2=c.N - n1, ld1=n1 + PAD1, ld2=c.N - n1 + PAD2)


def shape_op(c, ptr):
    """the case's op with `ptr` (16-byte aligned) in every pointer field the case sets: what the library's validation and its
    choice of kernel look at.  test_gpu_ring_ext_exact.py puts the device buffers in."""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_GEMM, AvlSegOp
    g = geometry(c)
    prec, nsub = MODES[c.mode]
    op = AvlSegOp()
    op.kind, op.dtype = OP_GEMM, _lib.AVL_BF16 if prec == "bf16" else _lib.AVL_F16
    op.in_ = op.weight = op.bias = op.out = ptr
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = c.ih, c.iw, K, K + c.extra, g["in_rows"]
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = g["oh"], g["ow"], c.N, g["ld1"], g["out_rows"]
    op.relu, op.w_rows, op.ksize, op.stride, op.dil, op.groups, op.batch = int(c.relu), g["w_rows"], 1, c.s, 1, 1, c.B
    op.w_layout, op.w_split = c.wl, int(nsub > 1)
    if nsub == 3:
        op.in_lo = ptr
    if c.lo1:
        op.out_lo = ptr
    if c.n_split:
        op.out2, op.out2_ld, op.n_split = ptr, g["ld2"], c.n_split
        if c.lo2:
            op.out2_lo = ptr
    return op


def claimed_variant(c):
    """the tile variant a case is written for (INSTANTIATION's second key): the one its w_layout forces (N is a multiple of 256 wherever
    that is 3); the w_layout-0 cases here are small shapes of N = 384, which the library runs on 256 x 128 tiles"""
    return c.wl or 2


def route(c):
    """the library's answer for the case's op (network.gemm_route)"""
    from vision_semantic_segmentation_amd.network import gemm_route
    return gemm_route(shape_op(c, 16))


def variant(c):
    """the tile variant the case runs with, in w_layout's numbering: 2 = 256 x 128 tiles, 3 = 256 x 256"""
    return {128: 2, 256: 3}[route(c)["tile_n"]]


def tiles(c):
    """(mtiles, ntiles) of the launch"""
    r = route(c)
    return r["m_tiles"], r["n_tiles"]


def instantiation(r):
    """a route of the ring kernel in INSTANTIATION's form"""
    from vision_semantic_segmentation_amd.network import gemm_kernel_name
    name = gemm_kernel_name(r)
    assert name.startswith("k_gemm_ring<"), name
    return name[len("k_gemm_ring<"):-1]


def row_map(c, wrong=None):
    """input row of every output row; wrong = "unstrided" | "stride_x_only" | "image0_base": the maps a broken loader would use"""
    g = geometry(c)
    m = torch.arange(g["M"])
    if wrong == "unstrided":
        return m
    ohw = g["oh"] * g["ow"]
    img, rem = m // ohw, m % ohw
    oy, ox = rem // g["ow"], rem % g["ow"]
    base = 0 if wrong == "image0_base" else img * (c.ih * c.iw)
    return base + oy * (1 if wrong == "stride_x_only" else c.s) * c.iw + ox * c.s


@functools.lru_cache(maxsize=3)
def _planes(rows):
    return X.ints(X._seed(rows, 1), rows, K), X.ints(X._seed(rows, 2), rows, K)


@functools.lru_cache(maxsize=3)
def _weights(w_rows):
    """W1, W2, W3 [w_rows][K]: rows past N hold values too, they must reach no output"""
    return tuple(X.ints(X._seed(w_rows, 10 + j), w_rows, K) for j in range(3))


def bias(c):
    prec = MODES[c.mode][0]
    return X.bias_for(c.N, X._seed(c.N, c.n_split, len(c.mode), c.relu), prec, c.relu)


def _prod(a, w, check64):
    p = a @ w.t()
    if check64:
        assert torch.equal(p.double(), a.double() @ w.double().t()), "the float32 and float64 host products differ"
    return p.double()


def exact_v(c, rows=None, lo_rows=None, w3_is_w1=False, check64=False, b=None):
    """the exact result [M][N] as float64.  rows / lo_rows = wrong row maps of the hi / lo plane (row_map's names); b = another
    bias [N] (the non-finite tests: the bound is on its finite entries)"""
    g = geometry(c)
    nsub = MODES[c.mode][1]
    xh, xl = _planes(g["in_rows"])
    W = [w[:c.N] for w in _weights(g["w_rows"])]
    b = bias(c) if b is None else b
    bound = 36.0 * K * nsub + float(b[torch.isfinite(b)].abs().max())
    assert bound < X.LIMIT, "exactness bound: %g >= 2^24" % bound
    a = xh[row_map(c, rows)]
    acc = _prod(a, W[0] + W[1] if nsub >= 2 else W[0], check64)         # (W1 + W2: |.| <= 12, the same bound)
    if nsub == 3:
        acc = acc + _prod(xl[row_map(c, lo_rows)], W[0] if w3_is_w1 else W[2], check64)
    v = acc + b.double()
    return torch.relu(v) if c.relu else v


def stored(c, v, wrong=None):
    """every byte of both destinations after the op, as {"out": [2][out_rows][ld1], "out2": [2][out_rows][ld2]} in the case's
    type (plane 1 = the lo plane).  wrong = "split_to_first": the tiles from n_split on written to the first destination too;
    "cbase_not_reduced": the second destination written from its column n_split on"""
    g = geometry(c)
    prec = MODES[c.mode][0]
    dt = X.DTYPES[prec]
    hi = v.to(dt)
    assert bool(torch.isfinite(hi).all())
    lo = (v - hi.double()).to(torch.float16).to(dt)
    M, n1 = g["M"], g["n1"]
    out = torch.full((2, g["out_rows"], g["ld1"]), FILL, dtype=dt)
    out2 = torch.full((2, g["out_rows"], g["ld2"]), FILL, dtype=dt)

    def put(buf, with_lo, col, src0, n):
        n = max(0, min(n, buf.shape[2] - col))
        buf[0, :M, col:col + n] = hi[:, src0:src0 + n]
        if with_lo:
            buf[1, :M, col:col + n] = lo[:, src0:src0 + n]
    put(out, c.lo1, COL, 0, n1)
    if c.n_split:
        if wrong == "split_to_first":
            put(out, c.lo1, COL + n1, n1, g["n2"])
        elif wrong == "cbase_not_reduced":
            put(out2, c.lo2, n1, n1, g["n2"])
        else:
            put(out2, c.lo2, 0, n1, g["n2"])
    return {"out": out, "out2": out2}


def want(c, check64=False):
    """(v, expected buffers); asserts the case's conditions: the exactness bound, >= 20 % of the outputs round, ties in both
    directions, a non-zero lo plane where one is written"""
    v = exact_v(c, check64=check64)
    prec = MODES[c.mode][0]
    hi = v.to(X.DTYPES[prec])
    X.rounding_conditions(v, hi, prec)
    if c.lo1 or c.lo2:
        assert prec == "f16" and MODES[c.mode][1] > 1
        lo = v - hi.double()
        n1 = geometry(c)["n1"]
        assert (not c.lo1 or bool((lo[:, :n1] != 0).any())) and (not c.lo2 or bool((lo[:, n1:] != 0).any()))
    return v, stored(c, v)


MUTATIONS = ("unstrided", "stride_x_only", "image0_base", "split_to_first", "cbase_not_reduced", "lo_unstrided", "w3_is_w1")


def applicable(c, mut):
    if mut in ("unstrided", "stride_x_only"):
        return c.s > 1
    if mut == "image0_base":
        return c.s > 1 and c.B > 1
    if mut in ("split_to_first", "cbase_not_reduced"):
        return c.n_split > 0
    if mut == "lo_unstrided":
        return c.s > 1 and c.mode == "split"
    return c.mode == "split"


def mutated(c, mut):
    """the buffers a subtly wrong kernel would leave"""
    if mut in ("unstrided", "stride_x_only", "image0_base"):
        return stored(c, exact_v(c, rows=mut, lo_rows=mut))
    if mut == "lo_unstrided":
        return stored(c, exact_v(c, lo_rows="unstrided"))
    if mut == "w3_is_w1":
        return stored(c, exact_v(c, w3_is_w1=True))
    return stored(c, exact_v(c), wrong=mut)


def same(a, b):
    return all(torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)) for k in ("out", "out2"))


def device_input(c):
    """[2 | 1][in_rows][K + extra] in the case's type: the integer planes at the pixels the op reads, NaN everywhere else"""
    g = geometry(c)
    prec, nsub = MODES[c.mode]
    planes = 2 if nsub == 3 else 1
    a = torch.full((planes, g["in_rows"], K + c.extra), float("nan"), dtype=X.DTYPES[prec])
    rows = row_map(c)
    for p, x in zip(range(planes), _planes(g["in_rows"])):
        a[p, rows, :K] = x[rows].to(a.dtype)
    return a


def device_weights(c, b=None):
    """(packed weight rows [w_rows][K * passes] in the case's type, fp32 bias [w_rows] with 12345 past N)"""
    g = geometry(c)
    prec, nsub = MODES[c.mode]
    ws = _weights(g["w_rows"])[:nsub]
    packed = torch.cat([w.reshape(g["w_rows"], K // 64, 1, 64) for w in ws], dim=2).reshape(g["w_rows"], K * nsub)
    bp = torch.full((g["w_rows"],), 12345.0)
    bp[:c.N] = bias(c) if b is None else b
    return packed.to(X.DTYPES[prec]).contiguous(), bp


# ------------------------------------------------------------------------------------------------------------- the cases
CONFIGS = [("f16", 2), ("bf16", 2), ("f16", 3), ("bf16", 3), ("w2", 2), ("w2", 3), ("split", 2), ("split", 3)]
# strided geometries (B, ih, iw, s, extra): 35 rows = one tile, mostly padding; 180 = one ragged tile; stride 3 on an image whose
# sides are no multiples of 3, batch 2 (image 1's first pixel is row 168 of 336: inside row tile 0), input rows wider than K;
# batch 2 at stride 2 (image 1 starts at row 180 of 360)
GEO = [(1, 9, 13, 2, 0), (1, 20, 36, 2, 0), (2, 34, 41, 3, 64), (2, 20, 36, 2, 0)]
_S3 = GEO[2]


def _split(mode):
    return MODES[mode][1] > 1


def _small():
    strided, twin, both = [], [], []
    for i, (mode, wl) in enumerate(CONFIGS):
        sp = _split(mode)
        # strided rows, one destination (N = 256: two 128-wide N tiles or one 256-wide)
        strided.append(Case(mode, wl, *GEO[i % 4], 256, 0, sp, False, i % 2 == 0))
        # a second destination: N = 384 = 128 + 256 on 256 x 128 tiles, N = 512 = 256 + 256 on 256 x 256; M = 300: two row tiles
        N, ns = (384, 128) if wl == 2 else (512, 256)
        twin.append(Case(mode, wl, 1, 1, 300, 1, 0, N, ns, sp, sp, i % 2 == 1))
        # both in one op, at stride 3 and batch 2
        both.append(Case(mode, wl, *_S3, N, ns, sp, sp and i % 2 == 0, i % 2 == 0))
    strided += [Case("split", 2, *_S3, 256, 0, True, False, False), Case("f16", 3, *_S3, 256, 0, False, False, True),
                Case("bf16", 2, *_S3, 256, 0, False, False, False), Case("w2", 3, *_S3, 256, 0, True, False, True)]
    twin += [Case("split", 2, 1, 1, 300, 1, 0, 384, 128, True, False, True),       # out2_lo NULL beside out_lo
             Case("split", 3, 1, 1, 300, 1, 0, 512, 256, False, True, False),      # out2_lo alone
             Case("w2", 2, 1, 1, 300, 1, 0, 384, 256, False, True, True),          # n_split = two N tiles
             Case("w2", 3, 1, 1, 300, 1, 0, 512, 256, True, False, False),
             Case("split", 2, 1, 1, 35, 1, 0, 384, 128, True, True, True),         # one tile, mostly padding
             Case("f16", 0, 1, 1, 180, 1, 64, 384, 128, False, False, False)]      # w_layout 0: by shape (256 x 128), rows wider than K
    return strided, twin, both


SMALL_STRIDED, SMALL_TWIN, SMALL_BOTH = _small()
SMALL_CASES = SMALL_STRIDED + SMALL_TWIN + SMALL_BOTH

# Several tiles per workgroup: mtiles * ntiles > 256 (the grid's cap), so workgroups walk a second tile (258 tiles: workgroups 0
# and 1, whose second tiles are the ragged last row tile; 344: 88 of them; 513: every one, workgroup 0 a third); with three N tiles
# 256 % 3 = 1 and a workgroup's consecutive tiles t, t + 256 lie in different N tiles: across n_split they change destination.
#   one image of 1 x 21797 rows: 85 * 256 + 37, 86 row tiles, the last ragged
#   strided: two images of 125 x 345 read at stride 2 -> 63 x 173 = 10899 rows each, M = 21798 = 85 * 256 + 38: 86 row tiles; image 1
#   starts at row 10899 = 42 * 256 + 147, inside row tile 42; the clamp min(row, M - 1) runs on tile 85, no workgroup's first
#   one image of 1 x 43557 rows: 171 row tiles, the last ragged; 171 x 3 = 513 tiles: two full rounds of the grid and one more
_ONE, _TWO, _LONG = (1, 1, 21797, 1, 0), (2, 125, 345, 2, 0), (1, 1, 43557, 1, 0)
MULTI_TILE_CASES = [
    # ---- two destinations, N = 384 on 256 x 128 tiles: 86 x 3 = 258 tiles > 256, 256 % 3 = 1
    Case("split", 2, *_ONE, 384, 128, True, True, True),        # the network's layer2.0.conv1 + low_level_conv form
    Case("bf16", 2, *_ONE, 384, 128, False, False, False),
    Case("w2", 2, *_ONE, 384, 256, True, False, True),          # two of the three N tiles to the first destination
    # ---- two destinations, N = 768 on forced 256 x 256 tiles: 86 x 3 = 258 tiles > 256, 256 % 3 = 1
    Case("w2", 3, *_ONE, 768, 256, True, True, False),          # the AST = 2 variant
    Case("split", 3, *_ONE, 768, 512, True, False, True),
    Case("f16", 3, *_ONE, 768, 256, False, False, True),
    Case("bf16", 3, *_ONE, 768, 512, False, False, True),
    # ---- N = 512 on 256 x 128 tiles: 86 x 4 = 344 tiles > 256, 256 % 4 = 0: a workgroup keeps its destination
    Case("split", 2, *_ONE, 512, 256, True, True, False),
    # ---- strided rows, the same tile counts (86 x 3 = 258 > 256)
    Case("split", 2, *_TWO, 384, 0, True, False, True),
    Case("f16", 2, *_TWO, 384, 0, False, False, False),
    Case("w2", 3, *_TWO, 768, 0, True, False, True),
    Case("bf16", 3, *_TWO, 768, 0, False, False, False),
    # ---- both in one op (86 x 3 = 258 > 256, 256 % 3 = 1)
    Case("split", 2, *_TWO, 384, 128, True, True, True),
    Case("f16", 3, *_TWO, 768, 256, False, False, False),
    # ---- every workgroup walks two tiles and changes destination on the way: 171 x 3 = 513 tiles > 2 * 256, 256 % 3 = 1
    Case("split", 2, *_LONG, 384, 128, True, True, False),
    Case("w2", 3, *_LONG, 768, 256, True, True, True),
]
