"""Exactly computable cases for the split (WS = 1, WS = 1 + XS) and MX (WS = 2) forms of the grouped 3x3 on the matrix cores
(k_gconv_mfma<f16, WS, NJ, XS>, csrc/seg_gconv_mfma.hip), shared by test_gconv_mixed_operands_cpu.py (operand conditions, the
claims about tile heights and the teeth of the comparison, without a GPU) and test_gpu_gconv_mixed_exact.py (which runs the ops).

DECOUPLED operands: every term of the accumulator comes from a matrix of its own (integers of _exact_operands.VALUES), so all terms
are of one size and a dropped, doubled or mis-paired pass moves most outputs by hundreds of ulps:
    WS = 2:  acc = Wh * A + Wl * B (+ Wh' * C) + bias      A = the f16 input plane, B / C = the hi / lo half of in_mx (C only under
             AVL_MX_IN_LO), Wh = the f16 fragments, Wl / Wh' = pair 0 / pair 1 of w_mx
    WS = 1:  acc = W1 * A + W2 * A (+ W1 * A_lo) + bias    fragments [9 taps W1 | 9 taps W2]; the third term is XS (a real in_lo plane)
Scales that tell blocks apart: every activation block of B and C (one pixel x one 32-channel window) and every weight block of Wl and
Wh' (one output channel x one tap) is multiplied by its own factor of {1/2, 1, 2}.  Such blocks pass the host's FP4 quantiser unchanged
(asserted: the decoded bundles are the operands), neighbouring windows and the three tap groups of a row carry different E8M0 bytes,
and at least three distinct scale bytes occur in each bundle (asserted).  w_mx is spliced from three calls of the shipped packer
(pack_gconv_mx derives both pairs from ONE w): frag of pack_gconv_mx(Wh), pair 0 <- pair 1 of pack_gconv_mx(Wl), pair 1 <- pair 1 of
pack_gconv_mx(Wh'); decode_w4 reads the result back.

Exactness: products are multiples of 1/4 of magnitude <= 144; (3 passes * 9 taps * cg * 144 + max|bias|) * 4 < 2^24 at cg <= 32, so
fp32 accumulation is exact in any order; asserted per case together with float32 == float64 host evaluation of every pass.

Bias: integers; 3/8 of the columns in +2048 .. +7000 (the kernel always applies its ReLU; the integer sums of the WS = 1 forms round
only from 2048 up, and a bare quarter of the columns would leave them at ~16 % rounded outputs, below the 20 % every case asserts),
1/16 beyond -2048 (whole columns clamp to zero), the rest within +-40.  Per case: >= 20 % of the expected hi values are not
representable before rounding, exact ties (v midway between two neighbouring f16 values) round down to even and up to even, and the
lo part is non-zero in >= 10 % of the live elements.

Expected buffers (stored), with v the exact result after the ReLU: out = f16(v), out_lo = f16(v - out), the Q4(hi) half of out_mx =
mx_quant_fp4(out), the Q4(lo) half = mx_quant_fp4 of the f16 lo plane (out_lo set) or of the fp32 value v - out (AVL_MX_OUT_LO); rows
past the last pixel keep FILL / FILL_BYTE in every plane, FP4 plane and scale slab, and so do out_lo and the lo half where the form
does not write them.  NOTE: with integer biases v - out is a multiple of 1/4 below 8, exact in f16, so the two sources of Q4(lo) give
the same bytes and the mutation "lo_source" is shown NOT to be visible on those cases.  FRAC_CASES therefore add three cases whose
biases carry a 2^-10 part on 8192 .. 11000 in a third of the columns: still exact in fp32 in any order (every partial sum is a multiple
of 2^-10 below 2^14: asserted on the operands' own sum of |x| |w|), v - out then has up to twelve significant bits, the f16 lo plane
rounds it, and the two sources differ in FP4 bytes (asserted in both directions by the CPU test).

pick_th / tile_bytes restate gconv_pick_th / gconv_tile_bytes of the launcher; every case names (WS, XS, NJ) and its tiles per
workgroup at 256 CUs, and both test files check the claim."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _exact_operands as X

G = 32
FILL, FILL_BYTE = 7.0, 0xA5
LIMIT = 2 ** 24
FORMS = ("mx_f32lo", "mx_lo", "lo", "single")      # out_mx + AVL_MX_OUT_LO | out_mx + out_lo | out_lo alone | one plane

# ws: 1 | 2; xs: WS = 1 with an in_lo plane; in_lo: WS = 2 under AVL_MX_IN_LO; form: FORMS; nj, tpw: the claim at 256 CUs
# bias: "int" | "frac" (FRAC_CASES: a third of the columns carry 8192 .. 11000 + 2^-10, see the module docstring)
Case = collections.namedtuple("Case", "ws xs in_lo form B H W C s d nj tpw bias", defaults=("int",))


def case_id(c):
    return "ws%d%s%s-%s-b%d-%dx%dx%d-s%d-d%d-nj%d-t%d%s" % (c.ws, "xs" if c.xs else "", "-inlo" if c.in_lo else "", c.form, c.B, c.H, c.W, c.C,
                                                          c.s, c.d, c.nj, c.tpw, "" if c.bias == "int" else "-" + c.bias)


_R, _S2, _D2, _D4, _LONG = (1, 23, 45, 256, 1, 1), (1, 23, 45, 256, 2, 1), (1, 30, 41, 512, 1, 2), (1, 19, 67, 1024, 1, 4), (1, 19, 401, 512, 1, 1)
CASES = [
    # ---- WS = 2: (AVL_MX_IN_LO off / on) x the four output forms, each at least once
    Case(2, False, True, "mx_f32lo", *_R, 2, 1),            # the default plan's form; ragged in both directions: 6 x 2 tiles of 4 x 32
    Case(2, False, False, "mx_f32lo", *_R, 2, 1),
    Case(2, False, True, "mx_lo", *_S2, 1, 1),              # stride 2: two four-row MX tiles do not fit 160 KB: the two-row tile
    Case(2, False, False, "mx_lo", *_D2, 2, 1),             # comb, 4 residue classes
    Case(2, False, True, "lo", *_D4, 2, 2),                 # comb, 16 classes x 2 tiles of 4 x 32 on 16 slots: two per workgroup
    Case(2, False, False, "lo", *_D2, 2, 1),
    Case(2, False, False, "single", *_S2, 1, 1),
    Case(2, False, True, "single", *_D2, 2, 1),
    Case(2, False, True, "mx_f32lo", *_LONG, 2, 3),         # 5 x 13 tiles on 32 slots: three per workgroup, runs cross tile columns
    Case(2, False, False, "mx_lo", *_LONG, 2, 3),
    Case(2, False, True, "mx_f32lo", 2, 23, 45, 256, 1, 1, 2, 1),      # batch 2: 1035 pixels per image, image 1 starts inside a 256-row block
    Case(2, False, False, "mx_lo", 2, 23, 45, 256, 2, 1, 1, 1),
    # ---- WS = 1
    Case(1, False, False, "single", 1, 23, 45, 128, 1, 1, 2, 1),
    Case(1, False, False, "lo", *_S2, 2, 1),                # stride 2, dilation 1: four-row tiles
    Case(1, False, False, "mx_lo", 1, 23, 45, 256, 2, 2, 1, 1),        # stride 2 with dilation 2: the two-row tile
    Case(1, False, False, "mx_f32lo", *_D2, 2, 1),
    Case(1, False, False, "lo", *_D4, 4, 1),                # comb: a class's 5 x 17 grid is one eight-row tile, 16 tiles on 16 slots
    Case(1, False, False, "single", 1, 97, 33, 1024, 1, 1, 4, 2),      # 13 x 2 tiles of 8 rows on 16 slots: the eight-row tile
    Case(1, False, False, "mx_lo", 1, 97, 33, 1024, 1, 1, 4, 2),
    Case(1, False, False, "mx_lo", *_LONG, 2, 3),
    # ---- WS = 1 + XS (the split16 plan: out_lo)
    Case(1, True, False, "lo", 1, 23, 45, 128, 1, 1, 2, 1),
    Case(1, True, False, "lo", *_D2, 2, 1),
    Case(1, True, False, "lo", *_D4, 2, 2),
    Case(1, True, False, "lo", *_LONG, 2, 3),
]
# Which value the Q4(lo) half is quantised from -- the fp32 difference v - out under AVL_MX_OUT_LO, the stored f16 lo plane with out_lo --
# cannot show on integer biases (module docstring).  These three cases add 2^-10 to biases of 8192 .. 11000: the difference then has twelve
# significant bits from |lo| = 2 up, f16 rounds it, and FP4 ties such as 2.5 + 2^-10 fall to different sides.
FRAC_CASES = [Case(2, False, True, "mx_f32lo", *_R, 2, 1, "frac"), Case(2, False, True, "mx_lo", *_R, 2, 1, "frac"),
              Case(1, False, False, "mx_f32lo", *_R, 2, 1, "frac")]
CASES += FRAC_CASES


def _up(n, m):
    return (n + m - 1) // m * m


def geometry(c):
    oh, ow = (c.H - 1) // c.s + 1, (c.W - 1) // c.s + 1           # pad = dilation
    m_in, m = c.B * c.H * c.W, c.B * oh * ow
    return dict(oh=oh, ow=ow, m_in=m_in, m=m, rows_in=_up(m_in, 256), rows=_up(m, 256), cg=c.C // G, nwin=c.C // 32)


def has_lo(c):
    return c.form in ("mx_lo", "lo")


def has_mx(c):
    return c.form in ("mx_f32lo", "mx_lo")


# ------------------------------------------------------------------------- the launcher's choice of tile height, restated
def tile_bytes(stride, dil, th, mx=False, xs=False):
    """one LDS tile buffer (gconv_tile_bytes): the f16 tile in whole 8-pixel groups of 1 KB, twice with a split input; MX adds four FP4
    tiles (plane 2 x window 2) and two scale-dword tiles in whole 64-pixel groups"""
    in_th, in_tw = (th - 1) * stride + 2 * dil + 1, 31 * stride + 2 * dil + 1
    npix = in_th * in_tw
    n64 = (npix + 63) // 64
    return (npix + 7) // 8 * 1024 * (2 if xs else 1) + (4 * n64 * 1024 + 2 * n64 * 256 if mx else 0)


def pick_th(c, cus=256):
    """gconv_pick_th: among tile heights 8 and 4 (2 only when nothing else fits) whose two buffers fit 160 KB -- 8 skipped for MX and
    for a split input -- the one with the lowest rounds * (th + 0.5); -> dict(th, nj, comb, tiles_x, tiles_y, nsp, nslots, tpw) or None"""
    mx, xs = c.ws == 2, c.xs
    g = geometry(c)
    comb = c.s == 1 and c.d > 1
    d = 1 if comb else c.d
    gh, gw = (-(-g["oh"] // c.d), -(-g["ow"] // c.d)) if comb else (g["oh"], g["ow"])
    ncomb, cchunks = (c.d * c.d if comb else 1), c.C // 64
    best = None
    for th in (8, 4, 2):
        if 2 * tile_bytes(c.s, d, th, mx, xs) > 160 * 1024 or ((mx or xs) and th == 8):
            continue
        tiles_x, tiles_y = -(-gw // 32), -(-gh // th)
        nsp = tiles_x * tiles_y * ncomb
        nslots = max(1, min(cus // cchunks, nsp))
        rounds = -(-nsp // nslots)
        cost = rounds * (th + 0.5)
        if th == 2 and best is not None:
            break
        if best is None or cost < best["cost"]:
            best = dict(th=th, nj=th // 2, comb=comb, tiles_x=tiles_x, tiles_y=tiles_y, nsp=nsp, nslots=nslots, tpw=rounds, cost=cost)
    return best


def accepted(c):
    """validate_gconv_mfma's LDS checks: the two-row tile must fit (with the FP4 tiles for MX, with the lo tile for a split input)"""
    d = 1 if c.s == 1 else c.d
    return 2 * tile_bytes(c.s, d, 2, c.ws == 2, False) <= 160 * 1024 and 2 * tile_bytes(c.s, d, 2, False, c.xs) <= 160 * 1024


def walk_crosses_columns(t):
    """a workgroup's run of `tpw` tiles, numbered down the tile columns, goes from the bottom of one column to the top of the next"""
    per = t["tpw"]
    return any((slot * per) // t["tiles_y"] != (min(t["nsp"], (slot + 1) * per) - 1) // t["tiles_y"]
               for slot in range(t["nslots"]) if slot * per < t["nsp"])


# ------------------------------------------------------------------------------------------------------------- operands
def _factors(seed, shape):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=torch.Generator().manual_seed(seed))]


def bias_for(n, seed, kind="int"):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=g)
    small = torch.randint(-40, 41, (n,), generator=g).float()
    pos = torch.randint(2048, 7000, (n,), generator=g).float()
    neg = -torch.randint(2049, 7000, (n,), generator=g).float()
    b = torch.where(u < 0.375, pos, torch.where(u < 0.4375, neg, small))
    if kind == "frac":
        # 14 + 10 bits: exact in fp32; the half lets the integer sums of WS = 1 reach FP4 ties (2.5, 3.5) too
        frac = torch.randint(8192, 11000, (n,), generator=g).float() + (0.5 + 2.0 ** -10)
        b = torch.where(u >= 0.67, frac, b)
    return b


def _weights(seed, C, scaled):
    """float32 [C][cg][3][3]; scaled: every (output channel, tap) block times its own factor"""
    cg = C // G
    w = X.conv_weights(seed, G, cg, 9, cg).reshape(C, 9, cg).permute(0, 2, 1).contiguous()
    if scaled:
        w = w * _factors(seed + 7, (C, 1, 9))
    return w.reshape(C, cg, 3, 3)


def _plane(seed, c, scaled):
    """float32 [B][H][W][C]; scaled: every (pixel, 32-channel window) block times its own factor"""
    x = X.ints(seed, c.B * c.H * c.W, c.C).reshape(c.B, c.H, c.W, c.C // 32, 32)
    if scaled:
        x = x * _factors(seed + 7, (c.B, c.H, c.W, c.C // 32, 1))
    return x.reshape(c.B, c.H, c.W, c.C)


@functools.lru_cache(maxsize=3)
def operands(shape, ws, bias_kind):
    """the matrices of a shape (B, H, W, C): planes "A", "B", "C" and weights "W0", "W1", "W2", the accumulator being
    W0 * A + W1 * B + W2 * C for WS = 2 (Wh, Wl, Wh') and W0 * A + W1 * A + W0 * B for WS = 1 (W1, W2; B = the in_lo plane)"""
    c = Case(ws, False, False, "single", *shape, 1, 1, 0, 0)
    s = X._seed(*shape, ws)
    mx = ws == 2
    return {"A": _plane(s, c, False), "B": _plane(s + 1, c, mx), "C": _plane(s + 2, c, mx),
            "W0": _weights(s + 3, c.C, False), "W1": _weights(s + 4, c.C, mx), "W2": _weights(s + 5, c.C, mx),
            "bias": bias_for(c.C, s + 6, bias_kind)}


def ops_of(c):
    return operands((c.B, c.H, c.W, c.C), c.ws, c.bias)


def conv(c, x, w, dtype=torch.float64, clamp=False):
    """the grouped 3x3 of plane x [B][H][W][C] with weights w [C][cg][3][3] -> [M][C]; clamp: the halo replicates the border pixel"""
    xn = x.to(dtype).permute(0, 3, 1, 2)
    pad = c.d
    if clamp:
        xn, pad = F.pad(xn, (c.d,) * 4, mode="replicate"), 0
    y = F.conv2d(xn, w.to(dtype), None, stride=c.s, padding=pad, dilation=c.d, groups=G)
    return y.permute(0, 2, 3, 1).reshape(-1, c.C)


def _without_tap8(w):
    w = w.clone()
    w[:, :, 2, 2] = 0
    return w


PASS_MUTATIONS = ("drop_pass", "drop_lo_pass", "double_pass", "second_weights_with_lo_input", "tap8_missing", "clamped_border")


def passes(c, o, mut=None):
    """the (plane, weights, clamp) terms of the case's accumulator on operand set o; mut: a PASS_MUTATIONS name.  The "corrections"
    of WS = 1 are its second weight block and the lo plane's pass."""
    A, B, Cc, W0, W1, W2 = (o[k] for k in ("A", "B", "C", "W0", "W1", "W2"))
    third = c.in_lo or c.xs
    if c.ws == 2:
        p = [(A, W0), (B, W1)] + ([(Cc, W2)] if third else [])
    else:
        p = [(A, W0), (A, W1)] + ([(B, W0)] if third else [])
    if mut == "drop_pass":
        del p[1]
    elif mut == "drop_lo_pass":
        del p[2]
    elif mut == "double_pass":
        p.append(p[1])
    elif mut == "second_weights_with_lo_input":
        p[1] = (p[2][0], p[1][1])
    elif mut == "tap8_missing":
        p = p[:1] + [(x, _without_tap8(w)) for x, w in p[1:]]
    p = [(x, w, mut == "clamped_border" and i > 0) for i, (x, w) in enumerate(p)]
    return p


def exact_v(c, o, mut=None, check=False):
    """the exact result after the ReLU, float64 [M][C]; check: assert the bound and float32 == float64 for every pass"""
    acc = None
    for x, w, clamp in passes(c, o, mut):
        y = conv(c, x, w, clamp=clamp)
        if check:
            assert torch.equal(conv(c, x, w, torch.float32, clamp).double(), y), "the float32 and float64 host evaluations differ"
        acc = y if acc is None else acc + y
    v = acc + o["bias"].double()
    if check:
        amax = max(float(x.abs().max()) * float(w.abs().max()) for x, w, _ in passes(c, o))
        assert amax <= 144.0
        if c.bias == "int":
            units = 4.0
            bound = (3 * 9 * geometry(c)["cg"] * 144.0 + float(o["bias"].abs().max())) * units
        else:
            # biases with a 2^-10 part: units of 2^-10, and the bound of THESE operands instead of the worst case -- no partial sum of
            # an output, in any order, exceeds |bias| + sum |x| |w| over its terms
            units = 1024.0
            mag = sum(conv(c, x.abs(), w.abs(), clamp=cl) for x, w, cl in passes(c, o)) + o["bias"].abs().double()
            bound = float(mag.max()) * units
        assert bound < LIMIT, "exactness bound: %g units of 1/%d >= 2^24" % (bound, units)
        assert torch.equal(v * units, torch.round(v * units)) and float(v.abs().max()) * units < LIMIT
        assert torch.equal(v.float().double(), v)
    return torch.relu(v)


# -------------------------------------------------------------------------------------------------- what the device reads
def frag16(w):
    """[C][cg][3][3] -> f16 fragments [window][nj 2][tap 9][16][32] through the shipped MX packer (its hi fragments)"""
    from vision_semantic_segmentation_amd.network import pack_gconv_mx, pack_gconv_windows
    frag, _ = pack_gconv_mx(w.double(), G)
    assert torch.equal(frag, pack_gconv_windows(w.double(), G).to(torch.float16))
    return frag.reshape(w.shape[0] // 32, 2, 9, 16, 32)


def _pair1(w):
    """(FP4 fragments [window][nj 2][g 3][lane 64][16], scale bytes [window][lane 64][nj 2][g 3]) of pair 1 = Q4(f16(w)) of pack_gconv_mx(w)"""
    from vision_semantic_segmentation_amd.network import pack_gconv_mx
    nwin = w.shape[0] // 32
    _, bundle = pack_gconv_mx(w.double(), G)
    n4 = nwin * 2 * 2 * 3 * 64 * 16
    w4, w4s = bundle[:n4].reshape(nwin, 2, 2, 3, 64, 16), bundle[n4:].reshape(nwin, 64, 2, 2, 3)
    return w4[:, :, 1], w4s[:, :, :, 1]


def splice_w_mx(wl, whp):
    """w_mx = [window][nj 2][pair 2][g 3][lane 64][16 B] then [window][lane 64][12 B] (byte nj * 6 + pair * 3 + g) with pair 0 = Q4(wl), pair 1 = Q4(whp)"""
    (q0, s0), (q1, s1) = _pair1(wl), _pair1(whp)
    w4 = torch.stack([q0, q1], dim=2)                   # [win][nj][pair][g][lane][16]
    w4s = torch.stack([s0, s1], dim=3)                  # [win][lane][nj][pair][g]
    return torch.cat([w4.reshape(-1), w4s.reshape(-1)]).contiguous()


def _oihw(dense, cg):
    """dense block-diagonal windows [window][co 32][tap 9][ci 32] -> [C][cg][3][3]; asserts the zeros between different groups"""
    nwin = dense.shape[0]
    co = torch.arange(nwin * 32)
    win, col = co // 32, co % 32
    gbase = (col // cg) * cg
    w = torch.stack([dense[win, col, :, gbase + ci] for ci in range(cg)], dim=1)
    assert float(w.abs().sum()) == float(dense.abs().sum())
    return w.reshape(nwin * 32, cg, 3, 3)


def decode_frag(frag, cg):
    """f16 fragments [window][nj 2][tap 9][16][32] -> float64 [C][cg][3][3]"""
    nwin = frag.shape[0]
    dense = torch.zeros((nwin, 32, 9, 32), dtype=torch.float64)
    i = torch.arange(16)
    for nj in range(2):
        dense[:, (i >> 2) * 8 + nj * 4 + (i & 3)] = frag[:, nj].double().permute(0, 2, 1, 3)
    return _oihw(dense, cg)


def decode_w4(w_mx, nwin, cg, pair, scale_from_next_group=False):
    """pair `pair` of a w_mx bundle -> float64 [C][cg][3][3] as the kernel multiplies it: lane kb * 16 + i of scaled MFMA g holds tap
    4 g + kb of output channel (i >> 2) * 8 + nj * 4 + (i & 3), scaled by byte nj * 6 + pair * 3 + g of that lane (or, wrongly, g + 1's)"""
    from vision_semantic_segmentation_amd.network import _FP4_GRID
    n4 = nwin * 2 * 2 * 3 * 64 * 16
    w4, w4s = w_mx[:n4].reshape(nwin, 2, 2, 3, 64, 16), w_mx[n4:].reshape(nwin, 64, 12)
    dense = torch.zeros((nwin, 32, 12, 32), dtype=torch.float64)
    i = torch.arange(16)
    gs = (torch.arange(3) + int(scale_from_next_group)) % 3
    for nj in range(2):
        p = w4[:, nj, pair].to(torch.int64)                                              # [win][g][lane][16]
        code = torch.stack([p & 15, p >> 4], dim=-1).reshape(nwin, 3, 64, 32)
        val = _FP4_GRID[code & 7] * torch.where((code & 8) != 0, -1.0, 1.0)
        sb = w4s[:, :, nj * 6 + pair * 3 + gs].permute(0, 2, 1).double()                 # [win][g][lane]
        val = val * torch.exp2(sb - 127).unsqueeze(-1)
        dense[:, (i >> 2) * 8 + nj * 4 + (i & 3)] = val.reshape(nwin, 3, 4, 16, 32).permute(0, 3, 1, 2, 4).reshape(nwin, 16, 12, 32)
    if not scale_from_next_group:
        assert not bool(dense[:, :, 9:].any())
    return _oihw(dense[:, :, :9].contiguous(), cg)


def in_bundle(c, o):
    """in_mx: [Q4(B) | scales | Q4(C) | scales] over rows_in rows; FILL_BYTE in the rows past the last pixel and in the whole lo half
    when the op does not read it"""
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes, mx_quant_fp4
    g = geometry(c)
    rows, m, hb = g["rows_in"], g["m_in"], mx_bundle_bytes(g["rows_in"], c.C)
    buf = torch.full((2, hb), FILL_BYTE, dtype=torch.uint8)
    for half, key in ((0, "B"), (1, "C")):
        if half == 1 and not c.in_lo:
            continue
        q, s = mx_quant_fp4(o[key].reshape(m, c.C).double())
        buf[half, :rows * (c.C // 2)].view(rows, c.C // 2)[:m] = q
        buf[half, rows * (c.C // 2):].view(c.C // 256, rows, 8)[:, :m] = s
    return buf.reshape(-1)


def decode_in_bundle(c, buf, half, neighbour_scale=False):
    """one half of in_mx -> float64 [B][H][W][C]; neighbour_scale: every window decoded with the scale byte of the window next to it"""
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes, mx_dequant_fp4
    g = geometry(c)
    rows, m = g["rows_in"], g["m_in"]
    b = buf.reshape(2, mx_bundle_bytes(rows, c.C))[half]
    q = b[:rows * (c.C // 2)].view(rows, c.C // 2)[:m]
    s = b[rows * (c.C // 2):].view(c.C // 256, rows, 8)[:, :m]
    if neighbour_scale:
        s = s[:, :, [1, 0, 3, 2, 5, 4, 7, 6]]
    return mx_dequant_fp4(q, s).reshape(c.B, c.H, c.W, c.C)


@functools.lru_cache(maxsize=3)
def _device_inputs(shape, ws, third, bias_kind):
    c = Case(ws, ws == 1 and third, ws == 2 and third, "single", *shape, 1, 1, 0, 0, bias_kind)
    o = ops_of(c)
    g = geometry(c)
    f16 = torch.float16
    planes = torch.full((2, g["rows_in"], c.C), float("nan"), dtype=f16)               # rows past the last pixel are never read
    planes[0, :g["m_in"]] = o["A"].reshape(-1, c.C).to(f16)
    if c.xs:
        planes[1, :g["m_in"]] = o["B"].reshape(-1, c.C).to(f16)
    d = {"planes": planes, "bias": o["bias"].clone()}
    if ws == 2:
        d["weight"] = frag16(o["W0"]).reshape(-1).contiguous()
        d["w_mx"] = splice_w_mx(o["W1"], o["W2"])
        d["in_mx"] = in_bundle(c, o)
        w4s = d["w_mx"][-g["nwin"] * 64 * 12:].reshape(g["nwin"], 64, 2, 2, 3)
        assert all(len(torch.unique(w4s[:, :, :, pair])) >= 3 for pair in range(2)), "fewer than three distinct scale bytes in a pair of w_mx"
        assert all(len(torch.unique(s)) >= 3 for s in decode_scale_bytes(c, d["in_mx"])), "fewer than three distinct scale bytes in in_mx"
        # ... and they tell neighbours apart: the two windows of a pair / the tap groups of a row differ somewhere
        assert all(bool((s[:, :, 0::2] != s[:, :, 1::2]).any()) for s in decode_scale_bytes(c, d["in_mx"]))
        assert bool((w4s[..., 0] != w4s[..., 1]).any()) and bool((w4s[..., 1] != w4s[..., 2]).any())
    else:
        d["weight"] = torch.cat([frag16(o["W0"]), frag16(o["W1"])], dim=2).reshape(-1).contiguous()      # [window][nj][9 W1 | 9 W2][16][32]
    return d


def decode_scale_bytes(c, buf):
    """the live scale bytes of the halves of in_mx the op reads"""
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes
    g = geometry(c)
    rows = g["rows_in"]
    b = buf.reshape(2, mx_bundle_bytes(rows, c.C))
    return [b[h, rows * (c.C // 2):].view(c.C // 256, rows, 8)[:, :g["m_in"]] for h in range(2 if c.in_lo else 1)]


def device_inputs(c):
    """{"planes": f16 [2][rows_in][C] (plane 1 = in_lo, NaN where unused), "weight": f16 fragments, "bias", "w_mx", "in_mx"}"""
    return _device_inputs((c.B, c.H, c.W, c.C), c.ws, bool(c.in_lo or c.xs), c.bias)


def decoded_operands(c, mut=None):
    """the operand set as decoded from what the device reads (device_inputs); mut: "neighbour_window_scale" | "weight_scale_next_group" """
    d = device_inputs(c)
    g = geometry(c)
    A = d["planes"][0, :g["m_in"]].double().reshape(c.B, c.H, c.W, c.C)
    o = {"A": A, "bias": d["bias"]}
    if c.ws == 2:
        o["W0"] = decode_frag(d["weight"].reshape(g["nwin"], 2, 9, 16, 32), g["cg"])
        o["W1"] = decode_w4(d["w_mx"], g["nwin"], g["cg"], 0, mut == "weight_scale_next_group")
        o["W2"] = decode_w4(d["w_mx"], g["nwin"], g["cg"], 1, mut == "weight_scale_next_group")
        o["B"] = decode_in_bundle(c, d["in_mx"], 0, mut == "neighbour_window_scale")
        o["C"] = decode_in_bundle(c, d["in_mx"], 1, mut == "neighbour_window_scale") if c.in_lo else None
    else:
        fr = d["weight"].reshape(g["nwin"], 2, 18, 16, 32)
        o["W0"], o["W1"], o["W2"] = decode_frag(fr[:, :, :9], g["cg"]), decode_frag(fr[:, :, 9:], g["cg"]), None
        o["B"] = d["planes"][1, :g["m_in"]].double().reshape(c.B, c.H, c.W, c.C) if c.xs else None
        o["C"] = None
    return o


# ----------------------------------------------------------------------------------------------------- expected buffers
def ties(v, hi):
    """(exact ties rounded down in magnitude, up in magnitude): v midway between hi and hi's f16 neighbour on v's side"""
    vn, hn = v.numpy(), hi.numpy()
    other = np.nextafter(hn, np.where(vn > hn.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)).astype(np.float64)
    h64 = hn.astype(np.float64)
    tie = (vn != h64) & (np.abs(vn - h64) == np.abs(other - vn))
    return int((tie & (np.abs(h64) < np.abs(vn))).sum()), int((tie & (np.abs(h64) > np.abs(vn))).sum())


def stored(c, v, truncate=False, lo_source_swapped=False, last_row_past_m=False):
    """every byte the op may touch: {"out", "out_lo": f16 [rows][C], "out_mx": uint8 [2][half bundle]}.  Wrong variants: the hi plane
    truncated; Q4(lo) quantised from the other source (fp32 <-> the f16 plane); the last output row written again to the rows past M"""
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes, mx_quant_fp4
    g = geometry(c)
    rows, m, C = g["rows"], g["m"], c.C
    f16 = torch.float16
    hi = X.round_toward_zero(v, "f16") if truncate else v.to(f16)
    assert bool(torch.isfinite(hi).all())
    lo32 = v - hi.double()
    assert torch.equal(lo32.float().double(), lo32)
    lo16 = lo32.to(f16)
    extra = min(g["ow"], rows - m) if last_row_past_m else 0
    src = torch.arange(m).tolist() + list(range(m - g["ow"], m - g["ow"] + extra))

    def put(buf, t):
        buf[:m + extra] = t[src]
    out = torch.full((rows, C), FILL, dtype=f16)
    out_lo = torch.full((rows, C), FILL, dtype=f16)
    mx = torch.full((2, mx_bundle_bytes(rows, C) if C % 256 == 0 else 0), FILL_BYTE, dtype=torch.uint8)
    put(out, hi)
    if has_lo(c):
        put(out_lo, lo16)
    if has_mx(c):
        lo_q = lo16.double() if has_lo(c) != lo_source_swapped else lo32
        for half, t in ((0, hi.double()), (1, lo_q)):
            q, s = mx_quant_fp4(t)
            put(mx[half, :rows * (C // 2)].view(rows, C // 2), q)
            sl = mx[half, rows * (C // 2):].view(C // 256, rows, 8)
            sl[:, :m + extra] = s[:, src]
    return {"out": out, "out_lo": out_lo, "out_mx": mx}


@functools.lru_cache(maxsize=2)
def want(c):
    """(v, expected buffers) from the ORIGINAL matrices; asserts every condition of the module docstring"""
    o = ops_of(c)
    v = exact_v(c, o, check=True)
    hi = v.to(torch.float16)
    share = float((hi.double() != v).double().mean())
    assert share >= 0.2, "only %.1f %% of the expected hi values round" % (100 * share)
    down, up = ties(v, hi)
    assert down > 0 and up > 0, "exact ties rounding down %d, up %d" % (down, up)
    lo_share = float(((v - hi.double()) != 0).double().mean())
    assert lo_share >= 0.1, "the lo part is non-zero in only %.1f %%" % (100 * lo_share)
    assert bool((v == 0).all(dim=0).any()), "no column clamps to zero as a whole"
    return v, stored(c, v)


def same(a, b):
    return all(torch.equal(a[k].view(torch.int16) if a[k].dtype == torch.float16 else a[k], b[k].view(torch.int16) if b[k].dtype == torch.float16 else b[k])
               for k in ("out", "out_lo", "out_mx"))


MUTATIONS = PASS_MUTATIONS + ("neighbour_window_scale", "weight_scale_next_group", "truncate", "lo_source", "last_row_past_m")
def invisible(c, mut):
    """shown to leave every byte as it is: the source of Q4(lo) on integer biases (module docstring; FRAC_CASES make it visible)"""
    return mut == "lo_source" and c.bias == "int"


def applicable(c, mut):
    if mut in ("drop_lo_pass", "second_weights_with_lo_input"):
        return bool(c.in_lo or c.xs)
    if mut in ("neighbour_window_scale", "weight_scale_next_group"):
        return c.ws == 2
    if mut == "lo_source":
        return has_mx(c)
    return True


def evaluate(c, mut=None):
    """the buffers a host evaluation of WHAT THE DEVICE READS leaves (the decoded fragments, bundles and planes), optionally subtly wrong"""
    o = decoded_operands(c, mut if mut in ("neighbour_window_scale", "weight_scale_next_group") else None)
    v = exact_v(c, o, mut if mut in PASS_MUTATIONS else None)
    return stored(c, v, truncate=mut == "truncate", lo_source_swapped=mut == "lo_source", last_row_past_m=mut == "last_row_past_m")


# -------------------------------------------------------------------------------------------------------------- the op
def make_op(c, ptr):
    """the case's op; ptr: {"in", "in_lo", "weight", "bias", "out", "out_lo", "w_mx", "in_mx", "out_mx"} -> address (only those the form sets are read)"""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AVL_MX_IN_LO, AVL_MX_OUT_LO, OP_GCONV, AvlSegOp
    g = geometry(c)
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = OP_GCONV, _lib.AVL_F16, c.B if c.B > 1 else 0
    op.in_, op.out, op.weight, op.bias = ptr["in"], ptr["out"], ptr["weight"], ptr["bias"]
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = c.H, c.W, c.C, c.C, g["rows_in"]
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = g["oh"], g["ow"], c.C, c.C, g["rows"]
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu, op.w_layout, op.w_split = 3, c.s, c.d, c.d, G, 1, 1, c.ws
    if c.xs:
        op.in_lo = ptr["in_lo"]
    if has_lo(c):
        op.out_lo = ptr["out_lo"]
    if has_mx(c):
        op.out_mx = ptr["out_mx"]
    flags = 0
    if c.ws == 2:
        op.w_mx, op.in_mx = ptr["w_mx"], ptr["in_mx"]
        flags |= AVL_MX_IN_LO if c.in_lo else 0
    if c.form == "mx_f32lo":
        flags |= AVL_MX_OUT_LO
    op.mx_flags = flags
    return op


def shape_op(c, ptr=16):
    """the op with one placeholder address everywhere: what the library's validation looks at (no GPU)"""
    return make_op(c, collections.defaultdict(lambda: ptr))
