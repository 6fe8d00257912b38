"""Exactly computable cases for layer2's fused identity Bottleneck, k_bottleneck_w256 (AVL_OP_BOTTLENECK with in_c = 512), shared by
test_bottleneck2_operands_cpu.py (operand conditions, the dispatch claim and the teeth of the comparison, without a GPU) and
test_gpu_bottleneck2_exact.py (which runs the op and compares every buffer for equality).  The pattern, and most helpers, are those of
_fused_mixed_operands.py (layer1's k_bottleneck<...>).

WHAT THE KERNEL COMPUTES (read from csrc/seg_bottleneck.hip; the expected values mirror exactly this).  Width 256, 32 groups of 8,
512 -> 512 channels, trunk in and out in the MX form.  blockIdx.z selects the image (row0 = z H W in every plane and bundle); a tile is
4 x 16 output pixels with a 6 x 18 halo.
    conv1     t1 = relu(b1 + sum W1h x_hi + W1l x_hi) over 512 channels in eight 64-channel slabs; x_lo never enters; stored as ONE f16
              plane, zero outside the image (and on the halo rows >= 108)
    conv2     t2 = relu(b2 + sum W2h t1 + W2l t1): block-diagonal 16-channel windows, five K-steps of two taps; the tenth tap slot
              re-reads tap 8 with the zero weights pack_bottleneck puts there; always split hi = f16(t2), lo = f16(t2 - hi)
    conv3     v = b3 + sum W3h t2h + W3l t2h + W3h t2l (W3l t2l is never formed)
    residual  v += (float)x_hi + dec(x_lo): the FP4 lo half of in_mx with its E8M0 byte, scale slabs [K / 256][in_rows][8]
    output    y = relu(v), out = f16(y), lo32 = y - out in fp32; Q4(hi) = FP4 of out, Q4(lo) = FP4 of lo32 (NOT of an f16 rounding of
              it), one scale byte per 32 channels; bundle [Q4(hi) | scales | Q4(lo) | scales] over out_rows rows; pixels outside the
              image store nothing
    overflow  a stored t1 value >= 0x7c00 at an in-image halo pixel of a tile sets the exponent bits of every f16 of that tile's hi plane
              (one LDS word, cleared at slab 0 of every tile, set before barrier B2): overflow_inputs / flagged_tiles below

OPERANDS.  x_hi: small integers (_exact_operands.ints).  W1h, W1l: INDEPENDENT sparse matrices in {0, +-1}, spliced through two calls
of pack_bottleneck (splice_fragments), as are W2h / W2l and W3h / W3l (hi: small integers, lo: +-{1/2, 1}).  t1 is an integer below
2048: its single f16 plane is exact (asserted).  A quarter of the t2 channels (the eight groups g % 4 == 1) carry a bias in 2048 ..
4000, which populates the in-LDS t2l tile; conv3's weights on those channels are sparse and within +-1 so that every output stays
below 65504.  Two output columns carry a bias of -200000 and clamp to zero as a whole.  x_lo is an INDEPENDENT tensor on the FP4 grid
(no remainder of x_hi): every 32-block has the scale 2^-2, 2^-1 or 1 (bytes 125, 126, 127, drawn per pixel and block) and holds one
element of magnitude 4 or 6 in that scale, so mx_quant_fp4 -> mx_dequant_fp4 is the identity (asserted); it reaches the device as the lo
half of in_mx.  The hi half of in_mx, which the kernel does not read, holds 0x77 / 0x8C (6 x 2^13 everywhere); the rows past B H W hold
NaN in the f16 plane and the byte 0x7A in the bundle.

EXACTNESS.  Every term of every stage is a multiple of 1/8 and sum|term| + |bias| + |residual| stays below 2^24 units at every stage,
so fp32 accumulation is exact in any order; asserted per case and stage on the operands' own sum of |x| |w|, together with float32
evaluation == float64 evaluation of every pass.

CONDITIONS asserted on the expected buffers of every shape but 1 x 1: >= 20 % of the output hi values are not representable before
rounding; exact ties round down to even and up to even in the output split and in the t2 split; t2l is non-zero on >= 10 % of its live
elements (the channels beyond 2048); lo32 is non-zero on >= 10 %; each output scale slab holds >= 3 distinct bytes and neighbouring
blocks differ; >= 10 % of the Q4(lo) bytes are non-zero; at least one output column clamps to zero as a whole.

THE SOURCE OF Q4(lo).  With every term a multiple of 1/8 and y < 65504, lo32 = y - f16(y) is a multiple of 1/8 of magnitude <= 16: an
f16 value.  Quantising f16(lo32) instead of lo32 then gives the same bytes, and the mutation "q4lo_from_f16" is shown NOT to be visible
on the cases of the table (invisible()).  As _gconv_mixed_operands.FRAC_CASES do for the grouped conv, one more case (frac) gives a
third of the output columns a bias in 8192 .. 11000 with a 2^-10 part and at most three conv3 weights within +-1 on t2 channels below
2048: on those columns every partial sum is a multiple of 2^-10 below 2^14 (asserted on the operands' own sum of |x| |w|), still exact
in fp32 in any order; lo32 then has up to twelve significant bits and the two sources differ in FP4 bytes.

EXPECTED BUFFERS, compared whole: out f16 [rows][512] around the fill 7.0, out_mx uint8 [2][half bundle] around 0xA5, byte for byte
what mx_quant_fp4 gives for out and for lo32; rows = up(B H W + 1, 256), so the scale slabs' stride differs from B H W and the rows
past the last pixel keep their fill.  No expected value mirrors an instruction's behaviour beyond what is stated here."""
import collections
import functools

import torch
import torch.nn.functional as F

import _exact_operands as X
from _fused_mixed_operands import (FILL, LIMIT, _big_bias, _conditions, _exact_split, _mm, _pick, _round, _scatter_rows, _split, _up, f16, f64,
                                   same, splice_fragments)
from _gconv_mixed_operands import ties

FILL_BYTE, IN_FILL_BYTE, IN_HI_Q, IN_HI_S = 0xA5, 0x7A, 0x77, 0x8C
CIN, WIDTH, COUT, GROUPS = 512, 256, 512, 32
CG = WIDTH // GROUPS
TH, TW = 4, 16
KERNEL = "k_bottleneck_w256"
EDGE_COL, EDGE_VALUE = 70, 13313.0

B2Case = collections.namedtuple("B2Case", "B H W frac", defaults=(False,))
MANY = (270, 240)                                              # 68 x 15 = 1020 tiles: four per workgroup on 256 CUs
CASES = [B2Case(1, 1, 1), B2Case(1, 4, 16), B2Case(1, 5, 17), B2Case(1, 70, 5), B2Case(1, 3, 200), B2Case(1, 23, 45), B2Case(2, 23, 45),
         B2Case(1, *MANY), B2Case(1, 5, 17, True)]


def case_id(c):
    return "b%d-%dx%d%s" % (c.B, c.H, c.W, "-frac" if c.frac else "")


def dispatch(in_c):
    """launch_bottleneck's first branch, restated"""
    return KERNEL if in_c == CIN else "k_bottleneck<...>"


def geometry(c, cus=256):
    m = c.H * c.W
    tx, ty = (c.W + TW - 1) // TW, (c.H + TH - 1) // TH
    grid = min(tx * ty, cus)
    return dict(m=m, bm=c.B * m, rows=_up(c.B * m + 1, 256), tiles_x=tx, tiles_y=ty, tiles=tx * ty, tpw=-(-tx * ty // grid))


def _bound(mag, what, unit=0.125):
    assert float(mag.max()) / unit < LIMIT, "%s: exactness bound %g units of %g >= 2^24" % (what, float(mag.max()) / unit, unit)


def _unit(v, what, unit=0.125):
    assert torch.equal(torch.round(v / unit) * unit, v), "%s is not a multiple of %g" % (what, unit)


def _xlo(g, bm):
    """float32 [bm][512] on the FP4 grid: per 32-block a scale 2^k, k in {-2, -1, 0}, grid values in that scale, one element of magnitude 4 or 6"""
    k = -torch.randint(0, 3, (bm, CIN // 32, 1), generator=g).float()
    v = _pick(g, (bm, CIN // 32, 32), [0, 0.5, -0.5, 1, -1, 1.5, -1.5, 2, -2, 3, -3, 4, -4, 6, -6, 1])
    top = torch.randint(0, 32, (bm, CIN // 32, 1), generator=g) == torch.arange(32).view(1, 1, 32)
    v = torch.where(top, _pick(g, (bm, CIN // 32, 1), [4, -4, 6, -6]).expand(-1, -1, 32), v)
    return (v * torch.exp2(k)).reshape(bm, CIN)


@functools.lru_cache(maxsize=2)
def operands(c):
    from vision_semantic_segmentation_amd.network import mx_dequant_fp4, mx_quant_fp4
    bm = c.B * c.H * c.W
    s = X._seed(CIN, c.B, c.H, c.W, int(c.frac), 2)
    g = torch.Generator().manual_seed(s)
    o = {"xh": X.ints(s, bm, CIN), "xl": _xlo(g, bm)}
    o["xq"], o["xs"] = mx_quant_fp4(o["xl"].double())
    assert torch.equal(mx_dequant_fp4(o["xq"], o["xs"]), o["xl"].double()), "x_lo does not survive mx_quant_fp4 -> mx_dequant_fp4"
    bigg = torch.arange(GROUPS)[torch.arange(GROUPS) % 4 == 1]
    big2 = (bigg.view(-1, 1) * CG + torch.arange(CG)).reshape(-1)                # the 64 t2 channels with a bias beyond 2048
    o["W1h"] = _pick(g, (WIDTH, CIN), [0, 0, 0, 0, 0, 0, 1, -1])
    o["W1l"] = _pick(g, (WIDTH, CIN), [0, 0, 0, 0, 0, 0, 1, -1])
    o["b1"] = torch.randint(-10, 11, (WIDTH,), generator=g).float()
    o["W2h"] = _pick(g, (WIDTH, CG, 9), [0, 0, 0, 0, 0, 1, -1, 2, -2, 1, -1]).reshape(WIDTH, CG, 3, 3)
    o["W2l"] = _pick(g, (WIDTH, CG, 9), [0, 0, 0, 0.5, -0.5, 1, -1]).reshape(WIDTH, CG, 3, 3)
    b2 = torch.randint(-20, 21, (WIDTH,), generator=g).float()
    b2[big2] = torch.randint(2048, 4000, (len(big2),), generator=g).float()
    o["b2"] = b2
    w3h = _scatter_rows(g, _pick(g, (COUT, WIDTH), [0, 0, 0, 0, 0, 1, -1, 1, -1, 2, -2]), big2, 3, [1.0, -1.0])
    w3l = _scatter_rows(g, _pick(g, (COUT, WIDTH), [0, 0, 0, 0, 0.5, -0.5, 1, -1]), big2, 1, [0.5, -0.5])
    b3 = _big_bias(g, COUT, 0.6, hi=4000)
    blk = torch.arange(COUT) // 32                                                # per 32-block, so that the scale bytes of Q4(hi) spread:
    b3 = torch.where((blk % 4 == 3) & (b3 >= 2048), b3 + 12000.0, b3)             # ... larger outputs
    b3 = torch.where(blk % 8 == 2, torch.randint(-40, 41, (COUT,), generator=g).float() - 9000.0, b3)     # ... mostly clamped, some blocks all zero
    b3 = torch.where(blk % 8 == 6, torch.randint(-40, 41, (COUT,), generator=g).float(), b3)              # ... sums alone
    zero = torch.tensor([7, 333])
    b3[zero] = -200000.0                                                          # these columns clamp to zero as a whole
    b3[EDGE_COL] = 0.0
    fcols = torch.zeros(COUT, dtype=torch.bool)
    if c.frac:
        fcols[2::3] = True
        fcols[zero] = False
        small = torch.nonzero(~torch.isin(torch.arange(WIDTH), big2)).reshape(-1)
        nf = int(fcols.sum())
        w3h[fcols] = _scatter_rows(g, torch.zeros(nf, WIDTH), small, 2, [1.0, -1.0])
        w3l[fcols] = _scatter_rows(g, torch.zeros(nf, WIDTH), small, 1, [0.5, -0.5])
        b3[fcols] = (torch.randint(8192, 11000, (nf,), generator=g).double() + torch.randint(1, 1024, (nf,), generator=g).double() / 1024).float()
    o["W3h"], o["W3l"], o["b3"], o["big2"], o["zero"], o["fcols"] = w3h, w3l, b3, big2, zero, fcols
    # pixel 0, column EDGE_COL (a block whose other outputs are mostly clamped): y = 13313 = 1.625 x 2^13 + 1, which f16 rounds to 13312.  The
    # block's scale byte is one higher from y than from out (the quantiser's "> 1.625" test), in every case: Q4(hi) quantised from y shows.
    # Pixel 0 depends on the image's first 2 x 2 pixels only.
    hh, ww = min(c.H, 2), min(c.W, 2)
    idx = (torch.arange(hh).view(-1, 1) * c.W + torch.arange(ww)).reshape(-1)
    crop = dict(o, xh=o["xh"][idx], xq=o["xq"][idx], xs=o["xs"][:, idx].contiguous())
    b3[EDGE_COL] = float(EDGE_VALUE - exact(B2Case(1, hh, ww), crop)["v"][0, EDGE_COL])
    return o


MUTATIONS = ("c1_drop_lo", "c2_drop_lo", "c3_drop_pass_0", "c3_drop_pass_1", "c3_drop_pass_2", "c3_double_pass", "c3_add_wl_tl", "swap_slots",
             "tap8_twice", "tap8_missing", "t1_not_zeroed", "t2_truncate", "t2_half_away", "out_truncate", "out_half_away", "drop_res_lo",
             "res_neighbour_scale", "res_after_relu", "q4lo_from_f16", "q4hi_from_y", "in_scale_stride", "out_scale_stride", "row_past_m",
             "batch_halo")


def applicable(c, mut):
    if mut in ("tap8_twice", "tap8_missing"):
        return c.H > 1 and c.W > 1                             # (tap 8 is the pixel below and to the right)
    return c.B > 1 if mut == "batch_halo" else True


def invisible(c, mut):
    """shown to leave every byte as it is: the source of Q4(lo) where every term is a multiple of 1/8 (module docstring; the frac case
    makes it visible)"""
    return mut == "q4lo_from_f16" and not c.frac


def in_bundle(c, o):
    """in_mx as the device reads it: uint8 [2][half]; half 0 (never read) a pattern that decodes to 6 x 2^13, half 1 = x_lo, fill past B H W"""
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes
    g = geometry(c)
    rows, bm = g["rows"], g["bm"]
    mx = torch.full((2, mx_bundle_bytes(rows, CIN)), IN_FILL_BYTE, dtype=torch.uint8)
    mx[0, :rows * (CIN // 2)] = IN_HI_Q
    mx[0, rows * (CIN // 2):] = IN_HI_S
    mx[1, :rows * (CIN // 2)].view(rows, CIN // 2)[:bm] = o["xq"]
    mx[1, rows * (CIN // 2):].view(CIN // 256, rows, 8)[:, :bm] = o["xs"]
    return mx


def _residual_lo(c, o, mut):
    """dec(x_lo) float64 [bm][512] as the kernel decodes it from in_mx (or subtly wrong)"""
    from vision_semantic_segmentation_amd.network import mx_dequant_fp4
    g = geometry(c)
    rows, bm = g["rows"], g["bm"]
    if mut == "drop_res_lo":
        return torch.zeros((bm, CIN), dtype=f64)
    if mut == "res_neighbour_scale":                           # block j decoded with the byte of block j + 1 of its slab
        return mx_dequant_fp4(o["xq"], torch.roll(o["xs"], -1, dims=2))
    if mut == "in_scale_stride":                               # the slabs addressed as [K / 256][B H W][8] inside the [K / 256][rows][8] area
        flat = in_bundle(c, o)[1, rows * (CIN // 2):]
        idx = (torch.arange(CIN // 256).view(-1, 1, 1) * bm + torch.arange(bm).view(1, -1, 1)) * 8 + torch.arange(8).view(1, 1, -1)
        return mx_dequant_fp4(o["xq"], flat[idx])
    return mx_dequant_fp4(o["xq"], o["xs"])


def exact(c, o, mut=None, check=False):
    """-> dict(t1, t2, t2l, y): the exact values of every stage (float64 [B H W][channels]), optionally subtly wrong (MUTATIONS)"""
    B, H, W = c.B, c.H, c.W
    w = {k: o[k].double() for k in ("W1h", "W1l", "W2h", "W2l", "W3h", "W3l")}
    if mut == "swap_slots":
        w = {k[:-1] + ("l" if k[-1] == "h" else "h"): v for k, v in w.items()}
    if mut in ("tap8_missing", "tap8_twice"):                  # (twice: the tenth tap slot, which re-reads tap 8, with tap 8's weights instead of zeros)
        for k in ("W2h", "W2l"):
            w[k] = w[k].clone()
            w[k][:, :, 2, 2] *= 0 if mut == "tap8_missing" else 2
    x = o["xh"].double()
    # ---- conv1
    p1 = [w["W1h"]] + ([] if mut == "c1_drop_lo" else [w["W1l"]])
    t1 = torch.relu(o["b1"].double() + sum(_mm(x, m, check, "conv1") for m in p1))
    if check:
        _bound(sum(x.abs() @ m.abs().t() for m in p1) + o["b1"].abs().double(), "conv1")
        assert float(t1.max()) < 2048 and torch.equal(t1.to(f16).double(), t1) and torch.equal(torch.round(t1), t1), "t1 must be an f16 integer below 2048"
    t1 = t1.to(f16).double()                                   # ONE f16 plane

    def conv2(t, m, dtype=f64):
        tn = t.reshape(B, H, W, WIDTH).permute(0, 3, 1, 2).to(dtype)
        pad = 1
        if mut == "batch_halo":                                # the images stacked: image 1's top halo reads image 0's last row
            tn = tn.permute(1, 0, 2, 3).reshape(1, WIDTH, B * H, W)
        if mut == "t1_not_zeroed":                             # conv1 of the clamped pixel, which is what the X slabs hold there
            tn, pad = F.pad(tn, (1, 1, 1, 1), mode="replicate"), 0
        y = F.conv2d(tn, m.to(dtype), None, padding=pad, groups=GROUPS)
        if mut == "batch_halo":
            y = y.reshape(WIDTH, B, H, W).permute(1, 0, 2, 3)
        return y.permute(0, 2, 3, 1).reshape(-1, WIDTH)
    p2 = [w["W2h"]] + ([] if mut == "c2_drop_lo" else [w["W2l"]])
    t2 = torch.relu(o["b2"].double() + sum(conv2(t1, m) for m in p2))
    if check:
        for m in p2:
            assert torch.equal(conv2(t1, m, torch.float32).double(), conv2(t1, m)), "conv2: the float32 and float64 host evaluations differ"
        _bound(sum(conv2(t1, m.abs()) for m in p2) + o["b2"].abs().double(), "conv2")
        _unit(t2, "t2")
        _exact_split(t2, "t2")
    t2h, t2l = _split(t2, {"t2_truncate": "truncate", "t2_half_away": "half_away"}.get(mut))
    # ---- conv3 + residual
    p3 = [(t2h, w["W3h"]), (t2h, w["W3l"]), (t2l, w["W3h"])]
    if mut is not None and mut.startswith("c3_drop_pass_"):
        del p3[int(mut[-1])]
    elif mut == "c3_double_pass":
        p3.append(p3[1])
    elif mut == "c3_add_wl_tl":
        p3.append((t2l, w["W3l"]))
    res = x + _residual_lo(c, o, mut)
    v = o["b3"].double() + sum(_mm(t, m, check, "conv3") for t, m in p3)
    if check:
        mag = sum(t.abs() @ m.abs().t() for t, m in p3) + o["b3"].abs().double() + res.abs()
        fc = o["fcols"]
        _bound(mag[:, ~fc], "conv3")
        _unit((v + res)[:, ~fc], "the output")
        if bool(fc.any()):
            _bound(mag[:, fc], "conv3 on the columns with a 2^-10 bias", 2.0 ** -10)
            _unit((v + res)[:, fc], "the output on the columns with a 2^-10 bias", 2.0 ** -10)
        assert torch.equal((v.float() + res.float()).double(), v + res)
    y = torch.relu(v) + res if mut == "res_after_relu" else torch.relu(v + res)
    return {"t1": t1, "t2": t2, "t2l": t2l, "v": v + res, "y": y}


def _put_scales(c, slab, s, n, src, stride):
    """scale bytes s [2][bm][8] of rows src -> rows 0 .. n - 1 of the flat slab area, the slabs `stride` rows apart"""
    idx = (torch.arange(COUT // 256).view(-1, 1, 1) * stride + torch.arange(n).view(1, -1, 1)) * 8 + torch.arange(8).view(1, 1, -1)
    slab[idx.reshape(-1)] = s[:, src].reshape(-1)


def stored(c, r, mut=None):
    """every byte the op may touch, around its fill: {"out": f16 [rows][512], "out_mx": uint8 [2][half bundle]}"""
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes, mx_quant_fp4
    g = geometry(c)
    rows, bm = g["rows"], g["bm"]
    y = r["y"]
    hi = _round(y, {"out_truncate": "truncate", "out_half_away": "half_away"}.get(mut))
    assert mut is not None or bool(torch.isfinite(hi).all()), "an expected output overflows f16"
    lo32 = y - hi.double()
    assert mut is not None or torch.equal(lo32.float().double(), lo32), "lo32 is no fp32 value"
    n = bm + (1 if mut == "row_past_m" else 0)
    src = torch.arange(n).clamp_max(bm - 1)
    out = torch.full((rows, COUT), FILL, dtype=f16)
    out[:n] = hi[src]
    mx = torch.full((2, mx_bundle_bytes(rows, COUT)), FILL_BYTE, dtype=torch.uint8)
    parts = (y if mut == "q4hi_from_y" else hi.double(), lo32.to(f16).double() if mut == "q4lo_from_f16" else lo32)
    for half, t in enumerate(parts):
        q, s = mx_quant_fp4(t)
        mx[half, :rows * (COUT // 2)].view(rows, COUT // 2)[:n] = q[src]
        _put_scales(c, mx[half, rows * (COUT // 2):], s, n, src, bm if mut == "out_scale_stride" else rows)
    return {"out": out, "out_mx": mx}


def evaluate(c, mut=None):
    return stored(c, exact(c, operands(c), mut), mut)


def unbundle(c, mx, half):
    """(FP4 plane [rows][256], scale slabs [2][rows][8]) of one half of an output bundle"""
    rows = geometry(c)["rows"]
    return mx[half, :rows * (COUT // 2)].view(rows, COUT // 2), mx[half, rows * (COUT // 2):].view(COUT // 256, rows, 8)


@functools.lru_cache(maxsize=3)
def want(c):
    """(exact stages, expected buffers); asserts every condition of the module docstring"""
    o = operands(c)
    r = exact(c, o, check=True)
    bufs = stored(c, r)
    bm = geometry(c)["bm"]
    y = r["y"]
    hi = y.to(f16).double()
    lo32 = y - hi
    assert bool((y[:, o["zero"]] == 0).all()), "no column clamps to zero as a whole"
    eb = EDGE_COL // 32 * 32
    assert float(y[0, EDGE_COL]) == EDGE_VALUE and float(hi[0, EDGE_COL]) == EDGE_VALUE - 1 and float(y[0, eb:eb + 32].max()) == EDGE_VALUE
    if not c.frac:
        assert torch.equal(lo32.to(f16).double(), lo32)        # (why "q4lo_from_f16" is invisible here)
    if bm < 64:                                                # the 1 x 1 image: 512 outputs cannot hold every kind of tie
        assert bool((hi != y).any()) and bool((r["t2l"] != 0).any())
        return r, bufs
    r["mid2"] = _conditions(r["t2"][:, o["big2"]], "t2 on its channels beyond 2048", hi_share=False)
    share = float((r["t2l"][:, o["big2"]] != 0).double().mean())
    assert share >= 0.1, "t2's lo tile is non-zero on only %.1f %% of its live elements" % (100 * share)
    share, (down, up), lo_share = float((hi != y).double().mean()), ties(y, hi.to(f16)), float((lo32 != 0).double().mean())
    assert share >= 0.2, "only %.1f %% of the output hi values round" % (100 * share)
    assert down > 0 and up > 0, "the output: exact ties rounding down %d, up %d" % (down, up)
    assert lo_share >= 0.1, "lo32 is non-zero in only %.1f %%" % (100 * lo_share)
    r["out"] = (share, down, up, lo_share)
    for half in (0, 1):
        q, s = unbundle(c, bufs["out_mx"], half)
        live = s[:, :bm]
        assert len(torch.unique(live)) >= 3, "half %d: fewer than three distinct scale bytes" % half
        assert bool((live[:, :, 1:] != live[:, :, :-1]).any()) and bool((live[:, 1:] != live[:, :-1]).any()), "half %d: neighbouring blocks never differ" % half
        if half:
            qs = float((q[:bm] != 0).double().mean())
            assert qs >= 0.1, "only %.1f %% of the Q4(lo) bytes are non-zero" % (100 * qs)
    return r, bufs


def weights(c):
    """(p1, p2, p3): pack_bottleneck's three outputs with INDEPENDENT hi and lo fragments"""
    from vision_semantic_segmentation_amd.network import pack_bottleneck
    o = operands(c)
    hi = pack_bottleneck(o["W1h"].double(), o["W2h"].double(), o["W3h"].double(), None, GROUPS)
    lo = pack_bottleneck(o["W1l"].double(), o["W2l"].double(), o["W3l"].double(), None, GROUPS)
    return tuple(splice_fragments(a, b) for a, b in zip(hi, lo))


def device_inputs(c):
    """{"x": f16 [rows][512] (NaN past the last pixel), "in_mx": uint8 [2][half], "p1", "p2", "p3", "bias": b1 | b2 | b3}"""
    o, g = operands(c), geometry(c)
    x = torch.full((g["rows"], CIN), float("nan"), dtype=f16)
    x[:g["bm"]] = o["xh"].to(f16)
    p1, p2, p3 = weights(c)
    return {"x": x, "in_mx": in_bundle(c, o), "p1": p1, "p2": p2, "p3": p3, "bias": torch.cat([o["b1"], o["b2"], o["b3"]])}


def make_op(c, ptr):
    """ptr: {"in", "in_mx", "p1", "p2", "p3", "bias", "out", "out_mx"} -> address of element 0 of each buffer"""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AVL_MX_IN_LO, AVL_MX_OUT_LO, OP_BOTTLENECK, AvlSegOp
    g = geometry(c)
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = OP_BOTTLENECK, _lib.AVL_F16, c.B if c.B > 1 else 0
    op.in_, op.out, op.in_mx, op.out_mx, op.mx_flags = ptr["in"], ptr["out"], ptr["in_mx"], ptr["out_mx"], AVL_MX_IN_LO | AVL_MX_OUT_LO
    op.weight, op.in2, op.in3, op.in3_c, op.bias = ptr["p1"], ptr["p2"], ptr["p3"], WIDTH, ptr["bias"]
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = c.H, c.W, CIN, CIN, g["rows"]
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = c.H, c.W, COUT, COUT, g["rows"]
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu = 3, 1, 1, 1, GROUPS, 1
    op.w_layout, op.w_split = 0, 0
    return op


# ------------------------------------------------------------------------------------------------------------------ overflow
def overflow_pixel(c):
    """(image, y, x): the corner where four tiles meet, in the second half of the image's tiles"""
    g = geometry(c)
    return c.B - 1, TH * (g["tiles_y"] // 2), TW * (g["tiles_x"] // 2)


def overflow_inputs(c):
    """device_inputs with x_hi of ONE pixel = 2048 sign(W1h + W1l)[channel 0]: t1 of channel 0 there is 2048 sum|W1h + W1l| > 65504"""
    o, d = operands(c), device_inputs(c)
    n, py, px = overflow_pixel(c)
    wsum = o["W1h"][0].double() + o["W1l"][0].double()
    x = 2048.0 * torch.sign(wsum)
    t1 = float(o["b1"][0]) + float((x * wsum).sum())
    assert t1 >= 65520.0 and float((x.abs() * wsum.abs()).sum()) * 8 < LIMIT, "t1 = %g does not round to an f16 Inf" % t1
    d["x"][(n * c.H + py) * c.W + px] = x.to(f16)
    return d


def flagged_tiles(c):
    """bool [B][tiles_y][tiles_x]: the tiles whose in-image 6 x 18 halo holds the overflow pixel"""
    g = geometry(c)
    n, py, px = overflow_pixel(c)
    ty, tx = torch.arange(g["tiles_y"]).view(-1, 1), torch.arange(g["tiles_x"]).view(1, -1)
    hit = (ty * TH - 1 <= py) & (py <= ty * TH + TH) & (tx * TW - 1 <= px) & (px <= tx * TW + TW)
    f = torch.zeros((c.B, g["tiles_y"], g["tiles_x"]), dtype=torch.bool)
    f[n] = hit
    return f


def flagged_rows(c):
    """bool [rows]: the output pixels of the flagged tiles"""
    g = geometry(c)
    f = flagged_tiles(c)
    py, px = torch.arange(c.H).view(-1, 1) // TH, torch.arange(c.W).view(1, -1) // TW
    rows = torch.zeros(g["rows"], dtype=torch.bool)
    rows[:g["bm"]] = f[:, py, px].reshape(-1)
    return rows
