"""Exactly computable cases for the small ops that sit between the GEMMs and convolutions of every plan -- k_maxpool (single plane and
split), k_bilinear (every plane combination), k_dwconv_split (one side split) and the split k_stem_mfma (fp32 planes and uint8 in) --
shared by test_pool_resample_operands_cpu.py (operand conditions and the teeth of the comparison, without a GPU) and
test_gpu_pool_resample_exact.py (which runs each op alone and compares every buffer for equality).  Host only; the pattern is that of
_bottleneck2_operands.py, and ints / expect / split_planes come from _exact_operands.py.

WHAT THE KERNELS COMPUTE (read from csrc/seg_conv.hip and csrc/seg_stem_mfma.hip; the expected values mirror exactly this).
    k_maxpool       3 x 3, stride 2, pad 1: fmaxf from -INFINITY over the window positions inside the image.  Split: the maximum of the fp32
                    values hi + lo, split again (hi = f16(m), lo = f16(m - hi)).
    k_bilinear      align_corners: scale = (in - 1) / (out - 1) as a float32 division (0 when out = 1), f = scale * dst ROUNDED to float32
                    (src_coord of seg_types.h), corner (int)f, weight l = f - corner, h = 1 - l,
                    r = hy (hx a + lx b) + ly (hx c + lx d) in fp32 on the values hi + lo; out = T(r), out_lo = T(r - (float)T(r)).
    k_dwconv_split  acc = bias, then fmaf(x_tap, w_tap, acc) over the nine taps in order (x = hi + lo in fp32, 0 outside the image), ReLU,
                    out = f16(acc), out_lo = f16(acc - out).
    k_stem_mfma     split: the normalised image as two f16 tiles (xh, xl), zero outside the image; acc = Wh.xh + Wh.xl + Wl.xh (Wl.xl is
                    never formed), v = relu(acc + bias) with ONE fp32 rounding, hi = f16(v), lo = f16(v - hi).  AVL_IN_F32_CHW: xh = f16(x),
                    xl = f16(x - xh).  AVL_IN_U8_HWC: x = ((float)b / 255 - mean) / std in float32, the same split, through a table.

EXACTNESS.  Max-pool is pure selection.  Bilinear (exact cases): the scale is a power of two, so every weight is a multiple of 1/4 and
r is a multiple of 2^-10 below 2^11: exact in fp32 whatever the order or contraction (asserted: float32 evaluation == float64).  The
depthwise chain sums multiples of 1/4 below 2^15.  The fp32-in stem sums multiples of 2^-13 below 2^10; the uint8 stem has one-hot
weights, so every output is one product pair and one add.  The expected output is the exact value rounded ONCE to the type.

POISON.  What an op must not read -- the columns of a wider input buffer, the rows past the last image -- holds NaN; for max-pool +Inf
(fmaxf drops a NaN, so NaN would not show there).  Outputs sit at column OUT_OFF of a buffer OUT_PAD columns wider, filled with FILL, with
TAIL rows past the last pixel: the whole buffer is compared.

No expected value mirrors an instruction's behaviour beyond what is stated here."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _exact_operands as X
from _gconv_mixed_operands import ties

f16, f64 = torch.float16, torch.float64
FILL, TAIL, OUT_OFF, OUT_PAD = 7.0, 5, 8, 16
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -24


def _dtype(prec):
    return X.DTYPES.get(prec, f16)                             # the split forms are f16


def _rows(x):
    """[B][C][H][W] -> [B H W][C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _unrows(m, B, H, W):
    return m.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _in_buffer(m, dtype, extra=0, poison=NAN):
    """[M][C] exact values -> [M + TAIL][C + extra] in the type, the values at column 8 when extra >= 16 (0 otherwise), poison elsewhere"""
    t = m.to(dtype)
    assert torch.equal(t.double(), m.double()), "an input is not exact in its type"
    off = 8 if extra >= 16 else 0
    out = torch.full((m.shape[0] + TAIL, m.shape[1] + extra), poison, dtype=dtype)
    out[:m.shape[0], off:off + m.shape[1]] = t
    return out, off


def _out_buffer(t):
    """[M][C] in its type -> the whole expected buffer [M + TAIL][C + OUT_PAD] around FILL"""
    out = torch.full((t.shape[0] + TAIL, t.shape[1] + OUT_PAD), FILL, dtype=t.dtype)
    out[:t.shape[0], OUT_OFF:OUT_OFF + t.shape[1]] = t
    return out


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and torch.equal(bits(a[k]), bits(b[k])) for k in a)


def changed_bytes(a, b):
    """the number of bytes in which two sets of expected buffers differ"""
    assert a.keys() == b.keys()
    return sum(int((a[k].contiguous().view(torch.uint8) != b[k].contiguous().view(torch.uint8)).sum()) for k in a)


def _split16(v, hi_how=None, lo_how=None, strict=True):
    """exact float64 -> (hi, lo) f16 as the kernels write them: hi = f16(v), lo = f16(v - hi) with v - hi taken in fp32 (strict: asserted to
    be exact there; a deliberately wrong value need not be)"""
    hi = {None: lambda t: t.to(f16), "truncate": lambda t: X.round_toward_zero(t.contiguous(), "f16"),
          "half_away": lambda t: X.round_half_away(t.contiguous(), "f16")}[hi_how](v)
    rem = v - hi.double()
    assert not strict or torch.equal(rem.float().double(), rem), "v - hi is no fp32 value"
    rem = rem.float().double()
    lo = X.round_toward_zero(rem.contiguous(), "f16") if lo_how == "truncate" else rem.to(f16)
    return hi, lo


def _finish16(v, form, mut, prec="f16"):
    """the exact result -> {"out"[, "out_lo"]} [M][C] in the type.  Wrong variants: half_away (the hi rounding), out_lo_truncated (the lo
    plane is the remainder of a TRUNCATED hi next to the rounded hi plane: with v - hi itself always an f16 value on these operands, a
    truncated rounding of the remainder alone could not show)"""
    if form in ("split", "out_lo"):
        hi, lo = _split16(v, "half_away" if mut == "half_away" else None, strict=mut is None)
        if mut == "out_lo_truncated":
            lo = _split16(v, "truncate", strict=False)[1]
        return {"out": hi, "out_lo": lo}
    if mut == "half_away" and prec != "f32":
        return {"out": X.round_half_away(v.contiguous(), prec)}
    return {"out": v.to(_dtype(prec))}


# ==================================================================================================================== max-pool
MPCase = collections.namedtuple("MPCase", "prec H W C B extra")
MP_SHAPES = [(1, 1, 8, 1, 0), (2, 2, 8, 1, 0), (7, 9, 24, 1, 0), (8, 10, 64, 3, 0), (35, 67, 64, 2, 8)]
MP_CASES = [MPCase(p, *s) for p in ("f32", "bf16", "f16") for s in MP_SHAPES]
MP_SPLIT_CASES = [MPCase("split", H, W, C, B, 8 if (H, W) == (35, 67) else 0)
                  for (H, W) in ((1, 1), (2, 2), (7, 9), (8, 10), (35, 67)) for C in (8, 64) for B in (1, 3)]
MP_MUTATIONS = ("pad_zero", "window_2x2", "window_from_2oy", "hi_only", "hi_lo_independent", "image_0")


def mp_id(c):
    return "%s-%dx%dx%d-b%d%s" % (c.prec, c.H, c.W, c.C, c.B, "-ld+%d" % c.extra if c.extra else "")


def mp_applicable(c, mut):
    if mut in ("hi_only", "hi_lo_independent"):                # (2 x 2 x 8: too few windows for two equal hi in one of them to be certain)
        return c.prec == "split" and c.H * c.W > 1 and c.H * c.W * c.C > 32
    if mut == "image_0":
        return c.B > 1
    if mut == "window_2x2":
        return c.H * c.W > 1
    if mut == "window_from_2oy":                               # (H <= 2: rows 0 .. 2 and rows -1 .. 1 hold the same pixels)
        return c.H > 2
    return True


def _sign_field(g, B, C, H, W, block=4):
    """-1 / +1, constant over 4 x 4 pixel blocks per channel: whole windows are negative"""
    s = torch.where(torch.rand((B, C, -(-H // block), -(-W // block)), generator=g) < 0.5, -1.0, 1.0)
    return s.repeat_interleave(block, 2).repeat_interleave(block, 3)[:, :, :H, :W].double()


@functools.lru_cache(maxsize=4)
def mp_operands(c):
    """single plane: {"x"}: non-zero integers within +-127 (exact in bf16) of both signs, -0.0 on a tenth of the negative elements and NO
    +0.0 anywhere (fmaxf and torch may order the two zeros differently; a pool that pads with 0 still shows, as +0.0 where -0.0 or a negative
    value is expected).  split: {"hi", "lo"}: hi = +-(1030 + 37 k), k < 8, so windows often hold the same hi twice; lo = m 2^-10, |m| <= 500 <
    half an ulp of hi."""
    g = torch.Generator().manual_seed(X._seed(c.H, c.W, c.C, c.B, len(c.prec), ord(c.prec[0]), 5))
    shape = (c.B, c.C, c.H, c.W)
    sign = _sign_field(g, *shape)
    if c.prec != "split":
        x = sign * torch.randint(1, 128, shape, generator=g).double()
        x = torch.where((sign < 0) & (torch.rand(shape, generator=g) < 0.1), torch.tensor(-0.0, dtype=f64), x)
        return {"x": x}
    hi = sign * (1030.0 + 37.0 * torch.randint(0, 8, shape, generator=g).double())
    lo = torch.randint(-500, 501, shape, generator=g).double() / 1024.0
    return {"hi": hi, "lo": lo}


def _windows(t, pad, taps, yshift):
    """[B][C][H][W] -> [taps][B][C][OH][OW]: the window elements, `pad` outside the image"""
    B, C, H, W = t.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = torch.full((B, C, 2 * OH + 3, 2 * OW + 3), pad, dtype=t.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = t
    return torch.stack([p[:, :, ky + yshift:ky + yshift + 2 * OH:2, kx:kx + 2 * OW:2] for ky, kx in taps])


def _select(key, planes, mut=None):
    """planes gathered at the arg-max of `key` over each window (float64 [B][C][H][W]); -0.0 orders below +0.0"""
    key = torch.where((key == 0) & torch.signbit(key), torch.tensor(-2.0 ** -40, dtype=f64), key)
    if mut == "image_0":
        key, planes = key[:1].expand_as(key), [p[:1].expand_as(p) for p in planes]
    taps = [(ky, kx) for ky in range(2 if mut == "window_2x2" else 3) for kx in range(2 if mut == "window_2x2" else 3)]
    yshift = 1 if mut == "window_from_2oy" else 0
    idx = _windows(key, 0.0 if mut == "pad_zero" else -INF, taps, yshift).argmax(dim=0, keepdim=True)
    return [_windows(p, 0.0, taps, yshift).gather(0, idx)[0] for p in planes]


def mp_exact(c, mut=None):
    """{"out"[, "out_lo"]} float64 [B][C][OH][OW], optionally subtly wrong"""
    o = mp_operands(c)
    if c.prec != "split":
        return {"out": _select(o["x"], [o["x"]], mut)[0]}
    value = o["hi"] + o["lo"]
    if mut == "hi_only":                                       # the maximum over hi alone: the first of equal hi wins
        hi, lo = _select(o["hi"], [o["hi"], o["lo"]])
    elif mut == "hi_lo_independent":
        hi, lo = _select(o["hi"], [o["hi"]])[0], _select(o["lo"], [o["lo"]])[0]
    else:
        hi, lo = _select(value, [o["hi"], o["lo"]], mut)
    return {"out": hi, "out_lo": lo}


def mp_stored(c, mut=None):
    dt = _dtype(c.prec)
    out = {}
    for k, v in mp_exact(c, mut).items():
        t = _rows(v).to(dt)
        assert torch.equal(t.double(), _rows(v))
        out[k] = _out_buffer(t)
    return out


@functools.lru_cache(maxsize=4)
def mp_want(c):
    """the expected buffers; asserts the case's conditions -> (buffers, figures)"""
    o, r = mp_operands(c), mp_exact(c)
    fig = {}
    if c.prec != "split":
        x = o["x"]
        assert not bool(((x == 0) & ~torch.signbit(x)).any()) and (bool(((x == 0) & torch.signbit(x)).any()) or x.numel() < 500)
        ref = F.max_pool2d(x.float(), 3, 2, 1)                                     # pure selection
        assert torch.equal(bits(ref), bits(r["out"].float())), "the host selection and F.max_pool2d differ"
        fig["negative"] = float((torch.signbit(r["out"])).double().mean())
        assert fig["negative"] >= 0.1, "%s: only %.1f %% of the outputs are negative" % (mp_id(c), 100 * fig["negative"])
    else:
        v32 = (o["hi"] + o["lo"]).float()
        assert torch.equal(v32.double(), o["hi"] + o["lo"]), "float32(hi) + float32(lo) is not exact"
        hi, lo = X.split_planes(v32.double())
        assert torch.equal(hi.double(), o["hi"]) and torch.equal(lo.double(), o["lo"]), "hi + lo does not split back to the same pair"
        assert torch.equal(r["out"] + r["out_lo"], F.max_pool2d(o["hi"] + o["lo"], 3, 2, 1)), "the selected pair is not the float64 maximum"
        taps = [(ky, kx) for ky in range(3) for kx in range(3)]
        wh, wl = _windows(o["hi"], NAN, taps, 0), _windows(o["lo"], NAN, taps, 0)
        fig["decided_by_lo"] = float(((wh == r["out"]) & (wl != r["out_lo"])).any(dim=0).double().mean())
        if c.H * c.W > 1:
            assert fig["decided_by_lo"] >= 0.05, "%s: only %.1f %% of the windows are decided by lo" % (mp_id(c), 100 * fig["decided_by_lo"])
    return mp_stored(c), fig


def mp_device_inputs(c):
    """{"in"[, "in_lo"]}: [B H W + TAIL][C + extra], +Inf in the columns past C and the rows past the last image"""
    o, dt = mp_operands(c), _dtype(c.prec)
    names = {"in": "x"} if c.prec != "split" else {"in": "hi", "in_lo": "lo"}
    return {k: _in_buffer(_rows(o[v]), dt, c.extra, INF)[0] for k, v in names.items()}


def _dtype_id(prec):
    from vision_semantic_segmentation_amd import _lib
    return {"f32": _lib.AVL_F32, "bf16": _lib.AVL_BF16}.get(prec, _lib.AVL_F16)


def _op(kind, prec, ptr, in_hw, cin, in_ld, in_rows, out_hw, cout, out_rows, batch, out_off=OUT_OFF, **f):
    """ptr: {"in", "out"[, "in_lo", "out_lo"]} -> address of element 0 of each BUFFER; the output slice starts at column out_off"""
    from vision_semantic_segmentation_amd.network import AvlSegOp
    es = 4 if prec == "f32" else 2
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = kind, _dtype_id(prec), batch if batch > 1 else 0
    op.in_, op.out = ptr["in"] + f.pop("in_off", 0) * es, ptr["out"] + out_off * es
    if "in_lo" in ptr:
        op.in_lo = ptr["in_lo"] + (op.in_ - ptr["in"])
    if "out_lo" in ptr:
        op.out_lo = ptr["out_lo"] + out_off * es
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = in_hw[0], in_hw[1], cin, in_ld, in_rows
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = out_hw[0], out_hw[1], cout, cout + OUT_PAD, out_rows
    for k, v in f.items():
        setattr(op, k, v)
    return op


def mp_make_op(c, ptr):
    from vision_semantic_segmentation_amd.network import OP_MAXPOOL
    OH, OW = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    return _op(OP_MAXPOOL, c.prec, ptr, (c.H, c.W), c.C, c.C + c.extra, c.B * c.H * c.W + TAIL, (OH, OW), c.C, c.B * OH * OW + TAIL, c.B,
               ksize=3, stride=2, pad=1, dil=1)


# ==================================================================================================================== bilinear
BLCase = collections.namedtuple("BLCase", "form h w OH OW C B")
BL_SIZES = [(5, 9, 9, 17, 8, 1), (3, 5, 9, 17, 64, 1), (9, 17, 5, 9, 8, 1), (2, 2, 2, 2, 64, 1), (1, 1, 4, 7, 8, 1), (1, 6, 5, 6, 64, 1),
            (4, 6, 1, 1, 8, 1), (9, 3, 33, 9, 8, 3)]
BL_FORMS = ("f32", "bf16", "f16", "split", "in_lo", "out_lo")               # the last three: f16 with both sides / one side split
BL_CASES = [BLCase(f, *s) for f in BL_FORMS for s in BL_SIZES]
BL_FRACTIONAL = [(5, 9, 9, 17), (3, 5, 9, 17), (9, 3, 33, 9)]               # the sizes with weights that are no integers
BL_TOL_SIZES = [(3, 266, 5, 1080), (266, 3, 1080, 5), (17, 30, 68, 120)]
BL_TOL_CASES = [BLCase(f, *s, 8, 1) for f in ("f32", "split") for s in BL_TOL_SIZES]
BL_MUTATIONS = ("scale_in_over_out", "swap_lx_hx", "drop_in_lo", "out_lo_truncated", "half_away", "out1_nonzero_scale")
BL_BAR_U = 8.0                                                 # |got - ref| <= 8 u max|four corners| (+ 2^-22 |ref| for a split output)


def bl_id(c):
    return "%s-%dx%d-%dx%d-c%d-b%d" % (c.form, c.h, c.w, c.OH, c.OW, c.C, c.B)


def bl_prec(c):
    return c.form if c.form in X.DTYPES else "f16"


def bl_applicable(c, mut):
    if mut == "scale_in_over_out":                             # (where it moves a corner or a weight at all)
        return any(n > 1 and not all(torch.equal(a, b) for a, b in zip(coords(n, m), coords(n, m, mut))) for n, m in ((c.h, c.OH), (c.w, c.OW)))
    if mut == "swap_lx_hx":
        return (c.h, c.w, c.OH, c.OW) in BL_FRACTIONAL and c.w > 1
    if mut == "drop_in_lo":                                    # (a single-plane output of exact samples is hi itself: |lo| < ulp / 2)
        return c.form == "split" or (c.form == "in_lo" and (c.h, c.w, c.OH, c.OW) in BL_FRACTIONAL)
    if mut == "out_lo_truncated":
        return c.form == "split" or (c.form == "out_lo" and (c.h, c.w, c.OH, c.OW) in BL_FRACTIONAL)
    if mut == "half_away":
        return c.form != "f32" and (c.h, c.w, c.OH, c.OW) in BL_FRACTIONAL
    if mut == "out1_nonzero_scale":
        return c.OH == 1 and c.OW == 1
    return True


def coords(n_in, n_out, mode="rule"):
    """(corner, neighbour, weight float64) of every destination index.
      rule               scale = float32(in - 1) / float32(out - 1) (0 when out = 1), f = float32(scale * dst), weight = f - (int)f (exact)
      contracted         the corner from f, the weight float32(float64(scale) * dst - corner): scale * dst - corner as ONE fused operation
      scale_in_over_out  scale = in / out
      out1_nonzero_scale out = 1 maps to the centre (in - 1) / 2 instead of 0"""
    dst = np.arange(n_out, dtype=np.float32)
    if mode == "scale_in_over_out":
        s = np.float32(n_in) / np.float32(n_out)
    else:
        s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    f = (s * dst).astype(np.float32)
    if mode == "out1_nonzero_scale" and n_out == 1:
        f = np.array([(n_in - 1) / 2.0], dtype=np.float32)
    i0 = f.astype(np.int64)
    assert int(i0.max()) <= n_in - 1
    i1 = i0 + (i0 < n_in - 1)
    if mode == "contracted":
        l = (np.float64(s) * dst.astype(np.float64) - i0).astype(np.float32).astype(np.float64)
    else:
        l = f.astype(np.float64) - i0
        assert np.array_equal(l.astype(np.float32).astype(np.float64), l)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l)


def interp(x, OH, OW, dt, mode="rule", swap=False):
    """x [B][h][w][C] -> [B][OH][OW][C], the kernel's expression evaluated in `dt` (every operation rounded on its own)"""
    B, h, w, C = x.shape
    y0, y1, ly = coords(h, OH, mode)
    x0, x1, lx = coords(w, OW, mode)
    ly, lx = ly.to(dt).view(1, OH, 1, 1), lx.to(dt).view(1, 1, OW, 1)
    hy, hx = 1 - ly, 1 - lx
    if swap:
        lx, hx = hx, lx
    x = x.to(dt)
    a, b, c, d = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return hy * (hx * a + lx * b) + ly * (hx * c + lx * d)


def corner_max(x, OH, OW):
    """max |value| of the four corners of every output element: the scale of the tolerance test's bar"""
    y0, y1, _ = coords(x.shape[1], OH)
    x0, x1, _ = coords(x.shape[2], OW)
    a = x.abs().double()
    return torch.stack([a[:, y0][:, :, x0], a[:, y0][:, :, x1], a[:, y1][:, :, x0], a[:, y1][:, :, x1]]).amax(dim=0)


@functools.lru_cache(maxsize=4)
def bl_operands(c):
    """{"hi"[, "lo"]} float64 [B][h][w][C].  Exact cases: integers, |hi| in 1024 .. 2000 (bf16: 128 .. 255: the type's ulp is 1 there), the
    sign drawn per image and channel (so that interpolated values keep that magnitude), lo = m 2^-6 with |m| <= 15 (below half an ulp of hi).  Tolerance cases: Gaussian with sigma = 16; the split form is the canonical pair of it (the bar has no absolute term, and an f16 lo plane underflows
    by up to 2^-25: at this sigma no output has four corners small enough for that to count, which the CPU test shows on the float32 evaluation)."""
    g = torch.Generator().manual_seed(X._seed(c.h, c.w, c.OH, c.OW, c.C, c.B, ord(c.form[0]), len(c.form)))
    shape = (c.B, c.h, c.w, c.C)
    if (c.h, c.w, c.OH, c.OW) in BL_TOL_SIZES:
        v = 16.0 * torch.randn(shape, generator=g, dtype=torch.float32)
        if c.form == "f32":
            return {"hi": v.double()}
        hi = v.to(f16)
        lo = (v - hi.float()).to(f16)
        return {"hi": hi.double(), "lo": lo.double()}
    lo_, hi_ = (128, 256) if c.form == "bf16" else (1024, 2001)
    sign = torch.where(torch.rand((c.B, 1, 1, c.C), generator=g) < 0.5, -1.0, 1.0).double()
    o = {"hi": sign * torch.randint(lo_, hi_, shape, generator=g).double()}
    if c.form in ("split", "in_lo"):
        o["lo"] = torch.randint(-15, 16, shape, generator=g).double() / 64.0
    return o


def bl_value(o, mut=None):
    return o["hi"] + (o["lo"] if "lo" in o and mut != "drop_in_lo" else 0.0)


def bl_exact(c, mut=None, check=False):
    """the exact result float64 [B OH OW][C] of an exact case, optionally subtly wrong"""
    x = bl_value(bl_operands(c), mut)
    mode = mut if mut in ("scale_in_over_out", "out1_nonzero_scale") else "rule"
    v = interp(x, c.OH, c.OW, f64, mode, swap=mut == "swap_lx_hx")
    if check:
        assert torch.equal(interp(x, c.OH, c.OW, torch.float32, mode).double(), v), "the float32 and float64 host evaluations differ"
        if bl_prec(c) == "f32":
            ref = F.interpolate(x.permute(0, 3, 1, 2), size=(c.OH, c.OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
            assert torch.equal(ref, v), "F.interpolate (float64) differs"
    return v.reshape(-1, c.C)


def bl_stored(c, mut=None):
    return {k: _out_buffer(t) for k, t in _finish16(bl_exact(c, mut), c.form, mut, bl_prec(c)).items()}


@functools.lru_cache(maxsize=4)
def bl_want(c):
    v = bl_exact(c, check=True)
    o = bl_operands(c)
    fig = {}
    if "lo" in o:
        hi = o["hi"].to(f16)
        ulp = (torch.from_numpy(np.nextafter(hi.abs().numpy(), np.float16(np.inf))).double() - hi.abs().double())
        assert torch.equal(hi.double(), o["hi"]) and bool((o["lo"].abs() < ulp / 2).all()) and bool((o["lo"] != 0).any())
    res = _finish16(v, c.form, None, bl_prec(c))
    if bl_prec(c) == "f32":
        assert torch.equal(res["out"].double(), v)
    elif (c.h, c.w, c.OH, c.OW) in BL_FRACTIONAL:
        out = res["out"]
        fig["rounded"] = float((out.double() != v).double().mean())
        assert fig["rounded"] >= 0.2, "%s: only %.1f %% of the outputs round" % (bl_id(c), 100 * fig["rounded"])
        if bl_prec(c) == "f16":
            fig["ties"] = ties(v, out)
        else:                                                  # bf16: an exact tie is a value with exactly one bit below the type's last
            rem = v.float().view(torch.int32) & 0xffff
            up = out.float().abs() > v.float().abs()
            fig["ties"] = (int(((rem == 0x8000) & ~up).sum()), int(((rem == 0x8000) & up).sum()))
        assert fig["ties"][0] > 0 and fig["ties"][1] > 0, "%s: exact ties rounding down %d, up %d" % ((bl_id(c),) + fig["ties"])
    if "out_lo" in res:
        assert torch.equal(res["out"].double() + res["out_lo"].double(), v)
        if (c.h, c.w, c.OH, c.OW) in BL_FRACTIONAL:
            assert float((res["out_lo"] != 0).double().mean()) >= 0.2
    return bl_stored(c), fig


def bl_device_inputs(c):
    """{"in"[, "in_lo"]}: [B h w + TAIL][C + 16] with the values at column 8, NaN everywhere else"""
    o, dt = bl_operands(c), _dtype(bl_prec(c))
    return {k: _in_buffer(o[v].reshape(-1, c.C), dt, 16)[0] for k, v in (("in", "hi"), ("in_lo", "lo")) if v in o}


def bl_make_op(c, ptr):
    from vision_semantic_segmentation_amd.network import OP_BILINEAR
    return _op(OP_BILINEAR, bl_prec(c), ptr, (c.h, c.w), c.C, c.C + 16, c.B * c.h * c.w + TAIL, (c.OH, c.OW), c.C, c.B * c.OH * c.OW + TAIL, c.B,
               in_off=8)


def bl_tolerance(c):
    """the tolerance cases: (ref float64 [B][OH][OW][C], bar of the same shape): float64 interpolation with the coordinate of the stated rule;
    bar = 8 u max|four corners| (hx and hy carry one rounding each, the five-operation lerp gives gamma_5, with or without FMA), plus
    2^-22 |ref| where the output is a split pair"""
    x = bl_value(bl_operands(c))
    ref = interp(x, c.OH, c.OW, f64)
    bar = BL_BAR_U * U * corner_max(x, c.OH, c.OW)
    if c.form == "split":
        bar = bar + 2.0 ** -22 * ref.abs()
    return ref, bar


def bl_host_float32(c, mode):
    """what a float32 evaluation gives (the output split and summed again for the split form), with the coordinate by `mode`"""
    r = interp(bl_value(bl_operands(c)), c.OH, c.OW, torch.float32, mode)
    if c.form == "split":
        hi = r.to(f16)
        return hi.double() + (r - hi.float()).to(f16).double()
    return r.double()


# =========================================================================================================== one-side split depthwise
DWCase = collections.namedtuple("DWCase", "side H W C dil pad relu B")
DW_SHAPES = [(9, 9, 64, 1, 1, True, 1), (19, 27, 128, 2, 2, False, 2), (8, 30, 64, 12, 12, True, 1), (11, 13, 64, 1, 0, False, 1)]
DW_CASES = [DWCase(s, *g) for s in ("in_lo", "out_lo") for g in DW_SHAPES]
DW_MUTATIONS = ("drop_in_lo", "outside_tap_reads_pixel_0", "relu_before_bias", "dilation_ignored", "out_lo_truncated")


def dw_id(c):
    return "%s-%dx%dx%d-d%d-p%d-%s-b%d" % (c.side, c.H, c.W, c.C, c.dil, c.pad, "relu" if c.relu else "lin", c.B)


def dw_applicable(c, mut):
    return {"drop_in_lo": c.side == "in_lo", "outside_tap_reads_pixel_0": c.pad > 0, "relu_before_bias": c.relu, "dilation_ignored": c.dil > 1,
            "out_lo_truncated": c.side == "out_lo"}[mut]


@functools.lru_cache(maxsize=4)
def dw_operands(c):
    """hi: the integers of _exact_operands.ints; lo in {0, +-1/4, +-1/2} (in_lo cases); weights [9][C] in {0, +-1, +-2}; bias: integers, a third
    of the channels in 2048 .. 4000 (both signs without a ReLU), where f16 no longer holds every integer, the rest within 0 .. 80 (+-80 without a
    ReLU)"""
    s = X._seed(c.H, c.W, c.C, c.dil, c.pad, c.B, 9)
    g = torch.Generator().manual_seed(s)
    o = {"hi": X.ints(s, c.B * c.H * c.W, c.C).reshape(c.B, c.H, c.W, c.C).double()}
    pick = lambda shape, values: torch.tensor(values, dtype=f64)[torch.randint(0, len(values), shape, generator=g)]
    o["lo"] = pick((c.B, c.H, c.W, c.C), [0.0, 0.25, -0.25, 0.5, -0.5])
    o["w"] = pick((9, c.C), [0.0, 1.0, -1.0, 2.0, -2.0, 1.0, -1.0, 2.0, -2.0])
    small = torch.randint(0 if c.relu else -80, 81, (c.C,), generator=g).double()
    big = torch.randint(2048, 4000, (c.C,), generator=g).double() * (1.0 if c.relu else torch.where(torch.rand(c.C, generator=g) < 0.5, -1.0, 1.0).double())
    o["bias"] = torch.where(torch.arange(c.C) % 3 == 1, big, small)
    return o


def dw_exact(c, mut=None, check=False):
    """exact float64 [B OH OW][C], optionally subtly wrong"""
    o = dw_operands(c)
    x = o["hi"] + (o["lo"] if c.side == "in_lo" and mut != "drop_in_lo" else 0.0)
    OH, OW = c.H + 2 * c.pad - 2 * c.dil, c.W + 2 * c.pad - 2 * c.dil
    step = 1 if mut == "dilation_ignored" else c.dil
    acc = torch.zeros((c.B, OH, OW, c.C), dtype=f64)
    mag = torch.zeros_like(acc)
    for t in range(9):
        iy = torch.arange(OH) - c.pad + (t // 3) * step
        ix = torch.arange(OW) - c.pad + (t % 3) * step
        ok = ((iy >= 0) & (iy < c.H)).view(1, OH, 1, 1) & ((ix >= 0) & (ix < c.W)).view(1, 1, OW, 1)
        tap = x[:, iy.clamp(0, c.H - 1)][:, :, ix.clamp(0, c.W - 1)]
        tap = torch.where(ok, tap, x[:, :1, :1] if mut == "outside_tap_reads_pixel_0" else torch.zeros((), dtype=f64))
        acc += tap * o["w"][t]
        mag += tap.abs() * o["w"][t].abs()
    if check:
        assert float((mag + o["bias"].abs()).max()) * 4 < X.LIMIT and torch.equal(torch.round(acc * 4), acc * 4)        # multiples of 1/4 below 2^22
    if mut == "relu_before_bias":
        v = torch.relu(acc) + o["bias"]
    else:
        v = acc + o["bias"]
        v = torch.relu(v) if c.relu else v
    return v.reshape(-1, c.C)


def dw_stored(c, mut=None):
    return {k: _out_buffer(t) for k, t in _finish16(dw_exact(c, mut), c.side, mut).items()}


@functools.lru_cache(maxsize=4)
def dw_want(c):
    v = dw_exact(c, check=True)
    res = _finish16(v, c.side, None)
    fig = {"rounded": float((res["out"].double() != v).double().mean()), "ties": ties(v, res["out"])}
    assert float(v.abs().max()) > 2048 and fig["ties"][0] > 0 and fig["ties"][1] > 0, "%s: ties %s" % (dw_id(c), fig["ties"])
    if c.side == "in_lo":
        fig["lo_shows"] = float((dw_exact(c, "drop_in_lo").to(f16) != res["out"]).double().mean())
        assert fig["lo_shows"] >= 0.3, "%s: dropping in_lo changes only %.1f %% of the f16 outputs" % (dw_id(c), 100 * fig["lo_shows"])
    else:
        assert torch.equal(res["out"].double() + res["out_lo"].double(), v) and bool((res["out_lo"] != 0).any())
        fig["lo_nonzero"] = float((res["out_lo"] != 0).double().mean())
    return dw_stored(c), fig


def dw_device_inputs(c):
    """{"in"[, "in_lo"]: f16 [B H W + TAIL][C + 16], the values at column 8, NaN elsewhere; "weight": fp32 [9][C]; "bias": fp32 [C];
    "zero": the 64-byte zero page the op's validation asks for}"""
    o = dw_operands(c)
    d = {"in": _in_buffer(o["hi"].reshape(-1, c.C), f16, 16)[0], "weight": o["w"].float().contiguous(), "bias": o["bias"].float(),
         "zero": torch.zeros(64, dtype=torch.uint8)}
    if c.side == "in_lo":
        d["in_lo"] = _in_buffer(o["lo"].reshape(-1, c.C), f16, 16)[0]
    return d


def dw_make_op(c, ptr):
    from vision_semantic_segmentation_amd.network import OP_DWCONV
    OH, OW = c.H + 2 * c.pad - 2 * c.dil, c.W + 2 * c.pad - 2 * c.dil
    return _op(OP_DWCONV, "f16", ptr, (c.H, c.W), c.C, c.C + 16, c.B * c.H * c.W + TAIL, (OH, OW), c.C, c.B * OH * OW + TAIL, c.B, in_off=8,
               weight=ptr["weight"], bias=ptr["bias"], in2=ptr["zero"], ksize=3, stride=1, pad=c.pad, dil=c.dil, groups=c.C, relu=int(c.relu))


# ================================================================================================================== split stem
STCase = collections.namedtuple("STCase", "fmt H W B")
ST_CASES = [STCase("f32", H, W, 1) for H, W in X.STEM_SIZES] + [STCase("f32", 37, 53, 2), STCase("u8", 33, 47, 1), STCase("u8", 7, 250, 1)]
ST_MUTATIONS = ("drop_wl_xh", "drop_wh_xl", "add_wl_xl", "lo_table_of_wrong_channel", "pad_normalised_zero", "lo_truncated", "lo_before_relu")


def st_id(c):
    return "%s-%dx%d-b%d" % (c.fmt, c.H, c.W, c.B)


def st_applicable(c, mut):
    return c.fmt == "u8" if mut == "lo_table_of_wrong_channel" else True


def _norm_split(b):
    """bytes [..][3] -> (xh, xl) float64: the kernel's table"""
    v = X.normalise_u8(b)
    hi = v.to(f16)
    return hi.double(), (v - hi.float()).to(f16).double()


@functools.lru_cache(maxsize=2)
def st_operands(c):
    """f32: x = xh + xl [B][3][H][W], xh in {+-1, +-1.5, +-2, +-3} (0 on a few pixels, where xl is 0 too: the split of a bare xl would put it
    into the hi plane; with |xh| = 1 it has xh's sign), xl in {0, +-1, +-2, +-3} 2^-13; Wh in {0, +-1, +-2}, Wl in {0, +-1, +-2} 2^-12, independent; bias: fp32 multiples of
    2^-16; 58 channels in 256 .. 900 (v = fp32(acc + bias) then has 24 significant bits, of which f16 + f16 hold 22: a quarter of the lo values
    round, and no magnitude gives more), two at minus that (always clamped), four within +-8 (the ReLU cuts through them).  u8: random bytes; channel n has ONE non-zero tap, ((23 n + 7 H) mod 147);
    even channels Wh = +-2^k, odd channels Wl = 2^(k - 12) with Wh = 0, k in -1 .. 2; the same kind of bias."""
    s = X._seed(c.H, c.W, c.B, ord(c.fmt[0]), 3)
    g = torch.Generator().manual_seed(s)
    pick = lambda shape, values: torch.tensor(values, dtype=f64)[torch.randint(0, len(values), shape, generator=g)]
    big = ((torch.randint(256, 900, (32, 64), generator=g) * 65536 + torch.randint(0, 65536, (32, 64), generator=g)).double() / 65536).float().double()
    rem = big - big.to(f16).double()                           # of 32 candidates per channel the first whose own lo part rounds
    big = big.gather(0, (rem.to(f16).double() != rem).double().argmax(dim=0, keepdim=True))[0]
    small = (torch.randint(-8 * 65536, 8 * 65536, (64,), generator=g).double() / 65536).float().double()
    ch = torch.arange(64)
    o = {"bias": torch.where(ch % 16 == 5, small, torch.where(ch % 32 == 11, -big, big))}
    if c.fmt == "f32":
        xh = pick((c.B, 3, c.H, c.W), [1, -1, 1.5, -1.5, 2, -2, 3, -3, 1, -1.5, 2, -3, 0])
        xl = torch.where(xh == 0, torch.zeros((), dtype=f64), pick((c.B, 3, c.H, c.W), [0, 1, -1, 2, -2, 3, -3]) * 2.0 ** -13)
        xl = torch.where(xh.abs() == 1, xl.abs() * xh, xl)      # below 1 the ulp of f16 halves: there xl points away from zero
        o.update(xh=xh, xl=xl, Wh=pick((64, 3, 7, 7), [0, 0, 1, -1, 2, -2]), Wl=pick((64, 3, 7, 7), [0, 0, 1, -1, 2, -2]) * 2.0 ** -12)
        return o
    o["img"] = torch.randint(0, 256, (c.B, c.H, c.W, 3), generator=g, dtype=torch.uint8)
    tap = (23 * torch.arange(64) + 7 * c.H) % 147                              # tap = (ky 7 + kx) 3 + ci
    w = torch.zeros((64, 147), dtype=f64)
    w[torch.arange(64), tap] = torch.exp2(torch.randint(-1, 3, (64,), generator=g).double()) * torch.where(torch.rand(64, generator=g) < 0.5, -1.0, 1.0)
    w = w.reshape(64, 7, 7, 3).permute(0, 3, 1, 2)
    odd = (torch.arange(64) % 2 == 1).view(64, 1, 1, 1)
    o.update(tap=tap, Wh=torch.where(odd, torch.zeros((), dtype=f64), w).contiguous(), Wl=torch.where(odd, w.abs() * 2.0 ** -12, torch.zeros((), dtype=f64)).contiguous())
    return o


def st_planes(c, mut=None):
    """(xh, xl, pad_h, pad_l): the two f16 tiles' contents [B][3][H][W] as float64 and what they hold outside the image, per channel"""
    o = st_operands(c)
    zero = torch.zeros(3, dtype=f64)
    if c.fmt == "f32":
        xh, xl = X.split_planes(o["xh"] + o["xl"])
        xh, xl, ph, pl = xh.double(), xl.double(), zero, zero
        if mut == "pad_normalised_zero":                       # the fp32 planes hold a normalised image: the value of a black pixel
            ph, pl = [t.reshape(3) for t in _norm_split(torch.zeros((1, 3), dtype=torch.uint8))]
    else:
        xh, xl = [t.permute(0, 3, 1, 2) for t in _norm_split(o["img"])]
        ph, pl = zero, zero
        if mut == "lo_table_of_wrong_channel":                 # lut_lo[((ci + 1) % 3) * 256 + byte]
            xl = torch.stack([_norm_split(o["img"][..., ci:ci + 1].expand(-1, -1, -1, 3))[1][..., (ci + 1) % 3] for ci in range(3)], dim=1)
        if mut == "pad_normalised_zero":
            ph, pl = [t.reshape(3) for t in _norm_split(torch.zeros((1, 3), dtype=torch.uint8))]
    return xh, xl, ph, pl


def _conv7(x, pad, w, dt=f64):
    """7 x 7 stride 2 on x padded by 3 with the per-channel value `pad` -> [B][64][OH][OW]"""
    B, C, H, W = x.shape
    p = pad.view(1, 3, 1, 1).expand(B, 3, H + 6, W + 6).clone()
    p[:, :, 3:H + 3, 3:W + 3] = x
    return F.conv2d(p.to(dt), w.to(dt), None, stride=2)


def st_exact(c, mut=None, check=False):
    """{"v": relu(float32(acc + bias)), "pre": before the ReLU} float64 [B OH OW][64], optionally subtly wrong"""
    o = st_operands(c)
    xh, xl, ph, pl = st_planes(c, mut)
    passes = [(xh, ph, o["Wh"]), (xh, ph, o["Wl"]), (xl, pl, o["Wh"])]
    if mut == "drop_wl_xh":
        del passes[1]
    elif mut == "drop_wh_xl":
        del passes[2]
    elif mut == "add_wl_xl":
        passes.append((xl, pl, o["Wl"]))
    acc = sum(_conv7(x, p, w) for x, p, w in passes)
    if check:
        if c.fmt == "f32":
            assert all(torch.equal(_conv7(x, p, w, torch.float32).double(), _conv7(x, p, w)) for x, p, w in passes), "float32 and float64 differ"
            mag = sum(_conv7(x.abs(), p, w.abs()) for x, p, w in passes)
            assert float(mag.max()) < 2 ** 10 and torch.equal(torch.round(acc * 2 ** 13), acc * 2 ** 13), "multiples of 2^-13 below 2^10"
        else:
            assert int(((o["Wh"] != 0) | (o["Wl"] != 0)).reshape(64, -1).sum(dim=1).max()) == 1            # one product pair per output
    pre = (acc + o["bias"].view(1, 64, 1, 1)).float().double()                  # acc + bias is exact in float64: ONE rounding, to fp32
    return {"v": _rows(torch.relu(pre)), "pre": _rows(pre)}


def st_stored(c, mut=None):
    r = st_exact(c, mut)
    hi, lo = _split16(r["v"], None, "truncate" if mut == "lo_truncated" else None, strict=mut is None)
    if mut == "lo_before_relu":
        lo = _split16(r["pre"], strict=False)[1]
    return {"out": _out_buffer(hi), "out_lo": _out_buffer(lo)}


@functools.lru_cache(maxsize=2)
def st_want(c):
    o, r = st_operands(c), st_exact(c, check=True)
    fig = {}
    if c.fmt == "f32":
        xh, xl = X.split_planes(o["xh"] + o["xl"])             # the kernel's own split of x returns exactly (xh, xl)
        assert torch.equal(xh.double(), o["xh"]) and torch.equal(xl.double(), o["xl"])
        x = o["xh"] + o["xl"]
        border = torch.cat([x[:, :, 0].reshape(-1), x[:, :, -1].reshape(-1), x[:, :, :, 0].reshape(-1), x[:, :, :, -1].reshape(-1)])
        assert float((border != 0).double().mean()) > 0.8 and float((o["xl"] != 0).double().mean()) > 0.5
        assert bool((o["bias"] * 65536 == torch.round(o["bias"] * 65536)).all()) and torch.equal(o["bias"].float().double(), o["bias"])
    else:
        t = o["tap"]
        assert len(torch.unique(t)) == 64 and set((t // 21).tolist()) == set(range(7)) and set((t // 3 % 7).tolist()) == set(range(7)) and set((t % 3).tolist()) == {0, 1, 2}
        assert torch.equal(o["Wl"].to(f16).double(), o["Wl"]) and float(o["Wl"][o["Wl"] != 0].min()) >= 2.0 ** -14
    rem = r["v"] - r["v"].to(f16).double()
    fig["lo_rounds"] = float((rem.to(f16).double() != rem).double().mean())
    assert fig["lo_rounds"] >= 0.2, "%s: only %.1f %% of the lo values round" % (st_id(c), 100 * fig["lo_rounds"])
    fig["clamped"] = float((r["pre"] < 0).double().mean())
    assert fig["clamped"] > 0.02
    return st_stored(c), fig


def st_device_inputs(c):
    """{"in": fp32 planes [B 3 H W + TAIL] (NaN past the last image) or the bytes [B][H][W][3], "weight": cat(pack(Wh), pack(Wl)) f16, "bias"}"""
    from vision_semantic_segmentation_amd.network import pack_stem_mfma
    o = st_operands(c)
    if c.fmt == "f32":
        x = (o["xh"] + o["xl"]).float()
        assert torch.equal(x.double(), o["xh"] + o["xl"])
        src = torch.cat([x.reshape(-1), torch.full((TAIL,), NAN)])
    else:
        src = o["img"].contiguous()
    w = torch.cat([pack_stem_mfma(o["Wh"]), pack_stem_mfma(o["Wl"])])
    assert torch.equal(w.to(f16).double(), w)
    return {"in": src, "weight": w.to(f16), "bias": o["bias"].float()}


def st_make_op(c, ptr):
    from vision_semantic_segmentation_amd.network import AVL_IN_F32_CHW, AVL_IN_U8_HWC, OP_STEM, AvlSegOp
    OH, OW = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = OP_STEM, _dtype_id("f16"), c.B if c.B > 1 else 0
    op.in_format = AVL_IN_F32_CHW if c.fmt == "f32" else AVL_IN_U8_HWC
    op.in_, op.out, op.out_lo, op.weight, op.bias = ptr["in"], ptr["out"] + 2 * OUT_OFF, ptr["out_lo"] + 2 * OUT_OFF, ptr["weight"], ptr["bias"]
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = c.H, c.W, 3, 3, c.B * c.H * c.W
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = OH, OW, 64, 64 + OUT_PAD, c.B * OH * OW + TAIL
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu, op.w_layout, op.w_split = 7, 2, 3, 1, 1, 1, 1, 1
    return op


# ------------------------------------------------------------------------------------------------------------ the tables of the suite
FAMILIES = {
    "maxpool": (MP_CASES + MP_SPLIT_CASES, mp_id, MP_MUTATIONS, mp_applicable, mp_want, mp_stored, mp_device_inputs, mp_make_op),
    "bilinear": (BL_CASES, bl_id, BL_MUTATIONS, bl_applicable, bl_want, bl_stored, bl_device_inputs, bl_make_op),
    "dwconv_split": (DW_CASES, dw_id, DW_MUTATIONS, dw_applicable, dw_want, dw_stored, dw_device_inputs, dw_make_op),
    "stem_split": (ST_CASES, st_id, ST_MUTATIONS, st_applicable, st_want, st_stored, st_device_inputs, st_make_op),
}
KERNELS = {"maxpool": "k_maxpool<T>", "bilinear": "k_bilinear<T>", "dwconv_split": "k_dwconv_split<f16>",
           "stem_split": "k_stem_mfma<f16, false, true, F32IN>"}
