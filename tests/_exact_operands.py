"""Exactly computable operands for the single-plane GEMM / convolution kernels, shared by test_exact_operands_cpu.py (which
checks the operand conditions and that the comparison has teeth, without a GPU) and test_gpu_exact_ops.py (which runs the ops).

Every op here is a sum of products over (tap, channel) plus a bias (plus a residual), optionally through a ReLU:
    A3 float32 [M][T][C]       the input at every tap of every output pixel (im2col; zeros where the tap is padding)
    W4 float32 [G][co][T][cg]  the weights of group g (C = G * cg input channels, G * co outputs); a GEMM has T = G = 1
Values are the integers {0, +-1, +-2, +-3, +-4, +-6}, zeros frequent, some 32-blocks along the channels all zero or holding one
non-zero.  bf16, f16 and f32 hold them exactly, every product is an integer of magnitude <= 36, and while
    36 * T * cg + max|bias| + max|residual| < 2^24
every partial sum in ANY order is an integer below 2^24: fp32 accumulation is exact, and the float32 host evaluation equals the
float64 one (exact_acc asserts both).  The expected output is the exact value rounded ONCE to the output type (round to nearest
even: torch's .to()).

Bias: integers; most columns lie in a range where the output type no longer holds every integer (bf16: 256 .. 1536, f16:
2048 .. 7000), so that outputs round and odd integers of [256, 512) (bf16) / [2048, 4096) (f16) -- exact ties -- occur in both
directions.  rounding_conditions asserts that: >= 20 % of the expected 16-bit outputs are not representable before rounding, at
least one tie rounds down to even and one up to even.  Residual: integers exact in the type, both signs.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

VALUES = [0, 0, 0, 0, 0, 0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6]
SMALL_VALUES = [0, 0, 0, 0, 1, -1, 1, -1, 2, -2, 0, 0, 1, -1, 2, -2]      # the u8 stem cases (see stem_case)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
TIE_RANGE = {"bf16": (256, 512), "f16": (2048, 4096)}          # odd integers here are exact ties of the type
BIG_BIAS = {"bf16": (256, 1536), "f16": (2048, 7000), "f32": (2048, 7000)}
RESIDUAL_MAX = {"bf16": 256, "f16": 1000, "f32": 1000}          # integers up to here are exact in the type
LIMIT = 2 ** 24


def ints(seed, rows, cols, values=VALUES):
    """float32 [rows][cols] of `values`; ~5 % of the 32-blocks along a row all zero, ~5 % with a single non-zero"""
    g = torch.Generator().manual_seed(seed)
    cp = (cols + 31) // 32 * 32
    table = torch.tensor(values, dtype=torch.float32)
    x = table[torch.randint(0, len(values), (rows, cp), generator=g)].reshape(rows, cp // 32, 32)
    u = torch.rand((rows, cp // 32, 1), generator=g)
    one = torch.randint(0, 32, (rows, cp // 32, 1), generator=g) == torch.arange(32).view(1, 1, 32)
    x = torch.where(u < 0.05, torch.zeros(()), torch.where((u < 0.10) & ~one, torch.zeros(()), x))
    return x.reshape(rows, cp)[:, :cols].contiguous()


def bias_for(n, seed, prec, relu, big_share=0.7):
    """integer bias [n]: `big_share` of the columns in BIG_BIAS[prec] (where the type rounds integers; positive three times in
    four under a ReLU, which would hide the others), the rest within +-40"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = BIG_BIAS[prec]
    small = torch.randint(-40, 41, (n,), generator=g).float()
    sign = torch.where(torch.rand(n, generator=g) < (0.75 if relu else 0.5), 1.0, -1.0)
    big = torch.randint(lo, hi, (n,), generator=g).float() * sign
    return torch.where(torch.rand(n, generator=g) < big_share, big, small)


def residual_for(m, n, seed, prec):
    g = torch.Generator().manual_seed(seed)
    r = RESIDUAL_MAX[prec]
    return torch.randint(-r, r + 1, (m, n), generator=g).float()


def im2col(x, k, stride, pad, dil):
    """x float32 [B][H][W][C] -> (A3 [B * OH * OW][k * k][C], OH, OW); tap order ky * k + kx; zeros outside the image"""
    B, H, W, C = x.shape
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    assert OH > 0 and OW > 0
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    taps = [xp[:, ky * dil:ky * dil + (OH - 1) * stride + 1:stride, kx * dil:kx * dil + (OW - 1) * stride + 1:stride]
            for ky in range(k) for kx in range(k)]
    return torch.stack(taps, dim=3).reshape(B * OH * OW, k * k, C), OH, OW


def grouped_acc(A3, W4, dtype):
    """sum over (tap, channel) in `dtype`: [M][G * co]"""
    M, T, C = A3.shape
    G, co, T2, cg = W4.shape
    assert T == T2 and C == G * cg
    a = A3.to(dtype).reshape(M, T, G, cg).permute(2, 0, 1, 3).reshape(G, M, T * cg)
    w = W4.to(dtype).reshape(G, co, T * cg)
    return torch.bmm(a, w.transpose(1, 2)).permute(1, 0, 2).reshape(M, G * co)


def exact_acc(A3, W4, extra=0.0, unit=1.0):
    """the exact sum as float64; asserts the bound (with `extra` = max|bias| + max|residual|; every term a multiple of `unit`)
    and that the float32 evaluation equals the float64 one"""
    T, cg = W4.shape[2], W4.shape[3]
    bound = float(A3.abs().max()) * float(W4.abs().max()) * T * cg + extra
    assert bound < LIMIT * unit, "exactness bound: %g >= 2^24 * %g" % (bound, unit)
    a64 = grouped_acc(A3, W4, torch.float64)
    assert torch.equal(grouped_acc(A3, W4, torch.float32).double(), a64), "the float32 and float64 host evaluations differ"
    return a64


def rounding_conditions(v, out, prec, ties=True):
    """conditions on the OPERANDS of a 16-bit case (v exact float64, out = v in the type); -> (share not representable, ties down, up)"""
    o = out.double()
    share = float((o != v).double().mean())
    assert share >= 0.2, "%s: only %.1f %% of the expected outputs round" % (prec, 100 * share)
    lo, hi = TIE_RANGE[prec]
    a = v.abs()
    tie = (a >= lo) & (a < hi) & (a % 2 == 1)
    down, up = int((tie & (o.abs() < a)).sum()), int((tie & (o.abs() > a)).sum())
    if ties:
        assert down > 0 and up > 0, "%s: exact ties rounding down %d, up %d" % (prec, down, up)
    return share, down, up


def expect(v, prec, ties=True):
    """the exact result rounded once (nearest even) to the type; asserts the case's conditions"""
    out = v.to(DTYPES[prec])
    assert bool(torch.isfinite(out).all()), "%s: an expected output overflows the type" % prec
    if prec == "f32":
        assert torch.equal(out.double(), v)
    else:
        rounding_conditions(v, out, prec, ties)
    return out


def finish(c):
    """bias, residual, ReLU on the case's exact accumulator -> exact v (float64)"""
    v = c["acc"] + c["bias"].double()
    if c.get("res") is not None:
        v = v + c["res"].double()
    return torch.relu(v) if c["relu"] else v


# ---------------------------------------------------------------------------------------------- mutations (the CPU test's teeth)
def round_toward_zero(v, prec):
    """float64 -> the type, truncating"""
    if prec == "bf16":
        bits = v.float().view(torch.int32) & -65536
        return bits.view(torch.float32).to(torch.bfloat16)
    r = v.numpy().astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(v.numpy())
    r[over] = np.nextafter(r[over], np.float16(0))
    return torch.from_numpy(r)


def round_half_away(v, prec):
    """float64 -> the type, nearest with ties away from zero"""
    t = round_toward_zero(v, prec)
    if prec == "bf16":
        u = (t.float().view(torch.int32) + 65536).view(torch.float32).to(torch.bfloat16)
    else:
        tn = t.numpy()
        u = torch.from_numpy(np.nextafter(tn, np.where(np.signbit(tn), -np.inf, np.inf).astype(np.float16)))
    exact = t.double() == v
    away = (v - t.double()).abs() >= (u.double() - v).abs()
    return torch.where(~exact & away, u, t)


MUTATIONS = ("truncate", "half_away", "drop_product", "swap_taps", "skip_block_last_tile", "residual_after_relu")


def applicable(c, mut):
    if mut in ("truncate", "half_away"):
        return c["prec"] != "f32"
    if mut == "swap_taps":
        return c["A3"].shape[1] > 1
    if mut == "residual_after_relu":
        return c.get("res") is not None and bool(c["relu"])
    return True


def evaluate(c, mut=None):
    """host result of a case in its output type, optionally subtly wrong:
      truncate / half_away   the final rounding
      drop_product           one (tap, channel) product missing
      swap_taps              the weights of two taps exchanged
      skip_block_last_tile   32 consecutive K positions (tap-major, then channel) missing in the rows of the last row tile
      residual_after_relu    relu(acc + bias) + residual"""
    A3, W4 = c["A3"], c["W4"]
    M, T, C = A3.shape
    if mut == "drop_product":
        t, ch = T // 2, C // 3
        W4 = W4.clone()
        W4[ch // W4.shape[3], :, t, ch % W4.shape[3]] = 0
    elif mut == "swap_taps":
        W4 = W4.clone()
        W4[:, :, [0, T - 1]] = W4[:, :, [T - 1, 0]]
    elif mut == "skip_block_last_tile":
        tile = c.get("tile", 128)
        first = (M - 1) // tile * tile
        A3 = A3.clone()
        flat = A3.reshape(M, T * C)
        k0 = min((T * C) // 2 // 32 * 32, max(T * C - 32, 0))
        flat[first:, k0:k0 + 32] = 0
    acc = grouped_acc(A3, W4, torch.float64)
    v = acc + c["bias"].double()
    if mut == "residual_after_relu":
        v = torch.relu(v) + c["res"].double()
    else:
        if c.get("res") is not None:
            v = v + c["res"].double()
        if c["relu"]:
            v = torch.relu(v)
    if mut == "truncate":
        return round_toward_zero(v, c["prec"])
    if mut == "half_away":
        return round_half_away(v, c["prec"])
    return v.to(DTYPES[c["prec"]])


# ---------------------------------------------------------------------------------------------------------------- GEMM
# (M, K, N, residual, relu, form); forms: None = dense; "slices" = in_ld > K, out_ld > N at a column offset, in2_ld > N;
# "pad128" = rows padded to 128 only; "argmax" = N = 19, fp32 logits + the fused label map; "per_image" = bias_per_image, batch 3
# of M / 3 pixels.  Which kernel each reaches: the docstring of test_gpu_exact_ops.py.
GEMM_CASES = [
    (300, 64, 64, False, True, None),
    (65, 256, 64, True, False, None),
    (777, 256, 128, True, False, None),
    (65, 2048, 192, True, True, None),
    (4097, 256, 256, False, False, "slices"),
    (777, 2048, 512, True, True, "slices"),
    (300, 256, 256, False, True, "pad128"),
    (1131, 256, 256, False, True, "per_image"),
]
GEMM_RING256 = (12288, 64, 1024, False, True, None)            # ceil(M / 256) * N / 256 = 192: the 256 x 256 ring by shape
GEMM_ARGMAX = [(65, 64, 19, False, False, "argmax"), (777, 256, 19, False, False, "argmax")]


def _seed(*parts):
    s = 17
    for p in parts:
        s = (s * 1000003 + int(p)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=2)
def _gemm_acc(M, K, N):
    s = _seed(M, K, N)
    A, W = ints(s, M, K), ints(s + 1, N, K)
    return A, W, exact_acc(A.view(M, 1, K), W.view(1, N, 1, K), extra=8000.0)


def gemm_case(case, prec):
    M, K, N, res, relu, form = case
    A, W, acc = _gemm_acc(M, K, N)
    s = _seed(M, K, N, len(prec), ord(prec[0]))
    c = {"A3": A.view(M, 1, K), "W4": W.view(1, N, 1, K), "acc": acc, "relu": relu, "prec": prec, "tile": 128 if N > 64 else 256}
    if form == "per_image":
        m = M // 3
        c["bias_rows"] = torch.stack([bias_for(N, s + 10 + n, prec, relu) for n in range(3)])
        c["bias"] = c["bias_rows"].repeat_interleave(m, dim=0)
    elif form == "argmax":
        c["bias"] = torch.randint(-40, 41, (N,), generator=torch.Generator().manual_seed(s)).float()
    else:
        c["bias"] = bias_for(N, s + 10, prec, relu)
    c["res"] = residual_for(M, N, s + 20, prec) if res else None
    assert float(c["bias"].abs().max()) + (float(c["res"].abs().max()) if res else 0.0) <= 8000.0
    c["v"] = finish(c)
    if form == "argmax":
        c["want"] = c["v"].float()
        assert torch.equal(c["want"].double(), c["v"])
        c["labels"] = torch.argmax(c["v"], dim=1)               # the first maximal index (torch on the CPU)
        top = c["v"].max(dim=1, keepdim=True).values
        c["tied_rows"] = int(((c["v"] == top).sum(dim=1) > 1).sum())
        assert c["tied_rows"] > 0, "no row has two maximal logits"
        first = (c["v"] == top).double().argmax(dim=1)
        assert torch.equal(first, c["labels"])
    else:
        c["want"] = expect(c["v"], prec)
        if not relu:
            assert 0.3 < float((c["v"] < 0).double().mean()) < 0.7
    return c


# ------------------------------------------------------------------------------------------------------- convolutions
def conv_weights(seed, G, co, T, cg, values=VALUES):
    return ints(seed, G * co * T, cg, values).reshape(G, co, T, cg) if cg >= 32 else \
        ints(seed, G * co, T * cg, values).reshape(G, co, T, cg)


@functools.lru_cache(maxsize=2)
def _conv_acc(B, H, W, C, G, k, stride, pad, dil, tag):
    """input [B][H][W][C], weights [G][C / G][k * k][C / G]; (x, W4, A3, acc, OH, OW)"""
    s = _seed(B, H, W, C, G, k, stride, pad, dil, tag)
    x = ints(s, B * H * W, C).reshape(B, H, W, C)
    cg = C // G
    W4 = conv_weights(s + 1, G, cg, k * k, cg)
    A3, OH, OW = im2col(x, k, stride, pad, dil)
    return x, W4, A3, exact_acc(A3, W4, extra=8000.0), OH, OW


def conv_case(H, W, C, G, k, stride, pad, dil, prec, relu=True, batch=1, tag=0):
    """a grouped k x k convolution C -> C (dense: G = 1 .. 4, grouped: cg = C / G <= 32, depthwise: G = C)"""
    x, W4, A3, acc, OH, OW = _conv_acc(batch, H, W, C, G, k, stride, pad, dil, tag)
    s = _seed(H, W, C, G, k, stride, pad, dil, ord(prec[0]), len(prec))
    c = {"x": x, "A3": A3, "W4": W4, "acc": acc, "relu": relu, "prec": prec, "OH": OH, "OW": OW, "res": None, "tile": 128,
         "bias": bias_for(C, s, prec, relu)}
    c["v"] = finish(c)
    c["want"] = expect(c["v"], prec)
    return c


def split_planes(v):
    """exact float64 -> (f16 hi, f16 lo) as the split kernels write them: hi = f16(v), lo = f16(v - hi)"""
    hi = v.to(torch.float16)
    lo32 = (v - hi.double()).float()
    assert torch.equal(lo32.double(), v - hi.double())
    return hi, lo32.to(torch.float16)


@functools.lru_cache(maxsize=2)
def _conv_split_acc(H, W, C, G, stride, dil, with_lo):
    """the dense 3x3 in its split form on DECOUPLED operands (test_gpu_gemm_exact.py): x = (Xh, Xl), weights = (W1, W2) from
    independent matrices: accumulator = W1 . Xh + W2 . Xh (+ W1 . Xl when the input has a lo plane)"""
    s = _seed(H, W, C, G, stride, dil, 77)
    cg = C // G
    xh, xl = ints(s, H * W, C).reshape(1, H, W, C), ints(s + 1, H * W, C).reshape(1, H, W, C)
    W1, W2 = conv_weights(s + 2, G, cg, 9, cg), conv_weights(s + 3, G, cg, 9, cg)
    Ah, OH, OW = im2col(xh, 3, stride, dil, dil)
    acc = exact_acc(Ah, W1, extra=8000.0) + exact_acc(Ah, W2, extra=8000.0)
    if with_lo:
        acc = acc + exact_acc(im2col(xl, 3, stride, dil, dil)[0], W1, extra=8000.0)
    assert 3 * 36 * 9 * cg + 8000 < LIMIT
    return xh, xl, W1, W2, acc, OH, OW


def conv_split_case(H, W, C, G, stride, dil, with_lo):
    xh, xl, W1, W2, acc, OH, OW = _conv_split_acc(H, W, C, G, stride, dil, with_lo)
    c = {"xh": xh, "xl": xl, "W1": W1, "W2": W2, "acc": acc, "relu": True, "OH": OH, "OW": OW,
         "bias": bias_for(C, _seed(H, W, C, 5), "f16", True)}
    c["v"] = finish(c)
    c["hi"], c["lo"] = split_planes(c["v"])
    rounding_conditions(c["v"], c["hi"], "f16")
    assert bool((c["lo"] != 0).any())
    return c


# --------------------------------------------------------------------------------------------------------------- stem
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalise_u8(img):
    """uint8 [..][3] -> float32, operation for operation what the stem kernels compute: ((float)px / 255.0f - mean) / std"""
    mean, std = torch.tensor(MEAN, dtype=torch.float32), torch.tensor(STD, dtype=torch.float32)
    return (img.float() / torch.tensor(255.0) - mean) / std


def coarse_bytes(prec):
    """per channel, the byte values whose normalised value, rounded to the 16-bit type, has magnitude >= 0.5: a multiple of
    2^-11 (f16) / 2^-8 (bf16), so that a 7 x 7 x 3 sum with weights in +-2 stays exact in fp32 (stem_case asserts the bound)"""
    dt = DTYPES["f16" if prec == "f32" else prec]
    lut = normalise_u8(torch.arange(256, dtype=torch.uint8).view(256, 1).expand(256, 3)).to(dt).float()
    return [torch.nonzero(lut[:, ch].abs() >= 0.5).reshape(-1).to(torch.uint8) for ch in range(3)]


def fma_chain(A3, W4, bias):
    """k_stem's own order: acc = bias, then acc = fmaf(x, w, acc) tap by tap, channel by channel, in fp32.  x * w is exact in
    float64 (24 + 3 bits) and so is its sum with an fp32 acc (exponents within 2^-31 .. 2^14), so rounding that sum to float32
    once is the fused multiply-add."""
    M, T, C = A3.shape
    acc = bias.float().view(1, -1).expand(M, W4.shape[1]).contiguous()
    w = W4[0].double()
    for t in range(T):
        for ch in range(C):
            acc = (A3[:, t, ch].double().view(M, 1) * w[:, t, ch].view(1, -1) + acc.double()).float()
    return acc.double()


def stem_case(H, W, in_format, kernel, prec, batch=1):
    """in_format "f32": integer planes (exact as everywhere else).  "u8": bytes; both stem kernels normalise them IN the kernel,
    so the operands are not integers: the MFMA kernel multiplies the 16-bit-rounded normalised values -- bytes from coarse_bytes,
    weights in +-2, and the sum is still exact in any order; the direct kernel (kernel = "direct") multiplies the fp32 values in
    one fmaf chain, which fma_chain mirrors step by step.  No exact integer ties exist then, only the 20 % condition is asserted."""
    s = _seed(H, W, batch, ord(in_format[0]), ord(kernel[0]), ord(prec[0]), len(prec))
    g = torch.Generator().manual_seed(s)
    c = {"relu": True, "prec": prec, "res": None, "tile": 256, "bias": bias_for(64, s + 2, prec, True)}
    if in_format == "f32":
        x = ints(s, batch * H * W, 3).reshape(batch, H, W, 3)
        c["W4"] = conv_weights(s + 1, 1, 64, 49, 3)
        c["planes"] = x.permute(0, 3, 1, 2).contiguous()
        c["A3"], c["OH"], c["OW"] = im2col(x, 7, 2, 3, 1)
        c["acc"] = exact_acc(c["A3"], c["W4"], extra=8000.0)
        c["v"] = finish(c)
        c["want"] = expect(c["v"], prec)
        return c
    allowed = coarse_bytes(prec)
    img = torch.stack([allowed[ch][torch.randint(0, len(allowed[ch]), (batch, H, W), generator=g)] for ch in range(3)], dim=3)
    c["img"] = img.contiguous()
    c["W4"] = conv_weights(s + 1, 1, 64, 49, 3, SMALL_VALUES)
    xn = normalise_u8(img)
    if kernel == "mfma":
        xn = xn.to(DTYPES[prec]).float()
        unit = 2.0 ** -11 if prec == "f16" else 2.0 ** -8
        assert torch.equal(torch.round(xn.double() / unit) * unit, xn.double())
        c["A3"], c["OH"], c["OW"] = im2col(xn, 7, 2, 3, 1)
        c["acc"] = exact_acc(c["A3"], c["W4"], extra=float(c["bias"].abs().max()), unit=unit)
        c["v"] = finish(c)
    else:
        c["A3"], c["OH"], c["OW"] = im2col(xn, 7, 2, 3, 1)
        c["acc"] = None
        c["v"] = torch.relu(fma_chain(c["A3"], c["W4"], c["bias"]))
    c["want"] = c["v"].to(DTYPES[prec])
    assert bool(torch.isfinite(c["want"]).all())
    if prec != "f32":
        rounding_conditions(c["v"], c["want"], prec, ties=False)
    else:
        assert torch.equal(c["want"].double(), c["v"])
    return c


# ---------------------------------------------------------------------------------- fused depthwise 3x3 + pointwise
DW_VALUES = [0, 0, 0, 0, 0, 0, 1, -1, 1, -1, 1, -1, 0, 0, 1, -1]


def dwpw_case(H, W, K, N, dil, pad, prec, relu=True, dw_mut=None):
    """depthwise weights in {0, +-1}, bias within +-20: the intermediate relu(dw) is an integer below 256, exact in both 16-bit
    types; the pointwise stage is a GEMM on it under the usual bound (|mid| <= 74, |w| <= 6)"""
    s = _seed(H, W, K, N, dil, pad)
    x = ints(s, H * W, K).reshape(1, H, W, K)
    Wd = conv_weights(s + 1, K, 1, 9, 1, DW_VALUES)
    if dw_mut == "swap_taps":
        Wd = Wd.clone()
        Wd[:, :, [0, 8]] = Wd[:, :, [8, 0]]
    b1 = torch.randint(-20, 21, (K,), generator=torch.Generator().manual_seed(s + 2)).float()
    A1, OH, OW = im2col(x, 3, 1, pad, dil)
    mid = torch.relu(exact_acc(A1, Wd) + b1.double())
    assert float(mid.max()) < 256 and torch.equal(mid.to(DTYPES[prec]).double(), mid)
    W2 = ints(s + 3, N, K)
    M = OH * OW
    c = {"x": x, "Wd": Wd, "b1": b1, "A3": mid.float().view(M, 1, K), "W4": W2.view(1, N, 1, K), "relu": relu, "prec": prec, "res": None,
         "OH": OH, "OW": OW, "tile": 128, "bias": bias_for(N, _seed(s, ord(prec[0])), prec, relu)}
    c["acc"] = exact_acc(c["A3"], c["W4"], extra=8000.0)
    c["v"] = finish(c)
    c["want"] = expect(c["v"], prec)
    return c


# ------------------------------------------------------------------------------------------------------- the case lists
# dense 3x3 (w_layout 2): (H, W, cg, G, stride, dilation); the G = 4 case also runs as channel slices of wider buffers
CONV3X3_CASES = [(8, 16, 64, 1, 1, 1), (23, 45, 64, 1, 2, 1), (13, 21, 256, 1, 1, 2), (9, 19, 1024, 1, 1, 4), (3, 5, 256, 1, 1, 4),
                 (21, 35, 64, 4, 1, 4), (11, 18, 256, 1, 2, 1)]
CONV3X3_SPLIT = [(c, True) for c in CONV3X3_CASES] + [((23, 45, 64, 1, 2, 1), False), ((13, 21, 256, 1, 1, 2), False)]
# grouped 3x3 on the matrix cores (w_layout 1), G = 32: (H, W, cg, stride, dilation)
GCONV_MFMA_CASES = [(23, 45, 4, 1, 1), (23, 45, 8, 2, 1), (15, 21, 16, 1, 2), (9, 31, 32, 1, 4), (8, 8, 2, 1, 1), (23, 45, 8, 2, 2),
                    (5, 33, 2, 2, 1), (30, 41, 16, 1, 1), (19, 67, 32, 2, 1),
                    (97, 33, 32, 1, 1)]        # 16 slots for 26 tiles of 8 rows (2 rounds) or 50 of 4 rows (4 rounds): the 8-row tile, NJ = 4
# the direct grouped 3x3 (w_layout 0), G = 16: cg x (H, W, stride, dilation)
GCONV_DIRECT_CG = [2, 4, 8, 16, 32]
GCONV_DIRECT_SHAPES = [(13, 21, 1, 1), (11, 17, 2, 2), (9, 14, 1, 4)]
# depthwise 3x3: (H, W, C, dilation, pad, relu)
DW3_CASES = [(17, 23, 64, 1, 0, True), (17, 23, 128, 12, 12, False), (20, 31, 320, 24, 24, True), (40, 17, 64, 36, 36, False),
             (9, 9, 64, 2, 2, True), (3, 3, 320, 1, 1, False), (1, 70, 64, 6, 6, True)]
# depthwise k x k: ksize x (H, W, C, batch)
DWK_KS = [1, 2, 4, 5, 6, 7]
DWK_SHAPES = [(13, 29, 64, 1), (15, 37, 320, 2)]
STEM_SIZES = [(33, 47), (7, 250), (224, 9)]
# fused depthwise + pointwise: (H, W, K, N, dilation, pad, relu); the kernel always applies both ReLUs
DWPW_CASES = [(19, 27, 128, 256, 12, 12, True), (6, 11, 2048, 256, 24, 24, True), (9, 9, 64, 48, 2, 2, True), (16, 16, 256, 512, 1, 1, True),
              (13, 21, 512, 256, 1, 0, True), (11, 20, 64, 256, 3, 1, True)]
