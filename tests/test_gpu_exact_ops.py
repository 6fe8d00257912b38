"""The plain (single-plane) GEMM and convolution kernels, each op ALONE through avl_seg_plan_*, on operands whose result is known
to the bit: every element of everything the op writes is compared with torch.equal.

Why.  test_gpu_ops.py, test_gpu_conv3x3.py and test_gpu_refine_kernel.py compare these kernels on Gaussian operands with a bar
relative to the LARGEST output (1.5 * 2^-8 for bf16, 1.5 * 2^-11 for f16, twice that for the 3x3s).  Truncation instead of round to
nearest even, one missing K element, a missing 32-channel block of one tap or a wrong tap on a border row all pass that bar.
Everything chosen per type or per tile configuration -- the 16-bit MFMA and its operand packing, the 16-bit epilogue, the four
16-bit GEMM tile configurations -- was seen only through it.

Operand design (tests/_exact_operands.py; test_exact_operands_cpu.py checks every condition below without a GPU).
  * Activations and weights are integers of {0, +-1, +-2, +-3, +-4, +-6}, zeros frequent, some 32-blocks along K all zero or holding
    one non-zero: exact in bf16, f16 and f32; every product is an integer.
  * Bound: while 36 * K_total + |bias| + |residual| < 2^24 (K_total = taps x channels per group; at most 36 * 9216 + 8000 here)
    fp32 accumulation is exact in ANY order, and the float32 host evaluation equals the float64 one (asserted per case).
  * Bias: integers, most columns where the type rounds integers (bf16 256 .. 1536, f16 2048 .. 7000); residual: integers exact in
    the type, both signs.  >= 20 % of the expected 16-bit outputs are not representable before rounding, and exact ties (odd
    integers of [256, 512) in bf16, [2048, 4096) in f16) round down to even and up to even in every case.  Sums are negative about
    half the time; cases alternate ReLU on / off where the op has the switch (the grouped / dense 3x3, the stem and the fused op
    always apply it).
  * Expected, with v the exact float64 result: v.to(type) (round to nearest even) for the 16-bit ops, v.float() for fp32 ops and
    for the fp32 logits of the classifier, whose label map equals argmax with the first index winning ties (the integer logits
    hold ties: asserted).  Split dense 3x3: hi = f16(v), lo = f16(v - hi), on decoupled operands as in test_gpu_gemm_exact.py
    (weights W1 | W2 and planes Xh, Xl from independent matrices: W1.Xh + W2.Xh + W1.Xl).
  * Stem.  AVL_IN_F32_CHW planes hold the integers themselves.  A uint8 image is normalised IN both stem kernels
    (((float)px / 255 - mean) / std in fp32), so those operands are not integers: the MFMA kernel multiplies the normalised values
    rounded to the 16-bit type -- the image uses the bytes whose rounded value is a multiple of 2^-11 (f16) / 2^-8 (bf16), the weights
    +-2, and the sum is still exact in any order --; the direct kernel runs ONE fmaf chain over the fp32 values, which the host
    mirrors step by step (fma_chain).  These cases have no integer ties; they assert the 20 % condition only.
  * OP_DWPW: depthwise weights in {0, +-1}, bias within +-20: relu(depthwise) is an integer below 256, exact in both 16-bit types.

Which kernel a case reaches (the launchers of csrc/):
  OP_GEMM: GEMM_KERNELS below names the kernel of every case, type and w_layout; _run_gemm asserts it against the library's own answer
    (avl_seg_gemm_route, whose comment in include/avl_hip.h states the rule) for the op that runs.
  OP_GCONV w_layout 2: k_conv3x3<T, 0, false, NQ> with NQ = 2 iff cg % 128 == 0 (cg 256, 1024), NQ = 1 for cg 64; split:
    k_conv3x3<f16, 1, XS, NQ>, XS = the input has a lo plane.  Stride 1 with dilation > 1 walks the d x d residue classes ("comb").
  OP_GCONV w_layout 1: k_gconv_mfma<T, 0, NJ, false>, NJ (tile height 2 NJ) picked by gconv_pick_th from the shape;
    stride 2 + dilation 2 is its two-row tile (NJ = 1), (97, 33) at C = 1024 the eight-row tile (NJ = 4).  w_layout 0: k_gconv<T, CG>, CG in {2, 4, 8, 16, 32}.
  OP_DWCONV: ksize 3 -> k_dwconv<T, false> (C = 320: 40 channel chunks, the lanes do not fill the workgroup; dilation 1 walks
    bands, dilation > 1 combs, chained when small); other ksize -> k_dwconv_k<T, FORM_HALF or FORM_F32, KS>.
  OP_STEM: w_layout 0 -> k_stem<T, F32IN>; w_layout 1 -> k_stem_mfma<T, false, false, F32IN>.
  OP_DWPW: k_dwpw<T, 1>.

Hardware observation (MI355X): v_mfma_f32_16x16x32_bf16, v_mfma_f32_16x16x32_f16 and v_mfma_f32_16x16x4_f32 accumulate these dot
products exactly, and so do the fp32 FMA chains and the packed 16-bit dot products of the direct kernels: every case below is
bit-equal to the host's result rounded once to nearest even."""
import pytest

import _exact_operands as X

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def _types(prec):
    import torch
    from vision_semantic_segmentation_amd import _lib
    return X.DTYPES[prec], {"f32": _lib.AVL_F32, "bf16": _lib.AVL_BF16, "f16": _lib.AVL_F16}[prec]


def _up(n, m):
    return (n + m - 1) // m * m


def _same(got, want, what):
    """torch.equal on everything; the message says which elements differ and by how much (that pattern tells an indexing bug from a
    rounding rule from an inexact accumulation)"""
    import torch
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    bad = torch.nonzero(g != w)
    diff = (g - w).abs()
    first = [(tuple(i.tolist()), float(g[tuple(i)]), float(w[tuple(i)])) for i in bad[:6]]
    print("%s: %d of %d differ, max |diff| %g, rows %d..%d, columns %d..%d, first (index, got, want): %s"
          % (what, bad.shape[0], w.numel(), float(diff.max()), int(bad[:, 0].min()), int(bad[:, 0].max()), int(bad[:, 1].min()),
             int(bad[:, 1].max()), first))
    assert torch.equal(got, want), "%s: %d of %d values differ, max |diff| %g" % (what, bad.shape[0], w.numel(), float(diff.max()))


# ------------------------------------------------------------------------------------------------------------------- GEMM
# The kernel of every GEMM case: (under fp32, [under a 16-bit type T with w_layout 0, 1, 2, 3, 4]).  k_gemm<T, WM, WN> has tiles of
# WM * 64 x WN * 64, k_gemm_ring<T, WM, WN, MI, STAGES, NSUB, IO, AST, EXT> of 256 x WN * 64 (WM = MI = 2, 8: on four waves).
_P64, _P128, _F64, _F128 = "k_gemm<T, 4, 1>", "k_gemm<T, 2, 2>", "k_gemm<float, 4, 1>", "k_gemm<float, 2, 2>"
_R128, _R256, _R4W = ("k_gemm_ring<T, 4, 2, 4, 3, 1, 0, 3, false>", "k_gemm_ring<T, 2, 4, 8, 2, 1, 0, 2, false>",
                      "k_gemm_ring<T, 2, 2, 8, 3, 1, 0, 3, false>")
GEMM_KERNELS = {
    (300, 64, 64, False, True, None): (_F64, [_P64] * 5),                                   # N = 64: the small-N kernel, whatever is forced
    (65, 256, 64, True, False, None): (_F64, [_P64] * 5),
    (777, 256, 128, True, False, None): (_F128, [_R128, _P128, _R128, _R128, _R4W]),        # N = 128: a forced 256 x 256 falls back
    (65, 2048, 192, True, True, None): (_F128, [_P128] * 5),                                # N = 192 is no multiple of 128
    (4097, 256, 256, False, False, "slices"): (_F128, [_R128, _P128, _R128, _R256, _R4W]),  # 17 tiles of 256 x 256: by shape 256 x 128
    (777, 2048, 512, True, True, "slices"): (_F128, [_R128, _P128, _R128, _R256, _R4W]),
    (300, 256, 256, False, True, "pad128"): (_F128, [_P128] * 5),                           # rows padded to 128 only
    (1131, 256, 256, False, True, "per_image"): (_F128, [_R128]),                           # three launches of 377 rows
    X.GEMM_RING256: (_F128, [_R256]),                                                       # 48 x 4 = 192 tiles of 256 x 256
    X.GEMM_ARGMAX[0]: (_F64, [_P64]), X.GEMM_ARGMAX[1]: (_F64, [_P64]),                     # N = 19
}


def _run_gemm(case, prec, layout, dev):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import OP_GEMM, AvlSegOp, gemm_kernel_name, gemm_route
    M, K, N, res, relu, form = case
    c = X.gemm_case(case, prec)
    tdt, did = _types(prec)
    argmax, slices = form == "argmax", form == "slices"
    batch = 3 if form == "per_image" else 1
    m = M // batch
    Mp = (batch - 1) * m + _up(m, 128 if form == "pad128" else 256)
    Np = 64 if argmax else _up(N, 256)
    in_ld, in_off = (K + 96, 64) if slices else (K, 0)
    out_ld, out_off = (N + 128, 64) if slices else (N, 0)
    r_ld = N + 32 if slices else N
    seed = M + K + N
    a = torch.full((Mp, in_ld), float("nan"))                    # poison outside the input slice; rows past M hold values: they are
    a[:, in_off:in_off + K] = X.ints(seed, Mp, K)                # read and must reach no output
    a[:M, in_off:in_off + K] = c["A3"].view(M, K)
    w = X.ints(seed + 1, Np, K)                                  # so do the weight rows past N
    w[:N] = c["W4"].view(N, K)
    if batch > 1:
        b = torch.full((batch, Np), 12345.0)
        b[:, :N] = c["bias_rows"]
    else:
        b = torch.full((Np,), 12345.0)
        b[:N] = c["bias"]
    ad, wd, bd = a.to(tdt).to(dev), w.to(tdt).to(dev), b.to(dev)
    out = torch.full((Mp + 16, out_ld), SENTINEL, dtype=torch.float32 if argmax else tdt, device=dev)
    es = ad.element_size()
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = OP_GEMM, did, batch if batch > 1 else 0
    op.bias_per_image = int(batch > 1)
    op.in_, op.out, op.weight, op.bias = ad.data_ptr() + in_off * es, out.data_ptr() + out_off * es, wd.data_ptr(), bd.data_ptr()
    h, wdt = (13, 29) if batch > 1 else (1, M)
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = h, wdt, K, in_ld, Mp
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = h, wdt, N, out_ld, Mp
    op.relu, op.out_f32, op.w_rows, op.ksize, op.stride, op.dil, op.groups = int(relu), int(argmax), Np, 1, 1, 1, 1
    op.w_layout = layout
    if res:
        r = torch.full((Mp, r_ld), float("nan"))
        r[:M, :N] = c["res"]
        rd = r.to(tdt).to(dev)
        op.in2, op.in2_ld = rd.data_ptr(), r_ld
    if argmax:
        labels = torch.full((Mp,), 99, dtype=torch.uint8, device=dev)
        op.out_mx = labels.data_ptr()
    route = gemm_route(op)
    f32_kernel, half_kernels = GEMM_KERNELS[case]
    assert gemm_kernel_name(route) == (f32_kernel if prec == "f32" else half_kernels[layout].replace("T", prec)), (case, prec, layout)
    assert route["launches"] == batch
    _run_plan([op])
    o = out.cpu()
    _same(o[:M, out_off:out_off + N], c["want"], "gemm %s %s layout %d" % (case, prec, layout))
    assert torch.all(o[M:] == SENTINEL)                                                     # rows past M
    assert torch.all(o[:, :out_off] == SENTINEL) and torch.all(o[:, out_off + N:] == SENTINEL)      # columns outside the slice
    if argmax:
        lab = labels.cpu()
        assert torch.equal(lab[:M].long(), c["labels"]), "%d labels differ" % int((lab[:M].long() != c["labels"]).sum())
        assert torch.all(lab[M:] == 99)


_GEMM_PARAMS = [(case, prec, layout) for case in X.GEMM_CASES for prec in ("f32", "bf16", "f16")
                for layout in ((0,) if prec == "f32" or case[5] == "per_image" else (0, 1, 2, 3, 4))]


@pytest.mark.parametrize("case,prec,layout", _GEMM_PARAMS, ids=lambda p: str(p).replace(" ", ""))
def test_gemm_exact(case, prec, layout, cuda_device):
    _run_gemm(case, prec, layout, cuda_device)


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
def test_gemm_exact_ring_256x256_by_shape(prec, cuda_device):
    """(12288, 64, 1024): 48 row tiles x 4 = 192 tiles of 256 x 256, the smallest count at which w_layout 0 picks that ring"""
    _run_gemm(X.GEMM_RING256, prec, 0, cuda_device)


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", X.GEMM_ARGMAX, ids=lambda c: "%d-%d-%d" % c[:3])
def test_gemm_exact_classifier_and_labels(case, prec, cuda_device):
    """N = 19, fp32 logits (exact) with out_ld = 19 and the fused label map; ties between integer logits are plentiful"""
    _run_gemm(case, prec, 0, cuda_device)


# ------------------------------------------------------------------------------------------------------- convolutions
def _rows(t, rows, ld=None, off=0, fill=0.0):
    """[m][c] -> [rows][ld] with the values at column `off`"""
    import torch
    out = torch.full((rows, ld or t.shape[1]), fill, dtype=t.dtype)
    out[:t.shape[0], off:off + t.shape[1]] = t
    return out


def _conv_op(kind, did, src, dst, c, H, W, Cc, in_off=0, out_off=0, **f):
    """the op of a C -> C convolution on row buffers src / dst (the channels at column in_off / out_off)"""
    from test_gpu_ops import _spatial_op
    op = _spatial_op(kind, did, src, (H, W), Cc, dst, (c["OH"], c["OW"]), Cc, **f)
    op.in_ += in_off * src.element_size()
    op.out += out_off * dst.element_size()
    return op


def _check_conv(dst, want, M, Cc, out_off, what):
    import torch
    o = dst.cpu()
    _same(o[:M, out_off:out_off + Cc], want, what)
    assert torch.all(o[M:] == SENTINEL) and torch.all(o[:, :out_off] == SENTINEL) and torch.all(o[:, out_off + Cc:] == SENTINEL)


def _w_oihw(W4, k):
    """[G][co][T][cg] -> float64 [C][cg][k][k]"""
    G, co, T, cg = W4.shape
    return W4.reshape(G * co, k, k, cg).permute(0, 3, 1, 2).double().contiguous()


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", X.CONV3X3_CASES, ids=str)
def test_dense_conv3x3_exact(case, prec, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import OP_GCONV, pack_conv3x3
    H, W, cg, G, s, d = case
    Cc = cg * G
    c = X.conv_case(H, W, Cc, G, 3, s, d, d, prec)
    tdt, did = _types(prec)
    M = c["OH"] * c["OW"]
    ci0, co0, in_ld, out_ld = (64, 128, Cc + 128, Cc + 192) if G == 4 else (0, 0, Cc, Cc)
    src = _rows(c["x"].reshape(H * W, Cc).to(tdt), _up(H * W, 256), in_ld, ci0, SENTINEL).to(cuda_device)
    dst = torch.full((_up(M, 256), out_ld), SENTINEL, dtype=tdt, device=cuda_device)
    wd = pack_conv3x3(_w_oihw(c["W4"], 3), G, 4 if prec == "f32" else 8).to(tdt).to(cuda_device)
    bd = c["bias"].to(cuda_device)
    _run_plan([_conv_op(OP_GCONV, did, src, dst, c, H, W, Cc, ci0, co0, weight=wd.data_ptr(), bias=bd.data_ptr(), ksize=3, stride=s,
                        pad=d, dil=d, groups=G, relu=1, w_layout=2)])
    _check_conv(dst, c["want"], M, Cc, co0, "dense 3x3 %s %s" % (case, prec))


@pytest.mark.parametrize("case,with_lo", X.CONV3X3_SPLIT, ids=str)
def test_dense_conv3x3_split_exact(case, with_lo, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_GCONV, pack_conv3x3
    H, W, cg, G, s, d = case
    Cc = cg * G
    c = X.conv_split_case(H, W, Cc, G, s, d, with_lo)
    M = c["OH"] * c["OW"]
    ci0, co0, in_ld, out_ld = (64, 128, Cc + 128, Cc + 192) if G == 4 else (0, 0, Cc, Cc)
    f16 = torch.float16
    src = torch.stack([_rows(c[k].reshape(H * W, Cc).to(f16), _up(H * W, 256), in_ld, ci0, SENTINEL) for k in ("xh", "xl")]).to(cuda_device)
    dst = torch.full((2, _up(M, 256), out_ld), SENTINEL, dtype=f16, device=cuda_device)
    # fragments [g][chunk][tap][nb][nj][part][1024]: part 0 = W1, part 1 = W2 (pack_conv3x3 lays hi | lo out this way)
    parts = [pack_conv3x3(_w_oihw(c[k], 3), G, 8).reshape(G, cg // 64, 9, cg // 32, 2, 1, 1024) for k in ("W1", "W2")]
    wd = torch.cat(parts, dim=5).reshape(-1).to(f16).contiguous().to(cuda_device)
    bd = c["bias"].to(cuda_device)
    op = _conv_op(OP_GCONV, _lib.AVL_F16, src[0], dst[0], c, H, W, Cc, ci0, co0, weight=wd.data_ptr(), bias=bd.data_ptr(), ksize=3,
                  stride=s, pad=d, dil=d, groups=G, relu=1, w_layout=2, w_split=1)
    op.out_lo = dst[1].data_ptr() + co0 * 2
    if with_lo:
        op.in_lo = src[1].data_ptr() + ci0 * 2
    _run_plan([op])
    _check_conv(dst[0], c["hi"], M, Cc, co0, "split dense 3x3 %s hi" % (case,))
    _check_conv(dst[1], c["lo"], M, Cc, co0, "split dense 3x3 %s lo" % (case,))


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("case", X.GCONV_MFMA_CASES, ids=str)
def test_grouped_conv_mfma_exact(case, prec, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import OP_GCONV, pack_gconv_windows
    H, W, cg, s, d = case
    G, Cc = 32, 32 * cg
    c = X.conv_case(H, W, Cc, G, 3, s, d, d, prec)
    tdt, did = _types(prec)
    M = c["OH"] * c["OW"]
    src = _rows(c["x"].reshape(H * W, Cc).to(tdt), _up(H * W, 256)).to(cuda_device)
    dst = torch.full((_up(M, 256), Cc), SENTINEL, dtype=tdt, device=cuda_device)
    wd = pack_gconv_windows(_w_oihw(c["W4"], 3), G).to(tdt).to(cuda_device)
    bd = c["bias"].to(cuda_device)
    _run_plan([_conv_op(OP_GCONV, did, src, dst, c, H, W, Cc, weight=wd.data_ptr(), bias=bd.data_ptr(), ksize=3, stride=s, pad=d, dil=d,
                        groups=G, relu=1, w_layout=1)])
    _check_conv(dst, c["want"], M, Cc, 0, "grouped MFMA conv %s %s" % (case, prec))


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("cg", X.GCONV_DIRECT_CG)
def test_grouped_conv_direct_exact(cg, prec, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import OP_GCONV
    G, Cc = 16, 16 * cg
    tdt, did = _types(prec)
    for H, W, s, d in X.GCONV_DIRECT_SHAPES:
        c = X.conv_case(H, W, Cc, G, 3, s, d, d, prec)
        M = c["OH"] * c["OW"]
        src = _rows(c["x"].reshape(H * W, Cc).to(tdt), _up(H * W, 256)).to(cuda_device)
        dst = torch.full((_up(M, 256), Cc), SENTINEL, dtype=tdt, device=cuda_device)
        wd = c["W4"].permute(0, 2, 3, 1).reshape(-1).contiguous().to(cuda_device)          # fp32 [g][tap][ci][co]
        bd = c["bias"].to(cuda_device)
        _run_plan([_conv_op(OP_GCONV, did, src, dst, c, H, W, Cc, weight=wd.data_ptr(), bias=bd.data_ptr(), ksize=3, stride=s, pad=d,
                            dil=d, groups=G, relu=1, w_layout=0)])
        _check_conv(dst, c["want"], M, Cc, 0, "direct grouped conv cg %d (%d, %d, s%d, d%d) %s" % (cg, H, W, s, d, prec))


def _run_depthwise(c, H, W, Cc, ks, pad, d, relu, batch, prec, dev, what):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import OP_DWCONV
    tdt, did = _types(prec)
    M = batch * c["OH"] * c["OW"]
    tail = 8 if batch > 1 else _up(H * W, 256) - H * W            # allocated rows past the input
    src = _rows(c["x"].reshape(batch * H * W, Cc).to(tdt), batch * H * W + tail).to(dev)
    dst = torch.full((M + 16, Cc), SENTINEL, dtype=tdt, device=dev)
    wd = c["W4"].reshape(Cc, ks * ks).t().contiguous().to(dev)                               # fp32 [tap][C]
    bd = c["bias"].to(dev)
    zero = torch.zeros(64, dtype=torch.uint8, device=dev)
    op = _conv_op(OP_DWCONV, did, src, dst, c, H, W, Cc, weight=wd.data_ptr(), bias=bd.data_ptr(), in2=zero.data_ptr(), ksize=ks, stride=1,
                  pad=pad, dil=d, groups=Cc, relu=int(relu), batch=batch if batch > 1 else 0)
    op.in_rows, op.out_rows = batch * H * W, M
    _run_plan([op])
    _check_conv(dst, c["want"], M, Cc, 0, what)


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", X.DW3_CASES, ids=str)
def test_depthwise_3x3_exact(case, prec, cuda_device):
    H, W, Cc, d, pad, relu = case
    c = X.conv_case(H, W, Cc, Cc, 3, 1, pad, d, prec, relu=relu)
    _run_depthwise(c, H, W, Cc, 3, pad, d, relu, 1, prec, cuda_device, "depthwise 3x3 %s %s" % (case, prec))


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("ks", X.DWK_KS)
def test_depthwise_kxk_exact(ks, prec, cuda_device):
    for H, W, Cc, batch in X.DWK_SHAPES:
        relu = bool(ks & 1)
        c = X.conv_case(H, W, Cc, Cc, ks, 1, 0, 1, prec, relu=relu, batch=batch)
        _run_depthwise(c, H, W, Cc, ks, 0, 1, relu, batch, prec, cuda_device, "depthwise k = %d (%d, %d, C %d, batch %d) %s" % (ks, H, W, Cc, batch, prec))


# --------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("prec,kernel", [("f32", "direct"), ("bf16", "direct"), ("f16", "direct"), ("bf16", "mfma"), ("f16", "mfma")])
@pytest.mark.parametrize("in_format", ["u8", "f32"])
@pytest.mark.parametrize("hw", X.STEM_SIZES, ids=str)
def test_stem_exact(hw, in_format, prec, kernel, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import AVL_IN_F32_CHW, AVL_IN_U8_HWC, OP_STEM, AvlSegOp, pack_stem_mfma
    H, W = hw
    c = X.stem_case(H, W, in_format, kernel, prec)
    tdt, did = _types(prec)
    M = c["OH"] * c["OW"]
    src = (c["img"] if in_format == "u8" else c["planes"]).to(cuda_device)
    out = torch.full((M + 16, 64), SENTINEL, dtype=tdt, device=cuda_device)
    w = c["W4"][0].reshape(64, 7, 7, 3)                                                       # [co][ky][kx][ci]
    if kernel == "mfma":
        wd = pack_stem_mfma(w.permute(0, 3, 1, 2).double()).to(tdt).to(cuda_device)
    else:
        wd = w.permute(1, 2, 3, 0).reshape(-1).contiguous().to(cuda_device)                 # fp32 [7][7][3][64]
    bd = c["bias"].to(cuda_device)
    op = AvlSegOp()
    op.kind, op.dtype = OP_STEM, did
    op.in_format = AVL_IN_U8_HWC if in_format == "u8" else AVL_IN_F32_CHW
    op.in_, op.out, op.weight, op.bias = src.data_ptr(), out.data_ptr(), wd.data_ptr(), bd.data_ptr()
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = H, W, 3, 3, H * W
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = c["OH"], c["OW"], 64, 64, M
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu, op.w_layout = 7, 2, 3, 1, 1, 1, int(kernel == "mfma")
    _run_plan([op])
    _check_conv(out, c["want"], M, 64, 0, "stem %s %s %s %s" % (hw, in_format, kernel, prec))


# ---------------------------------------------------------------------------------- fused depthwise 3x3 + pointwise
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("case", X.DWPW_CASES, ids=str)
def test_fused_depthwise_pointwise_exact(case, prec, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import OP_DWPW, AvlSegOp, dwpw_tile_order, pack_dw_pairs
    H, W, K, N, d, pad, relu = case
    c = X.dwpw_case(H, W, K, N, d, pad, prec, relu)
    tdt, did = _types(prec)
    OH, OW = c["OH"], c["OW"]
    M, Mp, Np = OH * OW, _up(OH * OW, 256), _up(N, 256)
    src = _rows(c["x"].reshape(H * W, K).to(tdt), _up(H * W, 256)).to(cuda_device)
    w1 = c["Wd"].reshape(K, 1, 3, 3).double()
    params = torch.cat([pack_dw_pairs(w1, c["b1"].double(), tdt), dwpw_tile_order(OH, OW, d)]).to(cuda_device)
    w2 = X.ints(K + N, Np, K)                                    # rows past N hold values: they must reach no output
    w2[:N] = c["W4"].view(N, K)
    b2 = torch.full((Np,), 12345.0)
    b2[:N] = c["bias"]
    w2d, b2d = w2.to(tdt).to(cuda_device), b2.to(cuda_device)
    out = torch.full((Mp, N + 16), SENTINEL, dtype=tdt, device=cuda_device)            # a column slice of a wider buffer
    op = AvlSegOp()
    op.kind, op.dtype = OP_DWPW, did
    op.in_, op.in2, op.out = src.data_ptr(), params.data_ptr(), out.data_ptr() + 16 * out.element_size()
    op.weight, op.bias = w2d.data_ptr(), b2d.data_ptr()
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = H, W, K, K, src.shape[0]
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = OH, OW, N, N + 16, Mp
    op.relu, op.w_rows, op.ksize, op.stride, op.pad, op.dil, op.groups = int(relu), Np, 3, 1, pad, d, K
    _run_plan([op])
    _check_conv(out, c["want"], M, N, 16, "dwpw %s %s" % (case, prec))
