"""The small ops of the segmentation plan run ALONE through avl_seg_plan_*: AVL_OP_GAP (the ASPP pooling branch), AVL_OP_GEMV (its two
1x1 convs on the pooled vector), AVL_OP_SUBSAMPLE (the strided 1x1 convs' input rows) and AVL_OP_ARGMAX (torch.argmax over the logits).

GAP and GEMV are fed small integers (exact in bf16 / f16 / fp32, every partial sum below 2^24), so every fp32 sum the kernels form is
exact whatever its order: the expected values are exact too (GAP: float32(sum) / float32(M), correctly rounded), and one dropped or
repeated row, column or vector element fails the comparison.  SUBSAMPLE copies bits; ARGMAX is compared with torch.argmax on the CPU.
Every output sits between sentinels (columns outside the op's slice, rows past the output) that must survive; inputs carry poison
(large values or NaN) in the rows and columns the op must not read.

avl_seg_plan_nonfinite (the load-time self-check of a checkpoint) is run on one- to three-op plans of every rule it has: the exact
counts come from a host model of the op's stored planes."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _did(name):
    from vision_semantic_segmentation_amd import _lib
    return {"f32": _lib.AVL_F32, "bf16": _lib.AVL_BF16, "f16": _lib.AVL_F16}[name]


def _run(op):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan)), "avl_seg_plan_create")
    try:
        _lib.check(_lib.lib().avl_seg_plan_run(plan, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "avl_seg_plan_run")
        torch.cuda.synchronize()
    finally:
        _lib.lib().avl_seg_plan_destroy(plan)


def _op(kind, dtype_id, **f):
    from vision_semantic_segmentation_amd.network import AvlSegOp
    op = AvlSegOp()
    op.kind, op.dtype = kind, dtype_id
    op.ksize = op.stride = op.dil = op.groups = 1
    for k, v in f.items():
        setattr(op, k, v)
    return op


# ------------------------------------------------------------------------------------------------ AVL_OP_GAP
# (h, w): M = h * w straddles the 256 slices of k_gap_partial (G = 256) and its loop of four rows in flight
GAP_HW = {1: (1, 1), 81: (9, 9), 255: (15, 17), 256: (16, 16), 257: (1, 257), 1023: (31, 33), 1024: (32, 32), 1027: (13, 79),
          32400: (135, 240)}


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", [  # (M, C, in_ld - C, batch, out_ld - C)
    (1, 8, 0, 1, 0), (81, 256, 8, 1, 0), (255, 8, 8, 3, 5), (256, 256, 0, 1, 0), (257, 2048, 64, 1, 0), (1023, 256, 0, 3, 3),
    (1024, 8, 16, 1, 0), (1027, 2048, 0, 3, 1), (32400, 256, 8, 1, 0), (32400, 8, 0, 3, 7),
])
def test_gap_exact(case, dtype, cuda_device):
    from vision_semantic_segmentation_amd.network import OP_GAP
    M, Cc, ldpad, batch, opad = case
    h, w = GAP_HW[M]
    tdt = DTYPES[dtype]
    in_ld, out_ld = Cc + ldpad, Cc + opad
    g = torch.Generator().manual_seed(M + Cc + batch)
    vals = torch.randint(-8, 9, (batch * M, Cc), generator=g, dtype=torch.int64)
    x = torch.full((batch * M + 300, in_ld), 1000.0)          # poison: rows past the last image, columns past C
    x[:batch * M, :Cc] = vals.float()
    xd = x.to(tdt).to(cuda_device)
    scratch = torch.full((batch, 256, Cc), float("nan"), device=cuda_device)
    out = torch.full((batch + 1, out_ld), float("nan"), device=cuda_device)
    _run(_op(OP_GAP, _did(dtype), in_=xd.data_ptr(), in2=scratch.data_ptr(), out=out.data_ptr(), in_h=h, in_w=w, in_c=Cc, in_ld=in_ld,
             in_rows=xd.shape[0], out_h=1, out_w=1, out_c=Cc, out_ld=out_ld, out_rows=batch, batch=batch))
    sums = vals.reshape(batch, M, Cc).sum(1)                  # exact (int64)
    want = sums.to(torch.float32) / torch.tensor(float(M), dtype=torch.float32)
    got = out.cpu()
    assert torch.equal(got[:batch, :Cc], want), "gap M=%d C=%d batch %d %s: max |d| %g" % (
        M, Cc, batch, dtype, float((got[:batch, :Cc] - want).abs().nan_to_num(1e30).max()))
    assert bool(got[:batch, Cc:].isnan().all()) and bool(got[batch:].isnan().all())       # columns past C, rows past the batch


# ------------------------------------------------------------------------------------------------ AVL_OP_GEMV
@pytest.mark.parametrize("case", [  # (K, N, batch, in_ld - K, out_ld - N, input 4 bytes off 16-byte alignment, relu, bias)
    (4, 5, 1, 0, 0, False, True, True), (7, 19, 1, 0, 0, False, False, True), (256, 257, 1, 0, 0, False, True, True),
    (2048, 130, 1, 0, 0, False, True, False), (2052, 6, 1, 0, 0, False, False, True), (256, 19, 1, 0, 0, True, True, True),
    (2048, 7, 3, 4, 3, False, True, True), (2052, 21, 3, 1, 1, False, False, True), (7, 9, 3, 3, 2, True, True, True),
    (256, 255, 3, 4, 1, True, False, False),
])
def test_gemv_exact(case, cuda_device):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_GEMV
    K, N, batch, ipad, opad, misalign, relu, has_bias = case
    in_ld, out_ld = K + ipad, N + opad
    g = torch.Generator().manual_seed(K * 7 + N + batch)
    wt = torch.randint(-4, 5, (N, K), generator=g, dtype=torch.int64)
    x = torch.randint(-4, 5, (batch, K), generator=g, dtype=torch.int64)
    b = torch.randint(-64, 65, (N,), generator=g, dtype=torch.int64)
    want = x @ wt.t() + (b if has_bias else 0)                # exact (int64); |.| < 2^24
    if relu:
        want = want.clamp_min(0)
    off = 1 if misalign else 4                                # floats in front of the first vector (4 bytes off 16 when misaligned)
    xin = torch.full((off + batch * in_ld + 64,), 1e30)       # poison between the vectors and behind the last one
    for n in range(batch):
        xin[off + n * in_ld:off + n * in_ld + K] = x[n].float()
    xd, wd, bd = xin.to(cuda_device), wt.float().to(cuda_device), b.float().to(cuda_device)
    out = torch.full((batch + 1, out_ld), float("nan"), device=cuda_device)
    in_ptr = xd.data_ptr() + 4 * off
    assert (in_ptr % 16 == 4) == misalign
    _run(_op(OP_GEMV, _lib.AVL_F32, in_=in_ptr, out=out.data_ptr(), weight=wd.data_ptr(), bias=bd.data_ptr() if has_bias else 0,
             in_h=1, in_w=1, in_c=K, in_ld=in_ld, in_rows=batch, out_h=1, out_w=1, out_c=N, out_ld=out_ld, out_rows=batch,
             relu=int(relu), batch=batch))
    flat = out.cpu().reshape(-1)
    got = torch.stack([flat[n * out_ld:n * out_ld + N] for n in range(batch)])
    assert torch.equal(got, want.float()), "gemv K=%d N=%d batch %d: max |d| %g" % (K, N, batch, float((got - want.float()).abs().nan_to_num(1e30).max()))
    written = torch.zeros_like(flat, dtype=torch.bool)
    for n in range(batch):
        written[n * out_ld:n * out_ld + N] = True
    assert bool(flat[~written].isnan().all())                 # the gaps between the vectors and everything behind the last one


# ------------------------------------------------------------------------------------------------ AVL_OP_SUBSAMPLE
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", [  # (H, W, C, stride, batch)
    (9, 13, 64, 2, 1), (17, 31, 256, 2, 3), (7, 5, 8, 3, 2), (1, 1, 16, 2, 3), (33, 65, 512, 2, 1),
])
def test_subsample_bit_exact(case, dtype, cuda_device):
    from vision_semantic_segmentation_amd.network import OP_SUBSAMPLE
    H, W, Cc, s, batch = case
    tdt = DTYPES[dtype]
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    ioff, ooff = 8, 16                                        # channel slices of wider buffers (16-byte aligned in every type)
    in_ld, out_ld = Cc + 16, Cc + 40
    g = torch.Generator().manual_seed(H * W + Cc + s)
    x = torch.randn((batch, H, W, Cc), generator=g).to(tdt)
    src = torch.full((batch * H * W + 7, in_ld), float("nan"), dtype=tdt)
    src[:batch * H * W, ioff:ioff + Cc] = x.reshape(-1, Cc)
    srcd = src.to(cuda_device)
    dst = torch.full((batch * OH * OW + 9, out_ld), 7.0, dtype=tdt, device=cuda_device)
    es = src.element_size()
    _run(_op(OP_SUBSAMPLE, _did(dtype), in_=srcd.data_ptr() + ioff * es, out=dst.data_ptr() + ooff * es, in_h=H, in_w=W, in_c=Cc, in_ld=in_ld,
             in_rows=batch * H * W, out_h=OH, out_w=OW, out_c=Cc, out_ld=out_ld, out_rows=batch * OH * OW, stride=s, batch=batch))
    got = dst.cpu()
    want = x[:, ::s, ::s].reshape(-1, Cc)
    assert torch.equal(got[:batch * OH * OW, ooff:ooff + Cc], want), (case, dtype)
    assert bool((got[:, :ooff] == 7.0).all()) and bool((got[:, ooff + Cc:] == 7.0).all()) and bool((got[batch * OH * OW:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ AVL_OP_ARGMAX
@pytest.mark.parametrize("case", [  # (h, w, C, ld - C, batch)
    (7, 9, 1, 3, 1), (13, 29, 19, 5, 2), (11, 17, 33, 31, 1), (9, 10, 256, 4, 2), (31, 17, 19, 0, 1),
])
def test_argmax_matches_torch(case, cuda_device):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_ARGMAX
    h, w, Cc, ldpad, batch = case
    ld, M = Cc + ldpad, batch * h * w
    g = torch.Generator().manual_seed(h * w + Cc + batch)
    z = torch.randint(0, 4, (M, Cc), generator=g).float()    # few values: ties everywhere, the first maximal index wins
    r = torch.rand(M, generator=g)
    for m in range(M):
        if r[m] < 0.1:                                        # rows of all -inf
            z[m] = float("-inf")
        elif r[m] < 0.2:                                      # one or two NaN: the first NaN wins
            j = torch.randint(0, Cc, (2,), generator=g)
            z[m, j] = float("nan")
        elif r[m] < 0.25:
            z[m, torch.randint(0, Cc, (1,), generator=g)] = float("inf")
        elif r[m] < 0.3:
            z[m] = float("-inf")
            z[m, -1] = float("nan")
    logits = torch.full((M + 40, ld), float("inf"))          # poison: columns past C and rows past M would win every arg-max
    logits[:M, :Cc] = z
    ld_dev = logits.to(cuda_device)
    labels = torch.full((M + 40,), 0xEE, dtype=torch.uint8, device=cuda_device)
    _run(_op(OP_ARGMAX, _lib.AVL_F32, in_=ld_dev.data_ptr(), out=labels.data_ptr(), in_h=h, in_w=w, in_c=Cc, in_ld=ld, in_rows=M,
             out_h=h, out_w=w, out_c=1, out_ld=1, out_rows=M, batch=batch))
    want = torch.argmax(z, dim=1)
    got = labels.cpu()
    assert torch.equal(got[:M].long(), want), "argmax %s: %d rows differ" % (case, int((got[:M].long() != want).sum()))
    assert bool((got[M:] == 0xEE).all())
    if Cc > 1:
        assert bool((want > 0).any()) and bool(z.isnan().any()) and bool((z == float("-inf")).all(1).any())      # the edges are there


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_nonfinite_counts_each_ops_output(dtype, cuda_device):
    """avl_seg_plan_nonfinite counts the Inf / NaN values of every op's output where it is produced (the self-check of a loaded
    checkpoint): two SUBSAMPLE ops, the first copying some NaN / Inf into a channel slice, the second copying a clean input; the counts
    are exact, and the op's neighbouring columns (sentinel NaN) are not counted."""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_SUBSAMPLE
    H, W, Cc, s = 11, 13, 64, 2
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    tdt = DTYPES[dtype]
    g = torch.Generator().manual_seed(5)
    x = torch.randn((H * W, Cc), generator=g)
    bad = torch.rand((H * W, Cc), generator=g)
    x[bad < 0.02] = float("nan")
    x[(bad >= 0.02) & (bad < 0.03)] = float("inf")
    x[(bad >= 0.03) & (bad < 0.035)] = float("-inf")
    want = int((~torch.isfinite(x.reshape(H, W, Cc)[::s, ::s])).sum())
    assert want > 0
    xd, clean = x.to(tdt).to(cuda_device), torch.randn((H * W, Cc), generator=g).to(tdt).to(cuda_device)
    out = torch.full((2, OH * OW, Cc + 16), float("nan"), dtype=tdt, device=cuda_device)
    ops = [_op(OP_SUBSAMPLE, _did(dtype), in_=src.data_ptr(), out=out[i].data_ptr(), in_h=H, in_w=W, in_c=Cc, in_ld=Cc, in_rows=H * W,
               out_h=OH, out_w=OW, out_c=Cc, out_ld=Cc + 16, out_rows=OH * OW, stride=s) for i, src in enumerate((xd, clean))]
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * 2)(*ops), 2, C.byref(plan)), "avl_seg_plan_create")
    try:
        counts = (C.c_ulonglong * 2)()
        _lib.check(_lib.lib().avl_seg_plan_nonfinite(plan, C.c_void_p(torch.cuda.current_stream().cuda_stream), counts), "avl_seg_plan_nonfinite")
    finally:
        _lib.lib().avl_seg_plan_destroy(plan)
    assert list(counts) == [want, 0], (list(counts), want)


# ------------------------------------------------------------------------------------------------ avl_seg_plan_nonfinite, rule by rule
# Every expected count comes from the op's operands on the host (a float64 model of what the op stores), never from reading the
# GPU buffer back.  Inf / NaN enter by construction: bias entries of +Inf / -Inf / NaN on chosen columns (+Inf alone where a ReLU
# follows: the kernels' fmaxf drops a NaN, torch.relu keeps it), and for f16 a bias of 2^17, an exact integer result beyond the
# type's range.  Every finite expected value stays below 2^15.  Everything around an op's output holds NaN that must not be counted.
INF, NAN = float("inf"), float("nan")


def _nonfinite(plan, n):
    from vision_semantic_segmentation_amd import _lib
    counts = (C.c_ulonglong * n)()
    try:
        _lib.check(_lib.lib().avl_seg_plan_nonfinite(plan, C.c_void_p(torch.cuda.current_stream().cuda_stream), counts), "avl_seg_plan_nonfinite")
    finally:
        _lib.lib().avl_seg_plan_destroy(plan)
    return list(counts)


def _create(ops):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * len(ops))(*ops), len(ops), C.byref(plan)), "avl_seg_plan_create")
    return plan


def _bad(n):
    return int((~torch.isfinite(n)).sum())


def _ring_case(mode, lo1, lo2, relu, strided=False, twin=True):
    import _ring_ext_operands as R
    geo = R.GEO[2] if strided else (1, 1, 300, 1, 0)           # stride 3, batch 2, rows wider than K | one image of 300 rows
    return R.Case(mode, 2, *geo, 384 if twin else 256, 128 if twin else 0, lo1, lo2, relu)


@pytest.mark.parametrize("where", ["first", "second", "both"])
@pytest.mark.parametrize("mode,lo1,lo2,relu", [("f16", False, False, False), ("bf16", False, False, False), ("bf16", False, False, True),
                                               ("split", True, True, False), ("split", True, False, True), ("w2", False, True, False)])
def test_nonfinite_counts_a_two_destination_gemm(mode, lo1, lo2, relu, where, cuda_device):
    """the column split c1 = n_split, c2 = out_c - c1 and both destinations' lo planes: f16(Inf - Inf) is NaN in a lo plane, so a
    bad column counts twice where its destination has one"""
    _check_ring_nonfinite(_ring_case(mode, lo1, lo2, relu), where, cuda_device)


@pytest.mark.parametrize("mode,lo1,relu", [("f16", False, False), ("bf16", False, True), ("split", True, False)])
def test_nonfinite_counts_a_strided_gemm(mode, lo1, relu, cuda_device):
    """rows = the SUB-SAMPLED pixel count times the batch (stride 3, batch 2)"""
    _check_ring_nonfinite(_ring_case(mode, lo1, False, relu, strided=True, twin=False), "first", cuda_device)


def _check_ring_nonfinite(c, where, cuda_device):
    import _ring_ext_operands as R
    from test_gpu_ring_ext_exact import _plan
    g = R.geometry(c)
    prec = R.MODES[c.mode][0]
    b = R.bias(c).clone()
    assert float(R.exact_v(c).abs().max()) < 2 ** 15           # every finite expected value
    kinds = [INF] if c.relu else [INF, -INF, NAN]
    if prec == "f16":
        kinds.append(2.0 ** 17)                                # finite in fp32, Inf once rounded to f16
    n1 = g["n1"]
    cols = ([3, 17, 64, 127] if where != "second" else []) + ([n1 + 5, n1 + 100, n1 + 128, c.N - 1] if where != "first" else [])
    for i, col in enumerate(cols):
        b[col] = kinds[i % len(kinds)]
    v = R.exact_v(c, b=b)
    hi = v.to(R.X.DTYPES[prec])
    lo = (v - hi.double()).to(torch.float16)
    want = _bad(hi[:, :n1]) + (_bad(lo[:, :n1]) if c.lo1 else 0)
    if c.n_split:
        want += _bad(hi[:, n1:]) + (_bad(lo[:, n1:]) if c.lo2 else 0)
    first_cols = len([x for x in cols if x < n1])
    assert want == g["M"] * (first_cols * (2 if c.lo1 else 1) + (len(cols) - first_cols) * (2 if c.lo2 else 1)) > 0
    plan, bufs, keep = _plan(c, cuda_device, fill=NAN, bias=b)          # NaN: rows past M, the columns beside both slices, unwritten planes
    got = _nonfinite(plan, 1)
    assert got == [want], (R.case_id(c), where, got, want)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_nonfinite_counts_the_pooled_stem_of_a_batch(precision, cuda_device):
    """rows = the POOLED size times the batch: +Inf bias on two channels (f16: one of them 2^17) under the ReLU and the max-pool"""
    from test_gpu_fused_passes import _stem_ops
    from vision_semantic_segmentation_amd.network import pack_stem_mfma
    H, W, B = 37, 53, 2
    tdt = DTYPES[precision]
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(cuda_device)
    w = torch.randn((64, 3, 7, 7), generator=g, dtype=torch.float64) * (2.0 / 147) ** 0.5       # |conv| <= 147 * 2.7 * max|w|: far below 2^15
    bias = torch.randn(64, generator=g) * 0.1
    bias[7], bias[40] = INF, (2.0 ** 17 if precision == "f16" else INF)
    wd, bd = pack_stem_mfma(w).to(tdt).to(cuda_device), bias.to(cuda_device)
    h4, w4 = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    rows = (B * h4 * w4 + 255) // 256 * 256 + 256
    out = torch.full((rows, 64), NAN, dtype=tdt, device=cuda_device)
    unused = torch.zeros((1, 64), dtype=tdt, device=cuda_device)
    _, one, hw4 = _stem_ops(_did(precision), img, wd, bd, unused, unused, out, (H, W), B)
    assert hw4 == (h4, w4) and float(w.abs().max()) * 147 * 3 < 2 ** 15
    assert _nonfinite(_create(one), 1) == [B * h4 * w4 * 2]


def test_nonfinite_counts_gap_and_gemv_rows_as_fp32(cuda_device):
    """GAP and GEMV: rows = the batch, fp32 outputs inside wider rows of NaN"""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_GAP, OP_GEMV
    B, h, w, Cc, N = 3, 9, 9, 64, 21
    M = h * w
    g = torch.Generator().manual_seed(4)
    x = torch.full((B * M + 300, Cc), INF)                    # rows past the last image: never read
    x[:B * M] = torch.randint(-8, 9, (B * M, Cc), generator=g).float()
    x[5, 3] = INF                                              # image 0, channel 3: +Inf
    x[M + 2, 9], x[M + 70, 9] = INF, -INF                      # image 1, channel 9: Inf - Inf = NaN
    x[2 * M + 1, 20] = NAN                                     # image 2
    x[2 * M + 8, 3] = -INF
    want_gap = _bad(x[:B * M].double().reshape(B, M, Cc).mean(1))
    assert want_gap == 4
    xd = x.to(torch.float16).to(cuda_device)
    scratch = torch.full((B, 256, Cc), NAN, device=cuda_device)
    pooled = torch.full((B + 1, Cc + 8), NAN, device=cuda_device)
    gap = _op(OP_GAP, _lib.AVL_F16, in_=xd.data_ptr(), in2=scratch.data_ptr(), out=pooled.data_ptr(), in_h=h, in_w=w, in_c=Cc, in_ld=Cc,
              in_rows=xd.shape[0], out_h=1, out_w=1, out_c=Cc, out_ld=Cc + 8, out_rows=B, batch=B)
    vec = torch.randint(-4, 5, (B, Cc), generator=g).float()
    wt = torch.randint(-4, 5, (N, Cc), generator=g).float()
    bias = torch.randint(-64, 65, (N,), generator=g).float()
    bias[2], bias[11], bias[20] = INF, -INF, NAN
    want_gemv = _bad(vec.double() @ wt.double().t() + bias.double())
    assert want_gemv == 3 * B
    vd, wd, bd = vec.to(cuda_device), wt.to(cuda_device), bias.to(cuda_device)
    y = torch.full((B + 1, N + 3), NAN, device=cuda_device)
    gemv = _op(OP_GEMV, _lib.AVL_F32, in_=vd.data_ptr(), out=y.data_ptr(), weight=wd.data_ptr(), bias=bd.data_ptr(), in_h=1, in_w=1, in_c=Cc,
               in_ld=Cc, in_rows=B, out_h=1, out_w=1, out_c=N, out_ld=N + 3, out_rows=B, relu=0, batch=B)
    brelu = torch.randint(-64, 65, (N,), generator=g).float()
    brelu[0], brelu[19] = INF, INF                             # a ReLU follows: +Inf alone
    brd = brelu.to(cuda_device)
    y2 = torch.full((B + 1, N + 3), NAN, device=cuda_device)
    gemv_relu = _op(OP_GEMV, _lib.AVL_F32, in_=vd.data_ptr(), out=y2.data_ptr(), weight=wd.data_ptr(), bias=brd.data_ptr(), in_h=1, in_w=1,
                    in_c=Cc, in_ld=Cc, in_rows=B, out_h=1, out_w=1, out_c=N, out_ld=N + 3, out_rows=B, relu=1, batch=B)
    assert _nonfinite(_create([gap, gemv, gemv_relu]), 3) == [want_gap, want_gemv, 2 * B]


def test_nonfinite_counts_a_classifier_gemm_and_nothing_for_argmax(cuda_device):
    """a classifier GEMM (out_f32, labels through out_mx): N fp32 columns of an out_ld-wide row, the uint8 labels not at all; the
    AVL_OP_ARGMAX op behind it reads those very logits and counts nothing"""
    import _exact_operands as X
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_ARGMAX, OP_GEMM
    M, K, N, Np, Mp = 300, 64, 19, 64, 512
    a, w = X.ints(31, Mp, K), X.ints(32, Np, K)
    bias = torch.full((Np,), INF)                              # the padding rows' bias: never part of the output
    bias[:N] = torch.randint(-40, 41, (N,), generator=torch.Generator().manual_seed(33)).float()
    bias[1], bias[8], bias[18] = NAN, INF, -INF
    want = _bad(a[:M].double() @ w[:N].double().t() + bias[:N].double())
    assert want == 3 * M and 36 * K + 40 < 2 ** 15
    ad, wd, bd = a.to(torch.float16).to(cuda_device), w.to(torch.float16).to(cuda_device), bias.to(cuda_device)
    logits = torch.full((Mp, N + 5), NAN, device=cuda_device)
    labels = torch.full((Mp,), 99, dtype=torch.uint8, device=cuda_device)
    labels2 = torch.full((Mp,), 99, dtype=torch.uint8, device=cuda_device)
    gemm = _op(OP_GEMM, _lib.AVL_F16, in_=ad.data_ptr(), out=logits.data_ptr(), weight=wd.data_ptr(), bias=bd.data_ptr(), out_mx=labels.data_ptr(),
               in_h=1, in_w=M, in_c=K, in_ld=K, in_rows=Mp, out_h=1, out_w=M, out_c=N, out_ld=N + 5, out_rows=Mp, out_f32=1, w_rows=Np)
    amax = _op(OP_ARGMAX, _lib.AVL_F32, in_=logits.data_ptr(), out=labels2.data_ptr(), in_h=1, in_w=M, in_c=N, in_ld=N + 5, in_rows=M,
               out_h=1, out_w=M, out_c=1, out_ld=1, out_rows=M)
    assert _nonfinite(_create([gemm, amax]), 2) == [want, 0]
    assert torch.equal(labels[:M].cpu(), labels2[:M].cpu()) and bool((labels2[M:] == 99).all())


def test_nonfinite_counts_the_classifier_epilogue_of_the_fused_depthwise_pointwise(cuda_device):
    """AVL_OP_DWPW with out_f32: in3_c fp32 columns (the logits), not the block's out_c; classifier bias +Inf / -Inf / NaN on three
    classes, and +Inf on a padding class past in3_c that is neither written nor counted"""
    from test_gpu_mixed import _split
    from test_gpu_ops import _nhwc_rows
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_DWPW, dwpw_tile_order, pack_dw_f32, pack_split_rows, split_f16
    H, W, K, N, ncls = 11, 30, 64, 256, 19
    OH, OW = H - 2, W - 2
    M, Mp = OH * OW, (OH * OW + 255) // 256 * 256
    g = torch.Generator().manual_seed(8)
    xh, xl = _split(torch.randn((1, K, H, W), generator=g, dtype=torch.float64))
    w1, b1 = (torch.randn((K, 1, 3, 3), generator=g) * 0.3).double(), (torch.randn(K, generator=g) * 0.1).double()
    w2, b2 = torch.randn((N, K), generator=g, dtype=torch.float64) / K ** 0.5, torch.randn(N, generator=g) * 0.1
    wc32 = torch.zeros((32, N), dtype=torch.float64)
    wc32[:ncls] = torch.randn((ncls, N), generator=g, dtype=torch.float64) / N ** 0.5
    bc32 = torch.zeros(32)
    bc32[0], bc32[9], bc32[18], bc32[25] = INF, -INF, NAN, INF
    # (every finite logit is a sum of 256 products of unit-variance values scaled by N^-0.5: far below 2^15; the expected count is
    # the non-finite classifier bias entries among the ncls real classes, once per pixel)
    want = M * _bad(bc32[:ncls])
    src = torch.stack([_nhwc_rows(xh), _nhwc_rows(xl)]).to(cuda_device)
    w2d, b2d = pack_split_rows(w2, 2).to(cuda_device), b2.to(cuda_device)
    wcd, bcd = torch.stack(split_f16(wc32)).to(cuda_device), bc32.to(cuda_device)
    logits = torch.full((Mp, ncls), NAN, dtype=torch.float32, device=cuda_device)
    labels = torch.full((Mp,), 99, dtype=torch.uint8, device=cuda_device)
    params = torch.cat([pack_dw_f32(w1, b1), dwpw_tile_order(OH, OW, 1)]).to(cuda_device)
    op = _op(OP_DWPW, _lib.AVL_F16, in_=src[0].data_ptr(), in_lo=src[1].data_ptr(), in2=params.data_ptr(), in2_lo=bcd.data_ptr(), in3=wcd.data_ptr(),
             in3_c=ncls, out=logits.data_ptr(), out_mx=labels.data_ptr(), out_f32=1, weight=w2d.data_ptr(), bias=b2d.data_ptr(), w_split=3, w_layout=0,
             in_h=H, in_w=W, in_c=K, in_ld=K, in_rows=src.shape[1], out_h=OH, out_w=OW, out_c=N, out_ld=ncls, out_rows=Mp,
             relu=1, w_rows=256, ksize=3, stride=1, pad=0, dil=1, groups=K)
    assert want == 3 * M and _nonfinite(_create([op]), 1) == [want]
