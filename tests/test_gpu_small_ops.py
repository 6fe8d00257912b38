"""The small ops of the segmentation plan run ALONE through avl_seg_plan_*: AVL_OP_GAP (the ASPP pooling branch), AVL_OP_GEMV (its two
1x1 convs on the pooled vector), AVL_OP_SUBSAMPLE (the strided 1x1 convs' input rows) and AVL_OP_ARGMAX (torch.argmax over the logits).

GAP and GEMV are fed small integers (exact in bf16 / f16 / fp32, every partial sum below 2^24), so every fp32 sum the kernels form is
exact whatever its order: the expected values are exact too (GAP: float32(sum) / float32(M), correctly rounded), and one dropped or
repeated row, column or vector element fails the comparison.  SUBSAMPLE copies bits; ARGMAX is compared with torch.argmax on the CPU.
Every output sits between sentinels (columns outside the op's slice, rows past the output) that must survive; inputs carry poison
(large values or NaN) in the rows and columns the op must not read."""
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
