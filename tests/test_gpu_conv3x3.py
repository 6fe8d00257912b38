"""The dense 3x3 convolution (AVL_OP_GCONV, w_layout 2: seg_conv3x3.hip) alone through avl_seg_plan_*, against a float64
F.conv2d, in every variant: fp32 (v_mfma_f32_16x16x4_f32), bf16 / f16 (one plane) and the f16 hi + lo split (split input,
split weights, split output).  Shapes are no multiple of the 8 x 16 tile; dilations reach past small images; one case reads
and writes channel slices of wider buffers.  Rows past the output keep their sentinel.

Tolerances (of max|ref|): fp32 1e-5; bf16 / f16 the grouped-conv bounds of test_gpu_ops.py (the reference is fed the same
rounded inputs and weights); split within the fp32 bound (the operands keep ~22 bits; measured on
MI355X: fp32 <= 4.0e-6, split <= 2.8e-6 over these cases)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

CASES = [  # (H, W, cg, groups, stride, dil)
    (23, 45, 64, 1, 1, 1), (23, 45, 128, 1, 2, 1), (30, 41, 256, 1, 1, 2), (19, 67, 512, 1, 1, 4),
    (17, 29, 1024, 1, 1, 2), (21, 35, 64, 4, 1, 4), (8, 8, 64, 1, 2, 1), (5, 33, 128, 1, 1, 4),
]
TOL = {"f32": 1e-5, "bf16": 2 ** -8 * 1.5 * 2, "f16": 2 ** -11 * 1.5 * 2, "split": 1e-5}
SENTINEL = 7.0


def _run(op):
    import torch
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan)), "avl_seg_plan_create")
    try:
        _lib.check(_lib.lib().avl_seg_plan_run(plan, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "avl_seg_plan_run")
        torch.cuda.synchronize()
    finally:
        _lib.lib().avl_seg_plan_destroy(plan)


@pytest.mark.parametrize("variant", ["f32", "bf16", "f16", "split"])
@pytest.mark.parametrize("case", CASES)
def test_dense_conv3x3(case, variant, cuda_device):
    import torch
    import torch.nn.functional as F
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_GCONV, AvlSegOp, pack_conv3x3, split_f16
    H, W, cg, G, s, d = case
    C_ = cg * G
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    g = torch.Generator().manual_seed(H * 131 + W + cg + G)
    x = torch.randn((1, C_, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((C_, cg, 3, 3), generator=g, dtype=torch.float64) * (2.0 / (cg * 9)) ** 0.5
    b = torch.randn(C_, generator=g, dtype=torch.float64) * 0.1
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "split": torch.float16}[variant]
    did = {"f32": _lib.AVL_F32, "bf16": _lib.AVL_BF16, "f16": _lib.AVL_F16, "split": _lib.AVL_F16}[variant]
    if variant in ("bf16", "f16"):          # the reference sees the same rounded operands
        xq, wq = x.to(tdt).double(), w.to(tdt).double()
    else:
        xq, wq = x, w
    ref = F.relu(F.conv2d(xq, wq, b, stride=s, padding=d, dilation=d, groups=G))[0].permute(1, 2, 0).reshape(OH * OW, C_)
    # channel slices: the input sits at column 64 of a wider buffer, the output at column 128 of another (the (21, 35, 64, 4) case)
    slices = case == (21, 35, 64, 4, 1, 4)
    ci0, co0 = (64, 128) if slices else (0, 0)
    in_ld, out_ld = C_ + (128 if slices else 0), C_ + (192 if slices else 0)
    rows_in, rows_out = (H * W + 255) // 256 * 256, (OH * OW + 255) // 256 * 256
    xm = x[0].permute(1, 2, 0).reshape(H * W, C_)
    planes = 2 if variant == "split" else 1
    src = torch.full((planes, rows_in, in_ld), SENTINEL, dtype=tdt)
    if variant == "split":
        hi, lo = split_f16(xm)
        src[0, :H * W, ci0:ci0 + C_], src[1, :H * W, ci0:ci0 + C_] = hi, lo
    else:
        src[0, :H * W, ci0:ci0 + C_] = xm.to(tdt)
    src = src.to(cuda_device)
    dst = torch.full((planes, rows_out, out_ld), SENTINEL, dtype=tdt, device=cuda_device)
    if variant == "split":
        wd = pack_conv3x3(w, G, 8, split=True).to(cuda_device)
    else:
        wd = pack_conv3x3(w, G, 4 if variant == "f32" else 8).to(tdt).to(cuda_device)
    bd = b.float().to(cuda_device)
    es = src.element_size()
    op = AvlSegOp()
    op.kind, op.dtype = OP_GCONV, did
    op.in_, op.out = src[0].data_ptr() + ci0 * es, dst[0].data_ptr() + co0 * es
    op.weight, op.bias = wd.data_ptr(), bd.data_ptr()
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = H, W, C_, in_ld, rows_in
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = OH, OW, C_, out_ld, rows_out
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu, op.w_layout = 3, s, d, d, G, 1, 2
    if variant == "split":
        op.w_split = 1
        op.in_lo, op.out_lo = src[1].data_ptr() + ci0 * es, dst[1].data_ptr() + co0 * es
    _run(op)
    out = dst.double().cpu()
    got = out[0, :OH * OW, co0:co0 + C_] + (out[1, :OH * OW, co0:co0 + C_] if variant == "split" else 0)
    err = float((got - ref).abs().max() / ref.abs().max())
    print("dense 3x3 %s %s: %.3e of max|ref|" % (case, variant, err))
    assert err <= TOL[variant], "dense 3x3 %s %s: %.3e" % (case, variant, err)
    # nothing written past out_h * out_w rows, nor outside the output's channel slice
    assert bool((out[:, OH * OW:] == SENTINEL).all())
    if slices:
        assert bool((out[:, :, :co0] == SENTINEL).all()) and bool((out[:, :, co0 + C_:] == SENTINEL).all())
