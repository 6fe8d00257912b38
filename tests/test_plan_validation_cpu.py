"""avl_seg_plan_create's host-side refusals for the ops tests/test_gpu_small_ops.py and the GEMM cases of tests/test_gpu_ops.py run:
an op the kernels cannot run as described is refused when the plan is created (no GPU call), not when it is launched."""
import ctypes as C

import torch

_BUF = torch.zeros(1 << 20, dtype=torch.uint8)
PTR = (_BUF.data_ptr() + 255) // 256 * 256          # host memory: validation only looks at values and alignment


def _create(op):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    rc = _lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan))
    if rc == 0:
        _lib.lib().avl_seg_plan_destroy(plan)
    return rc, _lib.last_error()


def _gemm(dtype, layout=0):
    from vision_semantic_segmentation_amd.network import OP_GEMM, AvlSegOp
    g = AvlSegOp()
    g.kind, g.dtype, g.w_layout = OP_GEMM, dtype, layout
    g.in_ = g.out = g.weight = g.bias = PTR
    g.in_h, g.in_w, g.in_c, g.in_ld, g.in_rows = 1, 256, 256, 256, 256
    g.out_h, g.out_w, g.out_c, g.out_ld, g.out_rows = 1, 256, 256, 256, 256
    g.relu, g.w_rows, g.ksize, g.stride, g.dil, g.groups = 1, 256, 1, 1, 1, 1
    return g


def test_gemm_tile_configuration_is_validated_at_creation():
    from vision_semantic_segmentation_amd import _lib
    for dt in (_lib.AVL_BF16, _lib.AVL_F16):
        for layout in range(5):
            assert _create(_gemm(dt, layout))[0] == 0, (dt, layout)
        for layout in (5, -1, 9):
            rc, msg = _create(_gemm(dt, layout))
            assert rc != 0 and "w_layout %d" % layout in msg, (dt, layout, msg)
    assert _create(_gemm(_lib.AVL_F32, 0))[0] == 0
    for layout in (1, 2, 3, 4):
        rc, msg = _create(_gemm(_lib.AVL_F32, layout))
        assert rc != 0 and "16-bit" in msg, (layout, msg)


def test_gemm_bias_per_image_needs_the_last_images_whole_tiles():
    from vision_semantic_segmentation_amd import _lib
    for h, w in ((13, 29), (16, 16), (1, 300)):
        m = h * w
        op = _gemm(_lib.AVL_BF16)
        op.batch, op.bias_per_image = 3, 1
        op.in_h = op.out_h = h
        op.in_w = op.out_w = w
        rows = 2 * m + (m + 255) // 256 * 256
        op.in_rows = op.out_rows = rows
        assert _create(op)[0] == 0, (h, w)
        op.in_rows = rows - 256
        rc, msg = _create(op)
        assert rc != 0 and "per-image bias" in msg, (h, w, msg)


def test_small_ops_refuse_what_their_kernels_do_not_read():
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_ARGMAX, OP_GAP, OP_GEMV, AvlSegOp

    def op(kind, dtype, **f):
        o = AvlSegOp()
        o.kind, o.dtype = kind, dtype
        o.in_ = o.in2 = o.out = o.weight = PTR
        o.in_h, o.in_w, o.in_c, o.in_ld, o.in_rows = 4, 4, 64, 64, 16
        o.out_h, o.out_w, o.out_c, o.out_ld, o.out_rows = 1, 1, 64, 64, 16
        for k, v in f.items():
            setattr(o, k, v)
        return o

    assert _create(op(OP_GEMV, _lib.AVL_F32))[0] == 0
    assert _create(op(OP_GEMV, _lib.AVL_F32, in_=PTR + 4, in_c=7))[0] == 0      # the scalar path reads any alignment / K
    for dt in (_lib.AVL_BF16, _lib.AVL_F16):
        rc, msg = _create(op(OP_GEMV, dt))
        assert rc != 0 and "fp32" in msg, msg
        rc, msg = _create(op(OP_ARGMAX, dt, in_c=19, in_ld=19))
        assert rc != 0 and "fp32" in msg, msg
    assert _create(op(OP_ARGMAX, _lib.AVL_F32, in_c=19, in_ld=19))[0] == 0
    for dt in (_lib.AVL_F32, _lib.AVL_BF16, _lib.AVL_F16):
        assert _create(op(OP_GAP, dt))[0] == 0, dt
    rc, msg = _create(op(OP_GAP, _lib.AVL_F64))
    assert rc != 0 and "gap dtype" in msg, msg
    rc, msg = _create(op(OP_GAP, _lib.AVL_BF16, in_=PTR + 8))
    assert rc != 0 and "aligned" in msg, msg
    rc, msg = _create(op(OP_GAP, _lib.AVL_F32, in2=PTR + 4))
    assert rc != 0 and "aligned" in msg, msg
