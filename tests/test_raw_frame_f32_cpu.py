"""The fp32 plan's pre-processing stem without a GPU: SegNet builds its buffers on the CPU (the plan only validates pointers and
shapes), so avl_seg_plan_create sees the real stem op of a precision "f32" raw_frame plan and the forms it still refuses."""
import ctypes as C

import pytest

H, W = 100, 130

_STATE = []


def _state():
    from vision_semantic_segmentation_amd.network import random_state_dict
    if not _STATE:
        _STATE.append(random_state_dict(seed=0))
    return _STATE[0]


def _net(precision, raw_frame):
    from vision_semantic_segmentation_amd.network import SegNet
    return SegNet(_state(), H, W, precision=precision, raw_frame=raw_frame, device="cpu")


def _create(ops):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    rc = _lib.lib().avl_seg_plan_create((AvlSegOp * len(ops))(*ops), len(ops), C.byref(plan))
    if rc == 0:
        _lib.lib().avl_seg_plan_destroy(plan)
    return rc, _lib.last_error()


def _copy(op):
    from vision_semantic_segmentation_amd.network import AvlSegOp
    new = AvlSegOp()
    C.pointer(new)[0] = op
    return new


@pytest.fixture(scope="module")
def f32_raw():
    return _net("f32", (2 * H, 2 * W))       # (SegNet.__init__ ran avl_seg_plan_create on the whole op list)


def test_f32_plan_builds_on_a_raw_frame(f32_raw):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_STEM
    stem = f32_raw.ops[0]
    assert stem.kind == OP_STEM and stem.in2 and stem.w_layout == 0 and stem.dtype == _lib.AVL_F32
    assert stem.in_h == H and stem.in_w == W and stem.in2_ld == 2 * W and stem.in_rows == 4 * H * W
    assert f32_raw.image.shape == (2 * H, 2 * W, 3)
    rc, msg = _create([_copy(stem)])
    assert rc == 0, msg


def test_f32_raw_stem_takes_one_frame(f32_raw):
    op = _copy(f32_raw.ops[0])
    op.batch = 2
    rc, msg = _create([op])
    assert rc == -3 and "one raw frame" in msg, (rc, msg)


def test_raw_stem_layout_must_match_the_dtype(f32_raw):
    from vision_semantic_segmentation_amd.network import AVL_IN_F32_CHW
    # a 16-bit pre-processing stem is the MFMA kernel: w_layout 0 is refused
    half = _copy(_net("f16", (2 * H, 2 * W)).ops[0])
    assert half.in2 and half.w_layout == 1 and _create([half])[0] == 0
    half.w_layout = 0
    rc, msg = _create([half])
    assert rc != 0 and "w_layout" in msg, (rc, msg)
    # and the fp32 one has no MFMA layout
    op = _copy(f32_raw.ops[0])
    op.w_layout = 1
    assert _create([op])[0] != 0
    # a raw frame is uint8: never with the normalised fp32 planes
    op = _copy(f32_raw.ops[0])
    op.in_format = AVL_IN_F32_CHW
    rc, msg = _create([op])
    assert rc == -3 and "AVL_IN_F32_CHW" in msg, (rc, msg)


def test_raw_frame_must_scale_by_an_integer_factor():
    with pytest.raises(ValueError, match="integer factor"):
        _net("f32", (2 * H + 1, 2 * W - 3))
    with pytest.raises(ValueError, match="integer factor"):
        _net("f32", (H - 1, W - 1))
    # a remainder row / column is padding the factor drops (487 x 645 / 3 -> 162 x 215): accepted
    from vision_semantic_segmentation_amd.network import SegNet
    net = SegNet(_state(), 162, 215, precision="f32", raw_frame=(487, 645), device="cpu")
    assert net.ops[0].in2 and net.ops[0].in2_ld == 645 and net.ops[0].in_rows == 487 * 645
