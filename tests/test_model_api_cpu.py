"""The reference's model API without a GPU: float-input stems through avl_seg_plan_create (SegNet builds its buffers on the CPU
here, as in test_batch_cpu.py), the refusals of the new op field, and the DeepLabV3Plus module's weights and modes."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

H, W = 97, 131

_STATE = {}


def _state():
    from vision_semantic_segmentation_amd.network import random_state_dict
    if "s" not in _STATE:
        _STATE["s"] = random_state_dict(seed=0)
    return _STATE["s"]


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
    c = AvlSegOp()
    C.pointer(c)[0] = op
    return c


PRECISIONS = [("f32", dict(precision="f32")), ("f16", dict(precision="f16")), ("mixed", dict(precision="mixed")),
              ("split16", dict(precision="mixed", full_split=True))]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name,kw", PRECISIONS, ids=[p[0] for p in PRECISIONS])
def test_float_input_stem_is_accepted(name, kw, batch):
    from vision_semantic_segmentation_amd.network import AVL_IN_F32_CHW, OP_STEM, SegNet
    net = SegNet(_state(), H, W, device="cpu", batch=batch, input_format="f32_nchw", **kw)      # (ran avl_seg_plan_create)
    stem = net.ops[0]
    assert stem.kind == OP_STEM and stem.in_format == AVL_IN_F32_CHW
    assert all(op.in_format == 0 for op in net.ops[1:])
    assert net.image.dtype == torch.float32
    assert tuple(net.image.shape) == ((batch,) if batch > 1 else ()) + (3, H, W)
    assert stem.in_rows == batch * H * W
    assert _create(net.ops)[0] == 0


def test_u8_plans_keep_in_format_zero():
    from vision_semantic_segmentation_amd.network import SegNet
    for name, kw in PRECISIONS:
        net = SegNet(_state(), H, W, device="cpu", **kw)
        assert all(op.in_format == 0 for op in net.ops), name
        assert net.image.dtype == torch.uint8 and tuple(net.image.shape) == (H, W, 3)


def _f32_ops():
    from vision_semantic_segmentation_amd.network import SegNet
    return SegNet(_state(), H, W, device="cpu", precision="mixed", input_format="f32_nchw").ops


def test_float_input_refused_with_a_preprocessing_stem():
    from vision_semantic_segmentation_amd.network import SegNet
    raw = SegNet(_state(), H, W, device="cpu", precision="mixed", raw_frame=(2 * H, 2 * W))
    ops = [_copy(op) for op in raw.ops]
    assert ops[0].in2
    ops[0].in_format = 1
    rc, msg = _create(ops)
    assert rc != 0 and "in_format" in msg and "in2" in msg, msg


def test_float_input_refused_on_a_non_stem_op():
    ops = [_copy(op) for op in _f32_ops()]
    ops[1].in_format = 1
    rc, msg = _create(ops)
    assert rc != 0 and "op 1" in msg and "in_format 1 is a stem field" in msg, msg


@pytest.mark.parametrize("value", [2, -1, 255])
def test_unknown_in_format_refused(value):
    ops = [_copy(op) for op in _f32_ops()]
    ops[0].in_format = value
    rc, msg = _create(ops)
    assert rc != 0 and ("in_format %d is not an AVL_IN_* value" % value) in msg, msg


def test_float_input_refused_with_raw_frame_or_part_before_the_gpu():
    from vision_semantic_segmentation_amd.network import SegNet
    with pytest.raises(NotImplementedError, match="input_format"):
        SegNet(_state(), H, W, device="cpu", precision="mixed", raw_frame=(2 * H, 2 * W), input_format="f32_nchw")
    with pytest.raises(NotImplementedError, match="input_format"):
        SegNet({}, 16, 16, device="cpu", precision="mixed", part=("aspp", 2048), input_format="f32_nchw")
    with pytest.raises(ValueError, match="input_format"):
        SegNet(_state(), H, W, device="cpu", precision="mixed", input_format="f16_nchw")


def test_float_input_plan_takes_float_tensors_only():
    from vision_semantic_segmentation_amd.network import SegNet
    net = SegNet(_state(), H, W, device="cpu", precision="f32", input_format="f32_nchw")
    with pytest.raises(ValueError, match="float tensor"):
        net.forward(torch.zeros((3, H, W), dtype=torch.uint8))
    with pytest.raises(ValueError, match="float tensor"):
        net.forward(torch.zeros((H, W, 3), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------ build_model / DeepLabV3Plus
def _cfg():
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    return get_network_cfg_defaults()


def test_build_model_returns_the_reference_tuple():
    from vision_semantic_segmentation_amd import DeepLabV3Plus, build_model
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    cfg = _cfg()
    cfg.DATASET.NUM_CLASSES = 7
    net, loss_fn, train_metric, val_metric = build_model(cfg)
    assert isinstance(net, DeepLabV3Plus) and isinstance(net, nn.Module)
    assert net.out_channels == 7 and net.in_channels == 3 and net.output_stride == 8
    assert isinstance(loss_fn, nn.Module) and loss_fn.ignore_index == 255
    assert isinstance(train_metric, MeanIOU) and isinstance(val_metric, MeanIOU) and train_metric is not val_metric
    assert train_metric.num_class == 7 and val_metric.num_class == 7
    assert net.state_dict()["decoder.refine_layers.2.conv.weight"].shape[0] == 7
    pred = torch.randn(2, 7, 5, 6)
    label = torch.randint(0, 7, (2, 5, 6), dtype=torch.int32)
    label[0, 0, 0] = 255
    ref = nn.functional.cross_entropy(pred, label.long(), ignore_index=255)
    assert torch.equal(loss_fn(pred, label), ref)


def test_build_model_refuses_other_model_types():
    from vision_semantic_segmentation_amd import build_model
    cfg = _cfg()
    cfg.MODEL.TYPE = "Xception"
    with pytest.raises(NotImplementedError, match="DeepLabv3"):
        build_model(cfg)


def test_state_dict_keys_are_the_checkpoint_keys_plus_num_batches_tracked():
    from vision_semantic_segmentation_amd import build_model
    from vision_semantic_segmentation_amd.network import random_state_dict
    net = build_model(_cfg())[0]
    sd = net.state_dict()
    ref = random_state_dict(seed=0)
    bn = sorted(k[:-len(".running_mean")] for k in ref if k.endswith(".running_mean"))
    assert set(sd) == set(ref) | {p + ".num_batches_tracked" for p in bn}
    for k, v in ref.items():
        assert torch.equal(sd[k], v), k
    assert not list(net.parameters())          # buffers only: nothing for an optimiser to train


def test_strict_load_state_dict_and_the_dataparallel_prefix():
    from vision_semantic_segmentation_amd import build_model
    net = build_model(_cfg())[0]
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    missing = dict(sd)
    missing.pop("aspp.conv.bn.running_var")
    with pytest.raises(RuntimeError, match="Missing key"):
        net.load_state_dict(missing)
    unexpected = dict(sd)
    unexpected["decoder.extra.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        net.load_state_dict(unexpected)
    # the reference's checkpoint: 'module.' keys, loaded through nn.DataParallel (train.py / semantic_segmentation.py:27-32)
    other = {k: (v + 0.5 if v.is_floating_point() else v) for k, v in sd.items()}
    dp = nn.DataParallel(net, device_ids=[]) if not torch.cuda.is_available() else nn.DataParallel(net, device_ids=[0])
    dp.load_state_dict({"module." + k: v for k, v in other.items()})
    # (.cpu(): where a GPU is present, DataParallel with one device id moves the module there)
    assert torch.equal(net.backbone.conv1.weight.cpu(), other["backbone.conv1.weight"])
    assert net._loaded
    with pytest.raises(RuntimeError, match="Missing key"):
        dp.load_state_dict(sd)             # without the prefix


def test_nonfinite_weights_are_refused_before_they_are_copied():
    from vision_semantic_segmentation_amd import build_model
    net = build_model(_cfg())[0]
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    before = getattr(net.backbone.layer1, "0").conv1.weight.clone()
    sd["backbone.layer1.0.conv1.weight"][0, 0, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="Inf / NaN"):
        net.load_state_dict(sd)
    assert torch.equal(getattr(net.backbone.layer1, "0").conv1.weight, before)


def test_forward_in_train_mode_raises():
    from vision_semantic_segmentation_amd import build_model
    net = build_model(_cfg())[0]
    assert net.training
    with pytest.raises(NotImplementedError, match="inference only"):
        net(torch.zeros(1, 3, 32, 32))
    assert net.eval() is net and not net.training
