"""MODEL.DECODER.REFINE_KERNEL_SIZE without a GPU: the k x k depthwise weights in the state spec, the decoder's op list (SegNet builds
its buffers on the CPU here, as in test_batch_cpu.py), the plan validator's rules for a ksize != 3 AVL_OP_DWCONV, the configuration
rules, and the DeepLabV3Plus module's buffers."""
import ctypes as C

import pytest
import torch

H, W = 97, 131
PRECISIONS = [("f32", dict(precision="f32")), ("f16", dict(precision="f16")), ("bf16", dict(precision="bf16")),
              ("mixed", dict(precision="mixed")), ("split16", dict(precision="mixed", full_split=True))]

_STATES = {}


def _state(ks=None):
    from vision_semantic_segmentation_amd.network import random_state_dict
    if ks not in _STATES:
        _STATES[ks] = random_state_dict(seed=0, **({} if ks is None else dict(refine_kernel_size=ks)))
    return _STATES[ks]


def _create(ops):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    rc = _lib.lib().avl_seg_plan_create((AvlSegOp * len(ops))(*ops), len(ops), C.byref(plan))
    if rc == 0:
        _lib.lib().avl_seg_plan_destroy(plan)
    return rc, _lib.last_error()


def _depthwise_shapes(spec):
    return [s for k, s in spec if k.startswith("decoder.refine_layers.") and k.endswith("depthwise_cnn.conv.weight")]


def test_state_spec_takes_refine_kernel_size():
    from vision_semantic_segmentation_amd.network import state_spec
    base = state_spec()
    assert state_spec(refine_kernel_size=None) == base
    assert state_spec(refine_kernel_size=(3, 3)) == base
    assert state_spec(refine_kernel_size=[3, 3]) == base
    assert _depthwise_shapes(base) == [(512, 1, 3, 3), (256, 1, 3, 3)]
    spec = state_spec(refine_kernel_size=(5, 7))
    assert _depthwise_shapes(spec) == [(512, 1, 5, 5), (256, 1, 7, 7)]
    # only the depthwise weights change
    assert [k for k, _ in spec] == [k for k, _ in base]
    assert [(k, s) for k, s in spec if "depthwise_cnn.conv" not in k] == [(k, s) for k, s in base if "depthwise_cnn.conv" not in k]
    # the channels follow LOW_LEVEL_OUT_CHANNELS / REFINE_CHANNELS as before
    assert _depthwise_shapes(state_spec(low_level_out=48, refine_channels=(128, 64), refine_kernel_size=(1, 6))) == [(304, 1, 1, 1), (128, 1, 6, 6)]


def test_default_random_state_is_unchanged():
    from vision_semantic_segmentation_amd.network import random_state_dict
    a, b = random_state_dict(seed=3), random_state_dict(seed=3, refine_kernel_size=(3, 3))
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    c = random_state_dict(seed=3, refine_kernel_size=(5, 5))
    w = c["decoder.refine_layers.0.depthwise_cnn.conv.weight"]
    assert tuple(w.shape) == (512, 1, 5, 5)
    assert 0.5 < float(w.std()) * (25 ** 0.5) / (2 ** 0.5) < 1.5          # Kaiming: fan-in 25


def test_check_state_dict_follows_the_kernel_size():
    from vision_semantic_segmentation_amd.network import check_state_dict
    st5 = _state((5, 5))
    check_state_dict(st5, refine_kernel_size=(5, 5))
    with pytest.raises(KeyError, match="mis-shapes"):
        check_state_dict(st5)
    with pytest.raises(KeyError, match="mis-shapes"):
        check_state_dict(_state(), refine_kernel_size=(5, 5))


def _sig(net):
    return [(net.op_names[i], op.kind, op.ksize, op.in_h, op.in_w, op.in_c, op.out_h, op.out_w, op.out_c, op.w_split, op.w_layout,
             bool(op.in_lo), bool(op.out_lo), bool(op.out_mx), op.out_f32) for i, op in enumerate(net.ops)]


@pytest.mark.parametrize("name,kw", PRECISIONS, ids=[p[0] for p in PRECISIONS])
def test_default_op_list_is_unchanged(name, kw):
    from vision_semantic_segmentation_amd.network import SegNet
    a = SegNet(_state(), H, W, device="cpu", **kw)
    b = SegNet(_state((3, 3)), H, W, device="cpu", **kw)
    assert _sig(a) == _sig(b)
    assert a.out_h == (H + 3) // 4 - 4 and (a.out_h, a.out_w) == (b.out_h, b.out_w)


@pytest.mark.parametrize("name,kw", PRECISIONS, ids=[p[0] for p in PRECISIONS])
def test_5x5_decoder_op_list(name, kw):
    from vision_semantic_segmentation_amd.network import OP_DWCONV, OP_DWPW, OP_GEMM, SegNet
    net = SegNet(_state((5, 5)), H, W, device="cpu", **kw)         # (ran avl_seg_plan_create)
    dec = [(n, op) for n, op in zip(net.op_names, net.ops) if n.startswith("decoder.refine_layers")]
    dw = [(n, op) for n, op in dec if op.kind == OP_DWCONV]
    assert [n for n, _ in dw] == ["decoder.refine_layers.0.depthwise_cnn", "decoder.refine_layers.1.depthwise_cnn"]
    assert not any(op.kind == OP_DWPW for _, op in dec)                 # no fused block, no fused classifier
    low = ((H + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1, ((W + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1
    for i, (_, op) in enumerate(dw):
        assert op.ksize == 5 and op.pad == 0 and op.dil == 1 and op.stride == 1 and not op.out_mx and not op.in2
        assert (op.in_h, op.in_w) == (low[0] - 4 * i, low[1] - 4 * i)
        assert (op.out_h, op.out_w) == (op.in_h - 4, op.in_w - 4)
        assert bool(op.in_lo) == bool(op.out_lo) == (name in ("mixed", "split16"))
    assert (net.out_h, net.out_w) == (low[0] - 8, low[1] - 8)
    cls = [(n, op) for n, op in dec if n == "decoder.refine_layers.2"]
    assert len(cls) == 1 and cls[0][1].kind == OP_GEMM and cls[0][1].out_f32 and (cls[0][1].out_h, cls[0][1].out_w) == (net.out_h, net.out_w)


def test_mixed_5_3_keeps_the_fused_3x3_block():
    from vision_semantic_segmentation_amd.network import OP_DWCONV, OP_DWPW, SegNet
    net = SegNet(_state((5, 3)), H, W, device="cpu", precision="mixed")
    kinds = {n: op for n, op in zip(net.op_names, net.ops) if n.startswith("decoder.refine_layers")}
    assert kinds["decoder.refine_layers.0.depthwise_cnn"].kind == OP_DWCONV and kinds["decoder.refine_layers.0.depthwise_cnn"].ksize == 5
    fused = kinds["decoder.refine_layers.1+classifier"]
    assert fused.kind == OP_DWPW and fused.ksize == 3 and fused.out_f32
    low = ((H + 3) // 4, (W + 3) // 4)
    assert (net.out_h, net.out_w) == (low[0] - 6, low[1] - 6)
    net = SegNet(_state((3, 5)), H, W, device="cpu", precision="mixed")
    names = [n for n in net.op_names if n.startswith("decoder.refine_layers")]
    assert "decoder.refine_layers.0" in names and "decoder.refine_layers.1.depthwise_cnn" in names and "decoder.refine_layers.2" in names


# ---- the plan validator
def _dw_op(ks=5, dtype=None, split=False, h=13, w=29, c=64, **over):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp, OP_DWCONV
    dtype = _lib.AVL_F16 if dtype is None else dtype
    tdt = torch.float32 if dtype == _lib.AVL_F32 else torch.float16
    keep = [torch.zeros(2 * h * w * c + 64, dtype=tdt), torch.zeros(ks * ks * c + 16), torch.zeros(c + 16),
            torch.zeros(2 * h * w * c + 64, dtype=tdt)]
    _dw_op.keep = keep
    op = AvlSegOp()
    op.kind, op.dtype = OP_DWCONV, dtype
    al = lambda t: (t.data_ptr() + 63) // 64 * 64
    op.in_, op.weight, op.bias, op.out = al(keep[0]), al(keep[1]), al(keep[2]), al(keep[3])
    if split:
        op.in_lo = op.in_ + h * w * c * keep[0].element_size()
        op.out_lo = op.out + h * w * c * keep[3].element_size()
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = h, w, c, c, h * w
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = h - (ks - 1), w - (ks - 1), c, c, h * w
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu = ks, 1, 0, 1, c, 1
    for k, v in over.items():
        setattr(op, k, v)
    return op


@pytest.mark.parametrize("ks", [1, 2, 4, 5, 6, 7])
def test_plan_accepts_kxk_dwconv(ks):
    from vision_semantic_segmentation_amd import _lib
    for dtype, split in ((_lib.AVL_F32, False), (_lib.AVL_F16, False), (_lib.AVL_BF16, False), (_lib.AVL_F16, True)):
        rc, msg = _create([_dw_op(ks, dtype, split)])
        assert rc == 0, msg


@pytest.mark.parametrize("over,what", [
    (dict(ksize=8, out_h=6, out_w=22), "ksize 8"),
    (dict(ksize=0), "ksize 0"),
    (dict(out_h=10), "out_h"),
    (dict(out_w=24), "out_w"),
    (dict(pad=1), "pad"),
    (dict(dil=2), "dil"),
    (dict(stride=2), "stride"),
    (dict(out_c=32), "out_c"),
    (dict(in_c=48, in_ld=48, out_c=48, out_ld=48), "channels"),
])
def test_plan_refuses_bad_kxk_dwconv(over, what):
    rc, msg = _create([_dw_op(5, **over)])
    assert rc != 0 and what in msg, msg


def test_plan_refuses_out_mx_and_one_sided_split():
    op = _dw_op(5, split=True)
    op.out_mx = op.out
    rc, msg = _create([op])
    assert rc != 0 and "out_mx" in msg, msg
    op = _dw_op(5, split=True)
    op.out_lo = 0
    rc, msg = _create([op])
    assert rc != 0 and "in_lo and out_lo" in msg, msg


def test_plan_refuses_an_empty_output():
    rc, msg = _create([_dw_op(7, h=6, w=29)])
    assert rc != 0


def test_3x3_rule_is_unchanged():
    op = _dw_op(3)
    rc, msg = _create([op])
    assert rc != 0 and "zero page" in msg, msg          # the 3x3 op still needs in2


# ---- configuration
def test_refine_kernel_sizes_rules():
    from vision_semantic_segmentation_amd.network import refine_kernel_sizes
    assert refine_kernel_sizes(None, (256, 256)) == (3, 3)
    assert refine_kernel_sizes([5, 7], (256, 256)) == (5, 7)
    assert refine_kernel_sizes([3], (256, 256)) == (3, 3)              # all 3s: today's meaning whatever the length
    assert refine_kernel_sizes([3, 3, 3], (256,)) == (3,)
    with pytest.raises(ValueError, match="one kernel size per refine block"):
        refine_kernel_sizes([5], (256, 256))
    for bad in ([0, 3], [8, 3], [3, 9]):
        with pytest.raises(ValueError, match="1, 2, 3, 4, 5, 6, 7"):
            refine_kernel_sizes(bad, (256, 256))


def test_too_small_image_raises_before_any_buffer():
    from vision_semantic_segmentation_amd.network import SegNet
    # default [3, 3]: 17 x 17 is the smallest (low-level map 5 x 5 -> one pixel)
    assert SegNet(_state(), 17, 17, device="cpu", precision="f32").out_h == 1
    with pytest.raises(ValueError, match="smallest input that works is 17x17"):
        SegNet(_state(), 16, 16, device="cpu", precision="f32")
    with pytest.raises(ValueError, match="smallest input that works is 33x64"):
        SegNet(_state((5, 5)), 32, 64, device="cpu", precision="mixed")
    net = SegNet(_state((5, 5)), 33, 64, device="cpu", precision="mixed")
    assert net.out_h == 1


def test_semantic_segmentation_config_errors_before_any_gpu_call(monkeypatch):
    from vision_semantic_segmentation_amd import SemanticSegmentation
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)      # reach the configuration checks without a GPU
    for ks, match in (([5], "one kernel size per refine block"), ([9, 3], "1, 2, 3, 4, 5, 6, 7")):
        cfg = get_network_cfg_defaults()
        cfg.MODEL.DECODER.REFINE_KERNEL_SIZE = ks
        with pytest.raises(ValueError, match=match):
            SemanticSegmentation(cfg, device="cpu")


def test_build_model_5x5_buffers_and_strict_load():
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    from vision_semantic_segmentation_amd.models import build_model
    from vision_semantic_segmentation_amd.network import random_state_dict
    cfg = get_network_cfg_defaults()
    cfg.MODEL.DECODER.REFINE_KERNEL_SIZE = [5, 5]
    net = build_model(cfg)[0]
    sd = net.state_dict()
    assert tuple(sd["decoder.refine_layers.0.depthwise_cnn.conv.weight"].shape) == (512, 1, 5, 5)
    assert tuple(sd["decoder.refine_layers.1.depthwise_cnn.conv.weight"].shape) == (256, 1, 5, 5)
    assert net._spec_kw["refine_kernel_size"] == (5, 5)
    st = random_state_dict(seed=7, refine_kernel_size=(5, 5))
    holder = torch.nn.Module()                # what nn.DataParallel(net) saves: every key under 'module.'
    holder.module = net
    wrapped = {k: v for k, v in holder.state_dict().items() if k.endswith("num_batches_tracked")}
    wrapped.update({"module." + k: v for k, v in st.items()})
    res = holder.load_state_dict(wrapped, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.weights()["decoder.refine_layers.1.depthwise_cnn.conv.weight"], st["decoder.refine_layers.1.depthwise_cnn.conv.weight"])
    # a 3x3 checkpoint does not load into it
    with pytest.raises(RuntimeError, match="size mismatch"):
        net.load_state_dict(random_state_dict(seed=0), strict=False)
