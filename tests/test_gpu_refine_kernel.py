"""MODEL.DECODER.REFINE_KERNEL_SIZE on the GPU: the k x k depthwise op alone (seg_dwconv_k.hip, all three forms) against float64
F.conv2d(groups=C), and whole networks with k x k refine blocks through SemanticSegmentation, batched plans, the full-resolution
paths, DeepLabV3Plus and the raw-frame stem, against the torch-CPU oracle (which follows the weights' shapes).
Bars: op alone max|d| / max|ref| <= 1e-5 (f32, split), 1e-3 (f16), 8e-3 (bf16); networks as in test_gpu_backbones.py (f32, split16,
mixed <= 1e-3; f16 <= 4e-3, bf16 <= 4e-2)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_STATES = {}


def _state(ks):
    from vision_semantic_segmentation_amd.network import random_state_dict
    if ks not in _STATES:
        _STATES[ks] = random_state_dict(seed=0, refine_kernel_size=ks)
    return _STATES[ks]


def _cfg(precision, ks):
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_network_cfg_defaults()
    cfg.MODEL.PRECISION = precision
    cfg.MODEL.DECODER.REFINE_KERNEL_SIZE = list(ks)
    cfg.MODEL.MIXED_SELF_CHECK = False
    return cfg


def _seg(precision, ks, device):
    from vision_semantic_segmentation_amd import SemanticSegmentation
    seg = SemanticSegmentation(_cfg("mixed" if precision == "split16" else precision, ks), device=device, state_dict=_state(ks))
    if precision == "split16":
        seg._rung = "split16"
    return seg


def _low(n):
    return ((n + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1


# ------------------------------------------------------------------------------------------------ the op alone
FORMS = [("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16), ("split", torch.float16)]
OP_BAR = {"f32": 1e-5, "split": 1e-5, "f16": 1e-3, "bf16": 8e-3}


def _run_op(form, ks, h, w, c, batch, dev, seed, in_pad=0, in_off=0, out_pad=0, out_off=0):
    """the op alone on [batch][h][w][c] (optionally a column slice at in_off / out_off of rows in_ld = c + in_pad / out_ld = c + out_pad);
    NaN sentinels in the output columns outside the slice and in the rows past the output, NaN poison in the input's other columns
    and in rows past the last image.  Returns (got, ref) as float64 [batch][oh][ow][c]."""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp, OP_DWCONV
    dt = dict(FORMS)[form]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, h, w, c, generator=g, dtype=torch.float64)
    wt = torch.randn(c, 1, ks, ks, generator=g, dtype=torch.float64).float()
    b = (0.1 * torch.randn(c, generator=g, dtype=torch.float64)).float()
    oh, ow = h - (ks - 1), w - (ks - 1)
    hi = x.to(dt)
    lo = (x - hi.double()).to(dt) if form == "split" else None
    xin = hi.double() + (lo.double() if lo is not None else 0.0)                 # what the kernel reads
    ref = torch.relu(F.conv2d(xin.permute(0, 3, 1, 2), wt.double(), b.double(), groups=c)).permute(0, 2, 3, 1)
    rows_in, rows_out = batch * h * w, batch * oh * ow
    in_ld, out_ld = c + in_pad, c + out_pad
    tail = 5                                                                      # sentinel rows past the output / poison past the input

    def plane(t):
        buf = torch.full((rows_in + tail, in_ld), float("nan"), dtype=dt)
        buf[:rows_in, in_off:in_off + c] = t.reshape(rows_in, c)
        return buf.to(dev)
    d_in = plane(hi)
    d_in_lo = plane(lo) if lo is not None else None
    d_out = torch.full((rows_out + tail, out_ld), float("nan"), dtype=dt, device=dev)
    d_out_lo = torch.full((rows_out + tail, out_ld), float("nan"), dtype=dt, device=dev) if lo is not None else None
    d_w = wt.reshape(c, ks * ks).t().contiguous().to(dev)                         # [tap][C]
    d_b = b.to(dev)
    es = d_in.element_size()
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = OP_DWCONV, {"f32": _lib.AVL_F32, "bf16": _lib.AVL_BF16}.get(form, _lib.AVL_F16), batch
    op.in_, op.out, op.weight, op.bias = d_in.data_ptr() + in_off * es, d_out.data_ptr() + out_off * es, d_w.data_ptr(), d_b.data_ptr()
    if lo is not None:
        op.in_lo, op.out_lo = d_in_lo.data_ptr() + in_off * es, d_out_lo.data_ptr() + out_off * es
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = h, w, c, in_ld, rows_in
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = oh, ow, c, out_ld, rows_out
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu = ks, 1, 0, 1, c, 1
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan)), "avl_seg_plan_create")
    try:
        _lib.check(_lib.lib().avl_seg_plan_run(plan, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "avl_seg_plan_run")
        torch.cuda.synchronize(dev)
    finally:
        _lib.lib().avl_seg_plan_destroy(plan)
    for o in (d_out, d_out_lo):
        if o is None:
            continue
        oc = o.cpu()
        assert bool(oc[rows_out:].isnan().all()), "rows past the output written (%s k=%d)" % (form, ks)
        assert bool(oc[:, :out_off].isnan().all()) and bool(oc[:, out_off + c:].isnan().all()), "columns outside the slice written (%s k=%d)" % (form, ks)
    sl = slice(out_off, out_off + c)
    got = d_out[:rows_out, sl].double() + (d_out_lo[:rows_out, sl].double() if lo is not None else 0.0)
    return got.cpu().reshape(batch, oh, ow, c), ref


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
@pytest.mark.parametrize("ks", [1, 2, 4, 5, 6, 7])
def test_kxk_op_against_float64(form, ks, cuda_device):
    for (h, w), c, batch in (((13, 29), 64, 1), ((31, 47), 320, 3), ((13, 29), 320, 3), ((31, 47), 64, 1)):
        got, ref = _run_op(form, ks, h, w, c, batch, cuda_device, seed=ks * 100 + h + c + batch)
        assert bool(torch.isfinite(got).all()), (form, ks, h, w, c, batch)
        rel = float((got - ref).abs().max() / ref.abs().max())
        print("k=%d %s %dx%d C=%d batch %d: max rel err %.2e" % (ks, form, h, w, c, batch, rel))
        assert rel <= OP_BAR[form], (form, ks, h, w, c, batch, rel)


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
@pytest.mark.parametrize("ks", [2, 4, 6, 7])
def test_kxk_op_tile_edges_and_slices(form, ks, cuda_device):
    """Geometry at the 32 x 8 output tile's edges: a 1 x 1 output, an output one pixel past a tile in both directions, a channel slice
    of wider rows at column offsets, and a batch of 3 whose images end mid-tile (the halo must stay inside each image)."""
    cases = (  # (out_h, out_w, c, batch, in_pad, in_off, out_pad, out_off)
        (1, 1, 64, 1, 0, 0, 0, 0),
        (9, 33, 64, 1, 0, 0, 0, 0),
        (9, 33, 128, 1, 64, 64, 128, 64),
        (11, 45, 64, 3, 64, 0, 128, 128),
        (1, 1, 64, 3, 64, 32, 128, 64),
    )
    for oh, ow, c, batch, ip, io, op_, oo in cases:
        h, w = oh + ks - 1, ow + ks - 1
        got, ref = _run_op(form, ks, h, w, c, batch, cuda_device, seed=ks * 1000 + oh * 50 + ow + batch, in_pad=ip, in_off=io, out_pad=op_, out_off=oo)
        assert bool(torch.isfinite(got).all()), (form, ks, oh, ow, c, batch)
        rel = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        assert rel <= OP_BAR[form], (form, ks, oh, ow, c, batch, rel)


# ------------------------------------------------------------------------------------------------ whole networks
NET_BAR = {"f32": 1e-3, "split16": 1e-3, "mixed": 1e-3, "f16": 4e-3, "bf16": 4e-2}


@pytest.mark.parametrize("ks", [(5, 5), (7, 7), (5, 3), (4, 4), (6, 6), (4, 6)], ids=["5-5", "7-7", "5-3", "4-4", "6-6", "4-6"])
def test_network_against_oracle(ks, cuda_device):
    from oracle import network_oracle as no
    st = _state(ks)
    for h, w in ((96, 128), (97, 131)):
        img = np.random.default_rng(h + w + ks[0]).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        ref = no.forward_logits(st, img)[0]
        shrink = sum(k - 1 for k in ks)
        assert tuple(ref.shape[1:]) == (_low(h) - shrink, _low(w) - shrink)
        for precision in ("f32", "split16", "mixed", "f16", "bf16"):
            seg = _seg(precision, ks, cuda_device)
            got = seg.logits(img).cpu()
            assert tuple(got.shape) == tuple(ref.shape), (precision, got.shape, ref.shape)
            rel = float((got - ref).abs().max() / ref.abs().max())
            print("%s %dx%d %s: max rel err %.3e" % (ks, h, w, precision, rel))
            assert rel <= NET_BAR[precision], (ks, h, w, precision, rel)
            labels = seg.segmentation(img)
            assert labels.shape == (_low(h) - shrink, _low(w) - shrink)
            assert np.array_equal(labels, got.argmax(0).numpy())


def test_default_label_shape_is_h4_minus_4(cuda_device):
    from vision_semantic_segmentation_amd import SemanticSegmentation
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_network_cfg_defaults()
    cfg.MODEL.MIXED_SELF_CHECK = False
    seg = SemanticSegmentation(cfg, device=cuda_device)
    img = np.random.default_rng(1).integers(0, 256, size=(96, 128, 3), dtype=np.uint8)
    assert seg.segmentation(img).shape == (96 // 4 - 4, 128 // 4 - 4)


@pytest.mark.parametrize("precision", ["f32", "f16", "bf16", "mixed", "split16"])
def test_batch3_equals_batch1_bit_for_bit(precision, cuda_device):
    ks = (5, 5)
    seg = _seg(precision, ks, cuda_device)
    frames = np.random.default_rng(4).integers(0, 256, size=(3, 97, 131, 3), dtype=np.uint8)
    batch = seg.logits(frames).clone()
    assert tuple(batch.shape) == (3, 19, _low(97) - 8, _low(131) - 8)
    for i in range(3):
        one = seg.logits(frames[i])
        assert torch.equal(batch[i], one), (precision, i)


@pytest.mark.parametrize("precision", ["mixed", "f32"])
def test_batch3_equals_batch1_even_kernel(precision, cuda_device):
    ks = (6, 6)
    seg = _seg(precision, ks, cuda_device)
    frames = np.random.default_rng(8).integers(0, 256, size=(3, 97, 131, 3), dtype=np.uint8)
    batch = seg.logits(frames).clone()
    assert tuple(batch.shape) == (3, 19, _low(97) - 10, _low(131) - 10)
    for i in range(3):
        one = seg.logits(frames[i])
        assert torch.equal(batch[i], one), (precision, i)


def test_full_resolution_and_validate_step(cuda_device):
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    seg = _seg("mixed", (5, 5), cuda_device)
    H, W, K = 97, 131, 19
    img = np.random.default_rng(6).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    small = seg.logits(img).clone()
    up = seg.logits(img, upsample_pred=True).clone()
    assert tuple(up.shape) == (K, H, W)
    ref = F.interpolate(small[None].double(), size=(H, W), mode="bilinear", align_corners=True)[0]
    assert float((up.double() - ref).abs().max() / ref.abs().max()) <= 1e-5
    labels = seg.segmentation(img, upsample_pred=True)
    assert labels.shape == (H, W)
    assert float((torch.from_numpy(labels) == up.argmax(0).cpu()).float().mean()) >= 0.999
    rng = np.random.default_rng(2)
    gt = np.where(rng.random((H, W)) < 0.6, labels, rng.integers(0, K, size=(H, W)))
    gt[rng.random((H, W)) < 0.05] = 255
    metric = MeanIOU(K, device=cuda_device)
    loss = seg.validate_step(img, gt.astype(np.int64), metric)
    ref_loss = F.cross_entropy(up[None].double().cpu(), torch.from_numpy(gt.astype(np.int64))[None], ignore_index=255).item()
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert int(metric.confusion_matrix.sum()) == int((gt != 255).sum())


def test_deeplabv3plus_5x5(cuda_device):
    from oracle import network_oracle as no
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    from vision_semantic_segmentation_amd.models import build_model
    cfg = get_network_cfg_defaults()
    cfg.MODEL.DECODER.REFINE_KERNEL_SIZE = [5, 5]
    net = build_model(cfg)[0]
    st = _state((5, 5))
    net.load_state_dict(dict(net.state_dict(), **st), strict=True)
    net = net.to(cuda_device).eval()
    H, W = 96, 128
    img = np.random.default_rng(3).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    x = ((torch.from_numpy(img).float() / 255.0 - mean) / std).permute(2, 0, 1)[None].contiguous()
    got = net(x.to(cuda_device), upsample_pred=False).cpu()
    ref = no.forward_logits(st, img)
    assert tuple(got.shape) == tuple(ref.shape) == (1, 19, H // 4 - 8, W // 4 - 8)
    rel = float((got - ref).abs().max() / ref.abs().max())
    print("DeepLabV3Plus [5, 5] mixed: max rel err %.3e" % rel)
    assert rel <= 1e-3


def test_raw_frame_5x5_mixed(cuda_device):
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    seg = _seg("mixed", (5, 5), cuda_device)
    bgr = np.random.default_rng(9).integers(0, 256, size=(192, 256, 3), dtype=np.uint8)
    rgb = preprocess_device(bgr, None, 2)
    want = seg.segmentation_device(rgb).clone()
    assert tuple(want.shape) == (96 // 4 - 8, 128 // 4 - 8)
    assert torch.equal(seg.segmentation_device_raw(bgr, factor=2), want)
