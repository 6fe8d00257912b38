"""The reference's model API on the GPU: DeepLabV3Plus(x) on normalised float N x 3 x H x W tensors (models.py, the fp32-input stem
AVL_IN_F32_CHW) against the uint8 path bit for bit, against the torch-CPU oracle off the uint8 grid, through the reference's loading
sequence (nn.DataParallel, 'module.' keys) and its validation loop (CrossEntropyLoss + MeanIOU)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def _cfg(precision="mixed", self_check=False):
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_network_cfg_defaults()
    cfg.MODEL.PRECISION = precision
    cfg.MODEL.MIXED_SELF_CHECK = self_check
    return cfg


def _to_x(frames_u8):
    """uint8 [N,H,W,3] -> float32 [N,3,H,W] with the stem's own arithmetic: u8 / 255, - mean, / std, each rounded to fp32 (NumPy: a
    true division, where a GPU `div` may multiply by the reciprocal)"""
    import torch
    x = (frames_u8.astype(np.float32) / np.float32(255) - MEAN) / STD
    assert x.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _oracle(state, x):
    """DeepLabV3Plus.forward(x, upsample_pred=False) of the torch-CPU oracle on a float batch x [N,3,H,W]"""
    import torch
    from oracle import network_oracle as no
    with torch.no_grad():
        f = no.backbone_forward(state, x.cpu().float())
        return no.decoder_forward(state, no.aspp_forward(state, f["feature"]), f["low_feature"])


_MODELS = {}


def _model(precision, device):
    from vision_semantic_segmentation_amd import DeepLabV3Plus
    if precision not in _MODELS:
        cfg = _cfg(precision)
        m = cfg.MODEL
        _MODELS[precision] = DeepLabV3Plus(cfg.DATASET.IN_CHANNELS, cfg.DATASET.NUM_CLASSES, m.BACKBONE, m.ASPP, m.DECODER, m.OUTPUT_STRIDE,
                                           precision=precision, device=device, self_check=False).eval()
    return _MODELS[precision]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    import torch
    _MODELS.clear()
    torch.cuda.empty_cache()


CASES = [(p, hw, n) for p in ("f32", "f16", "bf16", "mixed", "split16") for hw in ((97, 131), (192, 256)) for n in (1, 3)] + [("mixed", (1080, 1920), 1)]


@pytest.mark.parametrize("precision,hw,n", CASES, ids=["%s-%dx%d-n%d" % (p, hw[0], hw[1], n) for p, hw, n in CASES])
def test_float_input_matches_the_u8_path_bit_for_bit(precision, hw, n, cuda_device):
    import torch
    model = _model(precision, cuda_device)
    h, w = hw
    frames = _frames(n, h, w, seed=h + n)
    x = _to_x(frames).to(cuda_device)
    got = model(x, upsample_pred=False)
    seg = model.segmentation()
    ref = seg.logits(frames[0] if n == 1 else frames)
    ref = ref.unsqueeze(0) if n == 1 else ref
    assert got.grad_fn is None and got.dtype == torch.float32 and got.is_contiguous()
    assert tuple(got.shape) == tuple(ref.shape) == (n, 19, ((h - 1) // 2) // 2 + 1 - 4, ((w - 1) // 2) // 2 + 1 - 4)
    assert torch.equal(got, ref), float((got - ref).abs().max())


def _off_grid_inputs(h, w):
    import torch
    import torch.nn.functional as F
    noise = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 3, h, w)).astype(np.float32))
    small = _to_x(_frames(1, h // 2, w // 2, seed=6))
    resized = F.interpolate(small, size=(h - 9, w - 13), mode="bilinear", align_corners=False)
    padded = F.pad(resized, (6, 7, 4, 5))              # zero padding in normalised space
    return {"noise": noise, "resized_padded": padded}


@pytest.mark.parametrize("precision,bar", [("f32", 1e-5), ("mixed", 1e-3), ("split16", 1e-4)])
def test_off_grid_inputs_against_the_oracle(precision, bar, cuda_device):
    model = _model(precision, cuda_device)
    h, w = 97, 131
    for name, x in _off_grid_inputs(h, w).items():
        ref = _oracle(model.weights(), x)
        got = model(x.to(cuda_device), upsample_pred=False).cpu()
        assert got.shape == ref.shape
        err = float((got - ref).abs().max() / ref.abs().max())
        print("%s %s: %.2e of max|logit|" % (precision, name, err))
        assert err <= bar, (precision, name, err)


@pytest.mark.parametrize("n", [1, 2])
def test_upsample_pred_is_the_default(n, cuda_device):
    import torch
    import torch.nn.functional as F
    model = _model("mixed", cuda_device)
    h, w = 97, 131
    frames = _frames(n, h, w, seed=11)
    x = _to_x(frames).to(cuda_device)
    full = model(x)
    assert tuple(full.shape) == (n, 19, h, w) and full.grad_fn is None
    seg = model.segmentation()
    ref = seg.logits(frames[0] if n == 1 else frames, upsample_pred=True)
    ref = ref.unsqueeze(0) if n == 1 else ref
    assert torch.equal(full, ref)
    low = model(x, upsample_pred=False)
    interp = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=True)
    assert float((full - interp).abs().max()) <= 1e-6 * float(interp.abs().max())
    # an unbatched [3,H,W] input gives unbatched logits, a CPU tensor is copied, another float dtype converted
    one = model(x[0].cpu(), upsample_pred=False)
    assert tuple(one.shape) == tuple(low.shape[1:]) and torch.equal(one, low[0])
    assert torch.equal(model(x.to(torch.float64), upsample_pred=False), low)


def test_the_reference_loading_sequence(cuda_device, tmp_path):
    import torch
    import torch.nn as nn
    from vision_semantic_segmentation_amd import SemanticSegmentation, build_model
    from vision_semantic_segmentation_amd.network import random_state_dict
    d = cuda_device.index if cuda_device.index is not None else torch.cuda.current_device()
    cfg = _cfg("mixed")
    h, w = 97, 131
    frames = _frames(2, h, w, seed=21)
    x = _to_x(frames)
    model = nn.DataParallel(build_model(cfg)[0], device_ids=[d]).cuda(d)
    for seed in (3, 4):
        state = random_state_dict(seed=seed)
        path = str(tmp_path / ("ckpt%d.pth" % seed))
        ckpt = {"module." + k: v for k, v in state.items()}
        ckpt.update({"module." + k: torch.tensor(7) for k in model.module.state_dict() if k.endswith("num_batches_tracked")})
        torch.save({"model": ckpt}, path)
        model.load_state_dict(torch.load(path)["model"])
        model.eval()
        with torch.no_grad():
            got = model(x.to(torch.device("cuda", d)), upsample_pred=False)
        ref = SemanticSegmentation(cfg, device=torch.device("cuda", d), state_dict=state).logits(frames)
        assert torch.equal(got, ref), (seed, float((got - ref).abs().max()))
        if seed == 3:
            first = got
    assert not torch.equal(first, got)            # the second weight set's logits, not the first's


def test_the_reference_validation_loop(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import build_model
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    cfg = _cfg("mixed")
    net, loss_fn, _, val_metric = build_model(cfg)
    model = net.to(cuda_device).eval()
    seg = model.segmentation()
    fused = MeanIOU(cfg.DATASET.NUM_CLASSES, device=cuda_device)
    h, w = 97, 131
    rng = np.random.default_rng(31)
    for i in range(3):
        frame = _frames(1, h, w, seed=40 + i)
        label = rng.integers(0, 19, size=(1, h, w)).astype(np.int64)
        label[rng.random((1, h, w)) < 0.1] = 255
        lab = torch.from_numpy(label).to(cuda_device)
        with torch.no_grad():
            preds = model(_to_x(frame).to(cuda_device))
            loss = float(loss_fn(preds, lab))
        val_metric.evaluate(preds, lab)
        ref_loss = seg.validate_step(frame[0], label[0], fused)
        assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (i, loss, ref_loss)
    assert torch.equal(val_metric.confusion_matrix, fused.confusion_matrix)
    assert int(val_metric.confusion_matrix.sum()) == int(fused.confusion_matrix.sum()) > 0


def test_each_call_returns_a_new_tensor(cuda_device):
    import torch
    model = _model("mixed", cuda_device)
    h, w = 97, 131
    x1, x2 = _to_x(_frames(1, h, w, seed=51)).to(cuda_device), _to_x(_frames(1, h, w, seed=52)).to(cuda_device)
    for upsample in (False, True):
        a = model(x1, upsample_pred=upsample)
        keep = a.clone()
        b = model(x2, upsample_pred=upsample)
        assert torch.equal(a, keep) and not torch.equal(a, b) and a.data_ptr() != b.data_ptr()


def _overflowing_state(base):
    """test_gpu_robust.py's checkpoint that overflows f16 in layer2.1 (bn1 x 1e5, undone by conv2 / 1e5) and is finite in fp32"""
    st = {k: v.clone() for k, v in base.items()}
    st["backbone.layer2.1.bn1.weight"] = st["backbone.layer2.1.bn1.weight"] * 1.0e5
    st["backbone.layer2.1.bn1.bias"] = st["backbone.layer2.1.bn1.bias"] * 1.0e5
    st["backbone.layer2.1.conv2.weight"] = st["backbone.layer2.1.conv2.weight"] / 1.0e5
    return st


def test_weights_that_force_the_f32_rung(cuda_device):
    import warnings

    import torch
    from vision_semantic_segmentation_amd import build_model
    from vision_semantic_segmentation_amd.network import random_state_dict
    cfg = _cfg("mixed", self_check="auto")          # weights loaded through load_state_dict: the self-check runs
    model = build_model(cfg)[0].to(cuda_device)
    st = _overflowing_state(random_state_dict(seed=0))
    sd = model.state_dict()
    sd.update(st)
    model.load_state_dict(sd)
    model.eval()
    h, w = 96, 128
    x = _to_x(_frames(1, h, w, seed=61))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = model(x.to(cuda_device), upsample_pred=False).cpu()
    seg = model.segmentation()
    assert seg.mixed_check is not None and seg.mixed_check["rung"] == "f32"
    assert any("no 16-bit plan" in str(c.message) for c in caught)
    ref = _oracle(st, x)
    err = float((got - ref).abs().max() / ref.abs().max())
    print("overflowing weights through the f32 rung: %.2e of max|logit|" % err)
    assert err <= 1e-4
