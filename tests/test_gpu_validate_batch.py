"""Batched full-resolution validation on the GPU (csrc/seg_head.hip through avl_upsample_logits_batch / avl_seg_eval_full_res_batch):
a batch of N images in one launch against N calls of the single-image entry points (bit for bit: labels, counts, every image's loss
sum; the batch sum is the left-to-right fp64 sum of the image sums), against torch on the CPU, and end to end through
SemanticSegmentation.validate_step on [N, h, w, 3] and the drop-in DeepLabV3Plus.validate_step."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# 266 x 476 -> 1080 x 1920 is the bench frame's head; 29 x 37 -> 131 x 163 has ragged tiles in both directions; 200 x 300 -> 21 x 31
# shrinks so strongly that a tile's window does not fit in LDS (the corners are read from global memory)
SHAPES = [((266, 476), (1080, 1920)), ((29, 37), (131, 163)), ((200, 300), (21, 31))]
BATCHES = [1, 2, 3, 5]
CLASSES = [5, 19, 64]
CASES = [(s, n, k) for s in SHAPES for n in BATCHES for k in CLASSES]
IDS = ["%dx%d-%dx%d-n%d-k%d" % (s[0] + s[1] + (n, k)) for s, n, k in CASES]


def _case(shape, N, K, invalid):
    """seeded logits [N, K, h, w] and ground truth uint8 [N, H, W]: ~10 % 255, K - 1 present, image 1 (when there is one) entirely 255;
    invalid: a few values in [K, 255) in the first and the last image"""
    (h, w), (H, W) = shape
    rng = np.random.default_rng(100000 * N + 1000 * K + h)
    x = torch.from_numpy((4.0 * rng.standard_normal((N, K, h, w), dtype=np.float32)))
    gt = rng.integers(0, K, size=(N, H, W)).astype(np.uint8)
    gt[rng.random((N, H, W)) < 0.1] = 255
    gt[:, H // 2, W // 3] = K - 1
    if N > 1:
        gt[1] = 255
    if invalid:
        for i, count in ((0, 7), (N - 1, 3)):
            flat = gt[i].reshape(-1)
            flat[rng.choice(H * W, count, replace=False)] = rng.integers(K, 255, size=count)
    return x, gt


def _dev(x, device, ld, image_rows):
    """[N, K, h, w] CPU -> a batched plan's layout on the device: NHWC rows of stride ld >= K, image i image_rows >= h * w rows after
    image i - 1; NaN wherever nothing may be read"""
    N, K, h, w = x.shape
    buf = torch.full((N * image_rows, ld), float("nan"), dtype=torch.float32, device=device)
    for i in range(N):
        buf[i * image_rows:i * image_rows + h * w, :K] = x[i].permute(1, 2, 0).reshape(h * w, K).to(device)
    return buf.as_strided((N, h, w, K), (image_rows * ld, w * ld, ld, 1))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _single_eval(x_hwk, H, W, gt, want_labels=True, want_cm=True):
    """avl_seg_eval_full_res (the single-image entry point, as it was before there was a batch) on one image's logits [h, w, K]
    -> (labels uint8 [H, W], confusion int64 [K, K], loss float64 [2], counts int64 [2]) on the device"""
    from vision_semantic_segmentation_amd import _lib
    L, dev = _lib.lib(), x_hwk.device
    h, w, K = x_hwk.shape
    ld = x_hwk.stride(1)
    assert x_hwk.stride(2) == 1 and x_hwk.stride(0) == w * ld
    labels = torch.full((H, W), 77, dtype=torch.uint8, device=dev) if want_labels else None
    cm = torch.zeros((K, K), dtype=torch.int64, device=dev) if want_cm else None
    loss = torch.zeros(2, dtype=torch.float64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    scratch = torch.empty((L.avl_seg_eval_scratch_bytes(H, W) + 7) // 8, dtype=torch.float64, device=dev)
    _lib.check(L.avl_seg_eval_full_res(_ptr(x_hwk), h, w, K, ld, H, W, _ptr(gt), 255, _ptr(labels), _ptr(cm), _ptr(loss), _ptr(counts),
                                       _ptr(scratch), _stream(dev)), "avl_seg_eval_full_res")
    return labels, cm, loss, counts


def _single_labels(x_hwk, H, W):
    from vision_semantic_segmentation_amd import _lib
    h, w, K = x_hwk.shape
    labels = torch.full((H, W), 77, dtype=torch.uint8, device=x_hwk.device)
    _lib.check(_lib.lib().avl_seg_eval_full_res(_ptr(x_hwk), h, w, K, x_hwk.stride(1), H, W, None, 255, _ptr(labels), None, None, None, None,
                                                _stream(x_hwk.device)), "avl_seg_eval_full_res")
    return labels


def _single_upsample(x_hwk, H, W):
    from vision_semantic_segmentation_amd import _lib
    h, w, K = x_hwk.shape
    out = torch.full((K, H, W), float("nan"), dtype=torch.float32, device=x_hwk.device)
    _lib.check(_lib.lib().avl_upsample_logits(_ptr(x_hwk), h, w, K, x_hwk.stride(1), _ptr(out), H, W, _stream(x_hwk.device)),
               "avl_upsample_logits")
    return out


def _bits(values):
    return np.asarray(values, dtype=np.float64).tobytes()


def _same_bits(a, b):
    """two device tensors hold the same bytes (NaN-safe)"""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)
    return a.shape == b.shape and bool(torch.equal(a, b))


@pytest.mark.parametrize("shape,N,K", CASES, ids=IDS)
def test_batched_eval_equals_the_single_image_entry_point_bit_for_bit(shape, N, K, cuda_device):
    from vision_semantic_segmentation_amd import seg_head
    (h, w), (H, W) = shape
    x, gt = _case(shape, N, K, invalid=True)
    gtd = torch.from_numpy(gt).to(cuda_device)
    invalid = [int(((gt[i] >= K) & (gt[i] != 255)).sum()) for i in range(N)]
    counted = [int((gt[i] < K).sum()) for i in range(N)]
    assert invalid[0] >= 7 and (gt == K - 1).any() and (N == 1 or counted[1] == 0)
    for ld, image_rows in ((K, h * w), (K + 3, h * w + 5)):        # dense, as a batched plan leaves it; padded rows and images
        xd = _dev(x, cuda_device, ld, image_rows)
        labels = torch.full((N, H, W), 99, dtype=torch.uint8, device=cuda_device)
        cm = torch.zeros((K, K), dtype=torch.int64, device=cuda_device)
        ws = seg_head.EvalWorkspace(H, W, cuda_device, batch=N)
        seg_head.full_res_eval(xd, H, W, gt=gtd, labels_out=labels, confusion=cm, workspace=ws)
        res = ws.result()
        cm_sum = torch.zeros_like(cm)
        sums = []
        for i in range(N):
            lab1, cm1, loss1, counts1 = _single_eval(xd[i], H, W, gtd[i])
            assert _same_bits(labels[i], lab1), (ld, i)
            cm_sum += cm1
            loss1, counts1 = loss1.cpu().tolist(), counts1.cpu().tolist()
            assert _bits(res["image_loss_sum"][i]) == _bits(loss1[0]), (ld, i, res["image_loss_sum"][i], loss1[0])
            assert _bits(res["image_loss"][i]) == _bits(loss1[1]), (ld, i)
            assert res["image_count"][i] == counts1[0] == counted[i] and res["image_invalid"][i] == counts1[1] == invalid[i], (ld, i)
            sums.append(loss1[0])
            if N == 1:                                              # a batch of one: every output word of the old entry point
                assert _bits(res["loss_sum"]) == _bits(loss1[0]) and _bits(res["loss"]) == _bits(loss1[1])
                assert [res["count"], res["invalid"]] == counts1
        assert torch.equal(cm, cm_sum) and int(cm.sum()) == sum(counted)
        total = sums[0]
        for s in sums[1:]:
            total = total + s                                       # left to right, in fp64 (Python floats)
        assert _bits(res["loss_sum"]) == _bits(total), (ld, res["loss_sum"], total)
        assert res["count"] == sum(counted) and res["invalid"] == sum(invalid)
        assert _bits(res["loss"]) == _bits(np.float64(total) / np.float64(res["count"]))
        if N > 1:
            assert res["image_count"][1] == 0 and np.isnan(res["image_loss"][1]) and res["image_loss_sum"][1] == 0.0
        # labels alone (no ground truth): the same labels; and the call is reproducible bit for bit
        labels2 = torch.full_like(labels, 98)
        seg_head.full_res_eval(xd, H, W, labels_out=labels2)
        assert _same_bits(labels, labels2)
        seg_head.full_res_eval(xd, H, W, gt=gtd, workspace=ws)
        again = ws.result()
        assert _bits(again["loss_sum"]) == _bits(res["loss_sum"]) and _bits(again["image_loss_sum"]) == _bits(res["image_loss_sum"])
        # every label of the batch 255: no pixel counts, the mean is NaN as torch's
        seg_head.full_res_eval(xd, H, W, gt=torch.full_like(gtd, 255), workspace=ws)
        none = ws.result()
        assert none["count"] == 0 and none["invalid"] == 0 and np.isnan(none["loss"]) and none["loss_sum"] == 0.0
        assert all(np.isnan(v) for v in none["image_loss"]) and none["image_count"] == [0] * N


def _near_tie(up, rel=4e-6):
    top2 = torch.topk(up, 2, dim=0).values
    return (top2[0] - top2[1]) <= rel * float(up.abs().max())


@pytest.mark.parametrize("shape,N,K", CASES, ids=IDS)
def test_batched_eval_matches_torch(shape, N, K, cuda_device):
    """F.interpolate(align_corners=True) -> argmax and cross_entropy(ignore_index=255) in float64 on the CPU, image by image (the batch
    mean is the sum of every counted pixel's term over their number); labels as tests/test_gpu_full_res.py compares them (equal away
    from near-ties), the loss within that file's 1e-5 of the float64 value"""
    from vision_semantic_segmentation_amd import seg_head
    (h, w), (H, W) = shape
    x, gt = _case(shape, N, K, invalid=False)
    xd = _dev(x, cuda_device, K, h * w)
    gtd = torch.from_numpy(gt).to(cuda_device)
    labels = torch.empty((N, H, W), dtype=torch.uint8, device=cuda_device)
    cm = torch.zeros((K, K), dtype=torch.int64, device=cuda_device)
    ws = seg_head.EvalWorkspace(H, W, cuda_device, batch=N)
    seg_head.full_res_eval(xd, H, W, gt=gtd, labels_out=labels, confusion=cm, workspace=ws)
    res = ws.result()
    got = labels.cpu().long()
    ref_sum, ref_count = 0.0, 0
    cm_ref = np.zeros((K, K), dtype=np.int64)
    for i in range(N):
        up = F.interpolate(x[i][None], size=(H, W), mode="bilinear", align_corners=True)[0]
        diff = got[i] != up.argmax(0)
        assert not bool((diff & ~_near_tie(up)).any()), "image %d: %d labels differ away from near-ties" % (i, int((diff & ~_near_tie(up)).sum()))
        g = torch.from_numpy(gt[i].astype(np.int64))
        ref_sum += F.cross_entropy(up[None].double(), g[None], ignore_index=255, reduction="sum").item()
        ref_count += int((g != 255).sum())
        mask = gt[i] < K
        cm_ref += np.bincount(K * gt[i][mask].astype(np.int64) + got[i].numpy()[mask], minlength=K * K).reshape(K, K)
    ref = ref_sum / ref_count
    print("%s N %d K %d: loss %.12g torch fp64 %.12g rel %.2e" % (shape, N, K, res["loss"], ref, abs(res["loss"] - ref) / abs(ref)))
    assert res["count"] == ref_count and res["invalid"] == 0
    assert abs(res["loss"] - ref) <= 1e-5 * abs(ref), (res["loss"], ref)
    assert np.array_equal(cm.cpu().numpy(), cm_ref)                # MeanIOU's bincount of the kernel's own labels


def test_the_batch_mean_is_over_pixels_not_over_images(cuda_device):
    """torch's reduction='mean' on the whole batch tensor, with images that count very different numbers of pixels"""
    from vision_semantic_segmentation_amd import seg_head
    shape, N, K = ((29, 37), (131, 163)), 3, 19
    (h, w), (H, W) = shape
    x, gt = _case(shape, N, K, invalid=False)
    gt[1] = gt[0][::-1]                                            # image 1 counts again
    gt[2, 5:] = 255                                                # image 2 counts five rows only
    up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True).double()
    ref = F.cross_entropy(up, torch.from_numpy(gt.astype(np.int64)), ignore_index=255).item()
    ws = seg_head.EvalWorkspace(H, W, cuda_device, batch=N)
    seg_head.full_res_eval(_dev(x, cuda_device, K, h * w), H, W, gt=torch.from_numpy(gt).to(cuda_device), workspace=ws)
    res = ws.result()
    assert abs(res["loss"] - ref) <= 1e-5 * abs(ref), (res["loss"], ref)
    mean_of_means = float(np.mean(res["image_loss"]))
    assert abs(mean_of_means - ref) > 1e-4 * abs(ref)              # the other definition is measurably different here


@pytest.mark.parametrize("shape,N,K", CASES, ids=IDS)
def test_batched_upsample_equals_the_single_image_entry_point_bit_for_bit(shape, N, K, cuda_device):
    from vision_semantic_segmentation_amd import seg_head
    (h, w), (H, W) = shape
    x, _ = _case(shape, N, K, invalid=False)
    for ld, image_rows in ((K, h * w), (K + 3, h * w + 5)):
        xd = _dev(x, cuda_device, ld, image_rows)
        out = seg_head.upsample_logits(xd, H, W)
        assert tuple(out.shape) == (N, K, H, W) and out.dtype == torch.float32
        for i in range(N):
            assert _same_bits(out[i], _single_upsample(xd[i], H, W)), (ld, i)
        del out
    if K == 5 and N == 2:                                          # against torch, as the single-image test does
        ref = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
        err = float((seg_head.upsample_logits(xd, H, W).cpu() - ref).abs().max())
        assert err <= 1e-6 * float(x.abs().max()), err


# ---------------------------------------------------------------------------------------------------------------- end to end

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
E2E_SIZES = [(96, 128), (100, 130)]


def _cfg(precision):
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_network_cfg_defaults()
    cfg.MODEL.PRECISION = precision
    cfg.MODEL.MIXED_SELF_CHECK = False
    cfg.MODEL.VALIDATE_BATCH = True          # validate_step takes [N, h, w, 3] (off by default: test_validate_step_refuses_a_batch_by_default)
    return cfg


_SEGS = {}


def _seg(precision, device):
    from _full_size import state_dict
    from vision_semantic_segmentation_amd import SemanticSegmentation
    if precision not in _SEGS:
        _SEGS[precision] = SemanticSegmentation(_cfg(precision), device=device, state_dict=state_dict(0))
    return _SEGS[precision]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _SEGS.clear()
    torch.cuda.empty_cache()


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _to_x(frames_u8):
    x = (frames_u8.astype(np.float32) / np.float32(255) - MEAN) / STD
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


def _labels_for(n, h, w, K, seed):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, K, size=(n, h, w)).astype(np.int64)
    gt[rng.random((n, h, w)) < 0.1] = 255
    return gt


@pytest.mark.parametrize("hw", E2E_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("precision", ["mixed", "f32"])
def test_validate_step_on_a_batch_against_single_images(precision, hw, cuda_device):
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    seg = _seg(precision, cuda_device)
    (h, w), N, K = hw, 3, seg.num_classes
    frames, gt = _frames(N, h, w, seed=h), _labels_for(N, h, w, K, seed=w)
    sums, counts = [], []
    single = MeanIOU(K, device=cuda_device)
    for i in range(N):
        seg.validate_step(frames[i], gt[i], single)
        r = seg._full_res(h, w).workspace.result()
        sums.append(r["loss_sum"])
        counts.append(r["count"])
    batched = MeanIOU(K, device=cuda_device)
    loss = seg.validate_step(frames, gt, batched)
    assert torch.equal(batched.confusion_matrix, single.confusion_matrix) and int(batched.confusion_matrix.sum()) == sum(counts) > 0
    expected = ((sums[0] + sums[1]) + sums[2]) / sum(counts)
    assert _bits(loss) == _bits(expected), (loss, expected)
    r = seg._full_res(h, w, N).workspace.result()
    assert _bits(r["image_loss_sum"]) == _bits(sums) and r["image_count"] == counts
    # tensors on the device and uint8 labels give the same; [1, h, w, 3] is a batch of one
    loss_dev = seg.validate_step(torch.from_numpy(frames).to(cuda_device), torch.from_numpy(gt.astype(np.uint8)).to(cuda_device), batched)
    assert _bits(loss_dev) == _bits(loss) and torch.equal(batched.confusion_matrix, 2 * single.confusion_matrix)
    one = seg.validate_step(frames[:1], gt[:1])
    assert _bits(one) == _bits(sums[0] / counts[0])
    assert (h, w, N) in seg._nets                                  # one forward of the batch-N plan
    assert np.isnan(seg.validate_step(frames, np.full((N, h, w), 255, dtype=np.uint8)))


def test_an_invalid_label_in_one_image_raises_and_leaves_the_metric(cuda_device):
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    seg = _seg("mixed", cuda_device)
    (h, w), N, K = E2E_SIZES[0], 3, seg.num_classes
    frames, gt = _frames(N, h, w, seed=5), _labels_for(N, h, w, K, seed=6)
    metric = MeanIOU(K, device=cuda_device)
    seg.validate_step(frames, gt, metric)
    before = metric.confusion_matrix.clone()
    for bad_value in (K, 254, -1, 300):
        bad = gt.copy()
        bad[1, 10, 10] = bad_value                                 # image 2 of 3
        with pytest.raises(ValueError, match="outside"):
            seg.validate_step(frames, bad, metric)
        assert torch.equal(metric.confusion_matrix, before)
    with pytest.raises(ValueError, match="label has shape"):
        seg.validate_step(frames, gt[:2], metric)
    with pytest.raises(ValueError, match="must hold integers"):
        seg.validate_step(frames, gt.astype(np.float32), metric)
    assert torch.equal(metric.confusion_matrix, before)


def test_validate_step_refuses_a_batch_by_default(cuda_device):
    """MODEL.VALIDATE_BATCH is off unless asked for: validate_step keeps refusing anything but one image, before any plan is built"""
    from _full_size import state_dict
    from vision_semantic_segmentation_amd import SemanticSegmentation
    cfg = _cfg("mixed")
    cfg.MODEL.VALIDATE_BATCH = False
    seg = SemanticSegmentation(cfg, device=cuda_device, state_dict=state_dict(0))
    (h, w), N = E2E_SIZES[0], 3
    frames, gt = _frames(N, h, w, seed=5), _labels_for(N, h, w, seg.num_classes, seed=6)
    for n in (N, 1):
        with pytest.raises(NotImplementedError, match="VALIDATE_BATCH"):
            seg.validate_step(frames[:n], gt[:n])
    assert not seg._nets
    assert np.isfinite(seg.validate_step(frames[0], gt[0]))


@pytest.mark.parametrize("precision", ["mixed", "f32"])
def test_full_resolution_outputs_of_a_batch_are_the_per_image_kernels(precision, cuda_device):
    seg = _seg(precision, cuda_device)
    (h, w), N = E2E_SIZES[1], 3
    frames = _frames(N, h, w, seed=17)
    labels = seg.segmentation_device(frames, upsample_pred=True)
    net = seg.net_for(h, w, batch=N)
    assert tuple(labels.shape) == (N, h, w) and labels.dtype == torch.uint8
    for i in range(N):
        assert _same_bits(labels[i], _single_labels(net.logits[i], h, w)), i
    up = seg.logits(frames, upsample_pred=True)
    assert tuple(up.shape) == (N, seg.num_classes, h, w)
    for i in range(N):
        assert _same_bits(up[i], _single_upsample(net.logits[i], h, w)), i
    x = _to_x(frames).to(cuda_device)
    out = seg.forward_tensor(x, upsample_pred=True)
    fnet = seg.net_for(h, w, batch=N, input_format="f32_nchw")
    assert tuple(out.shape) == (N, seg.num_classes, h, w) and out.data_ptr() != up.data_ptr()
    for i in range(N):
        assert _same_bits(out[i], _single_upsample(fnet.logits[i], h, w)), i
    one = seg.forward_tensor(x[:1], upsample_pred=True)            # a batch of one, and the unbatched form
    assert _same_bits(one[0], seg.forward_tensor(x[0], upsample_pred=True))


def test_drop_in_validate_step_against_the_reference_route(cuda_device):
    from vision_semantic_segmentation_amd import build_model
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    cfg = _cfg("mixed")
    net, loss_fn, _, val_metric = build_model(cfg)
    model = net.to(cuda_device).eval()
    assert getattr(loss_fn, "ignore_index", None) == 255
    K, N = cfg.DATASET.NUM_CLASSES, 3
    fused = MeanIOU(K, device=cuda_device)
    for (h, w), seed in zip(E2E_SIZES, (61, 62)):
        x = _to_x(_frames(N, h, w, seed=seed)).to(cuda_device)
        label = torch.from_numpy(_labels_for(N, h, w, K, seed=seed + 10)).to(cuda_device)
        with torch.no_grad():
            preds = model(x)
            ref_loss = float(loss_fn(preds, label))
        val_metric.evaluate(preds, label)
        loss = model.validate_step(x, label, fused)
        assert isinstance(loss, float)
        assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
        assert torch.equal(val_metric.confusion_matrix, fused.confusion_matrix)
    assert int(fused.confusion_matrix.sum()) > 0
    # a CPU batch and CPU labels are copied to the device; an invalid label raises and leaves the metric
    before = fused.confusion_matrix.clone()
    assert _bits(model.validate_step(x.cpu(), label.cpu())) == _bits(loss)
    bad = label.clone()
    bad[1, 3, 4] = K
    with pytest.raises(ValueError, match="outside"):
        model.validate_step(x, bad, fused)
    assert torch.equal(fused.confusion_matrix, before)
    model.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        model.validate_step(x, label, fused)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(x)
