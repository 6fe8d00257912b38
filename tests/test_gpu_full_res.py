"""Full-resolution predictions and validation on the GPU (csrc/seg_head.hip through avl_upsample_logits / avl_seg_eval_full_res):
the reference's DeepLabV3Plus.forward(x, upsample_pred=True) (deeplab_v3_plus.py:67-69: F.interpolate(..., mode='bilinear',
align_corners=True)), torch.argmax, MeanIOU's confusion matrix (models/metrics.py:29-59) and CrossEntropyLoss(ignore_index=255)
(models/loss.py, models/build.py:20), against torch CPU and the reference-generated fixture tests/golden/full_res_eval.npz."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [((266, 476), (1080, 1920)), ((1, 1), (20, 20)), ((2, 100), (20, 1000)), ((37, 53), (149, 211)),
          ((200, 300), (21, 31))]                     # the last one shrinks: its windows do not fit in LDS (the global-read path)
CLASSES = [5, 19, 33, 64]


def _logits(rng, K, h, w):
    return torch.from_numpy((4.0 * rng.standard_normal((K, h, w))).astype(np.float32))


def _dev(x_khw, device, ld=None):
    """[K, h, w] CPU -> the plan's layout on the device: NHWC [h, w, K] rows of stride ld (>= K)"""
    K, h, w = x_khw.shape
    ld = K if ld is None else ld
    buf = torch.full((h * w, ld), float("nan"), dtype=torch.float32, device=device)
    buf[:, :K] = x_khw.permute(1, 2, 0).reshape(h * w, K).to(device)
    return buf.as_strided((h, w, K), (w * ld, ld, 1))


def _up(x_khw, H, W):
    return F.interpolate(x_khw[None], size=(H, W), mode="bilinear", align_corners=True)[0]


def _near_tie(up, rel=4e-6):
    top2 = torch.topk(up, 2, dim=0).values
    return (top2[0] - top2[1]) <= rel * float(up.abs().max())


def _bincount(gt, pred, K):
    """models/metrics.py:52-55, restated"""
    gt, pred = gt.astype(np.int64), pred.astype(np.int64)
    mask = (gt >= 0) & (gt < K)
    return np.bincount(K * gt[mask] + pred[mask], minlength=K * K).reshape(K, K)


def _gt(rng, H, W, K, ignore_frac=0.1):
    gt = rng.integers(0, K, size=(H, W)).astype(np.uint8)
    gt[rng.random((H, W)) < ignore_frac] = 255
    return gt


@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_upsample_matches_torch(shape, K, cuda_device):
    from vision_semantic_segmentation_amd import seg_head
    (h, w), (H, W) = shape
    rng = np.random.default_rng(K * 1000 + h)
    x = _logits(rng, K, h, w)
    ref = _up(x, H, W)
    for ld in (K, K + 3):
        got = seg_head.upsample_logits(_dev(x, cuda_device, ld), H, W).cpu()
        assert got.shape == (K, H, W)
        err = float((got - ref).abs().max())
        assert err <= 1e-6 * float(x.abs().max()), "max|d| %g (ld %d)" % (err, ld)


@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_labels_equal_argmax_of_the_upsampled_logits(shape, K, cuda_device):
    from vision_semantic_segmentation_amd import seg_head
    (h, w), (H, W) = shape
    rng = np.random.default_rng(K * 7 + w)
    x = _logits(rng, K, h, w)
    ref = _up(x, H, W)
    lab = torch.empty((H, W), dtype=torch.uint8, device=cuda_device)
    seg_head.full_res_eval(_dev(x, cuda_device), H, W, labels_out=lab)
    got = lab.cpu().long()
    diff = got != ref.argmax(0)
    assert not bool((diff & ~_near_tie(ref)).any()), "%d labels differ away from near-ties" % int((diff & ~_near_tie(ref)).sum())


def test_labels_forced_ties_and_nan(cuda_device):
    """AVL_OP_ARGMAX's rule: the first maximal index wins, a NaN counts as maximal (the first NaN)"""
    from vision_semantic_segmentation_amd import seg_head
    K, h, w, H, W = 19, 9, 13, 40, 61
    rng = np.random.default_rng(5)
    x = _logits(rng, K, h, w)
    x[2] = x.max(0).values + 1.0
    x[5] = x[2]                                    # classes 2 and 5 tie everywhere: 2 wins
    x[7, 4, 6] = float("nan")                      # every output pixel that reads this source pixel: 7
    x[11, 0, 0] = float("nan")
    x[3, 0, 0] = float("nan")                      # at (0, 0) the first NaN is class 3
    ref = _up(x, H, W)
    lab = torch.empty((H, W), dtype=torch.uint8, device=cuda_device)
    seg_head.full_res_eval(_dev(x, cuda_device), H, W, labels_out=lab)
    got = lab.cpu().long()
    nan = torch.isnan(ref)
    expected = torch.where(nan.any(0), nan.float().argmax(0), torch.full_like(got, 2))
    assert nan[7].any() and nan[3].any() and bool((got == 7).any()) and bool((got == 3).any())
    assert torch.equal(got, expected)
    assert torch.equal(got, ref.argmax(0))          # torch.argmax follows the same rule


def test_confusion_matrix_accumulates_exactly(cuda_device):
    from vision_semantic_segmentation_amd import seg_head
    K, h, w, H, W = 19, 34, 60, 300, 517
    rng = np.random.default_rng(11)
    cm = torch.zeros((K, K), dtype=torch.int64, device=cuda_device)
    lab = torch.empty((H, W), dtype=torch.uint8, device=cuda_device)
    total = np.zeros((K, K), dtype=np.int64)
    counted = 0
    for call in range(3):
        x = _logits(rng, K, h, w)
        gt = _gt(rng, H, W, K)
        gt.reshape(-1)[rng.choice(H * W, 50, replace=False)] = rng.integers(K, 255, size=50)   # skipped by MeanIOU's mask
        seg_head.full_res_eval(_dev(x, cuda_device), H, W, gt=torch.from_numpy(gt).to(cuda_device), labels_out=lab, confusion=cm)
        total += _bincount(gt, lab.cpu().numpy(), K)
        counted += int((gt < K).sum())
        assert np.array_equal(cm.cpu().numpy(), total), "call %d" % call
    assert total.sum() == counted


def test_loss_matches_torch_fp64_and_is_reproducible(cuda_device):
    from vision_semantic_segmentation_amd import seg_head
    K, h, w, H, W = 19, 67, 119, 266, 476
    rng = np.random.default_rng(21)
    x = _logits(rng, K, h, w)
    gt = _gt(rng, H, W, K, ignore_frac=0.2)
    ref = F.cross_entropy(_up(x, H, W)[None].double(), torch.from_numpy(gt.astype(np.int64))[None], ignore_index=255).item()
    xd, gtd = _dev(x, cuda_device), torch.from_numpy(gt).to(cuda_device)
    ws = seg_head.EvalWorkspace(H, W, cuda_device)
    seg_head.full_res_eval(xd, H, W, gt=gtd, workspace=ws)
    r1 = ws.result()
    assert r1["count"] == int((gt != 255).sum()) and r1["invalid"] == 0
    assert abs(r1["loss"] - ref) <= 1e-5 * abs(ref), (r1["loss"], ref)
    seg_head.full_res_eval(xd, H, W, gt=gtd, workspace=ws, labels_out=torch.empty((H, W), dtype=torch.uint8, device=cuda_device),
                           confusion=torch.zeros((K, K), dtype=torch.int64, device=cuda_device))
    r2 = ws.result()
    assert np.float64(r1["loss"]).tobytes() == np.float64(r2["loss"]).tobytes()
    assert np.float64(r1["loss_sum"]).tobytes() == np.float64(r2["loss_sum"]).tobytes()
    # every label 255: no pixel contributes, the mean is NaN as torch's
    all_ign = torch.full((H, W), 255, dtype=torch.uint8, device=cuda_device)
    seg_head.full_res_eval(xd, H, W, gt=all_ign, workspace=ws)
    r3 = ws.result()
    t = F.cross_entropy(_up(x, H, W)[None].double(), torch.full((1, H, W), 255, dtype=torch.int64), ignore_index=255).item()
    assert np.isnan(t) and np.isnan(r3["loss"]) and r3["count"] == 0 and r3["invalid"] == 0
    # invalid labels are counted (torch raises on them) and skipped
    bad = gt.copy()
    bad[3, 4], bad[100, 200] = 19, 200
    seg_head.full_res_eval(xd, H, W, gt=torch.from_numpy(bad).to(cuda_device), workspace=ws)
    r4 = ws.result()
    assert r4["invalid"] == 2
    with pytest.raises((IndexError, RuntimeError)):
        F.cross_entropy(_up(x, H, W)[None], torch.from_numpy(bad.astype(np.int64))[None], ignore_index=255)


def test_golden_fixture_reproduces(golden_dir, cuda_device):
    from vision_semantic_segmentation_amd import seg_head
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    z = np.load(os.path.join(golden_dir, "full_res_eval.npz"))
    K, H, W = 19, 152, 256
    metric = MeanIOU(K, device=cuda_device)
    ws = seg_head.EvalWorkspace(H, W, cuda_device)
    lab = torch.empty((H, W), dtype=torch.uint8, device=cuda_device)
    cm_adjust = np.zeros((K, K), dtype=np.int64)
    for f in range(2):
        x = torch.from_numpy(z["logits_%d" % f])
        gt = z["gt_%d" % f]
        seg_head.full_res_eval(_dev(x, cuda_device), H, W, gt=torch.from_numpy(gt).to(cuda_device), labels_out=lab,
                               confusion=metric.confusion_matrix, workspace=ws)
        r = ws.result()
        got, exp = lab.cpu().numpy(), z["labels_%d" % f]
        diff = got != exp
        assert not (diff & ~z["near_tie_%d" % f]).any()
        m = diff & (gt < K)
        cm_adjust += _bincount(gt[m], got[m], K) - _bincount(gt[m], exp[m], K)
        assert r["invalid"] == int(z["invalid_%d" % f])
        assert abs(r["loss"] - float(z["loss_%d" % f])) <= 1e-5 * abs(float(z["loss_%d" % f]))
    assert np.array_equal(metric.confusion_matrix.cpu().numpy(), z["confusion"] + cm_adjust)
    if not cm_adjust.any():
        assert metric.global_avg == float(z["miou"])


@pytest.fixture(scope="module")
def seg480(cuda_device):
    from _full_size import state_dict
    from vision_semantic_segmentation_amd import SemanticSegmentation
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    return SemanticSegmentation(get_network_cfg_defaults(), device=cuda_device, state_dict=state_dict(0))


def test_end_to_end_480x640(seg480, cuda_device):
    """the default plan ("mixed"): upsampled logits within the plan's 1e-3 bound of the oracle's logits upsampled by torch; full-size
    labels; validate_step + MeanIOU against the bincount restatement and torch's fp64 cross-entropy"""
    from _full_size import image_for, oracle_logits
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    H, W, K = 480, 640, 19
    img = image_for(3, H, W)
    up_ref = _up(oracle_logits(0, 3, H, W), H, W)
    up = seg480.logits(img, upsample_pred=True)
    assert up.shape == (K, H, W) and up.dtype == torch.float32 and up.is_cuda
    up = up.cpu()
    rel = float((up - up_ref).abs().max() / up_ref.abs().max())
    print("480x640 upsampled logits: max rel err %.3e against the oracle" % rel)
    assert rel <= 1e-3
    labels = seg480.segmentation(img, upsample_pred=True)
    assert labels.shape == (480, 640) and labels.dtype == np.int64
    diff = torch.from_numpy(labels) != up.argmax(0)
    assert not bool((diff & ~_near_tie(up)).any())

    rng = np.random.default_rng(8)
    gt = np.where(rng.random((H, W)) < 0.6, labels, rng.integers(0, K, size=(H, W)))
    gt[rng.random((H, W)) < 0.05] = 255
    metric = MeanIOU(K, device=cuda_device)
    loss = seg480.validate_step(img, gt.astype(np.int64), metric)
    cm = _bincount(gt, labels, K)
    assert np.array_equal(metric.confusion_matrix.cpu().numpy(), cm)
    ref = F.cross_entropy(up[None].double(), torch.from_numpy(gt.astype(np.int64))[None], ignore_index=255).item()
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)
    loss_u8 = seg480.validate_step(img, torch.from_numpy(gt.astype(np.uint8)).to(cuda_device), metric)
    assert loss_u8 == loss
    assert np.array_equal(metric.confusion_matrix.cpu().numpy(), 2 * cm)
    ref_metric = MeanIOU(K, device="cpu")
    ref_metric.add_confusion(torch.from_numpy(2 * cm))
    assert metric.global_avg == ref_metric.global_avg
    # invalid labels raise and leave the metric as it was
    for bad_value in (19, 254, -1, 300):
        bad = gt.astype(np.int64).copy()
        bad[10, 10] = bad_value
        with pytest.raises(ValueError, match="outside"):
            seg480.validate_step(img, bad, metric)
    assert np.array_equal(metric.confusion_matrix.cpu().numpy(), 2 * cm)
    # all 255: NaN, as torch
    assert np.isnan(seg480.validate_step(img, np.full((H, W), 255, dtype=np.uint8)))


def test_defaults_unchanged(seg480, cuda_device):
    """no upsample_pred argument: the network-resolution outputs of before, byte for byte, whatever ran in between"""
    from _full_size import image_for
    H, W = 480, 640
    img = image_for(4, H, W)
    lg = seg480.logits(img).clone()
    lab = seg480.segmentation(img)
    lab_dev = seg480.segmentation_device(img).clone()
    assert lg.shape == (19, H // 4 - 4, W // 4 - 4) and lab.shape == (H // 4 - 4, W // 4 - 4)
    seg480.logits(img, upsample_pred=True)
    seg480.segmentation(img, upsample_pred=True)
    seg480.validate_step(img, np.zeros((H, W), dtype=np.uint8))
    assert torch.equal(seg480.logits(img), lg)
    assert np.array_equal(seg480.segmentation(img), lab)
    assert torch.equal(seg480.segmentation_device(img), lab_dev)
    # the same plan built directly (no SemanticSegmentation in between) writes the same bytes
    net = seg480._build(H, W, seg480._rung)
    net.forward(img)
    torch.cuda.synchronize()
    assert torch.equal(net.logits.permute(2, 0, 1), lg)
    assert torch.equal(net.labels, lab_dev)
