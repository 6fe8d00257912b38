"""Full-resolution validation without a GPU: metrics.MeanIOU against the reference's formula (models/metrics.py:70-80), its reset /
accumulation / two-rank gloo reduction, the reference-generated fixture's mIoU, and the argument checks of the two new entry points
(avl_upsample_logits, avl_seg_eval_full_res), which return before anything touches a GPU."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def reference_miou(cm):
    """models/metrics.py:70-80, restated"""
    cm = np.asarray(cm, dtype=np.float64)
    inter = np.diag(cm)
    union = cm.sum(axis=0) + cm.sum(axis=1) - inter
    iou = np.divide(inter, union, out=np.full(union.shape, np.nan), where=(union != 0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # nanmean of an all-NaN vector
        return float(np.nanmean(iou))


def test_mean_iou_matches_the_reference_formula_with_an_empty_union_class():
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    m = MeanIOU(4, device="cpu")
    cm = np.array([[5, 1, 0, 0],
                   [2, 7, 0, 1],
                   [0, 0, 0, 0],          # class 2: never in the ground truth, never predicted -> NaN, left out of the mean
                   [0, 3, 0, 4]], dtype=np.int64)
    m.add_confusion(torch.from_numpy(cm))
    iou = m.iou()
    assert np.isnan(iou[2]) and not np.isnan(iou[[0, 1, 3]]).any()
    assert iou[0] == 5 / (7 + 6 - 5) and iou[1] == 7 / (11 + 10 - 7) and iou[3] == 4 / (5 + 7 - 4)
    assert m.global_avg == reference_miou(cm) == pytest.approx(np.mean(iou[[0, 1, 3]]), abs=0)
    assert str(m) == "{:.4f}".format(reference_miou(cm)) == m.summary_str
    assert m.confusion_matrix.dtype == torch.int64
    empty = MeanIOU(3, device="cpu")
    assert np.isnan(empty.global_avg)                          # every union empty: nanmean of nothing


def test_mean_iou_evaluate_reset_and_accumulation():
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    K = 5
    rng = np.random.default_rng(3)
    m = MeanIOU(K, device="cpu")
    total = np.zeros((K, K), dtype=np.int64)
    for _ in range(3):
        preds = torch.from_numpy(rng.normal(size=(2, K, 7, 9)).astype(np.float32))
        labels = rng.integers(0, K, size=(2, 7, 9))
        labels[:, 0, :3] = 255
        labels[1, 3, 3] = K + 2
        labels = torch.from_numpy(labels)
        m.evaluate(preds, labels)
        p = preds.argmax(1).numpy()
        lab = labels.numpy()
        mask = (lab >= 0) & (lab < K)
        total += np.bincount(K * lab[mask] + p[mask], minlength=K * K).reshape(K, K)       # metrics.py:52-55
        assert np.array_equal(m.confusion_matrix.numpy(), total)
    assert m.global_avg == reference_miou(total)
    m.reset()
    assert int(m.confusion_matrix.abs().sum()) == 0
    m.synchronize_between_processes()                        # no process group: nothing happens
    assert int(m.confusion_matrix.abs().sum()) == 0


def test_fixture_miou_equals_global_avg_of_its_matrix(golden_dir):
    from vision_semantic_segmentation_amd.metrics import MeanIOU
    z = np.load(os.path.join(golden_dir, "full_res_eval.npz"))
    cm = z["confusion"]
    assert cm.shape == (19, 19) and cm.sum() > 0
    m = MeanIOU(19, device="cpu")
    m.add_confusion(torch.from_numpy(cm))
    assert m.global_avg == float(z["miou"])
    # the fixture's matrix is the reference's bincount over both frames' stored labels (pixels with gt < 19)
    exp = np.zeros((19, 19), dtype=np.int64)
    for f in range(2):
        gt, lab = z["gt_%d" % f].astype(np.int64), z["labels_%d" % f].astype(np.int64)
        mask = gt < 19
        exp += np.bincount(19 * gt[mask] + lab[mask], minlength=361).reshape(19, 19)
        assert int(((gt >= 19) & (gt != 255)).sum()) == int(z["invalid_%d" % f]) > 0
        assert (gt == 255).any()
    assert np.array_equal(exp, cm)


def _sync_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from vision_semantic_segmentation_amd.metrics import MeanIOU
        m = MeanIOU(3, device="cpu")
        m.add_confusion(torch.arange(9, dtype=torch.int64).reshape(3, 3) * (rank + 1))
        m.synchronize_between_processes()
        q.put(("ok", rank, m.confusion_matrix.numpy().tolist(), m.global_avg))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put(("error", rank, traceback.format_exc(limit=3), None))
        raise


def test_two_rank_gloo_synchronize_sums_the_matrices():
    import queue
    import socket
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sock:            # a free port
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(2):
            status, rank, payload, miou = q.get(timeout=240)
            if status != "ok":
                pytest.fail(payload)
            results[rank] = (payload, miou)
    except queue.Empty:
        pytest.fail("no result within 240 s (exit codes %r)" % [p.exitcode for p in procs])
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.terminate()
    expected = (np.arange(9).reshape(3, 3) * 3).tolist()
    assert results[0][0] == expected and results[1][0] == expected
    assert results[0][1] == results[1][1] == reference_miou(expected)
    assert all(p.exitcode == 0 for p in procs)


def test_new_entry_points_return_argument_errors_without_a_gpu():
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    host = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(host))                      # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(C.addressof(host) + 2)
    rc = L.avl_upsample_logits(None, 34, 60, 19, 19, p, 152, 256, None)
    assert rc == -1 and "logits is NULL" in _lib.last_error()
    rc = L.avl_upsample_logits(p, 34, 60, 19, 19, None, 152, 256, None)
    assert rc == -1 and "out is NULL" in _lib.last_error()
    rc = L.avl_upsample_logits(p, 34, 60, 19, 18, p, 152, 256, None)
    assert rc == -1 and "row stride" in _lib.last_error()
    rc = L.avl_upsample_logits(p, 0, 60, 19, 19, p, 152, 256, None)
    assert rc == -1 and "sizes" in _lib.last_error()
    rc = L.avl_upsample_logits(p, 34, 60, 19, 19, odd, 152, 256, None)
    assert rc == -1 and "aligned" in _lib.last_error()
    rc = L.avl_upsample_logits(p, 34, 60, 300, 300, p, 152, 256, None)
    assert rc == -3 and "256" in _lib.last_error()

    def ev(logits=p, K=19, ld=19, gt=p, labels=p, cm=p, loss=p, counts=p, scratch=p, H=152):
        return L.avl_seg_eval_full_res(logits, 34, 60, K, ld, H, 256, gt, 255, labels, cm, loss, counts, scratch, None), _lib.last_error()

    rc, msg = ev(K=65, ld=65)
    assert rc == -3 and "65" in msg and "64" in msg
    rc, msg = ev(logits=None)
    assert rc == -1 and "logits is NULL" in msg
    rc, msg = ev(H=-1)
    assert rc == -1 and "sizes" in msg
    rc, msg = ev(counts=None)
    assert rc == -1 and "go together" in msg
    rc, msg = ev(labels=None, cm=None, loss=None, counts=None, scratch=None)
    assert rc == -1 and "nothing to compute" in msg
    rc, msg = ev(gt=None)
    assert rc == -1 and "ground truth" in msg
    rc, msg = ev(cm=odd)
    assert rc == -1 and "confusion is not 8-byte aligned" in msg
    rc, msg = ev(scratch=odd)
    assert rc == -1 and "8-byte aligned" in msg
    assert L.avl_seg_eval_scratch_bytes(1080, 1920) == 68 * 30 * 16
    assert L.avl_seg_eval_scratch_bytes(0, 1920) == -1


def test_python_wrappers_refuse_host_tensors():
    from vision_semantic_segmentation_amd import seg_head
    x = torch.zeros((4, 5, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="CUDA"):
        seg_head.upsample_logits(x, 8, 10)
    with pytest.raises(ValueError, match="CUDA"):
        seg_head.full_res_eval(x, 8, 10)
