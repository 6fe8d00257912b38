"""Full-resolution predictions and validation terms from a plan's logits (csrc/seg_head.hip, include/avl_hip.h):
DeepLabV3Plus.forward(x, upsample_pred=True) (deeplab_v3_plus.py:51,67-69) and the validation step of train.py:138-141.

    upsample_logits(net.logits, H, W)                  # fp32 [K, H, W]: F.interpolate(..., align_corners=True)
    full_res_eval(net.logits, H, W, gt=gt_u8, labels_out=lab, confusion=cm, workspace=ws)   # fused arg-max / confusion / loss

`logits` is the plan's fp32 NHWC map [h, w, K] (SegNet.logits; a row stride ld >= K is allowed).  Everything is launched on the
current stream of the logits' device; nothing here synchronises except EvalWorkspace.result().
"""
import ctypes as C

import torch

from . import _lib

IGNORE_INDEX = 255          # CrossEntropyLoss(ignore_index=255) of models/build.py:20
MAX_EVAL_CLASSES = 64       # the fused kernel's limit (K x K LDS histogram, uint8 labels)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _nhwc(logits):
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3):
        raise ValueError("logits must be a float32 CUDA tensor [h, w, K]")
    h, w, K = logits.shape
    ld = logits.stride(1)
    if logits.stride(2) != 1 or (h > 1 and logits.stride(0) != w * ld):
        raise ValueError("logits must be NHWC rows of stride ld >= K (strides %s)" % (logits.stride(),))
    return int(h), int(w), int(K), int(ld)


def upsample_logits(logits, H, W, out=None):
    """fp32 [h, w, K] -> fp32 [K, H, W] (`out`, or a new tensor), bilinear with align_corners=True."""
    h, w, K, ld = _nhwc(logits)
    if out is None:
        out = torch.empty((K, H, W), dtype=torch.float32, device=logits.device)
    if tuple(out.shape) != (K, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != logits.device:
        raise ValueError("out must be a contiguous float32 tensor [%d, %d, %d] on %s" % (K, H, W, logits.device))
    _lib.check(_lib.lib().avl_upsample_logits(_ptr(logits), h, w, K, ld, _ptr(out), int(H), int(W), _stream(logits.device)),
               "avl_upsample_logits")
    return out


class EvalWorkspace(object):
    """The loss outputs of full_res_eval for an H x W output: loss = fp64 {sum, mean}, counts = {contributing pixels, invalid labels}."""

    def __init__(self, H, W, device):
        self.size = (int(H), int(W))
        nbytes = _lib.lib().avl_seg_eval_scratch_bytes(int(H), int(W))
        if nbytes < 0:
            raise RuntimeError("avl_seg_eval_scratch_bytes failed: %s" % _lib.last_error())
        self.scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        self.loss = torch.empty(2, dtype=torch.float64, device=device)
        self.counts = torch.empty(2, dtype=torch.int64, device=device)

    def result(self):
        """(synchronises) {"loss_sum", "loss" (NaN when no pixel counted), "count", "invalid"} of the last call"""
        loss, counts = self.loss.cpu().tolist(), self.counts.cpu().tolist()
        return {"loss_sum": loss[0], "loss": loss[1], "count": counts[0], "invalid": counts[1]}


def full_res_eval(logits, H, W, gt=None, labels_out=None, confusion=None, workspace=None, ignore_index=IGNORE_INDEX):
    """One fused pass over the H x W output: labels_out uint8 [H, W] (arg-max), confusion int64 [K, K] (+= MeanIOU's counts of the
    pixels with gt < K), workspace (EvalWorkspace: cross-entropy terms of the pixels with gt < K and gt != ignore_index, and the count of
    invalid ground-truth values).  gt: uint8 CUDA tensor [H, W]."""
    h, w, K, ld = _nhwc(logits)
    dev = logits.device

    def check(t, shape, dtype, what):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
            raise ValueError("%s must be a contiguous %s tensor %s on %s" % (what, dtype, list(shape), dev))

    check(gt, (H, W), torch.uint8, "gt")
    check(labels_out, (H, W), torch.uint8, "labels_out")
    check(confusion, (K, K), torch.int64, "confusion")
    if workspace is not None and workspace.size != (int(H), int(W)):
        raise ValueError("the workspace was made for %s, not %s" % (workspace.size, (H, W)))
    ws = workspace
    rc = _lib.lib().avl_seg_eval_full_res(_ptr(logits), h, w, K, ld, int(H), int(W), _ptr(gt), int(ignore_index), _ptr(labels_out),
                                          _ptr(confusion), _ptr(ws and ws.loss), _ptr(ws and ws.counts), _ptr(ws and ws.scratch),
                                          _stream(dev))
    _lib.check(rc, "avl_seg_eval_full_res")
    return ws
