"""Full-resolution predictions and validation terms from a plan's logits (csrc/seg_head.hip, include/avl_hip.h):
DeepLabV3Plus.forward(x, upsample_pred=True) (deeplab_v3_plus.py:51,67-69) and the validation step of train.py:138-141.

    upsample_logits(net.logits, H, W)                  # fp32 [K, H, W]: F.interpolate(..., align_corners=True)
    full_res_eval(net.logits, H, W, gt=gt_u8, labels_out=lab, confusion=cm, workspace=ws)   # fused arg-max / confusion / loss

`logits` is the plan's fp32 NHWC map [h, w, K] (SegNet.logits; a row stride ld >= K is allowed), or a batched plan's [N, h, w, K]:
then gt / labels are [N, H, W], the up-sampled logits [N, K, H, W], and the whole batch is one launch of each kernel.  Everything is launched on the
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
    """-> (N or None, image_rows, h, w, K, ld) of an NHWC map [h, w, K] or a batch [N, h, w, K] (image i image_rows rows after i-1)"""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() in (3, 4)):
        raise ValueError("logits must be a float32 CUDA tensor [h, w, K] or [N, h, w, K]")
    n = None
    if logits.dim() == 4:
        n = int(logits.shape[0])
        if n < 1:
            raise ValueError("an empty batch of logits")
    h, w, K = logits.shape[-3:]
    ld = logits.stride(-2)
    if logits.stride(-1) != 1 or (h > 1 and logits.stride(-3) != w * ld):
        raise ValueError("logits must be NHWC rows of stride ld >= K (strides %s)" % (logits.stride(),))
    image_rows = h * w
    if n is not None and n > 1:
        if logits.stride(0) % ld or logits.stride(0) < h * w * ld:
            raise ValueError("the images of a logits batch must be a whole number of rows >= h * w apart (strides %s)" % (logits.stride(),))
        image_rows = logits.stride(0) // ld
    return n, int(image_rows), int(h), int(w), int(K), int(ld)


def _lead(n):
    return () if n is None else (n,)


def upsample_logits(logits, H, W, out=None):
    """fp32 [h, w, K] -> fp32 [K, H, W] (`out`, or a new tensor), bilinear with align_corners=True.
    A batch [N, h, w, K] -> [N, K, H, W] in one launch; out[i] is bit for bit the single-image result on logits[i]."""
    n, image_rows, h, w, K, ld = _nhwc(logits)
    shape = _lead(n) + (K, int(H), int(W))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=logits.device)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != logits.device:
        raise ValueError("out must be a contiguous float32 tensor %s on %s" % (list(shape), logits.device))
    _lib.check(_lib.lib().avl_upsample_logits_batch(_ptr(logits), n or 1, image_rows, h, w, K, ld, _ptr(out), int(H), int(W),
                                                    _stream(logits.device)), "avl_upsample_logits_batch")
    return out


class EvalWorkspace(object):
    """The loss outputs of full_res_eval for an H x W output and a batch of `batch` images (1: also the single-image call form):
    loss = fp64 {sum, mean} and counts = {contributing pixels, invalid labels} over the batch, image_loss [batch, 2] and image_counts
    [batch, 2] the same per image."""

    def __init__(self, H, W, device, batch=1):
        self.size = (int(H), int(W))
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("a workspace for a batch of %d" % self.batch)
        nbytes = _lib.lib().avl_seg_eval_scratch_bytes_batch(self.batch, int(H), int(W))
        if nbytes < 0:
            raise RuntimeError("avl_seg_eval_scratch_bytes_batch failed: %s" % _lib.last_error())
        self.scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        # one block of 8-byte words, so that result() is one copy: loss[2] counts[2] image_loss[batch][2] image_counts[batch][2]
        n = self.batch
        self._words = torch.empty(4 + 4 * n, dtype=torch.int64, device=device)
        self.loss = self._words[0:2].view(torch.float64)
        self.counts = self._words[2:4]
        self.image_loss = self._words[4:4 + 2 * n].view(torch.float64).view(n, 2)
        self.image_counts = self._words[4 + 2 * n:].view(n, 2)

    def result(self):
        """(synchronises) {"loss_sum", "loss" (NaN when no pixel counted), "count", "invalid"} of the last call over its batch, and
        per image the lists "image_loss_sum", "image_loss", "image_count", "image_invalid"."""
        n = self.batch
        words = self._words.cpu()
        loss, counts = words[0:2].view(torch.float64).tolist(), words[2:4].tolist()
        il, ic = words[4:4 + 2 * n].view(torch.float64).view(n, 2), words[4 + 2 * n:].view(n, 2)
        return {"loss_sum": loss[0], "loss": loss[1], "count": counts[0], "invalid": counts[1],
                "image_loss_sum": il[:, 0].tolist(), "image_loss": il[:, 1].tolist(),
                "image_count": ic[:, 0].tolist(), "image_invalid": ic[:, 1].tolist()}


def full_res_eval(logits, H, W, gt=None, labels_out=None, confusion=None, workspace=None, ignore_index=IGNORE_INDEX):
    """One fused pass over the H x W output: labels_out uint8 [H, W] (arg-max), confusion int64 [K, K] (+= MeanIOU's counts of the
    pixels with gt < K), workspace (EvalWorkspace: cross-entropy terms of the pixels with gt < K and gt != ignore_index, and the count of
    invalid ground-truth values).  gt: uint8 CUDA tensor [H, W].
    A batch: logits [N, h, w, K] with gt / labels_out [N, H, W] and an EvalWorkspace(batch=N), still one pass (one launch, plus the
    finalize).  Every image's labels, counts and loss sum are bit for bit the single-image call's; the ONE confusion matrix takes all N
    images; the workspace's loss is the mean over every counted pixel of the batch (torch's reduction='mean')."""
    n, image_rows, h, w, K, ld = _nhwc(logits)
    dev = logits.device
    H, W = int(H), int(W)

    def check(t, shape, dtype, what):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()
                              or t.device != dev):
            raise ValueError("%s must be a contiguous %s tensor %s on %s" % (what, dtype, list(shape), dev))

    check(gt, _lead(n) + (H, W), torch.uint8, "gt")
    check(labels_out, _lead(n) + (H, W), torch.uint8, "labels_out")
    check(confusion, (K, K), torch.int64, "confusion")
    ws = workspace
    if ws is not None and ws.size != (H, W):
        raise ValueError("the workspace was made for %s, not %s" % (ws.size, (H, W)))
    if ws is not None and ws.batch != (n or 1):
        raise ValueError("the workspace was made for a batch of %d, not %d" % (ws.batch, n or 1))
    rc = _lib.lib().avl_seg_eval_full_res_batch(_ptr(logits), n or 1, image_rows, h, w, K, ld, H, W, _ptr(gt), int(ignore_index),
                                                _ptr(labels_out), _ptr(confusion), _ptr(ws and ws.loss), _ptr(ws and ws.counts),
                                                _ptr(ws and ws.image_loss), _ptr(ws and ws.image_counts), _ptr(ws and ws.scratch),
                                                _stream(dev))
    _lib.check(rc, "avl_seg_eval_full_res_batch")
    return ws
