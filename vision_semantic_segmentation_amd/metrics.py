"""MeanIOU of the reference (src/network/deeplab_v3_plus/models/metrics.py:9-80, core/utils/metric.py:13-49) with its confusion
matrix kept as an int64 tensor on the device until it is read.

    metric = MeanIOU(num_class)
    loss = seg.validate_step(image, label, metric)     # the fused HIP path adds the counts of the frame, or of a batch [N, h, w, 3]
    metric.evaluate(preds, labels)                     # or: full-res logits [B, K, H, W] through torch ops (not the hot path)
    metric.synchronize_between_processes()
    print(metric.global_avg)
"""
import warnings

import numpy as np
import torch
import torch.distributed as distributed


class MeanIOU(object):
    def __init__(self, num_class, device=None):
        self.num_class = int(num_class)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        # confusion_matrix[gt][pred]: pixel counts, rows = ground truth (metrics.py:52-55)
        self.confusion_matrix = torch.zeros((self.num_class, self.num_class), dtype=torch.int64, device=self.device)

    def reset(self):
        self.confusion_matrix.zero_()

    def add_confusion(self, counts):
        """adds a [K, K] count matrix (e.g. what the fused validation kernel produced) into the running one"""
        self.confusion_matrix += counts.to(device=self.confusion_matrix.device, dtype=torch.int64)

    def evaluate(self, preds, labels):
        """preds: logits [B, K, H, W]; labels: ground truth [B, H, W].  Pixels whose label is outside [0, K) are skipped (metrics.py:47-59)."""
        num_class = preds.shape[1]
        preds = torch.argmax(preds, dim=1)
        assert num_class == self.num_class
        assert preds.shape == labels.shape
        labels = torch.as_tensor(labels).to(preds.device).long()
        mask = (labels >= 0) & (labels < self.num_class)
        x = self.num_class * labels[mask] + preds[mask]
        count = torch.bincount(x, minlength=self.num_class ** 2)
        self.add_confusion(count.reshape(self.num_class, self.num_class))

    def synchronize_between_processes(self, group=None):
        """Sums the matrices of every rank (metrics.py:61-68): a device tensor for nccl, a CPU copy for other backends (gloo).
        Nothing happens when no process group is initialised."""
        if not distributed.is_available() or not distributed.is_initialized():
            return
        if distributed.get_backend(group) == "nccl":
            t = self.confusion_matrix
            if not t.is_cuda:
                t = t.to(torch.device("cuda", torch.cuda.current_device()))
        else:
            t = self.confusion_matrix.cpu()
        distributed.all_reduce(t, group=group)
        if t.data_ptr() != self.confusion_matrix.data_ptr():
            self.confusion_matrix.copy_(t)

    def iou(self):
        """per-class IoU (float64 ndarray), NaN for a class whose union is empty (metrics.py:70-80)"""
        cm = self.confusion_matrix.cpu().numpy().astype(np.float64)
        intersection = np.diag(cm)
        union = np.sum(cm, axis=0) + np.sum(cm, axis=1) - intersection
        return np.divide(intersection, union, out=np.full(union.shape, np.nan), where=(union != 0))

    @property
    def global_avg(self):
        """mean IoU over the classes whose union is not empty (NaN when none is)"""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # np.nanmean of an all-NaN vector
            return float(np.nanmean(self.iou()))

    def __str__(self):
        return "{:.4f}".format(self.global_avg)

    @property
    def summary_str(self):
        return self.__str__()
