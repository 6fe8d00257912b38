"""The reference's model API (src/network/deeplab_v3_plus/models/build.py:13-25,65-72 and models/deeplab_v3_plus.py:51-71) on the
HIP plans: scripts that build the network with ``build_model(cfg)`` and call ``model(x, upsample_pred=...)`` on normalised float
N x 3 x H x W tensors run unchanged on the evaluation path.

    net, loss_fn, train_metric, val_metric = build_model(cfg)
    model = nn.DataParallel(net, device_ids=[0]).cuda(0)
    model.load_state_dict(torch.load(path)["model"])          # 'module.' keys, as the reference saves them
    model.eval()
    with torch.no_grad():
        logits = model(x)                                      # fp32 [N, K, H, W]; upsample_pred=False: [N, K, H', W']
    loss = net.validate_step(x, label, val_metric)             # the validation step for the batch, fused (no [N, K, H, W] tensor)

The weights are BUFFERS named as the reference checkpoint's keys (plus one ``num_batches_tracked`` per BatchNorm, accepted and
unused), so ``state_dict()``, strict ``load_state_dict``, ``.cuda()`` / ``.to()`` and the ``module.`` prefix of a one-GPU
``nn.DataParallel`` behave as in the reference.  H' x W' (upsample_pred=False) is the low-level map (H/4 x W/4) less sum(k_i - 1)
over the refine blocks' depthwise kernel sizes (decoder_cfg.REFINE_KERNEL_SIZE, padding 0): H/4-4 x W/4-4 for the default [3, 3].
Inference only: a forward in train() mode raises NotImplementedError.
"""
import torch
import torch.nn as nn

from . import metrics
from .config import get_network_cfg_defaults
from .network import random_state_dict, refine_kernel_sizes, state_spec
from .semantic_segmentation import SemanticSegmentation

# build-specific MODEL.* settings build_model() hands on when the configuration has them (config.py)
MODEL_OPTIONS = ("MIXED_GCONV_MX", "MIXED_TRUNK_FP4", "MIXED_CONV2_SPLIT", "MIXED_LAYER1_LO", "HIP_GRAPH", "VALIDATE_BATCH")
PRECISIONS = ("mixed", "split16", "f32", "f16", "bf16")


def _get(node, key, default=None):
    try:
        return node[key] if isinstance(node, dict) else getattr(node, key)
    except (KeyError, AttributeError):
        return default


class DeepLabV3Plus(nn.Module):
    """DeepLabV3Plus(in_channels, out_channels, backbone, aspp_cfg, decoder_cfg, output_stride) of the reference as a drop-in module.
    Build-specific keywords: precision ("mixed", "split16", "f32", "f16", "bf16": MODEL.PRECISION), device (where the weight buffers
    start; None = the CPU, as a freshly built reference module), self_check ("auto", True, False: MODEL.MIXED_SELF_CHECK; "auto" checks
    weights that came in through load_state_dict, not the seeded initial ones), on_fail (MODEL.MIXED_ON_FAIL) and model_options (other
    MODEL.* settings of config.py, e.g. {"HIP_GRAPH": False})."""

    def __init__(self, in_channels, out_channels, backbone, aspp_cfg, decoder_cfg, output_stride, *, precision="mixed", device=None,
                 self_check="auto", on_fail="f32", model_options=None):
        super(DeepLabV3Plus, self).__init__()
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s, not %r" % (", ".join(PRECISIONS), precision))
        if output_stride not in (8, 16):
            raise NotImplementedError("output_stride %r: deeplab_v3_plus.py:30-36 knows 8 and 16" % (output_stride,))
        self.in_channels = int(in_channels)
        self.out_channels = int(out_channels)
        self.output_stride = int(output_stride)
        self.precision = precision
        self.self_check = self_check
        self.on_fail = on_fail
        self._cfg = get_network_cfg_defaults()
        m, d = self._cfg.MODEL, self._cfg.DATASET
        d.IN_CHANNELS, d.NUM_CLASSES = self.in_channels, self.out_channels
        m.BACKBONE, m.OUTPUT_STRIDE = str(backbone), self.output_stride
        m.ASPP.OUT_CHANNELS = int(_get(aspp_cfg, "OUT_CHANNELS", m.ASPP.OUT_CHANNELS))
        m.ASPP.ATROUS_CHANNELS = list(_get(aspp_cfg, "ATROUS_CHANNELS", m.ASPP.ATROUS_CHANNELS))
        m.DECODER.LOW_LEVEL_OUT_CHANNELS = int(_get(decoder_cfg, "LOW_LEVEL_OUT_CHANNELS", m.DECODER.LOW_LEVEL_OUT_CHANNELS))
        m.DECODER.REFINE_CHANNELS = list(_get(decoder_cfg, "REFINE_CHANNELS", m.DECODER.REFINE_CHANNELS))
        m.DECODER.REFINE_KERNEL_SIZE = list(refine_kernel_sizes(_get(decoder_cfg, "REFINE_KERNEL_SIZE", None), m.DECODER.REFINE_CHANNELS))
        m.PRECISION, m.MIXED_ON_FAIL = precision, on_fail
        for k, v in (model_options or {}).items():
            if k not in MODEL_OPTIONS:
                raise KeyError("model_options: %r is not one of %s" % (k, ", ".join(MODEL_OPTIONS)))
            m[k] = v
        self._spec_kw = dict(num_classes=self.out_channels, in_channels=self.in_channels, aspp_out=m.ASPP.OUT_CHANNELS,
                             atrous_channels=tuple(m.ASPP.ATROUS_CHANNELS), low_level_out=m.DECODER.LOW_LEVEL_OUT_CHANNELS,
                             refine_channels=tuple(m.DECODER.REFINE_CHANNELS), backbone=m.BACKBONE,
                             refine_kernel_size=tuple(m.DECODER.REFINE_KERNEL_SIZE))
        self._keys = [k for k, _ in state_spec(**self._spec_kw)]          # (NotImplementedError for an unsupported backbone)
        init = random_state_dict(seed=0, **self._spec_kw)
        for k in self._keys:
            self._node(k).register_buffer(k.rsplit(".", 1)[1], init[k].to(device) if device is not None else init[k])
            if k.endswith(".running_var"):             # BatchNorm2d's fifth entry, after running_var
                self._node(k).register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long, device=device))
        self._seg = None                 # SemanticSegmentation holding the plans, built by the first forward
        self._loaded = False             # the weights came in through load_state_dict ("auto" self-check)
        self.register_load_state_dict_pre_hook(DeepLabV3Plus._refuse_nonfinite)
        self.register_load_state_dict_post_hook(DeepLabV3Plus._weights_changed)

    def _node(self, key):
        """the submodule that holds `key`'s buffer (backbone.layer1.0.bn1.weight -> self.backbone.layer1[0].bn1), made on first use"""
        node = self
        for name in key.split(".")[:-1]:
            if name not in node._modules:
                node.add_module(name, nn.Module())
            node = node._modules[name]
        return node

    @staticmethod
    def _refuse_nonfinite(module, state_dict, prefix, *args):
        # before any buffer is overwritten: the kernels' ReLU is a max with 0, which would turn a NaN weight into 0 silently
        bad = [k for k in module._keys if isinstance(state_dict.get(prefix + k), torch.Tensor)
               and state_dict[prefix + k].is_floating_point() and not bool(torch.isfinite(state_dict[prefix + k]).all())]
        if bad:
            raise ValueError("state dict holds Inf / NaN in %d tensors, e.g. %s" % (len(bad), bad[:3]))

    @staticmethod
    def _weights_changed(module, incompatible_keys):
        module._seg = None
        module._loaded = True

    def _apply(self, fn, *args, **kwargs):
        out = super(DeepLabV3Plus, self)._apply(fn, *args, **kwargs)
        self._seg = None                 # .cuda() / .to(): the plans follow the buffers
        return out

    def _device(self):
        return self.backbone.conv1.weight.device

    def weights(self):
        """{reference key: fp32 CPU tensor} of the current buffers (num_batches_tracked left out)"""
        return {k: self._node(k)._buffers[k.rsplit(".", 1)[1]].detach().to("cpu", torch.float32) for k in self._keys}

    def segmentation(self):
        """the SemanticSegmentation that holds this module's plans (built on first use, on the buffers' device)"""
        dev = self._device()
        if self._seg is None:
            if dev.type != "cuda":
                raise RuntimeError("DeepLabV3Plus runs on a GPU: move it there first (.cuda() / .to(device)); its buffers are on %s" % dev)
            self._cfg.MODEL.MIXED_SELF_CHECK = self._loaded if self.self_check == "auto" else self.self_check
            seg = SemanticSegmentation(self._cfg, device=dev, state_dict=self.weights())      # (check_state_dict runs here)
            self._seg = seg
        return self._seg

    def forward(self, x, upsample_pred=True):
        """x: normalised float [N, 3, H, W] -> fp32 logits [N, K, H, W] (upsample_pred=True, F.interpolate with align_corners=True)
        or [N, K, H', W'] (H/4 - sum(k_i - 1), module docstring), in a new tensor without grad_fn."""
        self._check_call(x)
        with torch.no_grad():
            return self.segmentation().forward_tensor(x, upsample_pred=upsample_pred)

    def _check_call(self, *tensors):
        """what forward and validate_step refuse: train() mode, a DataParallel replica, tensors on another GPU than the buffers"""
        if self.training:
            raise NotImplementedError("DeepLabV3Plus here is inference only: call .eval() first (no training or backward)")
        if getattr(self, "_is_replica", False):
            raise RuntimeError("DeepLabV3Plus: nn.DataParallel over more than one GPU is not supported; use device_ids=[one GPU]")
        dev = self._device()
        if self._seg is not None and self._seg.device != dev:
            raise RuntimeError("DeepLabV3Plus: this module's plans live on %s, its buffers on %s (a DataParallel replica?)" % (self._seg.device, dev))
        for x in tensors:
            if isinstance(x, torch.Tensor) and x.is_cuda and x.device != dev:
                raise RuntimeError("DeepLabV3Plus: input on %s, model on %s" % (x.device, dev))

    def validate_step(self, x, label, metric=None):
        """The reference's validation step (train.py:138-141: preds = model(x); loss = loss_fn(preds, label); metric.evaluate(preds,
        label)) for a batch, fused: x normalised float [N, 3, H, W] as forward takes it, label integer [N, H, W] (255 = ignored).
        One forward of the batch plan, then one kernel at H x W that interpolates the logits, takes the arg-max, adds MeanIOU's
        counts into `metric` (a metrics.MeanIOU, or None) and sums CrossEntropyLoss(ignore_index=255) in fp64; the up-sampled logits
        are never written.  Returns the batch loss as a float (reduction='mean' over every counted pixel; NaN when all are 255).
        Labels outside [0, K) and not 255 raise ValueError, as torch's cross_entropy does, and leave `metric` unchanged."""
        self._check_call(x, label)
        with torch.no_grad():
            return self.segmentation().validate_step_tensor(x, label, metric)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """models/loss.py: nn.CrossEntropyLoss whose forward(pred, label) takes the label in any integer type (label.long())."""

    def forward(self, pred, label):
        return super(CrossEntropyLoss, self).forward(pred, label.long())


def build_model(cfg):
    """models/build.py:65-72 for MODEL.TYPE "DeepLabv3+" -> (net, loss_fn, train_metric, val_metric).  The build-specific MODEL.*
    keys (PRECISION, MIXED_SELF_CHECK, MIXED_ON_FAIL and MODEL_OPTIONS) are used when the configuration has them."""
    m = cfg.MODEL
    if _get(m, "TYPE") != "DeepLabv3+":
        raise NotImplementedError("MODEL.TYPE %r: only 'DeepLabv3+' is built" % (_get(m, "TYPE"),))
    options = {k: _get(m, k) for k in MODEL_OPTIONS if _get(m, k) is not None}
    net = DeepLabV3Plus(in_channels=cfg.DATASET.IN_CHANNELS, out_channels=cfg.DATASET.NUM_CLASSES, backbone=m.BACKBONE, aspp_cfg=m.ASPP,
                        decoder_cfg=m.DECODER, output_stride=m.OUTPUT_STRIDE, precision=_get(m, "PRECISION", "mixed"),
                        self_check=_get(m, "MIXED_SELF_CHECK", "auto"), on_fail=_get(m, "MIXED_ON_FAIL", "f32"), model_options=options)
    loss_fn = CrossEntropyLoss(ignore_index=255)
    return net, loss_fn, metrics.MeanIOU(cfg.DATASET.NUM_CLASSES), metrics.MeanIOU(cfg.DATASET.NUM_CLASSES)
