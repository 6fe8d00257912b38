"""SemanticSegmentation -- the reference's inference wrapper (src/semantic_segmentation.py:20-57)
on the HIP conv stack.

    seg = SemanticSegmentation(cfg.VISION_SEM_SEG.SEM_SEG_NETWORK)
    labels = seg.segmentation(image_rgb_u8)        # int64 ndarray [h', w'], as the reference returns
    labels = seg.segmentation(np.stack(frames))    # a batch [N, h, w, 3] -> [N, h', w'], one plan for all N

h' x w' is the low-level map (h/4 x w/4, rounded as the stem and max-pool round) less sum(k_i - 1) over the refine blocks'
depthwise kernel sizes k_i (MODEL.DECODER.REFINE_KERNEL_SIZE; padding 0): h/4-4 x w/4-4 for the default [3, 3].

Differences by design: weights come from a LOCAL checkpoint (``MODEL.WEIGHT``) in the reference's
format or, when that is empty, from a seeded random init -- the reference's
``resnext50_32x4d(pretrained=True)`` URL fetch (backbone/build.py:20) is never attempted;
normalisation (ToTensor + Normalize, :35-39) is fused into the stem kernel; the arg-max runs on the
GPU and ``segmentation_device`` hands back the uint8 label map without leaving HBM.
"""
import numpy as np
import torch

from . import _lib, seg_head
from .network import BACKBONES, SegNet, backbone_arch, check_state_dict, load_checkpoint, random_state_dict, refine_kernel_sizes


def _strict_bool(v, what):
    """True / False, or the strings yacs' merge_from_list may hand over; anything else is an error (bool('off') is True)."""
    if isinstance(v, bool):
        return v
    if isinstance(v, str) and v.strip().lower() in ("true", "on", "1", "yes"):
        return True
    if isinstance(v, str) and v.strip().lower() in ("false", "off", "0", "no"):
        return False
    raise ValueError("%s must be 'auto', True or False, not %r" % (what, v))


class SemanticSegmentation(object):
    def __init__(self, cfg, device=None, state_dict=None):
        """cfg: network configuration (cfg.VISION_SEM_SEG.SEM_SEG_NETWORK of base_cfg.py:96-112)."""
        _lib.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("SemanticSegmentation needs a GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if cfg.MODEL.TYPE != "DeepLabv3+" or cfg.MODEL.OUTPUT_STRIDE not in (8, 16):
            raise NotImplementedError("only DeepLabv3+ at output stride 8 or 16 is built (backbones: %s)" % ", ".join(sorted(BACKBONES)))
        backbone_arch(cfg.MODEL.BACKBONE)        # NotImplementedError naming the supported set
        self.backbone = str(cfg.MODEL.BACKBONE)
        self.output_stride = int(cfg.MODEL.OUTPUT_STRIDE)
        self.cfg = cfg
        self.num_classes = cfg.DATASET.NUM_CLASSES
        self.precision = getattr(cfg.MODEL, "PRECISION", "mixed")
        kw = dict(num_classes=self.num_classes, in_channels=cfg.DATASET.IN_CHANNELS, aspp_out=cfg.MODEL.ASPP.OUT_CHANNELS,
                  atrous_channels=tuple(cfg.MODEL.ASPP.ATROUS_CHANNELS), low_level_out=cfg.MODEL.DECODER.LOW_LEVEL_OUT_CHANNELS,
                  refine_channels=tuple(cfg.MODEL.DECODER.REFINE_CHANNELS), backbone=self.backbone,
                  refine_kernel_size=refine_kernel_sizes(getattr(cfg.MODEL.DECODER, "REFINE_KERNEL_SIZE", None),
                                                         cfg.MODEL.DECODER.REFINE_CHANNELS))
        # (every plan, those of the self-check ladder included, takes each refine block's kernel size from its depthwise weight)
        self.refine_kernel_size = kw["refine_kernel_size"]
        if state_dict is not None:
            self.state = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        elif cfg.MODEL.WEIGHT:
            self.state = load_checkpoint(cfg.MODEL.WEIGHT)                      # :31-32
        else:
            self.state = random_state_dict(seed=getattr(cfg.MODEL, "SEED", 0), **kw)
        check_state_dict(self.state, **kw)
        self._nets = {}
        self._heads = {}                   # (h, w) or (h, w, N) -> _FullResBuffers of the upsample_pred / validate_step paths
        self._batch_out = {}               # ("labels" | "logits", h, w, N) -> full-resolution output of a batch
        # "mixed" self-check: the logits error of the mixed mode follows the WEIGHTS and was measured on seeded
        # draws only, so a real checkpoint is checked once, before its first plan, against the fp32-input HIP path (itself 2e-6 from
        # the fp32 reference) on several seeded frames, and every 16-bit tensor of the plan is scanned for Inf / NaN where it is
        # produced.  The check walks a LADDER of plans and keeps the first one that passes:
        #   "mixed"       f16 + FP4 matrix cores, layer1's first two blocks write one f16 plane (MIXED_LAYER1_LO = False starts here)
        #   "mixed+lo"    every layer1 block keeps its lo plane (the default configuration starts here)
        #   "split16"     the COMPLETE hi + lo pipeline (SegNet(full_split=True)): every tensor two f16 planes, every product three f16 passes, no
        #                 FP4 and no single-plane tensor anywhere -- what a calibrated (trained) checkpoint needs
        #   "f32"         fp32-input MFMA, the reference's precision (50 frames/s)
        sc = getattr(cfg.MODEL, "MIXED_SELF_CHECK", "auto")
        self._self_check = (state_dict is None and bool(cfg.MODEL.WEIGHT)) if sc == "auto" else _strict_bool(sc, "MODEL.MIXED_SELF_CHECK")
        self._layer1_lo = bool(getattr(cfg.MODEL, "MIXED_LAYER1_LO", True))
        self._rung = "mixed+lo" if self._layer1_lo else "mixed"     # which plan of the ladder the "mixed" precision currently means
        self.on_fail = str(getattr(cfg.MODEL, "MIXED_ON_FAIL", "f32"))
        if self.on_fail not in ("f32", "raise", "warn"):
            raise ValueError("MODEL.MIXED_ON_FAIL must be 'f32', 'raise' or 'warn', not %r" % self.on_fail)
        self.mixed_check = None            # {"size", "rel_err", "rung", "tried", ...} once the check has run
        self.validate_batch = bool(getattr(cfg.MODEL, "VALIDATE_BATCH", False))      # validate_step also takes [N, h, w, 3]

    LADDER = ("mixed", "mixed+lo", "split16", "f32")

    def net_for(self, h, w, raw_frame=None, batch=1, input_format="u8_hwc", raw_batch=False):
        """The compiled plan for a batch of `batch` h x w network inputs (built on first use, kept per size, batch and input format).
        raw_frame = (src_h, src_w): the plan that takes the raw BGR camera frame and pre-processes inside its first kernel (one frame,
        unless raw_batch=True: `batch` raw frames, each with a camera model of its own -- SegNet(raw_batch=True); its key ends in
        "raw_batch", so it is neither the plain (h, w, N) plan nor the one-frame raw plan (h, w, 1, src_h, src_w)).
        input_format "f32_nchw": the plan takes normalised fp32 [N,3,h,w] tensors (SegNet); "u8_hwc" (default): uint8 RGB frames.
        The mixed self-check runs once, on h x w frames of a batch of one; the rung it picks serves every batch and input format."""
        batch = int(batch)
        if raw_batch and raw_frame is None:
            raise ValueError("raw_batch=True asks for a batch of raw camera frames and needs raw_frame=(src_h, src_w)")
        if batch > 1 and raw_frame is not None and not raw_batch:
            raise NotImplementedError("a raw_frame plan (pre-processing stem) takes one camera frame, not a batch of %d (raw_batch=True "
                                      "builds the plan for a batch of raw frames)" % batch)
        key = (int(h), int(w), batch) + (() if raw_frame is None else (int(raw_frame[0]), int(raw_frame[1])))
        if input_format != "u8_hwc":
            key += (input_format,)
        if raw_batch:
            key += ("raw_batch",)
        if key not in self._nets:
            if self._self_check and self.precision == "mixed" and self.mixed_check is None:
                self.check_mixed_against_f32(key[0], key[1])
            rung = self._rung if self.precision == "mixed" else self.precision
            net = self._build(key[0], key[1], rung, raw_frame, batch, input_format, raw_batch)
            if getattr(self.cfg.MODEL, "HIP_GRAPH", True):
                net.capture_graph()
            self._nets[key] = net
        return self._nets[key]

    def _build(self, h, w, rung, raw_frame=None, batch=1, input_format="u8_hwc", raw_batch=False):
        """rung: a plan of the ladder ("mixed", "mixed+lo", "split16") or a plain precision ("f32", "f16", "bf16")"""
        kw = dict(device=self.device, num_classes=self.num_classes, raw_frame=raw_frame, output_stride=self.output_stride, backbone=self.backbone,
                  batch=batch, input_format=input_format, raw_batch=raw_batch)
        if rung in ("f32", "f16", "bf16"):
            return SegNet(self.state, h, w, precision=rung, **kw)
        if rung == "split16":
            return SegNet(self.state, h, w, precision="mixed", full_split=True, **kw)
        return SegNet(self.state, h, w, precision="mixed",
                      conv2_split=bool(getattr(self.cfg.MODEL, "MIXED_CONV2_SPLIT", True)),
                      gconv_mx=bool(getattr(self.cfg.MODEL, "MIXED_GCONV_MX", True)),
                      trunk_fp4=bool(getattr(self.cfg.MODEL, "MIXED_TRUNK_FP4", True)),
                      layer1_lo=(rung == "mixed+lo"), **kw)

    @staticmethod
    def decide_rung(tried, on_fail, n_frames=4):
        """The self-check's decision, apart from its measurements: `tried` = [{"rung", "rel_err", "finite", "nonfinite_ops", "passes"}] in
        ladder order -> (rung to use, its error, warning text or None).  The best PASSING rung wins; when none passes: on_fail "f32" ->
        the fp32 plan, "raise" -> RuntimeError, "warn" -> the best finite 16-bit plan (fp32 if there is none)."""
        ok = [t for t in tried if t["passes"]]
        if ok:
            t = min(ok, key=lambda t: t["rel_err"])
            return t["rung"], t["rel_err"], None
        summary = "; ".join("%s: %s" % (t["rung"], ("%.2e" % t["rel_err"]) if t["finite"] and not t["nonfinite_ops"]
                                        else "Inf/NaN in " + ", ".join(t["nonfinite_ops"] or ["the logits"])) for t in tried)
        msg = ("mixed precision: no 16-bit plan reproduces the fp32 logits of these weights within 1e-3 on %d frames (%s)" % (n_frames, summary))
        if on_fail == "raise":
            raise RuntimeError(msg)
        usable = [t for t in tried if t["finite"] and not t["nonfinite_ops"] and t["rel_err"] == t["rel_err"]]
        if on_fail == "warn" and usable:
            t = min(usable, key=lambda t: t["rel_err"])
            return t["rung"], t["rel_err"], msg + "; keeping '%s' (MODEL.MIXED_ON_FAIL = 'warn')" % t["rung"]
        return "f32", 0.0, msg + "; using the fp32 plan (4x slower)"

    @staticmethod
    def check_frames(h, w, seed=1, n_noise=3):
        """The self-check's frames: `n_noise` uniform-noise frames and one smooth frame (low-frequency colour ramps + a few blobs: real
        camera frames excite far fewer high-frequency channels than noise does)."""
        rng = np.random.default_rng(seed)
        frames = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(n_noise)]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        smooth = np.stack([128 + 100 * np.sin(2 * np.pi * (xx / w * (1 + k) + yy / h * (2 - k) * 0.5) + k) for k in range(3)], axis=2)
        for _ in range(6):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * min(h, w)
            smooth += (rng.uniform(-80, 80, size=3) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))[..., None])
        frames.append(np.clip(smooth, 0, 255).astype(np.uint8))
        return frames

    def check_mixed_against_f32(self, h, w, threshold=8e-4, seed=1):
        """Several seeded h x w frames (check_frames) through the plans of the ladder and through the fp32-input plan: the WORST
        max |dlogit| / max |logit| over the frames decides.  A plan FAILS when that figure is not finite, when its logits hold an Inf /
        NaN, when any of its tensors does (avl_seg_plan_nonfinite: an f16 overflow that a later ReLU would hide), or when the error is
        above 1e-3; it is ACCEPTED at once when the error is at most `threshold`, otherwise the next rung is measured too and the best
        passing one is kept.  When no 16-bit plan passes: MODEL.MIXED_ON_FAIL = "f32" (default) uses the fp32 plan from now on,
        "raise" raises, "warn" keeps the best-effort 16-bit plan with a warning.  A checkpoint whose fp32 logits are not finite raises.
        Returns (and keeps in .mixed_check) what was measured."""
        import warnings
        frames = [torch.from_numpy(f).to(self.device) for f in self.check_frames(h, w, seed)]
        ref = self._build(h, w, "f32")
        refs = []
        for f in frames:
            ref.forward(f)
            refs.append(ref.logits.float().clone())
        del ref
        if not all(bool(torch.isfinite(r).all()) for r in refs):
            raise RuntimeError("the checkpoint's logits are not finite even in fp32: %s" % (self.cfg.MODEL.WEIGHT or "<state_dict>"))
        tried = []
        start = self.LADDER.index(self._rung)
        for rung in self.LADDER[start:-1]:
            net = self._build(h, w, rung)
            err, finite = 0.0, True
            for f, r in zip(frames, refs):
                net.forward(f)
                lg = net.logits.float()
                finite = finite and bool(torch.isfinite(lg).all())
                e = float((lg - r).abs().max()) / float(r.abs().max())
                err = e if not (e <= err) else err          # NaN-safe maximum: a NaN error sticks
            bad = net.nonfinite_counts() if finite else {"logits": 1}
            del net
            ok = finite and not bad and (err <= 1e-3)
            tried.append({"rung": rung, "rel_err": err, "finite": finite, "nonfinite_ops": sorted(bad)[:4], "passes": ok})
            if ok and err <= threshold:
                break
        torch.cuda.empty_cache()
        self.mixed_check = {"size": (h, w), "threshold": threshold, "frames": len(frames), "tried": tried}
        self._rung, err, warning = self.decide_rung(tried, self.on_fail, len(frames))
        if warning:
            warnings.warn(warning)
        self._layer1_lo = self._rung != "mixed"
        self.mixed_check.update(rung=self._rung, layer1_lo=self._layer1_lo, rel_err=err)
        return self.mixed_check

    @staticmethod
    def _geometry(image_in):
        """[h, w, 3] -> (None, h, w); a batch [N, h, w, 3] -> (N, h, w)"""
        if image_in.ndim == 4:
            if int(image_in.shape[0]) < 1:
                raise ValueError("an empty batch")
            return int(image_in.shape[0]), int(image_in.shape[1]), int(image_in.shape[2])
        if image_in.ndim != 3:
            raise ValueError("expected an RGB image [h, w, 3] or a batch [N, h, w, 3], got shape %s" % (tuple(image_in.shape),))
        return None, int(image_in.shape[0]), int(image_in.shape[1])

    def _run(self, image_in):
        """one forward of the plan for image_in's size and batch -> (plan, N or None, h, w)"""
        n, h, w = self._geometry(image_in)
        net = self.net_for(h, w, batch=n or 1)
        net.forward(image_in[0] if n == 1 else image_in)
        return net, n, h, w

    def _batch_buffer(self, what, shape, dtype):
        key = (what,) + tuple(shape)
        t = self._batch_out.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._batch_out[key] = t
        return t

    def segmentation_device(self, image_in, upsample_pred=False):
        """uint8 RGB [h,w,3] (ndarray or CUDA tensor) -> uint8 CUDA tensor [h', w'] (module docstring).
        upsample_pred=True: labels at the input's size [h, w] -- the arg-max of model(x, upsample_pred=True) (deeplab_v3_plus.py:67-69),
        from the fused full-resolution kernel (the upsampled logits are never written).  A view of a buffer owned per input size: the
        next call of the same size overwrites it.
        A batch [N,h,w,3] runs through one plan of batch N -> [N, h', w'] ([N, h, w] with upsample_pred: one launch of the
        full-resolution kernel for the batch, each image from its own logits)."""
        net, n, h, w = self._run(image_in)
        if n is None:
            if not upsample_pred:
                return net.labels
            head = self._full_res(h, w)
            seg_head.full_res_eval(net.logits, h, w, labels_out=head.labels)
            return head.labels
        logits = net.logits if n > 1 else net.logits.unsqueeze(0)
        if not upsample_pred:
            return net.labels if n > 1 else net.labels.unsqueeze(0)
        out = self._batch_buffer("labels", (n, h, w), torch.uint8)
        seg_head.full_res_eval(logits, h, w, labels_out=out)
        return out

    def segmentation_device_raw(self, bgr, K=None, dist=None, factor=1):
        """The node's chain from the camera frame on (vision_semantic_segmentation_node.py:83-102) in the network's own kernels:
        uint8 BGR [H,W,3] (ndarray or CUDA tensor) -> BGR->RGB, cv2.undistort(K, dist) (skipped when None), INTER_AREA by the integer
        `factor`, normalise, network, arg-max -> uint8 CUDA tensor.  Same labels as preprocess_device() + segmentation_device(), without
        the RGB frame in between.  Every precision and every rung of the self-check's ladder has such a stem (fp32: k_stem_pre_f32)."""
        return self._run_raw(bgr, K, dist, factor).labels

    def _run_raw(self, bgr, K, dist, factor):
        """one forward of the raw-frame plan for bgr's size -> the plan"""
        H, W = int(bgr.shape[0]), int(bgr.shape[1])
        net = self.net_for(H // factor, W // factor, raw_frame=(H, W))
        net.set_camera(K, dist)
        net.forward(bgr)
        return net

    def logits_device_raw(self, bgr, K=None, dist=None, factor=1):
        """segmentation_device_raw, returning the plan's logits instead of its labels: the fp32 CUDA view [h', w', classes] every plan
        writes (no extra pass), which SemanticMapping.frame_device(..., src_kind="logits") reads.  The next forward of the same size
        overwrites it."""
        return self._run_raw(bgr, K, dist, factor).logits

    def logits_device_raw_batch(self, frames, Ks=None, dists=None, factor=1):
        """segmentation_device_raw_batch, returning the batched plan's logits [V, h', w', classes] (V = 1 included) for
        SemanticMapping.frame_device_views(..., src_kind="logits")."""
        net, V = self._run_raw_batch(frames, Ks, dists, factor)
        return net.logits if V > 1 else net.logits.unsqueeze(0)

    def segmentation_device_raw_batch(self, frames, Ks=None, dists=None, factor=1):
        """segmentation_device_raw for the V frames of one trigger, each with its own camera, in ONE plan (net_for(raw_batch=True)):
        frames = uint8 BGR [V,H,W,3] (ndarray or CUDA tensor) or a list of V equal-sized [H,W,3] frames; Ks[v] / dists[v] = view v's
        3x3 K and (k1 k2 p1 p2 k3), None (per view, or Ks = dists = None for all) = that view is not undistorted.  Every frame is
        copied straight into the plan's input buffer and pre-processed inside the stem's loader with its own camera block, so view
        v's labels are bit for bit segmentation_device_raw(frames[v], Ks[v], dists[v], factor).  Returns the plan's uint8 CUDA labels
        [V, h', w'] (V = 1 included).  The mixed self-check and its fall-back ladder apply as for every other plan."""
        net, V = self._run_raw_batch(frames, Ks, dists, factor)
        return net.labels if V > 1 else net.labels.unsqueeze(0)

    def _run_raw_batch(self, frames, Ks, dists, factor):
        """one forward of the raw-batch plan for the frames' size and number -> (plan, V)"""
        if isinstance(frames, (list, tuple)):
            views = list(frames)
        else:
            if frames.ndim != 4:
                raise ValueError("expected BGR frames [V, H, W, 3] or a list of [H, W, 3] frames, got shape %s" % (tuple(frames.shape),))
            views = [frames[v] for v in range(int(frames.shape[0]))]
        V = len(views)
        if V < 1:
            raise ValueError("an empty batch")
        H, W = int(views[0].shape[0]), int(views[0].shape[1])
        for f in views:
            if tuple(f.shape) != (H, W, 3):
                raise ValueError("the frames of one batch must have one size: %s and %s" % ((H, W, 3), tuple(f.shape)))
        Ks = [None] * V if Ks is None else list(Ks)
        dists = [None] * V if dists is None else list(dists)
        if len(Ks) != V or len(dists) != V:
            raise ValueError("%d frames, %d camera matrices, %d distortion vectors" % (V, len(Ks), len(dists)))
        net = self.net_for(H // factor, W // factor, raw_frame=(H, W), batch=V, raw_batch=True)
        for v in range(V):
            net.set_camera(Ks[v], dists[v], image=v)
        if isinstance(frames, (list, tuple)):
            slots = net.image.view(V, H, W, 3)
            for v, f in enumerate(views):
                t = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))
                if t.dtype != torch.uint8:
                    raise ValueError("camera frames are uint8, not %s" % t.dtype)
                slots[v].copy_(t, non_blocking=True)
            net.forward()
        else:
            net.forward(frames)
        return net, V

    def segmentation(self, image_in, upsample_pred=False):
        """semantic_segmentation.py:41-57: numpy (h, w, 3) RGB -> int64 numpy label map ([h, w] with upsample_pred=True); a batch
        (N, h, w, 3) -> (N, h', w')."""
        labels = self.segmentation_device(image_in, upsample_pred=upsample_pred)
        return labels.cpu().numpy().astype(np.int64)

    def logits(self, image_in, upsample_pred=False):
        """float32 CUDA tensor [K, h', w'] (the reference's layout) of model(x, upsample_pred=False).
        upsample_pred=True: model(x) as the reference's default returns it for a batch of one -- [K, h, w] at the input's size,
        F.interpolate(..., mode='bilinear', align_corners=True) of the logits (deeplab_v3_plus.py:67-69).  Either way the result is a
        VIEW of a buffer the plan owns per input size: the next call of the same size overwrites it (clone() to keep it).
        A batch [N,h,w,3] -> [N, K, h', w'] (the reference's NCHW batch), [N, K, h, w] with upsample_pred."""
        net, n, h, w = self._run(image_in)
        if n is not None:
            logits = net.logits if n > 1 else net.logits.unsqueeze(0)
            if not upsample_pred:
                return logits.permute(0, 3, 1, 2)
            out = self._batch_buffer("logits", (n, self.num_classes, h, w), torch.float32)
            return seg_head.upsample_logits(logits, h, w, out=out)
        if not upsample_pred:
            return net.logits.permute(2, 0, 1)
        head = self._full_res(h, w)
        if head.logits is None:
            head.logits = torch.empty((self.num_classes, h, w), dtype=torch.float32, device=self.device)
        return seg_head.upsample_logits(net.logits, h, w, out=head.logits)

    def forward_tensor(self, x, upsample_pred=True):
        """DeepLabV3Plus.forward(x, upsample_pred) (deeplab_v3_plus.py:51-71) on the reference's own input: x = float [N,3,h,w],
        normalised as ToTensor + Normalize leave it (any float dtype; a CPU tensor is copied to the device).  Runs the plan of the rung
        the ladder picked, with the fp32-input stem (SegNet(input_format="f32_nchw")).  Returns a NEW fp32 tensor: the logits
        [N,K,h',w'], or [N,K,h,w] with upsample_pred (F.interpolate(..., align_corners=True), one seg_head.upsample_logits for the batch).
        An unbatched x [3,h,w] gives [K,h',w'] ([K,h,w]), as torch's convolutions treat an unbatched input."""
        logits, unbatched, n, h, w = self._run_tensor(x)
        if not upsample_pred:
            out = logits.permute(0, 3, 1, 2).contiguous()
        else:
            out = seg_head.upsample_logits(logits, h, w)
        return out[0] if unbatched else out

    @staticmethod
    def _tensor_geometry(x):
        """x = float [N,3,h,w] or [3,h,w] -> (unbatched, N, h, w)"""
        if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4) or x.shape[-3] != 3 or not x.dtype.is_floating_point:
            raise ValueError("expected a float tensor [N, 3, h, w] or [3, h, w], got %s" % (
                "%s %s" % (x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__))
        unbatched = x.dim() == 3
        n = 1 if unbatched else int(x.shape[0])
        if n < 1:
            raise ValueError("an empty batch")
        return unbatched, n, int(x.shape[-2]), int(x.shape[-1])

    def _run_tensor(self, x):
        """one forward of the "f32_nchw" plan for x (_tensor_geometry) -> (its logits as [N,h',w',K], unbatched, N, h, w)"""
        unbatched, n, h, w = self._tensor_geometry(x)
        net = self.net_for(h, w, batch=n, input_format="f32_nchw")
        net.forward(x if unbatched or n > 1 else x[0])
        logits = net.logits if n > 1 else net.logits.unsqueeze(0)          # [N, h', w', K]
        return logits, unbatched, n, h, w

    def validate_step(self, image_in, label, metric=None):
        """The reference's validation step (train.py:138-141: preds = model(x); loss = loss_fn(preds, label);
        metric.evaluate(preds, label)) on the current plan: one forward, then ONE fused kernel at the input's resolution that
        interpolates the logits, takes the arg-max, adds MeanIOU's counts into `metric` (a metrics.MeanIOU, or None) and sums
        CrossEntropyLoss(ignore_index=255) in fp64.  image_in: uint8 RGB [h, w, 3]; label: int64 or uint8 [h, w] (ndarray or tensor).
        Returns the frame's loss (NaN when every label is 255).  Labels outside [0, K) and not 255 raise ValueError, as torch's
        cross_entropy does, and then leave `metric` unchanged.
        With MODEL.VALIDATE_BATCH = True also a batch: image_in [N, h, w, 3] with label [N, h, w] ([1, h, w, 3] is a batch of one) ->
        one forward of the batch-N plan and one fused pass over the batch; the loss is the mean over every counted pixel of the
        batch (reduction='mean'), and an invalid label in any image raises and leaves `metric` unchanged.  Without it (the default)
        anything but one image raises NotImplementedError, as it always has."""
        if image_in.ndim != 3 and not self.validate_batch:
            raise NotImplementedError("validate_step takes one image [h, w, 3], not shape %s (MODEL.VALIDATE_BATCH = True lets it take a "
                                      "batch [N, h, w, 3])" % (tuple(image_in.shape),))
        n, h, w = self._geometry(image_in)
        head = self._full_res(h, w, n)
        head.gt.copy_(self._label_u8(label, h, w, n), non_blocking=True)
        net = self.net_for(h, w, batch=n or 1)
        net.forward(image_in[0] if n == 1 else image_in)
        logits = net.logits.unsqueeze(0) if n == 1 else net.logits
        return self._eval_into(head, logits, h, w, metric)

    def validate_step_tensor(self, x, label, metric=None):
        """validate_step on the reference's own input: x = normalised float [N, 3, h, w] (forward_tensor's) with label [N, h, w], or
        one image [3, h, w] with [h, w].  One forward of the "f32_nchw" plan and one fused pass over the batch; returns the batch loss."""
        unbatched, n, h, w = self._tensor_geometry(x)
        head = self._full_res(h, w, None if unbatched else n)
        head.gt.copy_(self._label_u8(label, h, w, None if unbatched else n), non_blocking=True)
        logits = self._run_tensor(x)[0]
        return self._eval_into(head, logits[0] if unbatched else logits, h, w, metric)

    def _eval_into(self, head, logits, h, w, metric):
        """the fused pass of validate_step: head.gt against `logits`; the counts go to `metric` only after the labels' check"""
        if metric is not None:
            if metric.num_class != self.num_classes:
                raise ValueError("the metric counts %d classes, the network has %d" % (metric.num_class, self.num_classes))
            head.confusion.zero_()
        seg_head.full_res_eval(logits, h, w, gt=head.gt, confusion=head.confusion if metric is not None else None,
                               workspace=head.workspace)
        res = head.workspace.result()
        if res["invalid"]:
            raise ValueError("%d label values are outside [0, %d) and not %d (the ignore index)"
                             % (res["invalid"], self.num_classes, seg_head.IGNORE_INDEX))
        if metric is not None:
            metric.add_confusion(head.confusion)
        return res["loss"]

    def _label_u8(self, label, h, w, n=None):
        """ground truth [h, w] ([n, h, w] for a batch of n) (int64 / uint8 ndarray or tensor) -> uint8 tensor; values that uint8 cannot
        hold raise ValueError"""
        t = label if isinstance(label, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(label))
        if n is None and tuple(t.shape) != (h, w):
            raise ValueError("label has shape %s, the image is %d x %d" % (tuple(t.shape), h, w))
        if n is not None and tuple(t.shape) != (n, h, w):
            raise ValueError("label has shape %s, the batch is %d images of %d x %d" % (tuple(t.shape), n, h, w))
        if t.dtype == torch.uint8:
            return t
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
            raise ValueError("label must hold integers, not %s" % t.dtype)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
            raise ValueError("label values outside [0, %d) and not %d (the ignore index): range [%d, %d]"
                             % (self.num_classes, seg_head.IGNORE_INDEX, int(t.min()), int(t.max())))
        return t.to(torch.uint8)

    def _full_res(self, h, w, n=None):
        """the buffers of the full-resolution paths for an h x w input, or a batch of n (made on first use, kept per size and batch)"""
        key = (int(h), int(w)) + (() if n is None else (int(n),))
        head = self._heads.get(key)
        if head is None:
            head = _FullResBuffers(self.device, h, w, self.num_classes, n)
            self._heads[key] = head
        return head


class _FullResBuffers(object):
    def __init__(self, device, h, w, num_classes, n=None):
        lead = () if n is None else (n,)   # a batch of n: validate_step's buffers only (its labels / logits outputs: _batch_buffer)
        self.logits = None                 # fp32 [K, h, w], allocated by the first logits(upsample_pred=True)
        self.labels = torch.empty((h, w), dtype=torch.uint8, device=device) if n is None else None
        self.gt = torch.empty(lead + (h, w), dtype=torch.uint8, device=device)
        self.confusion = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)
        self.workspace = seg_head.EvalWorkspace(h, w, device, batch=n or 1)
