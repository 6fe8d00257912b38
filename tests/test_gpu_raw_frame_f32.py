"""The fp32 plan's pre-processing stem (k_stem_pre_f32, seg_stem_f32.hip): a raw camera frame runs through every precision and
every rung of the self-check's ladder.

* PRECISION f32: segmentation_device_raw gives the SAME BITS as avl_preprocess_image -> the plain fp32 plan, at the camera's
  1440 x 1920 with camera1's and camera6's distortion models on one captured plan, at factor 2, with a factor that leaves a remainder,
  and on a frame narrower than one stem tile;
* the node's default configuration on a checkpoint that overflows f16: the self-check falls back to the fp32 plan and image_callback
  keeps serving raw frames (it raised NotImplementedError before);
* a PRECISION f32 node with two cameras;
* the fused stem's time against the stand-alone pair (k_preprocess + the plain fp32 stem), printed."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cfg(precision):
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_network_cfg_defaults()
    cfg.MODEL.PRECISION = precision
    return cfg


@pytest.fixture(scope="module")
def state():
    from vision_semantic_segmentation_amd.network import random_state_dict
    return random_state_dict(0)


def _overflowing_state(base):
    """(as tests/test_gpu_robust.py) layer2.1: bn1's scale x 1e5 (conv1's output reaches ~5e5 > 65504 = f16 max; fp32 does not care),
    undone exactly by dividing the 3x3's weights by 1e5 (conv2 is linear in its input and ReLU commutes with a positive scale, bn1's bias
    scaled too)"""
    st = {k: v.clone() for k, v in base.items()}
    st["backbone.layer2.1.bn1.weight"] = st["backbone.layer2.1.bn1.weight"] * 1.0e5
    st["backbone.layer2.1.bn1.bias"] = st["backbone.layer2.1.bn1.bias"] * 1.0e5
    st["backbone.layer2.1.conv2.weight"] = st["backbone.layer2.1.conv2.weight"] / 1.0e5
    return st


def _structured(rng, h, w, cell=32):
    """a camera-like frame: flat patches of `cell` pixels plus a little noise (undistortion then moves real edges)"""
    coarse = rng.integers(0, 256, size=((h + cell - 1) // cell, (w + cell - 1) // cell, 3), dtype=np.uint8)
    bgr = np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:h, :w]
    return (bgr.astype(np.int32) + rng.integers(-8, 9, size=bgr.shape)).clip(0, 255).astype(np.uint8)


def _stem_ms(net):
    return [r["ms"] for r in net.profile() if r["kind"] == "stem"][0]


def test_f32_raw_frame_is_bit_identical_to_the_stand_alone_pair(state, cuda_device):
    import torch
    from vision_semantic_segmentation_amd import SemanticSegmentation
    from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    rng = np.random.default_rng(31)
    cam1, cam6 = camera_setup_1(), camera_setup_6()
    seg = SemanticSegmentation(_cfg("f32"), device=cuda_device, state_dict=state)

    def both(bgr, cam, factor):
        rgb = preprocess_device(bgr, cam, factor)
        want = seg.logits(rgb).clone()
        want_labels = seg.segmentation_device(rgb).clone()
        got_labels = seg.segmentation_device_raw(bgr, None if cam is None else cam.K, None if cam is None else cam.dist, factor)
        net = seg.net_for(rgb.shape[0], rgb.shape[1], raw_frame=bgr.shape[:2])
        assert net.precision == "f32" and net.ops[0].in2 and net.ops[0].w_layout == 0
        assert torch.equal(net.logits.permute(2, 0, 1), want), (bgr.shape, factor, cam is None)
        assert torch.equal(got_labels, want_labels), (bgr.shape, factor, cam is None)
        return net

    bgr = _structured(rng, 1440, 1920)
    net = both(bgr, cam1, 1)
    both(bgr, cam6, 1)                                                          # same captured plan, other camera block
    both(bgr, None, 1)                                                          # ... and no undistortion
    assert len([k for k in seg._nets if len(k) > 3]) == 1

    # (d) the fused stem against the stand-alone pair, same process, same box
    stem_fused = min(_stem_ms(net) for _ in range(5))
    stem_plain = min(_stem_ms(seg.net_for(1440, 1920)) for _ in range(5))
    t = torch.from_numpy(bgr).to(cuda_device)
    preprocess_device(t, cam1, 1)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(20):
        preprocess_device(t, cam1, 1)
    ev[1].record()
    torch.cuda.synchronize()
    pre = ev[0].elapsed_time(ev[1]) / 20
    print("1440x1920 f32, camera1: k_preprocess %.3f ms + stem %.3f ms = %.3f ms  vs  pre-processing stem %.3f ms"
          % (pre, stem_plain, pre + stem_plain, stem_fused))
    del net
    seg._nets.clear()
    torch.cuda.empty_cache()

    both(bgr, cam1, 2)                                                          # IMAGE_SCALE 0.5 -> 720 x 960
    small = _structured(rng, 487, 645, cell=8)                                  # 487 x 645 / 3 -> 162 x 215: remainder rows and columns
    both(small, cam1, 3)
    both(small, None, 2)
    narrow = rng.integers(0, 256, size=(72, 50, 3), dtype=np.uint8)             # stem output 36 x 25: narrower than one 8 x 32 tile
    both(narrow, cam6, 1)


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_self_check_fallback_to_f32_serves_raw_frames(scale, cuda_device):
    """MODEL.MIXED_ON_FAIL = "f32" (the default): a checkpoint that overflows f16 in every 16-bit plan ends on the fp32 rung, and the node
    (precision "mixed") still routes its camera frames through segmentation_device_raw."""
    from vision_semantic_segmentation_amd import SemanticSegmentation, VisionSemanticSegmentationNode, get_cfg_defaults
    from vision_semantic_segmentation_amd.network import random_state_dict
    from vision_semantic_segmentation_amd.utils import Header, Message
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    st = _overflowing_state(random_state_dict(0))
    cfg = get_cfg_defaults()
    cfg.VISION_SEM_SEG.IMAGE_SCALE = scale
    net_cfg = cfg.VISION_SEM_SEG.SEM_SEG_NETWORK
    net_cfg.MODEL.MIXED_SELF_CHECK = True
    assert net_cfg.MODEL.PRECISION == "mixed" and net_cfg.MODEL.MIXED_ON_FAIL == "f32"
    seg = SemanticSegmentation(net_cfg, device=cuda_device, state_dict=st)
    node = VisionSemanticSegmentationNode(cfg, seg=seg)
    H, W = 192, 256
    bgr = _structured(np.random.default_rng(12), H, W, cell=8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # ("no 16-bit plan passes": the fallback this test is about)
        colour = node.image_callback(Message(Header(frame_id="camera1"), data=bgr))
    assert colour.shape == (H, W, 3) and colour.dtype == np.uint8
    assert seg.mixed_check is not None and seg.mixed_check["rung"] == "f32" and seg.precision == "mixed"
    f = int(round(1 / scale))
    ref = SemanticSegmentation(_cfg("f32"), device=cuda_device, state_dict=st)
    want = ref.segmentation_device(preprocess_device(bgr, node.cam1, f)).cpu().numpy()
    assert np.array_equal(node.last_labels.cpu().numpy(), want)
    raw = [net for k, net in seg._nets.items() if len(k) > 3]
    assert len(raw) == 1 and raw[0].precision == "f32" and raw[0].ops[0].in2


def test_f32_node_with_two_cameras(state, cuda_device):
    from vision_semantic_segmentation_amd import SemanticSegmentation, VisionSemanticSegmentationNode, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils import Header, Message
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    cfg = get_cfg_defaults()
    cfg.VISION_SEM_SEG.IMAGE_SCALE = 0.5
    seg = SemanticSegmentation(_cfg("f32"), device=cuda_device, state_dict=state)
    node = VisionSemanticSegmentationNode(cfg, seg=seg)
    rng = np.random.default_rng(5)
    frames = {"camera1": _structured(rng, 240, 320, cell=8), "camera6": _structured(rng, 240, 320, cell=8)}
    for frame_id in ("camera1", "camera6", "camera1", "camera6"):
        colour = node.image_callback(Message(Header(frame_id=frame_id), data=frames[frame_id]))
        assert colour.shape == (240, 320, 3)
        cam = node.cam1 if frame_id == "camera1" else node.cam6
        want = seg.segmentation_device(preprocess_device(frames[frame_id], cam, 2)).cpu().numpy()
        assert np.array_equal(node.last_labels.cpu().numpy(), want), frame_id
    assert any(len(k) > 3 for k in seg._nets)                # the raw-frame plan served them
