"""Batched raw-frame plans on the GPU (SegNet(raw_frame=..., batch=V, raw_batch=True), avl_seg_op.raw_batch): the three pre-processing
stems take the image index from blockIdx.z and every image reads its own camera block.  Everything here is bit-equality:

* per image, the batched plan's logits and labels are those of the one-frame raw plan on that frame with that camera, for every plan
  kind, V = 2 and 3, factors 1, 2 and 3 (with remainder rows), camera1, camera6 and no undistortion mixed in one batch;
* and those of the stand-alone pair (avl_preprocess_image per view -> the plain batch = V plan), what the node did before;
* at the camera's own 1440 x 1920 through SemanticSegmentation;
* camera blocks are per image and stream-ordered on a captured plan;
* the last image's offsets and the ranges the stem reads (guard bytes around the input);
* the node's image_callback_views and the self-check's fall-back to fp32 use the batched raw plan."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = {
    "f32": dict(precision="f32"),
    "f16": dict(precision="f16"),
    "bf16": dict(precision="bf16"),
    "mixed": dict(precision="mixed"),
    "split16": dict(precision="mixed", full_split=True),
}
NET_H, NET_W = 96, 128
# factor -> raw frame size; 290 x 386 / 3 -> 96 x 128 leaves 2 remainder rows and 2 remainder columns
RAW = {1: (96, 128), 2: (192, 256), 3: (290, 386)}


@pytest.fixture(scope="module")
def state():
    from vision_semantic_segmentation_amd.network import random_state_dict
    return random_state_dict(0)


def _structured(rng, h, w, cell=8):
    """a camera-like frame: flat patches of `cell` pixels plus a little noise, so that undistortion moves visible edges and two
    draws do not look alike"""
    coarse = rng.integers(0, 256, size=((h + cell - 1) // cell, (w + cell - 1) // cell, 3), dtype=np.uint8)
    bgr = np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:h, :w]
    return (bgr.astype(np.int32) + rng.integers(-8, 9, size=bgr.shape)).clip(0, 255).astype(np.uint8)


def _cameras(h, w):
    """camera1's and camera6's models brought to an h x w frame (their own size is 1440 x 1920), and no undistortion"""
    from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6
    return [camera_setup_1().scaled(w / 1920.0, h / 1440.0), camera_setup_6().scaled(w / 1920.0, h / 1440.0), None]


def _kd(cam):
    return (None, None) if cam is None else (cam.K, cam.dist)


def _overflowing_state(base):
    """layer2.1: bn1's scale x 1e5 (conv1's output reaches ~5e5 > 65504 = f16 max; fp32 does not care), undone exactly by dividing the
    3x3's weights by 1e5 (conv2 is linear in its input and ReLU commutes with a positive scale, bn1's bias scaled too)"""
    st = {k: v.clone() for k, v in base.items()}
    st["backbone.layer2.1.bn1.weight"] = st["backbone.layer2.1.bn1.weight"] * 1.0e5
    st["backbone.layer2.1.bn1.bias"] = st["backbone.layer2.1.bn1.bias"] * 1.0e5
    st["backbone.layer2.1.conv2.weight"] = st["backbone.layer2.1.conv2.weight"] / 1.0e5
    return st


def _one_frame_results(one, frames, cams):
    """[(logits, labels)] of the one-frame raw plan `one` on each frame with its camera"""
    import torch
    out = []
    for f, cam in zip(frames, cams):
        one.set_camera(*_kd(cam))
        one.forward(torch.from_numpy(f).to(one.device))
        torch.cuda.synchronize()
        out.append((one.logits.clone(), one.labels.clone()))
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_each_image_has_the_bits_of_the_one_frame_raw_plan(kind, state, cuda_device):
    import torch
    from vision_semantic_segmentation_amd.network import OP_STEM, SegNet
    rng = np.random.default_rng(41)
    for factor, raw in RAW.items():
        all_cams = _cameras(*raw)
        one = SegNet(state, NET_H, NET_W, device=cuda_device, raw_frame=raw, **KINDS[kind])
        for V, cams in ((2, [all_cams[1], all_cams[2]]), (3, [all_cams[0], all_cams[1], all_cams[2]])):
            frames = [_structured(rng, *raw) for _ in range(V)]
            want = _one_frame_results(one, frames, cams)
            assert not torch.equal(want[0][0], want[1][0])                       # two views do not look alike
            net = SegNet(state, NET_H, NET_W, device=cuda_device, raw_frame=raw, batch=V, raw_batch=True, **KINDS[kind])
            assert net.ops[0].kind == OP_STEM and net.ops[0].in2 and net.ops[0].raw_batch == 1 and net.ops[0].batch == V
            for v, cam in enumerate(cams):
                net.set_camera(*_kd(cam), image=v)
            labels = net.forward(torch.from_numpy(np.stack(frames)).to(cuda_device))
            torch.cuda.synchronize()
            assert tuple(labels.shape) == (V, net.out_h, net.out_w)
            for v in range(V):
                assert torch.equal(net.logits[v], want[v][0]), (kind, factor, V, v)
                assert torch.equal(net.labels[v], want[v][1]), (kind, factor, V, v)
            del net
        # the undistortion moved content: the same frame without a camera gives other logits
        one.set_camera(None, None)
        one.forward(torch.from_numpy(frames[0]).to(cuda_device))
        assert not torch.equal(one.logits, want[0][0]), (kind, factor)
        del one
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["f16", "f32"])
def test_same_bits_as_the_stand_alone_pair(kind, state, cuda_device):
    """avl_preprocess_image per view -> the plain batch = V plan: what image_callback_views ran before"""
    import torch
    from vision_semantic_segmentation_amd.network import SegNet
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    rng = np.random.default_rng(43)
    V, factor = 3, 2
    raw = RAW[factor]
    cams = _cameras(*raw)
    frames = [_structured(rng, *raw) for _ in range(V)]
    plain = SegNet(state, NET_H, NET_W, device=cuda_device, batch=V, **KINDS[kind])
    rgb = torch.stack([preprocess_device(f, cam, factor) for f, cam in zip(frames, cams)])
    assert tuple(rgb.shape) == (V, NET_H, NET_W, 3)
    plain.forward(rgb)
    net = SegNet(state, NET_H, NET_W, device=cuda_device, raw_frame=raw, batch=V, raw_batch=True, **KINDS[kind])
    for v, cam in enumerate(cams):
        net.set_camera(*_kd(cam), image=v)
    net.forward(torch.from_numpy(np.stack(frames)).to(cuda_device))
    torch.cuda.synchronize()
    assert torch.equal(net.logits, plain.logits) and torch.equal(net.labels, plain.labels)
    # image = None writes every block: one camera for all
    net.set_camera(*_kd(cams[0]))
    net.forward()
    plain.forward(torch.stack([preprocess_device(f, cams[0], factor) for f in frames]))
    torch.cuda.synchronize()
    assert torch.equal(net.logits, plain.logits)


def test_camera_sized_frames_through_semantic_segmentation(state, cuda_device):
    """1440 x 1920, IMAGE_SCALE 0.5, camera1 + camera6, the default ("mixed") precision on captured plans"""
    import torch
    from vision_semantic_segmentation_amd import SemanticSegmentation
    from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_network_cfg_defaults()
    assert cfg.MODEL.PRECISION == "mixed"
    seg = SemanticSegmentation(cfg, device=cuda_device, state_dict=state)
    rng = np.random.default_rng(47)
    cams = [camera_setup_1(), camera_setup_6()]
    frames = [_structured(rng, 1440, 1920, cell=32) for _ in cams]
    want = []
    for f, cam in zip(frames, cams):
        labels = seg.segmentation_device_raw(f, cam.K, cam.dist, 2)
        want.append((seg.net_for(720, 960, raw_frame=(1440, 1920)).logits.clone(), labels.clone()))
    got = seg.segmentation_device_raw_batch(frames, [c.K for c in cams], [c.dist for c in cams], 2)       # a list: copied frame by frame
    net = seg.net_for(720, 960, raw_frame=(1440, 1920), batch=2, raw_batch=True)
    assert net is seg._nets[(720, 960, 2, 1440, 1920, "raw_batch")] and getattr(net, "graphed", False)
    assert (720, 960, 2) not in seg._nets and tuple(got.shape) == (2, net.out_h, net.out_w)
    for v in range(2):
        assert torch.equal(net.logits[v], want[v][0]) and torch.equal(got[v], want[v][1]), v
    got4 = seg.segmentation_device_raw_batch(np.stack(frames), [c.K for c in cams], [c.dist for c in cams], 2)     # ... and as one array
    assert torch.equal(got4, torch.stack([w[1] for w in want]))
    del net
    seg._nets.clear()
    torch.cuda.empty_cache()


def test_cameras_are_per_image_and_stream_ordered_on_a_captured_plan(state, cuda_device):
    import torch
    from vision_semantic_segmentation_amd.network import SegNet
    rng = np.random.default_rng(53)
    raw = RAW[2]
    cam1, cam6, _ = _cameras(*raw)
    frames = [_structured(rng, *raw) for _ in range(2)]
    net = SegNet(state, NET_H, NET_W, device=cuda_device, raw_frame=raw, batch=2, raw_batch=True, precision="f16")
    net.capture_graph()
    net.set_camera(*_kd(cam1), image=0)
    net.set_camera(*_kd(cam1), image=1)
    net.forward(torch.from_numpy(np.stack(frames)).to(cuda_device))
    first = net.logits.clone()
    net.set_camera(*_kd(cam6), image=1)                   # between two replays: image 1's camera only
    net.forward()
    second = net.logits.clone()
    torch.cuda.synchronize()
    assert torch.equal(first[0], second[0])
    assert not torch.equal(first[1], second[1])
    one = SegNet(state, NET_H, NET_W, device=cuda_device, raw_frame=raw, precision="f16")
    want = _one_frame_results(one, [frames[1], frames[1], frames[0]], [cam1, cam6, cam1])
    assert torch.equal(first[1], want[0][0]) and torch.equal(second[1], want[1][0]) and torch.equal(first[0], want[2][0])


@pytest.mark.parametrize("kind", ["f16", "split16", "f32"])
def test_last_image_offsets_and_nothing_outside_the_batch_is_read(kind, state, cuda_device):
    """The last image carries its content at the frame's last row and column; the input sits between guard bytes (the stem op is
    pointed at a buffer of the test's own), and two runs with different guards give the same bits."""
    import torch
    from vision_semantic_segmentation_amd.network import SegNet
    rng = np.random.default_rng(59)
    V, factor = 3, 3
    raw = RAW[factor]
    cams = [None, _cameras(*raw)[1], _cameras(*raw)[0]]          # the last image is undistorted: its bilinear taps reach past the frame
    frames = [_structured(rng, *raw) for _ in range(V)]
    frames[-1][:-3] //= 8                                         # dim everywhere ...
    frames[-1][:, :-3] //= 8
    frames[-1][-3:, :, :] = 255                                   # ... but the last rows and columns
    frames[-1][:, -3:, :] = 255
    one = SegNet(state, NET_H, NET_W, device=cuda_device, raw_frame=raw, **KINDS[kind])
    want = _one_frame_results(one, frames, cams)
    net = SegNet(state, NET_H, NET_W, device=cuda_device, raw_frame=raw, batch=V, raw_batch=True, **KINDS[kind])
    for v, cam in enumerate(cams):
        net.set_camera(*_kd(cam), image=v)
    nbytes, guard = V * raw[0] * raw[1] * 3, 1 << 16
    assert net.image.numel() == nbytes
    results = []
    for sentinel in (0, 255, 0x5A):
        big = torch.full((guard + nbytes + guard,), sentinel, dtype=torch.uint8, device=cuda_device)
        big[guard:guard + nbytes].copy_(torch.from_numpy(np.stack(frames)).reshape(-1))
        net.ops[0].in_ = big.data_ptr() + guard
        net.run_prefix(len(net.ops))                              # a plan of its own from the edited op list; synchronises
        results.append((net.logits.clone(), net.labels.clone()))
        assert bool((big[:guard] == sentinel).all()) and bool((big[guard + nbytes:] == sentinel).all())
    for lg, lb in results:
        assert torch.equal(lg, results[0][0]) and torch.equal(lb, results[0][1])
        for v in range(V):
            assert torch.equal(lg[v], want[v][0]) and torch.equal(lb[v], want[v][1]), (kind, v)
    # the last image's border content reached the result
    dim = [f.copy() for f in frames]
    dim[-1][-3:, :, :] = 0
    dim[-1][:, -3:, :] = 0
    assert not torch.equal(_one_frame_results(one, dim[-1:], cams[-1:])[0][0], want[-1][0])


def _node(cuda_device, state, scale, undistort=True):
    from vision_semantic_segmentation_amd import SemanticSegmentation, VisionSemanticSegmentationNode, get_cfg_defaults
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.VISION_SEM_SEG.IMAGE_SCALE = scale
    seg = SemanticSegmentation(get_network_cfg_defaults(), device=cuda_device, state_dict=state)
    published = []
    node = VisionSemanticSegmentationNode(cfg, seg=seg, undistort=undistort, publish=lambda fid, img, header: published.append((fid, img)))
    return node, seg, published


@pytest.mark.parametrize("undistort", [True, False])
def test_node_views_use_the_batched_raw_plan(undistort, state, cuda_device):
    import torch
    from vision_semantic_segmentation_amd.utils import Header, Message
    node, seg, published = _node(cuda_device, state, 0.5, undistort)
    rng = np.random.default_rng(61)
    H, W = 240, 320
    for ids in (("camera1", "camera6"), ("camera6", "camera9", "camera1")):          # camera9: an unknown frame_id, never undistorted
        msgs = [Message(Header(frame_id=fid), data=_structured(rng, H, W)) for fid in ids]
        singles, colours = [], []
        for m in msgs:
            colours.append(node.image_callback(m))
            singles.append(node.last_labels.clone())
        if undistort:            # the cameras differ, and the unknown one is not undistorted
            probe = Message(Header(frame_id="camera9"), data=msgs[0].data)
            node.image_callback(probe)
            assert not torch.equal(node.last_labels, singles[0])
        published.clear()
        labels = node.image_callback_views(msgs)
        V = len(msgs)
        assert tuple(labels.shape)[0] == V and labels.dtype == torch.uint8 and labels.is_cuda and labels is node.last_labels
        for v in range(V):
            assert torch.equal(labels[v], singles[v]), (ids, v)
            assert published[v][0] == ids[v] and np.array_equal(published[v][1], colours[v])
        assert (H // 2, W // 2, V, H, W, "raw_batch") in seg._nets
        assert (H // 2, W // 2, V) not in seg._nets                                  # no plain batched plan, no RGB batch in between
        raw = seg._nets[(H // 2, W // 2, V, H, W, "raw_batch")]
        assert raw.ops[0].in2 and raw.ops[0].raw_batch == 1 and raw.batch == V
    assert all(len(k) > 3 for k in seg._nets)
    # one message is a batch of one
    one = node.image_callback_views(msgs[:1])
    assert tuple(one.shape) == (1,) + tuple(singles[0].shape) and torch.equal(one[0], singles[0])


def test_node_views_keep_the_area_route_for_a_non_integer_scale(state, cuda_device):
    import torch
    from vision_semantic_segmentation_amd.utils import Header, Message
    node, seg, _ = _node(cuda_device, state, 0.4)
    rng = np.random.default_rng(67)
    H, W = 240, 320
    msgs = [Message(Header(frame_id=fid), data=_structured(rng, H, W)) for fid in ("camera1", "camera6")]
    singles = []
    for m in msgs:
        node.image_callback(m)
        singles.append(node.last_labels.clone())
    labels = node.image_callback_views(msgs)
    for v in range(2):
        assert torch.equal(labels[v], singles[v])
    assert (96, 128, 2) in seg._nets and not any("raw_batch" in k for k in seg._nets)


def test_self_check_fallback_to_f32_serves_a_raw_batch(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import SemanticSegmentation
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    from vision_semantic_segmentation_amd.network import random_state_dict
    st = _overflowing_state(random_state_dict(0))
    cfg = get_network_cfg_defaults()
    cfg.MODEL.MIXED_SELF_CHECK = True
    assert cfg.MODEL.PRECISION == "mixed" and cfg.MODEL.MIXED_ON_FAIL == "f32"
    seg = SemanticSegmentation(cfg, device=cuda_device, state_dict=st)
    rng = np.random.default_rng(71)
    raw = RAW[2]
    cams = _cameras(*raw)[:2]
    frames = [_structured(rng, *raw) for _ in cams]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # ("no 16-bit plan passes": the fall-back this test is about)
        labels = seg.segmentation_device_raw_batch(frames, [c.K for c in cams], [c.dist for c in cams], 2)
    assert seg.mixed_check is not None and seg.mixed_check["rung"] == "f32" and seg.precision == "mixed"
    (key, net), = seg._nets.items()
    assert key == (NET_H, NET_W, 2) + raw + ("raw_batch",)
    assert net.precision == "f32" and net.ops[0].in2 and net.ops[0].raw_batch == 1 and net.ops[0].w_layout == 0
    cfg32 = get_network_cfg_defaults()
    cfg32.MODEL.PRECISION = "f32"
    ref = SemanticSegmentation(cfg32, device=cuda_device, state_dict=st)
    for v, (f, c) in enumerate(zip(frames, cams)):
        assert torch.equal(labels[v], ref.segmentation_device_raw(f, c.K, c.dist, 2)), v
