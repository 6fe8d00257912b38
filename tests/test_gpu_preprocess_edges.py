"""Camera pre-processing on the GPU against float64, at the zero border, with k3 != 0 and at odd scales (tests/_preprocess_reference.py;
its inputs and its bar are checked without a GPU in tests/test_preprocess_reference_cpu.py).

* k_preprocess (preprocess_device) at factor 1: every byte within 0.5 + delta of the float64 undistortion, for three synthetic cameras
  with k3 != 0 whose samples leave the frame on all four sides, on full-range noise.  Factors 2, 3, 4: the integer area mean of the GPU's
  own undistorted bytes, bit for bit.
* k_preprocess_area (preprocess_area_device): oracle/preprocess_oracle.resize_area of the GPU's own undistorted bytes, bit for bit, at
  (H - 1, W - 1), (1, 1), (1, W // 2), an integer ratio, the node's sizes for IMAGE_SCALE = 1 / 3 on 97 x 131, and three size pairs
  on which W / OW and OpenCV's 1. / (OW / W) put a ceil / floor edge elsewhere (both give the kernel's bytes).
* the fused loaders -- k_stem_mfma<f16 | bf16, PRE>, its pooled and its split-f16 form, k_stem_pre_f32 -- on the same cameras, where black
  undistortion pixels (-mean / std after normalisation) and the stem's own padding (0) meet at every image edge: the stem's output has the
  bits of the plain stem fed k_preprocess's bytes, at factors 1, 2, 3, one frame and a raw batch of three with a camera each."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _preprocess_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = list(pr.CAMERAS)


@pytest.fixture(scope="module")
def undistorted(cuda_device):
    """{(camera or None, factor): the GPU's undistorted RGB bytes of that factor's frame at full size}, computed once each"""
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    cache = {}

    def get(name, factor):
        if (name, factor) not in cache:
            got = preprocess_device(pr.noise_frame(factor), pr.camera(name, factor), 1).cpu().numpy()
            got.setflags(write=False)
            cache[(name, factor)] = got
        return cache[(name, factor)]
    return get


# ------------------------------------------------------------------------------------------------ k_preprocess
@pytest.mark.parametrize("factor", list(pr.RAW))
@pytest.mark.parametrize("name", NAMES)
def test_undistortion_is_within_the_bar_of_float64(name, factor, undistorted):
    """measured on an MI355X at 67 x 83: max|got - E| - 0.5 = -1.2e-4 (pincushion), 2.0e-4 (barrel), -5.2e-5 (off-centre) of a delta of
    4.1e-3 / 3.2e-3 / 4.1e-3; at 271 x 335 at most 3.2e-3 of 1.6e-2"""
    cam = pr.camera(name, factor)
    rgb = pr.noise_frame(factor)[:, :, ::-1]
    E, sx, sy = pr.exact_undistort(rgb, cam.K, cam.dist)
    bar = pr.bar(sx, sy)
    got = undistorted(name, factor)
    assert got.shape == rgb.shape and got.dtype == np.uint8
    print("%s, %d x %d: max|got - E| - 0.5 = %.2e (delta %.2e), %.5f of the bytes differ from rint(E)"
          % (name, rgb.shape[0], rgb.shape[1], pr.excess(got, E), bar - 0.5, float((got != pr.to_bytes(E)).mean())))
    assert np.abs(got.astype(np.float64) - E).max() <= bar               # every pixel and channel


@pytest.mark.parametrize("factor", list(pr.RAW))
def test_no_camera_is_the_channel_swap(factor, undistorted):
    assert np.array_equal(undistorted(None, factor), pr.noise_frame(factor)[:, :, ::-1])


@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("name", NAMES + [None])
def test_integer_factor_is_the_area_mean_of_the_gpus_own_undistortion(name, factor, undistorted):
    """integer arithmetic on bytes: no tolerance"""
    from oracle import preprocess_oracle as po
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    got = preprocess_device(pr.noise_frame(factor), pr.camera(name, factor), factor).cpu().numpy()
    want = po.resize_area_int(undistorted(name, factor), factor)
    assert got.shape == want.shape == (pr.NET_H, pr.NET_W, 3)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ k_preprocess_area
def _area_frame(h, w):
    return np.random.default_rng(100 * h + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# (frame rows, frame columns, output rows, output columns)
AREA_CASES = [
    (67, 83, 66, 82), (67, 83, 1, 1), (67, 83, 1, 41),                  # barely above 1 (every cell partial), one cell, one row
    (97, 131, 96, 130), (97, 131, 1, 1), (97, 131, 1, 65),
    (96, 129, 32, 43),                                                  # an exact integer ratio through the general entry point
    (97, 131, 32, 43),                                                  # what the node sends for IMAGE_SCALE = 1 / 3: 97 % 3 != 0
    (27, 22, 21, 18), (39, 26, 15, 10), (34, 34, 12, 12),               # both axes: a cell edge moves between the two scale expressions
]


@pytest.mark.parametrize("case", AREA_CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_area_resize_without_a_camera(case):
    from oracle import preprocess_oracle as po
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_area_device
    h, w, oh, ow = case
    bgr = _area_frame(h, w)
    got = preprocess_area_device(bgr, None, oh, ow).cpu().numpy()
    assert np.array_equal(got, po.preprocess_area(bgr, None, None, oh, ow))
    # the kernel's W / OW and OpenCV's 1. / (OW / W) give these bytes
    rgb = np.ascontiguousarray(bgr[:, :, ::-1])
    assert np.array_equal(got, pr.resize_area_with(rgb, oh, ow, pr.scale_plain))
    assert np.array_equal(got, pr.resize_area_with(rgb, oh, ow, pr.scale_opencv))


@pytest.mark.parametrize("name", ["pincushion", "offcentre"])
@pytest.mark.parametrize("case", AREA_CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_area_resize_of_the_gpus_own_undistortion(case, name):
    from oracle import preprocess_oracle as po
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_area_device, preprocess_device
    h, w, oh, ow = case
    bgr = _area_frame(h, w)
    cam = pr.camera(name, size=(h, w))
    own = preprocess_device(bgr, cam, 1).cpu().numpy()
    rgb = bgr[:, :, ::-1]
    E, sx, sy = pr.exact_undistort(rgb, cam.K, cam.dist)
    assert np.abs(own.astype(np.float64) - E).max() <= pr.bar(sx, sy)
    assert not np.array_equal(own, rgb)
    got = preprocess_area_device(bgr, cam, oh, ow).cpu().numpy()
    assert np.array_equal(got, po.resize_area(own, oh, ow))


# ------------------------------------------------------------------------------------------------ the fused loaders
KINDS = {
    "f16": dict(precision="f16", fuse_passes=False),                    # k_stem_mfma<f16, PRE>
    "bf16": dict(precision="bf16", fuse_passes=False),                  # k_stem_mfma<bf16, PRE>
    "f16_pooled": dict(precision="f16"),                                # ... with the max-pool in its epilogue
    "bf16_pooled": dict(precision="bf16"),
    "split16": dict(precision="mixed", full_split=True),                # the split-f16 form: hi and lo planes
    "f32": dict(precision="f32"),                                       # k_stem_pre_f32
}
STEM_CAMERAS = ["pincushion", None, "offcentre"]


@pytest.fixture(scope="module")
def state():
    from vision_semantic_segmentation_amd.network import random_state_dict
    return random_state_dict(0)


@pytest.fixture(scope="module")
def plain_nets(state, cuda_device):
    """{kind: the plain 67 x 83 plan}, built once"""
    from vision_semantic_segmentation_amd.network import SegNet
    nets = {}

    def get(kind):
        if kind not in nets:
            nets[kind] = SegNet(state, pr.NET_H, pr.NET_W, device=cuda_device, **KINDS[kind])
        return nets[kind]
    return get


def _stem_planes(net):
    """the bits of what the stem (op 0) wrote, after run_prefix(1): [images, pixels, 64] integer tensors, the hi plane and, where the
    plan has one, the lo plane"""
    import torch
    from vision_semantic_segmentation_amd import _lib
    op = net.ops[0]
    pixels, cols = op.out_h * op.out_w, op.out_c
    dt = torch.float32 if op.dtype == _lib.AVL_F32 else net.act_dtype
    bits = torch.int32 if dt == torch.float32 else torch.int16
    planes = []
    for ptr in (op.out, op.out_lo):
        if not ptr:
            continue
        for t in net._keep:
            lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
            if lo <= ptr < hi:
                flat = t.reshape(-1).view(torch.uint8)[ptr - lo:].view(dt)
                assert flat.numel() >= (net.batch * pixels - 1) * op.out_ld + cols
                rows = torch.as_strided(flat, (net.batch * pixels, cols), (op.out_ld, 1)).contiguous()
                planes.append(rows.view(bits).view(net.batch, pixels, cols).cpu())
                break
        else:
            raise KeyError("the stem's output pointer is not in the plan's buffers")
    return planes


def _run_stem(net, image):
    import torch
    net.image.copy_(torch.from_numpy(np.ascontiguousarray(image)).to(net.device) if isinstance(image, np.ndarray) else image)
    net.run_prefix(1)
    return _stem_planes(net)


@pytest.mark.parametrize("factor", [1, 2, 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_loader_has_the_bits_of_k_preprocess_and_the_plain_stem(kind, factor, state, plain_nets, cuda_device):
    import torch
    from vision_semantic_segmentation_amd.network import OP_STEM, SegNet
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import preprocess_device
    raw = pr.RAW[factor]
    plain = plain_nets(kind)
    one = SegNet(state, pr.NET_H, pr.NET_W, device=cuda_device, raw_frame=raw, **KINDS[kind])
    many = SegNet(state, pr.NET_H, pr.NET_W, device=cuda_device, raw_frame=raw, batch=3, raw_batch=True, **KINDS[kind])
    pooled = kind.endswith("_pooled")
    for net in (plain, one, many):
        op = net.ops[0]
        assert op.kind == OP_STEM and net.op_names[0] == ("backbone.conv1+maxpool" if pooled else "backbone.conv1")
        assert bool(op.in2) == (net is not plain) and bool(op.out_lo) == (kind == "split16") and op.w_layout == (0 if kind == "f32" else 1)
    assert many.ops[0].raw_batch == 1 and many.ops[0].batch == 3
    frames = [pr.noise_frame(factor, seed=v) for v in range(3)]
    cams = [pr.camera(name, factor) for name in STEM_CAMERAS]
    want = []
    for v, (frame, cam) in enumerate(zip(frames, cams)):
        K, dist = (None, None) if cam is None else (cam.K, cam.dist)
        ref = _run_stem(plain, preprocess_device(frame, cam, factor))             # k_preprocess's bytes -> the plain stem
        one.set_camera(K, dist)
        got = _run_stem(one, frame)
        assert len(got) == len(ref) == (2 if kind == "split16" else 1)
        for g, r in zip(got, ref):
            assert g.shape == r.shape and torch.equal(g, r), (kind, factor, STEM_CAMERAS[v])
        assert bool((ref[0] != 0).any())
        many.set_camera(K, dist, image=v)
        want.append(ref)
    # the camera moved content: frame 0 without one gives other bits
    one.set_camera(None, None)
    assert not torch.equal(_run_stem(one, frames[0])[0], want[0][0])
    # one raw batch of three frames, cameras [pincushion, none, off-centre]: each image equals its one-frame plan
    got = _run_stem(many, np.stack(frames))
    for v in range(3):
        for g, r in zip(got, want[v]):
            assert torch.equal(g[v], r[0]), (kind, factor, "image %d of the batch" % v)
