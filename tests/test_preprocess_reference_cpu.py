"""What tests/test_gpu_preprocess_edges.py stands on, without a GPU (tests/_preprocess_reference.py):

* the inputs test something: over the synthetic cameras every side of the frame has half-outside taps (x0 == -1, x0 == W - 1, y0 == -1,
  y0 == H - 1), one camera leaves 10-35 % of its pixels fully outside, every camera has k3 != 0, and a kernel that drops k3, swaps p1 and
  p2 or uses cv2.remap's 5-bit weights misses the bar on at least a fifth of the bytes, on every frame and camera;
* the bar holds for what it was made for: the NumPy restatement (oracle/preprocess_oracle.undistort) and the float64 evaluation at
  float32 parameters with a float32 map stay within it on every frame and camera;
* INTER_AREA's scale expression: W / OW against OpenCV's 1. / (OW / W) over every size pair up to 512 and every output size of a
  1440 and a 1920 axis -- the two move ceil / floor edges on 11490 pairs and change no byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _preprocess_reference as pr  # noqa: E402

NAMES = list(pr.CAMERAS)
CASES = [(name, f) for name in NAMES for f in pr.RAW]


@pytest.fixture(scope="module")
def exact():
    """{(camera, factor): (rgb, E, sx, sy, bar)}, computed once"""
    out = {}
    for name, f in CASES:
        cam = pr.camera(name, f)
        rgb = np.ascontiguousarray(pr.noise_frame(f)[:, :, ::-1])
        E, sx, sy = pr.exact_undistort(rgb, cam.K, cam.dist)
        out[(name, f)] = (rgb, E, sx, sy, pr.bar(sx, sy))
    return out


def _missed(real, E, bar):
    """share of the bytes of a kernel computing `real` that the bar refuses"""
    return float((np.abs(pr.to_bytes(real).astype(np.float64) - E) > bar).mean())


def test_frames_and_cameras_are_what_the_issue_names():
    assert pr.RAW == {1: (67, 83), 2: (135, 167), 3: (203, 251), 4: (271, 335)}
    for f, (h, w) in pr.RAW.items():
        assert (h // f, w // f) == (pr.NET_H, pr.NET_W) and (f == 1 or (h % f and w % f))
        frame = pr.noise_frame(f)
        assert frame.dtype == np.uint8 and frame.shape == (h, w, 3) and frame.min() == 0 and frame.max() == 255
    assert len(NAMES) >= 3
    for name in NAMES:
        k1, k2, p1, p2, k3 = pr.camera(name).dist
        assert k3 != 0 and p1 != 0 and p2 != 0, name
    k1, k2, p1, p2, k3 = pr.camera("pincushion").dist
    assert k1 > 0 and k2 < 0
    b1, b2, _, _, b3 = pr.camera("barrel").dist
    assert b1 < 0 and b2 > 0 and np.sign(b3) == -np.sign(k3)
    K = pr.camera("offcentre").K
    assert K[0, 2] < 0 and 0 <= K[1, 2] < pr.NET_H                      # the principal point: outside on x, inside on y
    # K scales with the frame as Camera.scaled does it
    from vision_semantic_segmentation_amd.camera import Camera
    ref = Camera(pr.camera("barrel").K, np.eye(3), np.zeros((3, 1)), dist=pr.camera("barrel").dist).scaled(251 / 83.0, 203 / 67.0)
    assert np.array_equal(ref.K, pr.camera("barrel", 3).K) and np.array_equal(ref.dist, pr.camera("barrel", 3).dist)


@pytest.mark.parametrize("factor", list(pr.RAW))
def test_the_zero_border_is_reached_on_all_four_sides(exact, factor):
    h, w = pr.RAW[factor]
    total = {"left": 0, "right": 0, "top": 0, "bottom": 0}
    shares = {}
    for name in NAMES:
        _, _, sx, sy, _ = exact[(name, factor)]
        for side, n in pr.half_outside_counts(sx, sy, h, w).items():
            total[side] += n
        shares[name] = pr.outside_share(sx, sy, h, w)
    print("factor %d: half-outside taps %s, fully outside %s" % (factor, total, {k: round(v, 3) for k, v in shares.items()}))
    assert all(n >= 20 for n in total.values()), total
    assert any(0.10 <= s <= 0.35 for s in shares.values()), shares
    # on the cameras the fused-loader tests use, black source pixels meet the stem's padding at every image edge
    # (a black pixel, -mean / std after normalisation, next to the padding's 0): the pincushion camera on all four edges; the
    # off-centre one has sampled pixels on two of them, the barrel camera and "no undistortion" on all
    for name in ("pincushion", "offcentre"):
        black = (exact[(name, factor)][1] == 0).all(axis=2)
        black_on = [int(line.sum()) for line in (black[0], black[-1], black[:, 0], black[:, -1])]
        print("factor %d, %s: black pixels on the image's top, bottom, left, right edge: %s" % (factor, name, black_on))
        assert min(black_on) >= 20 or name != "pincushion"
        assert max(black_on) >= 20


@pytest.mark.parametrize("name,factor", CASES)
def test_a_subtly_wrong_kernel_misses_the_bar(exact, name, factor):
    rgb, E, _, _, bar = exact[(name, factor)]
    cam = pr.camera(name, factor)
    k1, k2, p1, p2, k3 = cam.dist
    shares = {
        "k3 = 0": _missed(pr.model_undistort(rgb, cam.K, cam.with_dist(k3=0.0).dist), E, bar),
        "p1 <-> p2": _missed(pr.model_undistort(rgb, cam.K, cam.with_dist(p1=p2, p2=p1).dist), E, bar),
        "5-bit weights": _missed(pr.model_undistort(rgb, cam.K, cam.dist, weight_bits=5), E, bar),
    }
    cast = _missed(pr.model_undistort(rgb, cam.K, cam.dist, cast=True), E, bar)
    print("%s x %d: bytes beyond the bar: %s, (int) for floorf %.4f" % (name, factor, {k: round(v, 3) for k, v in shares.items()}, cast))
    for what, share in shares.items():
        assert share >= 0.20, (what, share)
    if name != "barrel":                       # (the barrel camera samples inside the frame only: no negative coordinate)
        assert cast > 0


@pytest.mark.parametrize("name,factor", CASES)
def test_restatement_and_float32_model_stay_within_the_bar(exact, name, factor):
    from oracle import preprocess_oracle as po
    rgb, E, sx, sy, bar = exact[(name, factor)]
    cam = pr.camera(name, factor)
    assert 0.5 < bar < 0.5 + 2e-2
    if factor == 1:
        assert bar < 0.5 + 5e-3
    restated = po.undistort(rgb, cam.K, cam.dist)
    model = pr.model_undistort(rgb, cam.K, cam.dist, f32=True)
    print("%s x %d: delta %.2e; restatement max|got - E| - 0.5 = %.2e, %.4f of its bytes differ from rint(E); float32 model |M - E| <= %.2e"
          % (name, factor, bar - 0.5, pr.excess(restated, E), float((restated != pr.to_bytes(E)).mean()), float(np.abs(model - E).max())))
    assert restated.dtype == np.uint8 and np.abs(restated.astype(np.float64) - E).max() <= bar
    assert np.abs(model - E).max() <= bar - 0.5                          # the real-valued model: within delta before rounding
    assert np.abs(pr.to_bytes(model).astype(np.float64) - E).max() <= bar
    # preprocess() is the channel swap, the restatement and the integer area mean
    bgr = pr.noise_frame(factor)
    assert np.array_equal(po.preprocess(bgr, cam.K, cam.dist, factor), po.resize_area_int(restated, factor) if factor > 1 else restated)


def test_area_table_arrays_are_the_restatements_table():
    from oracle import preprocess_oracle as po
    for ssize, dsize in [(11, 9), (13, 5), (17, 6), (22, 18), (26, 10), (34, 12), (131, 98), (97, 72), (129, 43), (83, 1), (1920, 1151)]:
        mine = pr.table_entries(pr.area_axis_table(dsize, ssize, pr.scale_plain(ssize, dsize)))
        theirs = po._area_table(dsize, ssize)
        assert len(mine) == len(theirs) == dsize
        for a, b in zip(mine, theirs):
            assert [(i, float(w)) for i, w in a] == [(i, float(w)) for i, w in b], (ssize, dsize)
    img = np.random.default_rng(3).integers(0, 256, size=(27, 22, 3), dtype=np.uint8)
    for oh, ow in ((21, 18), (1, 1), (26, 21), (9, 11)):
        assert np.array_equal(pr.resize_area_with(img, oh, ow, pr.scale_plain), po.resize_area(img, oh, ow)), (oh, ow)


# size pairs whose ceil / floor edges differ between the two expressions (found by the enumeration below): the GPU cases
EDGE_PAIRS = [(22, 18), (26, 10), (34, 12), (27, 21), (39, 15)]


def test_scale_expression_changes_no_byte():
    """ADVICE.md (round 5) on k_preprocess_area: scale = W / OW, where OpenCV has 1. / ((double)OW / W).  Every (ssize, dsize) with
    ssize <= 512 and every dsize of a 1440 and a 1920 axis: the table is built with both and a noise row is reduced with each.  (Where the
    two scales are the same double, or give the same table, there is one table and nothing to compare.)  The expressions differ on a
    quarter of the pairs and move a cell edge on 11490 of them -- f1 lands a few 1e-14 beside an integer, so ceil / floor step -- but
    the weight that appears there is below the 1e-3 that computeResizeAreaTab drops, or the whole-pixel weight 1 / cell under another
    name: the bytes are equal everywhere."""
    row = np.random.default_rng(5).integers(0, 256, size=1920, dtype=np.uint8)
    pairs = [(s, d) for s in range(1, 513) for d in range(1, s + 1)] + [(s, d) for s in (1440, 1920) for d in range(1, s + 1)]
    scale_differs, edges_differ, bytes_differ = 0, [], []
    for ssize, dsize in pairs:
        a, b = pr.scale_plain(ssize, dsize), pr.scale_opencv(ssize, dsize)
        if a == b:
            continue
        scale_differs += 1
        ta, tb = pr.area_axis_table(dsize, ssize, a), pr.area_axis_table(dsize, ssize, b)
        if all(np.array_equal(x, y) for x, y in zip(ta, tb)):
            continue
        if not (np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])):
            edges_differ.append((ssize, dsize))
        if not np.array_equal(pr.reduce_row(row[:ssize], ta), pr.reduce_row(row[:ssize], tb)):
            bytes_differ.append((ssize, dsize))
    print("%d pairs: the scale differs on %d, a ceil / floor edge on %d, a byte on %d" % (len(pairs), scale_differs, len(edges_differ), len(bytes_differ)))
    assert len(pairs) == 512 * 513 // 2 + 1440 + 1920 and scale_differs > 0
    assert not bytes_differ, bytes_differ[:10]
    assert set(EDGE_PAIRS) <= set(edges_differ)
    # in two dimensions, at the GPU test's sizes
    for (h, oh), (w, ow) in (((27, 21), (22, 18)), ((39, 15), (26, 10)), ((34, 12), (34, 12))):
        img = np.random.default_rng(h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        assert np.array_equal(pr.resize_area_with(img, oh, ow, pr.scale_plain), pr.resize_area_with(img, oh, ow, pr.scale_opencv))


def test_the_node_sends_a_third_of_97_x_131_through_the_general_resize():
    """image_callback's arithmetic for IMAGE_SCALE = 1 / 3: 96 x 129 shrinks by the integer factor, 97 x 131 goes to the general area
    resize as 32 x 43 (a GPU case of tests/test_gpu_preprocess_edges.py)"""
    import types
    from vision_semantic_segmentation_amd.config import get_cfg_defaults
    from vision_semantic_segmentation_amd.vision_semantic_segmentation_node import VisionSemanticSegmentationNode
    cfg = get_cfg_defaults()
    cfg.VISION_SEM_SEG.IMAGE_SCALE = 1.0 / 3.0
    node = VisionSemanticSegmentationNode(cfg, seg=types.SimpleNamespace(), undistort=False)
    assert node._downscale_factor(96, 129) == 3 and node._downscale_factor(97, 131) is None
    assert (int(97 * node.image_scale), int(131 * node.image_scale)) == (32, 43)
