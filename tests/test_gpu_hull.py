"""Semantic extraction on the GPU (csrc/seg_hull.hip) against its CPU restatement (tests/_hull_reference.py): labelling, erosion,
selection and hulls are integer results and must match exactly."""
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hull_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 97), (97, 1), (2, 2), (20, 20), (37, 53), (67, 131), (130, 259)]      # no multiple of the 64 x 16 tile; up to 9 x 5 tiles


def _hull(dev):
    from vision_semantic_segmentation_amd import semantic_convex_hull as sch
    return sch


@pytest.mark.parametrize("h,w", SIZES)
def test_labelling_matches_scipy_on_every_pattern(cuda_device, h, w):
    """erode=False: every pattern of one size as one batch of planes (class 1 of N maps); two runs are bit-identical."""
    sch = _hull(cuda_device)
    pats = ref.mask_patterns(h, w)
    names = sorted(pats)
    maps = torch.from_numpy(np.stack([pats[k] for k in names])).to(cuda_device)
    got = sch.label_components_device(maps, [1], erode=False)
    again = sch.label_components_device(maps, [1], erode=False)
    assert got.shape == (len(names), 1, h, w) and got.dtype == torch.int32
    assert torch.equal(got, again)
    got = got.cpu().numpy()
    for i, k in enumerate(names):
        want = ref.canonical_labels(pats[k] == 1)
        assert np.array_equal(got[i, 0], want), "%s at %dx%d: %d pixels differ" % (k, h, w, int((got[i, 0] != want).sum()))


def test_planes_of_several_maps_and_classes_with_erosion(cuda_device):
    """N = 3 maps x 2 classes in one call, erode=True, small-integer label maps (blobs touching every border); a 2-D input gives
    the same planes without the batch dimension."""
    sch = _hull(cuda_device)
    rng = np.random.default_rng(11)
    maps = np.stack([ref.blob_map(rng, (14, 19), 5, 3)[:67, :93] for _ in range(3)])
    assert all((maps[:, 0] == c).any() and (maps[:, -1] == c).any() and (maps[:, :, 0] == c).any() and (maps[:, :, -1] == c).any() for c in (1, 2))
    got = sch.label_components_device(maps, [2, 1], erode=True)
    assert torch.equal(got, sch.label_components_device(torch.from_numpy(maps).to(cuda_device), [2, 1], erode=True))
    got = got.cpu().numpy()
    for n in range(3):
        for k, c in enumerate((2, 1)):
            assert np.array_equal(got[n, k], ref.label_components(maps[n], c, True)), (n, c)
    assert np.array_equal(sch.label_components_device(maps[1], [1, 2]).cpu().numpy()[1], got[1, 0])
    # erosion really happened, and differs from the plain mask
    assert not np.array_equal(got[0, 0], ref.label_components(maps[0], 2, False))


def _check_against_helper(sch, label_map, classes, **kw):
    """class_hulls_device on one map == the helper, slot by slot; returns the helper's lists per class"""
    top = kw.get("top_number", 1)
    res = sch.class_hulls_device(label_map, classes, **kw).host()
    assert res.vertices.shape == (len(classes), top, 2 * label_map.shape[0] + 1, 2)
    wants = []
    for k, c in enumerate(classes):
        want = ref.class_hulls(label_map, c, top, kw.get("area_threshold", 30), kw.get("drop_first", True))
        full = ref.class_hulls(label_map, c, top, kw.get("area_threshold", 30), False)         # the slots, dropped or not
        assert [int(r) for r in res.roots[k] if r] == [lab for lab, _, _ in full]
        assert [int(a) for a in res.areas[k] if a] == [area for _, area, _ in full]
        got = [(int(res.roots[k, t]), res.vertices[k, t, :res.n_vertices[k, t]]) for t in range(top) if res.n_vertices[k, t] > 0]
        assert len(got) == len(want), (c, got, want)
        for (g_lab, g_v), (w_lab, _, w_v) in zip(got, want):
            assert g_lab == w_lab and np.array_equal(g_v, w_v), (c, g_v.tolist(), w_v.tolist())
        wants.append(want)
    return wants


def test_hulls_of_blobby_maps(cuda_device):
    sch = _hull(cuda_device)
    rng = np.random.default_rng(21)
    seen = 0
    for _ in range(6):
        lm = ref.blob_map(rng)                                             # 45 x 60, three classes
        for kw in (dict(), dict(top_number=3, area_threshold=5), dict(drop_first=False)):
            seen += sum(len(w) for w in _check_against_helper(sch, lm, [1, 2], **kw))
    assert seen >= 30


def test_drop_first_changes_the_hull(cuda_device):
    sch = _hull(cuda_device)
    lm = np.zeros((40, 50), dtype=np.uint8)
    lm[5:30, 8:41] = 1
    a = _check_against_helper(sch, lm, [1])[0][0][2]
    b = _check_against_helper(sch, lm, [1], drop_first=False)[0][0][2]
    # rectangle 8..40 x 5..29 eroded to 9..39 x 6..28: four corners; without its first pixel the corner (9, 6) becomes (9, 7), (10, 6)
    assert b.tolist() == [[9, 6], [39, 6], [39, 28], [9, 28]]
    assert a.tolist() == [[9, 7], [10, 6], [39, 6], [39, 28], [9, 28]]


def test_lines_ties_thresholds_and_empty_slots(cuda_device):
    sch = _hull(cuda_device)
    h, w = 48, 70

    def run(mask, **kw):                                                   # ready masks: class 1, no erosion
        kw.setdefault("area_threshold", 0)
        res = sch.class_hulls_device(mask, [1], erode=False, **kw).host()
        top = kw.get("top_number", 1)
        return [res.vertices[0, t, :res.n_vertices[0, t]].tolist() for t in range(top)], res

    m = np.zeros((h, w), dtype=np.uint8)
    m[7, 3:40] = 1
    assert run(m)[0] == [[[4, 7], [39, 7]]] and run(m, drop_first=False)[0] == [[[3, 7], [39, 7]]]
    m[:] = 0
    m[2:45, 66] = 1
    assert run(m)[0] == [[[66, 3], [66, 44]]] and run(m, drop_first=False)[0] == [[[66, 2], [66, 44]]]
    m[:] = 0
    m[np.arange(5, 40), np.arange(5, 40) + 20] = 1
    assert run(m)[0] == [[[26, 6], [59, 39]]]
    m[:] = 0
    m[np.arange(5, 40), 60 - np.arange(5, 40)] = 1                        # anti-diagonal: x falls as y grows
    assert run(m, drop_first=False)[0] == [[[21, 39], [55, 5]]]
    # one and two pixels: the drop leaves nothing / one point
    m[:] = 0
    m[4, 4] = 1
    got, res = run(m)
    assert got == [[]] and res.areas[0, 0] == 1 and res.roots[0, 0] == 4 * w + 4 + 1
    assert run(m, drop_first=False)[0] == [[[4, 4]]]
    m[4, 5] = 1
    assert run(m)[0] == [[[5, 4]]]
    # two equal squares: the raster-first one wins the tie; top_number = 3 with two components leaves an empty slot
    m[:] = 0
    m[20:26, 40:46] = 1
    m[22:28, 10:16] = 1
    got, res = run(m, drop_first=False)
    assert got == [[[40, 20], [45, 20], [45, 25], [40, 25]]] and res.roots[0, 0] == 20 * w + 40 + 1
    got, res = run(m, drop_first=False, top_number=3)
    assert got[1] == [[10, 22], [15, 22], [15, 27], [10, 27]] and got[2] == [] and res.areas[0].tolist() == [36, 36, 0] and res.roots[0, 2] == 0
    # strict threshold: area == area_threshold is excluded, area_threshold + 1 is included
    assert run(m, area_threshold=36)[0] == [[]] and run(m, area_threshold=36)[1].roots[0, 0] == 0
    assert run(m, area_threshold=35, drop_first=False)[0] == [[[40, 20], [45, 20], [45, 25], [40, 25]]]
    # no foreground at all
    m[:] = 0
    got, res = run(m, top_number=2)
    assert got == [[], []] and not res.roots.any() and not res.areas.any()


def test_tall_maps_use_the_scratch_stack(cuda_device):
    """h > 2047: the chain's stack no longer fits LDS and lives in the scratch buffer; a thin tall map keeps this cheap."""
    sch = _hull(cuda_device)
    rng = np.random.default_rng(4)
    h, w = 2100, 9
    lm = (rng.random((h, w)) < 0.8).astype(np.uint8)
    res = sch.class_hulls_device(lm, [1], erode=False, area_threshold=0).host()
    want = ref.class_hulls(lm, 1, 1, 0, True, do_erode=False)
    assert len(want) == 1 and np.array_equal(res.vertices[0, 0, :res.n_vertices[0, 0]], want[0][2]) and res.areas[0, 0] == want[0][1]


def test_generate_convex_hull_on_host_and_device_input(cuda_device):
    sch = _hull(cuda_device)
    rng = np.random.default_rng(8)
    lm = ref.blob_map(rng, (12, 14), 6, 3)
    for index in (1, 2):
        want = ref.generate_convex_hull(lm, index, top_number=2)
        assert len(want) >= 1
        for src in (lm, torch.from_numpy(lm).to(cuda_device)):
            got = sch.generate_convex_hull(src, index_care_about=index, top_number=2)
            assert len(got) == len(want)
            for g, wv in zip(got, want):
                assert g.dtype == np.int32 and g.shape[0] == 2 and np.array_equal(g, wv) and np.array_equal(g[:, 0], g[:, -1])
    assert sch.generate_convex_hull(np.zeros((9, 9), dtype=np.uint8)) == []
    assert sch.generate_convex_hull(lm, index_care_about=7) == []


class _StubSeg(object):
    """segmentation stand-in: a fixed device label map whatever the frame"""

    def __init__(self, labels):
        self.labels = labels

    def segmentation_device_raw(self, bgr, K, dist, factor):
        return self.labels

    def segmentation_device_raw_batch(self, frames, Ks, dists, factor):
        return torch.stack([self.labels for _ in frames])


def _msg(frame_id, h=48, w=64):
    return types.SimpleNamespace(data=np.zeros((h, w, 3), dtype=np.uint8), header=types.SimpleNamespace(frame_id=frame_id, stamp=0))


def test_node_publishes_back_projected_hulls(cuda_device, caplog):
    from vision_semantic_segmentation_amd import VisionSemanticSegmentationNode, get_cfg_defaults
    from vision_semantic_segmentation_amd.plane_3d import Plane3D
    rng = np.random.default_rng(31)
    lm = ref.blob_map(rng, (10, 13), 6, 3)                                # 60 x 78 labels for a 48 x 64 frame: any size will do
    seg = _StubSeg(torch.from_numpy(lm).to(cuda_device))
    plain = VisionSemanticSegmentationNode(get_cfg_defaults(), seg=seg, undistort=False)
    colour_plain = plain.image_callback(_msg("camera6"))
    cfg = get_cfg_defaults()
    cfg.VISION_SEM_SEG.CONVEX_HULL_CLASSES = [2, 1]
    sent = []
    node = VisionSemanticSegmentationNode(cfg, seg=seg, undistort=False, publish_markers=lambda topic, markers: sent.append((topic, markers)))
    # no plane yet: one warning for any number of frames, no markers, same colour image
    with caplog.at_level(logging.WARNING):
        assert np.array_equal(node.image_callback(_msg("camera6")), colour_plain)
        node.image_callback(_msg("camera1"))
    assert sent == [] and node.hull_id == 0
    assert len([r for r in caplog.records if "ground plane" in r.getMessage()]) == 1
    coef = [0.01, -0.02, 1.0, 1.8]
    node.plane_callback(types.SimpleNamespace(coef=coef))
    colour = node.image_callback(_msg("camera6"))
    assert colour.tobytes() == colour_plain.tobytes()
    plane = Plane3D(*coef)
    next_id = 1

    def expect(cam, frames):
        nonlocal next_id
        out = []
        for index in (2, 1):
            polys = ref.generate_convex_hull(lm, index)
            assert len(polys) == 1
            v = polys[0] * np.array([[float(cam.imSize[0]) / lm.shape[1], float(cam.imSize[1]) / lm.shape[0]]]).T
            d, Cw = cam.pixel_to_ray_vec(v)
            out.append((index, next_id, plane.plane_ray_intersection_vec(d, Cw).T))
            next_id += 1
        return out

    def check(got, want):
        assert len(got) == len(want)
        for (topic, markers), (index, mid, pts) in zip(got, want):
            assert topic == ("/crosswalk_convex_hull_rviz" if index == 1 else "/road_convex_hull_rviz") and len(markers) == 1
            m = markers[0]
            assert sorted(m) == ["color", "frame_id", "id", "lifetime", "points", "scale", "type"]
            assert m["id"] == mid and m["frame_id"] == "velodyne" and m["type"] == "line_strip" and m["scale"] == 0.1
            assert (m["color"], m["lifetime"]) == (([0.8, 0.0, 0.0, 0.8], 10.0) if index == 1 else ([0.0, 0, 0.8, 0.8], 3.0))
            assert m["points"].shape == pts.shape and pts.shape[1] == 3 and np.array_equal(m["points"], pts)
            # the strip is closed: first and last column are the same pixel.  Their float64 images agree to rounding only: the
            # matmuls and the norm of pixel_to_ray_vec sum one column in another order than its neighbour (vector body against
            # tail), the margin the fixture test gives the same expressions
            np.testing.assert_allclose(m["points"][-1], m["points"][0], rtol=1e-12, atol=0)

    check(sent, expect(node.cam6, 1))
    # the views form: one call for both cameras' labels, markers per view in order, ids running on
    sent.clear()
    labels = node.image_callback_views([_msg("camera1"), _msg("camera6")])
    assert labels.shape == (2,) + lm.shape
    check(sent, expect(node.cam1, 1) + expect(node.cam6, 1))
    assert node.hull_id == 6
    # the reference's own entry point, on the device labels
    sent.clear()
    markers = node.generate_and_publish_convex_hull(seg.labels, "camera1", index_care_about=1)
    want = expect(node.cam1, 1)[1]
    assert len(sent) == 1 and sent[0][0] == "/crosswalk_convex_hull_rviz" and markers[0]["id"] == 7 and np.array_equal(markers[0]["points"], want[2])
