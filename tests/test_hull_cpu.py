"""Semantic extraction without a GPU: the CPU restatement the GPU tests compare against (tests/_hull_reference.py), the host-side
back-projection (Camera.pixel_to_ray*, Plane3D) against values recorded from the reference's own classes
(tests/golden/hull_backproject.npz, tools/gen_golden_hull.py), the C ABI's argument checks and the node's default of leaving the
feature off."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hull_reference as ref  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hull_backproject.npz")
RTOL = 1e-12          # the float64 expressions are the reference's; the margin covers only the summation order inside np.matmul


def test_reference_hull_has_the_vertex_set_of_scipy():
    """The helper's monotone chain against scipy.spatial.ConvexHull (Qhull) on random pixel blobs: same vertex set, and the
    helper's order starts at the smallest (x, y) and turns with positive cross products throughout."""
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(60):
        h, w = int(rng.integers(6, 40)), int(rng.integers(6, 40))
        mask = ref.blob_map(rng, (h // 3 + 1, w // 3 + 1), 3, 2)[:h, :w] == 1
        lab = ref.canonical_labels(mask)
        if not lab.any():
            continue
        biggest = np.bincount(lab.ravel())[1:].argmax() + 1
        ys, xs = np.where(lab == biggest)
        pts = np.stack([xs, ys], axis=1)
        mine = ref.monotone_chain(pts.tolist())
        if len(mine) < 3:
            continue
        hull = ConvexHull(pts)
        assert sorted(mine) == sorted(map(tuple, pts[hull.vertices].tolist()))
        assert mine[0] == min(mine)
        for i in range(len(mine)):
            o, a, b = mine[i], mine[(i + 1) % len(mine)], mine[(i + 2) % len(mine)]
            assert (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0]) > 0
        checked += 1
    assert checked >= 40


def test_reference_labels_and_patterns():
    """canonical labels: a component's label is its first pixel's index + 1; the two interleaved spirals really are two components,
    the spiral, the checkerboard, the anti-diagonal and the comb one each."""
    m = np.array([[0, 1, 0, 0, 1], [1, 0, 0, 0, 1], [0, 0, 1, 0, 0]], dtype=np.uint8)
    assert ref.canonical_labels(m).tolist() == [[0, 2, 0, 0, 5], [2, 0, 0, 0, 5], [0, 0, 13, 0, 0]]
    for h, w in ((37, 53), (67, 131), (130, 259)):
        pats = ref.mask_patterns(h, w)
        count = {k: len(np.setdiff1d(ref.canonical_labels(v), [0])) for k, v in pats.items()}
        assert count["two_spirals"] == 2 and count["spiral"] == 1 and count["checkerboard"] == 1
        assert count["anti_diagonal"] == 1 and count["comb"] == 1 and count["zeros"] == 0 and count["ones"] == 1
        assert pats["spiral"].mean() > 0.45
    # the drop of the first pixel always shows: that pixel is the hull's first vertex in raster order
    rng = np.random.default_rng(2)
    changed = 0
    for _ in range(20):
        lm = ref.blob_map(rng)
        a = ref.class_hulls(lm, 1, area_threshold=0, drop_first=True)
        b = ref.class_hulls(lm, 1, area_threshold=0, drop_first=False)
        changed += bool(a and b and not np.array_equal(a[0][2], b[0][2]))
    assert changed >= 18


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name", ["camera1", "camera6"])
def test_camera_rays_match_the_reference(gold, name):
    from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6
    cam = {"camera1": camera_setup_1, "camera6": camera_setup_6}[name]()
    pts = gold[name + "_pts"]
    np.testing.assert_allclose(cam.K_inv, gold[name + "_K_inv"], rtol=RTOL, atol=0)
    d, Cw = cam.pixel_to_ray_vec(pts)
    assert d.shape == (3, pts.shape[1]) and Cw.shape == (3, 1)
    np.testing.assert_allclose(d, gold[name + "_d"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(Cw, gold[name + "_C"], rtol=RTOL, atol=0)
    assert np.all(d[0] > 0) and np.allclose(np.linalg.norm(d, axis=0), 1.0)
    for world in (True, False):
        for i in range(4):
            di, Ci = cam.pixel_to_ray(pts[0, i], pts[1, i], world=world)
            np.testing.assert_allclose(di, gold["%s_ray_d_%d" % (name, world)][i], rtol=RTOL, atol=0)
            np.testing.assert_allclose(Ci, gold["%s_ray_C_%d" % (name, world)][i], rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", ["camera1", "camera6"])
def test_plane_matches_the_reference(gold, name):
    from vision_semantic_segmentation_amd.plane_3d import Plane3D
    d, Cw, cloud = gold[name + "_d"], gold[name + "_C"], gold[name + "_cloud"]
    for k, raw in enumerate(gold["planes_raw"]):
        plane = Plane3D.create_plane_from_list(list(raw))
        direct = Plane3D(*raw)
        assert np.array_equal(plane.param, direct.param) and plane.c >= 0
        np.testing.assert_allclose(plane.param, gold["%s_plane%d_param" % (name, k)], rtol=RTOL, atol=0)
        assert abs(plane.a**2 + plane.b**2 + plane.c**2 - 1.0) < 1e-15
        hit = plane.plane_ray_intersection_vec(d, Cw)
        np.testing.assert_allclose(hit, gold["%s_plane%d_hit_vec" % (name, k)], rtol=RTOL, atol=0)
        np.testing.assert_allclose(plane.plane_ray_intersection(d[:, :1], Cw), gold["%s_plane%d_hit_one" % (name, k)], rtol=RTOL, atol=0)
        np.testing.assert_allclose(plane.distance_to_plane(cloud), gold["%s_plane%d_dist" % (name, k)], rtol=RTOL, atol=0)
        np.testing.assert_allclose(plane.distance_to_plane_signed(cloud), gold["%s_plane%d_dist_signed" % (name, k)], rtol=RTOL, atol=0)
        assert np.all(plane.distance_to_plane_signed(hit.T) < 1e-9)              # the intersections lie on the plane


def test_hull_argument_errors_do_not_need_a_gpu():
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    buf = np.zeros(4096, dtype=np.int32)                   # host memory: a refused call never looks at it
    p = C.c_void_p(buf.ctypes.data)

    def cls(*v):
        return (C.c_int32 * len(v))(*v)

    def labels(maps=p, n=1, h=4, w=4, classes=cls(1), n_classes=1, out=p):
        rc = L.avl_label_components(maps, n, h, w, classes, n_classes, 1, out, None, None)
        return rc, _lib.last_error()

    def hulls(maps=p, h=4, w=4, classes=cls(1), n_classes=1, top=1, vertices=p, n_vertices=p, areas=p, roots=p, scratch=p):
        rc = L.avl_class_hulls(maps, 1, h, w, classes, n_classes, 1, top, 30, 1, vertices, n_vertices, areas, roots, scratch, None)
        return rc, _lib.last_error()

    assert labels(maps=None) == (-1, "maps is NULL")
    assert labels(classes=None)[0] == -1 and labels(out=None) == (-1, "labels_out is NULL")
    for bad in (0, 256, -3):
        rc, msg = labels(classes=cls(bad))
        assert rc == -1 and "1 .. 255" in msg
        assert hulls(classes=cls(2, bad), n_classes=2)[0] == -1
    assert labels(h=0)[0] == -1 and labels(w=0)[0] == -1 and labels(n=0)[0] == -1 and hulls(h=0)[0] == -1 and hulls(w=-1)[0] == -1
    for top in (0, 9, -1):
        rc, msg = hulls(top=top)
        assert rc == -1 and "top_number" in msg
    for name in ("vertices", "n_vertices", "areas", "roots", "scratch", "maps"):
        assert hulls(**{name: None})[0] == -1, name
    assert labels(n_classes=0)[0] == -1 and labels(n_classes=65)[0] == -1
    assert L.avl_hull_scratch_bytes(0, 4, 1, 1) == 0 and L.avl_hull_scratch_bytes(4, 4, 1, 9) == 0
    # the scratch holds at least the labels and the areas of every plane
    assert L.avl_hull_scratch_bytes(266, 476, 2, 1) >= 2 * 2 * 266 * 476 * 4
    assert L.avl_hull_scratch_bytes(266, 476, 4, 1) > L.avl_hull_scratch_bytes(266, 476, 2, 1)


def test_python_argument_errors():
    from vision_semantic_segmentation_amd.semantic_convex_hull import generate_convex_hull
    img = np.zeros((8, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="cannot be zero"):
        generate_convex_hull(img, index_care_about=0)
    with pytest.raises(NotImplementedError):
        generate_convex_hull(img, vis=True)
    with pytest.raises(NotImplementedError):
        generate_convex_hull(img, index_to_vitualize=[1])


def test_feature_is_off_by_default(monkeypatch):
    """CONVEX_HULL_CLASSES defaults to []; a node built on the default configuration never reaches the hull code."""
    from vision_semantic_segmentation_amd import VisionSemanticSegmentationNode, get_cfg_defaults
    from vision_semantic_segmentation_amd import semantic_convex_hull, vision_semantic_segmentation_node as vn
    cfg = get_cfg_defaults()
    assert cfg.VISION_SEM_SEG.CONVEX_HULL_CLASSES == []

    def boom(*a, **k):
        raise AssertionError("the hull code ran with the feature off")
    for fn in ("class_hulls_device", "label_components_device", "generate_convex_hull", "hull_workspace_bytes"):
        monkeypatch.setattr(semantic_convex_hull, fn, boom)
    sent = []
    stub_seg = types.SimpleNamespace()
    node = VisionSemanticSegmentationNode(cfg, seg=stub_seg, publish_markers=lambda topic, markers: sent.append(topic))
    assert node.hull_classes == [] and node.plane is None and node.hull_id == 0
    node.plane_callback(types.SimpleNamespace(coef=[0.0, 0.0, 2.0, 3.0]))
    assert node.plane.param.ravel().tolist() == [0.0, 0.0, 1.0, 1.5]
    assert node._extract_hulls(None, ["camera1"]) == [] and sent == []
    # the two stages image_callback runs around the extraction, with stubs in place of the kernels: nothing else is called
    monkeypatch.setattr(vn, "colorize_labels_device", lambda labels, h, w, ref: types.SimpleNamespace(cpu=lambda: types.SimpleNamespace(numpy=lambda: "colour")))
    stub_seg.segmentation_device_raw = lambda bgr, K, dist, factor: "labels"
    msg = types.SimpleNamespace(data=np.zeros((4, 6, 3), dtype=np.uint8), header=types.SimpleNamespace(frame_id="camera1", stamp=0))
    assert node.image_callback(msg) == "colour" and node.last_labels == "labels" and sent == [] and node.hull_id == 0
