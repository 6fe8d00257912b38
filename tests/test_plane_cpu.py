"""The ground-plane pieces that need no GPU: Plane3D's fit / eval / rotation / angles and the tests' own restatement against the
reference's recorded results (tests/golden/plane_fit.npz, tools/gen_golden_plane.py), the argument checks of avl_plane_ransac, the
off-by-default wiring, and the decision-margin condition every GPU case relies on."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _plane_reference as ref  # noqa: E402

WEIGHTS = {"none": {'method': "none"}, "x1": {'method': "x norm", 'param': {'x0': 1.5, 'norm': 1}},
           "x2": {'method': "x norm", 'param': {'x0': 1.5, 'norm': 2}}}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "plane_fit.npz"))


def _within_ulp(got, want, ulps):
    return np.all(np.abs(got - want) <= ulps * np.spacing(np.abs(want)))


def test_plane3d_matches_the_reference(gold):
    """fit, create_plane_from_vectors_and_point, rotate_around_axis and both angles are scalar float64 arithmetic in the reference's
    order: exact.  eval goes through np.matmul, whose last bit depends on the BLAS: 4 ulp of the recorded cost."""
    from vision_semantic_segmentation_amd.plane_3d import Plane3D
    assert float(gold["x0"]) == WEIGHTS["x1"]['param']['x0']
    cloud = gold["cloud"]
    for t, triple in enumerate(gold["triples"]):
        plane = Plane3D.fit(triple, method="min")
        assert plane.weight == {'method': "x norm", 'param': {'x0': 0.0, 'norm': 1}}
        assert np.array_equal(plane.param.ravel(), gold["fit_param"][t]) and plane.param.shape == (4, 1)
        for key, weight in WEIGHTS.items():
            weighted = Plane3D.fit(triple, method="min", weight=weight)
            assert weighted.weight is weight and np.array_equal(weighted.param, plane.param)
            assert _within_ulp(weighted.eval(cloud), gold["eval_" + key][t], 4), (t, key)
        made = Plane3D.create_plane_from_vectors_and_point(gold["vec1"][t], gold["vec2"][t], gold["pt1"][t])
        assert np.array_equal(made.param.ravel(), gold["vec_param"][t])
        assert plane.normal_angle_to_vector(gold["vectors"][t]) == gold["angle"][t]
        assert plane.normal_angle_to_vector_xz(gold["vectors"][t]) == gold["angle_xz"][t]
        plane.rotate_around_axis("y", gold["angles"][t])
        assert np.array_equal(plane.param.ravel(), gold["rot_param"][t])
        assert [plane.a, plane.b, plane.c, plane.d] == gold["rot_param"][t].tolist()


def test_plane3d_refusals():
    from vision_semantic_segmentation_amd.plane_3d import Plane3D
    pts = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, 5.0, 7.0]])
    with pytest.raises(ValueError):
        Plane3D.fit(pts, method="min")                       # data[0] == data[1]: the reference exits
    with pytest.raises(ValueError):
        Plane3D.fit(np.ones((4, 3)), method="min")
    with pytest.raises(NotImplementedError):
        Plane3D.fit(pts, method="least_square")
    with pytest.raises(NotImplementedError):
        Plane3D.fit(pts)                                     # least_square is the default, as in the reference
    with pytest.raises(NotImplementedError):
        Plane3D.fit(pts, method="median")
    with pytest.raises(NotImplementedError):
        Plane3D(0, 0, 1, 0, weight={'method': "y norm"}).eval(pts)
    with pytest.raises(NotImplementedError):
        Plane3D(0, 0, 1, 0, weight={'method': "x norm", 'param': {'x0': 0.0, 'norm': 3}}).eval(pts)
    assert not hasattr(Plane3D, "vis")
    # a degenerate normal: infinite distances, as distance_to_plane gives them
    flat = Plane3D(0, 0, 1, 0, weight={'method': "none"})
    flat.a = flat.b = flat.c = 0.0
    assert np.all(np.isinf(flat.eval(pts)))


def test_the_restatement_matches_the_reference(gold):
    """tests/_plane_reference.py, which the GPU results are compared with, against the same fixture in the same way."""
    cloud = gold["cloud"]
    for t, triple in enumerate(gold["triples"]):
        plane = ref.fit_min(triple)
        assert list(plane) == gold["fit_param"][t].tolist()
        for key, (method, norm) in (("none", ("none", 1)), ("x1", ("x norm", 1)), ("x2", ("x norm", 2))):
            cost = ref.plane_cost(plane, cloud, ref.x_weight(cloud, method, float(gold["x0"]), norm), method)
            assert _within_ulp(cost, gold["eval_" + key][t], 4), (t, key)
    assert ref.fit_min(np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, 5.0, 7.0]])) is None
    assert ref.fit_min(np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [4.0, 8.0, 12.0]])) is None          # collinear: s == 0


def test_the_restatement_agrees_with_plane3d_on_a_case():
    """The restated RANSAC steps and the package's own Plane3D give the same planes and costs (same expressions, same NumPy)."""
    from vision_semantic_segmentation_amd.plane_3d import Plane3D
    cloud, triples = ref.shape_cloud(1025, 64, "f32")
    data = cloud[:, :3].astype(np.float64)
    r = ref.shape_case(1025, 64, "f32", "x norm", 2)
    weight = {'method': "x norm", 'param': {'x0': ref.X0, 'norm': 2}}
    checked = 0
    for h, tri in enumerate(triples):
        if not r.planes[h].any():
            continue
        plane = Plane3D.fit(data[tri], method="min", weight=weight)
        assert np.array_equal(plane.param.ravel(), r.planes[h])
        assert int(np.sum(plane.eval(data) < ref.TOLERANCE)) == r.counts[h]
        checked += 1
    assert checked == r.valid and checked > 40


def test_decision_margins_of_every_gpu_case():
    """No cost of any valid hypothesis and used point, in any case tests/test_gpu_plane.py runs, is within 1e-10 of the tolerance: the
    GPU's costs differ from the restatement's by a few ulp of 0.1 (1e-17) at most, so every inlier decision is the same and the GPU
    tests compare the counts exactly without leaving out any (hypothesis, point) pair."""
    worst = np.inf
    names = []
    for name, r in ref.all_cases():
        names.append(name)
        margin = r.margin[np.isfinite(r.margin)]
        assert margin.size == r.valid
        if margin.size:
            assert margin.min() > ref.MARGIN, (name, margin.min())
            worst = min(worst, margin.min())
        if not name.startswith("shape 3 "):
            assert r.valid >= 4 and r.best >= 0 and r.inliers >= 10, name
    assert len(names) == len(set(names)) == 7 * 2 * 3 + 5
    print("smallest margin over %d cases: %.3g" % (len(names), worst))


def test_sample_triples_is_the_documented_draw():
    from vision_semantic_segmentation_amd.ground_plane import sample_triples
    got = sample_triples(1000, 17, 5)
    assert got.dtype == np.int32 and got.shape == (17, 3)
    assert np.array_equal(got, np.random.default_rng(5).integers(0, 1000, (17, 3)))
    assert np.array_equal(got, ref.sample_triples(1000, 17, 5))


def test_plane_from_moments_recovers_a_plane():
    from vision_semantic_segmentation_amd.ground_plane import plane_from_moments
    rng = np.random.default_rng(3)
    xy = rng.uniform(-20, 20, (500, 2))
    pts = np.column_stack([xy, -1.7 + 0.04 * xy[:, 0] - 0.01 * xy[:, 1]])
    p0 = pts[7]
    delta = pts - p0
    s2 = [np.sum(delta[:, i] * delta[:, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    plane = plane_from_moments(p0, len(pts), delta.sum(axis=0), s2)
    want = np.array([-0.04, 0.01, 1.0, 1.7]) / np.sqrt(0.04**2 + 0.01**2 + 1.0)
    np.testing.assert_allclose(plane.param.ravel(), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.refit(p0, len(pts), delta.sum(axis=0), np.array(s2))[0], want, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        plane_from_moments(p0, 2, delta[:2].sum(axis=0), s2)


def test_plane_argument_errors_do_not_need_a_gpu():
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    buf = np.zeros(4096, dtype=np.float64)                 # host memory: a refused call never looks at it
    p = C.c_void_p(buf.ctypes.data)

    def call(pts=p, n=100, dtype=_lib.AVL_F32, ps=16, cs=4, triples=p, n_hyp=8, method=_lib.AVL_PLANE_W_XNORM, norm=1, tol=0.1,
             result=p, scratch=p):
        rc = L.avl_plane_ransac(pts, n, dtype, ps, cs, None, None, triples, n_hyp, method, 0.0, norm, tol, 0.5, None, None, result, scratch, None)
        return rc, _lib.last_error()

    assert call(pts=None) == (-1, "pts is NULL")
    assert call(triples=None) == (-1, "triples is NULL")
    assert call(result=None) == (-1, "result is NULL") and call(scratch=None) == (-1, "scratch is NULL")
    for n in (2, 0, -5):
        rc, msg = call(n=n)
        assert rc == -1 and "three points" in msg
    rc, msg = call(n=(1 << 27) + 1)
    assert rc == -1 and "at most" in msg and L.avl_plane_scratch_bytes((1 << 27) + 1, 8) == 0
    for n_hyp in (0, -1, _lib.AVL_PLANE_MAX_HYP + 1):
        rc, msg = call(n_hyp=n_hyp)
        assert rc == -1 and "n_hyp" in msg
    for norm in (0, 3, -1):
        rc, msg = call(norm=norm)
        assert rc == -1 and "norm" in msg
    for tol in (0.0, -0.1, float("nan")):
        rc, msg = call(tol=tol)
        assert rc == -1 and "tolerance" in msg
    assert call(dtype=_lib.AVL_F16)[0] == -1 and call(method=2)[0] == -1
    assert call(ps=6)[0] == -1 and call(cs=0)[0] == -1 and call(dtype=_lib.AVL_F64, ps=16, cs=4)[0] == -1
    assert L.avl_plane_scratch_bytes(2, 8) == 0 and L.avl_plane_scratch_bytes(100, 0) == 0
    assert L.avl_plane_scratch_bytes(100, _lib.AVL_PLANE_MAX_HYP + 1) == 0
    # the scratch holds at least the widened cloud
    assert L.avl_plane_scratch_bytes(120000, 256) >= 120000 * 32
    assert L.avl_plane_scratch_bytes(120000, 1024) > L.avl_plane_scratch_bytes(120000, 256)


def test_python_argument_errors():
    from vision_semantic_segmentation_amd import VisionSemanticSegmentationNode, get_cfg_defaults
    from vision_semantic_segmentation_amd.ground_plane import _weight_args
    with pytest.raises(NotImplementedError):
        _weight_args({'method': "y norm"})
    with pytest.raises(NotImplementedError):
        _weight_args({'method': "x norm", 'param': {'x0': 0.0, 'norm': 3}})
    assert _weight_args({'method': "x norm", 'param': {'x0': 2, 'norm': 2}}) == (1, 2.0, 2) and _weight_args({'method': "none"})[0] == 0
    cfg = get_cfg_defaults()
    cfg.VISION_SEM_SEG.GROUND_PLANE.SOURCE = "lidar"
    with pytest.raises(ValueError, match="SOURCE"):
        VisionSemanticSegmentationNode(cfg, seg=types.SimpleNamespace())


def test_cloud_source_is_off_by_default(monkeypatch):
    """GROUND_PLANE.SOURCE defaults to "callback": cloud_callback does nothing and the ground-plane module is never imported."""
    from vision_semantic_segmentation_amd import VisionSemanticSegmentationNode, get_cfg_defaults
    cfg = get_cfg_defaults()
    gp = cfg.VISION_SEM_SEG.GROUND_PLANE
    assert gp.SOURCE == "callback" and gp.ROI == [] and gp.HYPOTHESES == 256 and gp.TOLERANCE == 0.1 and gp.REFINE is True
    assert (gp.SEED, gp.MAX_TILT_DEG, gp.WEIGHT_X0, gp.WEIGHT_NORM) == (0, 30.0, 0.0, 1)
    name = "vision_semantic_segmentation_amd.ground_plane"
    monkeypatch.delitem(sys.modules, name, raising=False)

    class Boom(object):
        def find_spec(self, fullname, path=None, target=None):
            if fullname == name:
                raise AssertionError("the ground-plane code was imported with SOURCE = callback")
            return None
    monkeypatch.setattr(sys, "meta_path", [Boom()] + list(sys.meta_path))
    node = VisionSemanticSegmentationNode(cfg, seg=types.SimpleNamespace())
    assert node.plane is None
    assert node.cloud_callback(np.zeros((50, 4), dtype=np.float32)) is None and node.plane is None
    node.plane_callback(types.SimpleNamespace(coef=[0.0, 0.0, 2.0, 3.0]))
    assert node.cloud_callback(np.zeros((50, 4), dtype=np.float32), pcd_frame_id="world") is None
    assert node.plane.param.ravel().tolist() == [0.0, 0.0, 1.0, 1.5]
    assert name not in sys.modules


def test_origin_to_velodyne_is_the_mappers_transform(monkeypatch):
    """The transform cloud_callback and SemanticMapping.estimate_ground_plane hand the estimate for a cloud that is not in the velodyne
    frame: the module function both use against the oracle's own restatement of mapping.py:165-170 and :368-369, and the T that
    reaches the estimate from cloud_callback (the estimate itself replaced by a recorder: no GPU here)."""
    import torch
    from oracle import mapping_oracle as mo
    from vision_semantic_segmentation_amd import VisionSemanticSegmentationNode, get_cfg_defaults, ground_plane, mapping
    pose7 = np.array([1372.5, 560.25, 1.5, 0.01, -0.02, 0.38, 0.9245])
    pose7[3:] /= np.linalg.norm(pose7[3:])
    pose = types.SimpleNamespace(position=types.SimpleNamespace(x=pose7[0], y=pose7[1], z=pose7[2]),
                                 orientation=types.SimpleNamespace(x=pose7[3], y=pose7[4], z=pose7[5], w=pose7[6]))
    want = np.linalg.inv(np.matmul(mo.transform_from_pose(pose7), mo.velodyne_to_baselink()))
    got = mapping.origin_to_velodyne(pose, mapping.velodyne_to_baselink())
    assert got.shape == (4, 4) and np.array_equal(got, want)
    # the mapper's method is that function on its own constant
    stub = types.SimpleNamespace(T_velodyne_to_basklink=mapping.SemanticMapping.set_velodyne_to_baselink(None))
    assert np.array_equal(mapping.SemanticMapping._origin_to_velodyne(stub, pose), want)
    seen = []

    def record(points, **kw):
        seen.append(kw)
        return types.SimpleNamespace(host=lambda: types.SimpleNamespace(plane=None, used=0, valid=0))
    monkeypatch.setattr(ground_plane, "estimate_ground_plane_device", record)
    monkeypatch.setattr(ground_plane, "GroundPlaneWorkspace", lambda n, h, device: types.SimpleNamespace(fits=lambda *a: True))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    from vision_semantic_segmentation_amd import _lib
    monkeypatch.setattr(_lib, "points_view", lambda pcd, device: (pcd, int(pcd.shape[0]), 0, 16, 4))
    cfg = get_cfg_defaults()
    cfg.VISION_SEM_SEG.GROUND_PLANE.SOURCE = "cloud"
    cfg.VISION_SEM_SEG.GROUND_PLANE.ROI = [0.0, 50.0, -10.0, 10.0, -3.0, 0.0]
    node = VisionSemanticSegmentationNode(cfg, seg=types.SimpleNamespace())
    cloud = np.zeros((40, 4), dtype=np.float32)
    node.cloud_callback(cloud, "world", pose)
    node.cloud_callback(cloud)
    assert np.array_equal(seen[0]["T"], want) and seen[1]["T"] is None and node.plane is None
    assert seen[0]["roi"] == [0.0, 50.0, -10.0, 10.0, -3.0, 0.0] and seen[0]["hypotheses"] == 256 and seen[0]["refine"] is True
    with pytest.raises(ValueError, match="pose"):
        node.cloud_callback(cloud, "world")
