"""The points map's host side (vision_semantic_segmentation_amd/points_map.py, avl_points_map_window, MAPPING.POINTS_MAP) against
the NumPy restatement of tests/_points_map_reference.py -- no GPU: the frustum's window contains every voter, the host's run count,
the configuration and its refusals, loading, the drop rule and the size limits, and the restatement's own sensitivity."""
import ctypes as C
import sys
import types

import numpy as np
import pytest

import _points_map_reference as ref

H, W, RANGE_MAX = 1440, 1920, 100.0


def _cams():
    from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6
    return {"cam1": camera_setup_1(), "cam6": camera_setup_6()}


def _voters(world, pose7, cam):
    """src/mapping.py:367-383 on a float64 [4, N] world cloud -> (mask, the homogeneous w of every point)"""
    pm = _pm()
    T_origin_to_velodyne = np.linalg.inv(pm.velodyne_to_origin(pose7))
    pcd_velodyne = np.matmul(T_origin_to_velodyne, np.vstack((world[0:3, :], np.ones((1, world.shape[1])))))     # homogenize
    x = np.matmul(cam.P, pcd_velodyne)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        IXY = (x[:-1] / x[-1]).astype(np.int32)                                                                  # dehomogenize
    mask_positive = np.logical_and(0 < pcd_velodyne[0, :], pcd_velodyne[0, :] < RANGE_MAX)
    mask = np.logical_and(np.logical_and(0 <= IXY[0, :], IXY[0, :] < W), np.logical_and(0 <= IXY[1, :], IXY[1, :] < H))
    return np.logical_and(mask, mask_positive), x[-1]


def _pm():
    from vision_semantic_segmentation_amd import points_map
    return points_map


@pytest.mark.parametrize("name", ["cam1", "cam6"])
def test_the_frustum_box_contains_every_voter(name):
    """20 seeded poses (any yaw, roll and pitch within 0.1 rad), 200 000 float32 world points each, a quarter of them within 1 m of
    the sensor: every point the reference's own expressions let vote lies in window_box with no margin.  Camera 1 must have met a
    voter with a negative homogeneous w (behind the camera, in front of the sensor), or the near cloud did not do its job.
    The voters' transform and the box both come from pm.velodyne_to_origin: this test checks the frustum, not that transform,
    which test_frustum_vertices_and_window_equal_the_restatement holds against the restatement's own pose and lever matrices and
    the GPU tests against the frame kernels (a wrong transform would lose voters there)."""
    pm, cam = _pm(), _cams()[name]
    rng = np.random.default_rng(11 if name == "cam1" else 66)
    negative_w, total, slack = 0, 0, np.inf
    for _ in range(20):
        pose7 = ref.pose_from(rng.uniform(-500, 500), rng.uniform(-500, 500), rng.uniform(-2, 2), rng.uniform(-np.pi, np.pi),
                              rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
        far = np.stack([rng.uniform(-20, 120, 150000), rng.uniform(-150, 150, 150000), rng.uniform(-30, 30, 150000)])
        near = rng.uniform(-1.0, 1.0, (3, 50000))
        vel = np.hstack([far, near])
        world = np.matmul(pm.velodyne_to_origin(pose7), np.vstack([vel, np.ones((1, vel.shape[1]))]))
        world = world.astype(np.float32).astype(np.float64)                  # the index stores float32
        mask, w = _voters(world, pose7, cam)
        xmin, xmax, ymin, ymax = pm.window_box(pose7, [cam], (H, W), RANGE_MAX, 0.0, 0.0)
        x, y = world[0, mask], world[1, mask]
        assert mask.sum() > 1000
        assert (x >= xmin).all() and (x <= xmax).all() and (y >= ymin).all() and (y <= ymax).all()
        slack = min(slack, (x - xmin).min(), (xmax - x).min(), (y - ymin).min(), (ymax - y).min())
        negative_w += int((w[mask] < 0).sum())
        total += int(mask.sum())
    print("%s: %d voters, %d with negative w, smallest slack %.4g m" % (name, total, negative_w, slack))
    if name == "cam1":
        assert negative_w >= 1


def test_a_camera_that_looks_sideways_is_refused():
    from vision_semantic_segmentation_amd.camera import Camera
    pm, cam = _pm(), _cams()["cam1"]
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    turned = Camera(cam.K, np.matmul(cam.R, Rz), cam.t)
    with pytest.raises(ValueError, match="RADIUS_M"):
        pm.frustum_vertices(turned, (H, W), RANGE_MAX)
    with pytest.raises(ValueError, match="RADIUS_M"):
        pm.window_box(ref.pose_from(0, 0), [cam, turned], (H, W), RANGE_MAX)
    assert len(pm.window_box(ref.pose_from(0, 0), [turned], (H, W), RANGE_MAX, radius_m=30.0)) == 4      # the square needs no camera


def test_frustum_vertices_and_window_equal_the_restatement():
    pm = _pm()
    for cam in _cams().values():
        got = pm.frustum_vertices(cam, (H, W), RANGE_MAX)
        want = ref.frustum_vertices(cam.K, cam.R, cam.t, H, W, RANGE_MAX)
        assert got.shape == (3, 9)
        # the same nine points; the package lists them plane by plane as the restatement does
        assert np.allclose(got, want, rtol=0, atol=1e-9)
        assert np.allclose(got[0, 1:5], 0.0, atol=1e-12) and np.allclose(got[0, 5:9], RANGE_MAX, atol=1e-9)
    ix = ref.build(ref.cloud_8x6(), ref.TILE)
    index = types.SimpleNamespace(ox=ix["ox"], oy=ix["oy"], tile_m=ix["tile_m"], rows=ix["rows"], cols=ix["cols"])
    cams = [c.scaled(128 / 1920.0, 96 / 1440.0) for c in _cams().values()]
    rng = np.random.default_rng(5)
    seen = set()
    for k in range(40):
        pose7 = ref.pose_from(rng.uniform(-30, 40), rng.uniform(-20, 50), 0.0, rng.uniform(-np.pi, np.pi))
        radius, margin = (0.0, 1.0) if k % 2 else (5.0, 0.5)
        got = pm.window(index, pose7, cams[:1 + k % 2], (96, 128), ref.RANGE_MAX, radius, margin)
        assert got == ref.window(ix, pose7, cams[:1 + k % 2], 96, 128, ref.RANGE_MAX, radius, margin)
        seen.add("empty" if got[0] > got[1] or got[2] > got[3] else "some")
    assert seen == {"empty", "some"}


def _window_call(offsets, rows, cols, rect):
    from vision_semantic_segmentation_amd import _lib
    m, runs = C.c_int64(-7), C.c_int32(-7)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    rc = _lib.lib().avl_points_map_window(off.ctypes.data_as(C.c_void_p), rows, cols, *rect, C.byref(m), C.byref(runs))
    return rc, int(m.value), int(runs.value)


def test_window_function_counts_the_rectangles_runs():
    """avl_points_map_window on the 8 x 6 index with empty tiles: a rectangle inside, clipped on each side, wholly outside, the whole
    index and a single point -- M and the non-empty runs of the restatement.  It is a host function: no GPU is touched."""
    from vision_semantic_segmentation_amd import _lib
    pm = _pm()
    ix = ref.build(ref.cloud_8x6(), ref.TILE)
    assert (ix["rows"], ix["cols"]) == (8, 6)
    for name, rect in ref.RECTS.items():
        clipped = pm.clip_rect(rect, 8, 6)
        assert clipped == ref.clip(rect, 8, 6)
        rc, m, runs = _window_call(ix["offsets"], 8, 6, clipped)
        assert rc == 0, _lib.last_error()
        assert (m, runs) == ref.count(ix, clipped), name
        assert pm.window_count(ix["offsets"], 8, 6, clipped) == (m, runs)
    assert ref.count(ix, ref.clip(ref.RECTS["outside"], 8, 6)) == (0, 0)
    assert ref.count(ix, ref.RECTS["one_point"]) == (1, 1)
    assert ref.count(ix, ref.RECTS["whole"]) == (len(ix["points"]), 7)          # row 6 is empty
    assert ref.count(ix, ref.RECTS["inside"])[1] == 4
    rc, _, _ = _window_call(ix["offsets"], 8, 6, (2, 8, 1, 4))                   # not clipped
    assert rc == -1 and "leaves" in _lib.last_error()
    rc, _, _ = _window_call(ix["offsets"], 8, 6, (2, 5, -1, 4))
    assert rc == -1
    bad = ix["offsets"].copy()
    bad[20] = bad[24] + 1
    assert _window_call(bad, 8, 6, (3, 3, 2, 5))[0] == -1                        # a run whose offsets decrease


def test_config_defaults_and_refusals():
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = get_cfg_defaults()
    p = cfg.MAPPING.POINTS_MAP
    assert (p.SOURCE, p.PATH, p.TILE_M, p.RADIUS_M, p.MARGIN_M) == ("topic", "", 10.0, 0.0, 1.0)
    sm = SemanticMapping(cfg, device="cpu", logger=MyLogger("test", quiet=True))
    assert not sm.points_map_indexed() and sm.points_map_index is None and sm._reduced_buf is None and sm.last_reduced is None
    cfg.MAPPING.POINTS_MAP.SOURCE = "index"
    for method in ("points_raw", "planar"):
        cfg.MAPPING.DEPTH_METHOD = method
        with pytest.raises(ValueError, match="points_map"):
            SemanticMapping(cfg, device="cpu", logger=MyLogger("test", quiet=True))
    cfg.MAPPING.DEPTH_METHOD = "points_map"
    cfg.MAPPING.POINTS_MAP.SOURCE = "file"
    with pytest.raises(ValueError, match="SOURCE"):
        SemanticMapping(cfg, device="cpu", logger=MyLogger("test", quiet=True))
    cfg.MAPPING.POINTS_MAP.SOURCE = "index"
    sm = SemanticMapping(cfg, device="cpu", logger=MyLogger("test", quiet=True))
    assert sm.points_map_indexed()
    with pytest.raises(RuntimeError, match="no points map is loaded"):           # a missing index at the first frame says so
        sm.mapping(np.zeros((4, 4, 3), dtype=np.uint8), ref.pose_from(0, 0), sm.cam1)
    with pytest.raises(RuntimeError, match="no points map is loaded"):
        sm.mapping_views([np.zeros((4, 4, 3), dtype=np.uint8)], ref.pose_from(0, 0), [sm.cam1])


def _fake_ros(monkeypatch):
    topics = []
    rospy = types.ModuleType("rospy")
    rospy.Subscriber = lambda topic, cls, cb: topics.append(topic) or topic
    rospy.Publisher = lambda topic, cls, queue_size=1: topic
    monkeypatch.setitem(sys.modules, "rospy", rospy)
    for pkg, names in (("geometry_msgs", ["PoseStamped"]), ("sensor_msgs", ["Image", "PointCloud2"]), ("shape_msgs", ["Plane"])):
        mod, msg = types.ModuleType(pkg), types.ModuleType(pkg + ".msg")
        for n in names:
            setattr(msg, n, type(n, (), {}))
        mod.msg = msg
        monkeypatch.setitem(sys.modules, pkg, mod)
        monkeypatch.setitem(sys.modules, pkg + ".msg", msg)
    return topics


@pytest.mark.parametrize("source", ["topic", "index"])
def test_the_node_subscribes_to_reduced_map_only_without_the_index(source, monkeypatch):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    topics = _fake_ros(monkeypatch)
    cfg = get_cfg_defaults()
    cfg.MAPPING.POINTS_MAP.SOURCE = source
    cfg.MAPPING.POINTS_MAP.PATH = "site.npy"
    monkeypatch.setattr(SemanticMapping, "load_points_map", lambda self, path, tile_m=None: topics.append("load " + path))
    SemanticMapping(cfg, device="cpu", use_ros=True, logger=MyLogger("test", quiet=True))
    # PATH is loaded before the first subscriber exists (no frame can arrive ahead of the index), and only with the index
    assert (topics[0] == "load site.npy") == (source == "index") and topics.count("load site.npy") == (source == "index")
    assert ("/reduced_map" in topics) == (source == "topic")
    assert "/current_pose" in topics and "/camera1/semantic" in topics and "/points_raw" not in topics


def test_mapping_with_the_index_takes_the_cloud_from_reduced_map_device(monkeypatch):
    """mapping(), mapping_views() and the two image callbacks hand frame_device the cloud of reduced_map_device as a "world" cloud,
    with the frame's pose, cameras and image size, and never read self.pcd or the cloud queue."""
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger

    class NoPcd(SemanticMapping):
        pcd = property(lambda self: (_ for _ in ()).throw(AssertionError("self.pcd was read")), lambda self, v: None)

    cfg = get_cfg_defaults()
    cfg.MAPPING.POINTS_MAP.SOURCE = "index"
    sm = NoPcd(cfg, device="cpu", logger=MyLogger("test", quiet=True))
    calls = []
    monkeypatch.setattr(SemanticMapping, "reduced_map_device", lambda self, pose, cameras=None, image_size=None, stream=None:
                        calls.append(("reduce", tuple(pose), list(cameras), tuple(image_size))) or "CLOUD")
    monkeypatch.setattr(SemanticMapping, "frame_device", lambda self, pcd, frame, *a, **k: calls.append(("frame", pcd, frame)))
    monkeypatch.setattr(SemanticMapping, "frame_device_views", lambda self, pcd, frame, *a, **k: calls.append(("views", pcd, frame)))
    monkeypatch.setattr(SemanticMapping, "update_pcd", lambda self, stamp: (_ for _ in ()).throw(AssertionError("the cloud queue was read")))
    img = np.zeros((6, 8, 3), dtype=np.uint8)
    pose = tuple(ref.pose_from(3.0, 4.0))
    sm.mapping(img, pose, sm.cam1)
    sm.mapping_views([img, img], pose, [sm.cam1, sm.cam6])
    want = [("reduce", pose, [sm.cam1], (6, 8)), ("frame", "CLOUD", "world"), ("reduce", pose, [sm.cam1, sm.cam6], (6, 8)), ("views", "CLOUD", "world")]
    assert calls == want
    del calls[:]
    stamp = types.SimpleNamespace(secs=5, nsecs=0)
    header = types.SimpleNamespace(stamp=stamp, frame_id="camera1")
    sm.pose_queue.append(types.SimpleNamespace(header=header, pose=pose))
    sm.image_callback(types.SimpleNamespace(header=header, data=img))              # (the pose queue keeps its latest element)
    sm.image_callback_views([types.SimpleNamespace(header=header, data=img), types.SimpleNamespace(header=types.SimpleNamespace(stamp=stamp, frame_id="camera6"), data=img)])
    assert calls == want
    # estimate_ground_plane takes the crop of the vehicle's cameras around the pose, as a world cloud
    del calls[:]
    monkeypatch.setattr("vision_semantic_segmentation_amd.ground_plane.estimate_ground_plane_device",
                        lambda cloud, T=None, device=None, **kw: calls.append(("plane", cloud, np.asarray(T).shape, kw)) or "RESULT")
    monkeypatch.setattr(SemanticMapping, "reduced_map_device", lambda self, pose, cameras=None, image_size=None, stream=None:
                        calls.append(("reduce", tuple(pose), cameras, image_size, stream)) or "CLOUD")
    assert sm.estimate_ground_plane(pose, hypotheses=64) == "RESULT"
    assert calls == [("reduce", pose, None, None, None), ("plane", "CLOUD", (4, 4), {"hypotheses": 64})]
    with pytest.raises(ValueError, match="pose"):
        sm.estimate_ground_plane()


def test_loading_both_layouts_and_the_drop_rule(tmp_path):
    pm = _pm()
    cloud = ref.cloud_8x6()
    want = ref.as_aos32(cloud)
    np.save(str(tmp_path / "aos64.npy"), cloud.astype(np.float64))
    np.save(str(tmp_path / "soa32.npy"), np.ascontiguousarray(cloud.T))
    for name in ("aos64.npy", "soa32.npy"):
        got = pm.load_points(str(tmp_path / name))
        assert got.dtype.is_floating_point and got.element_size() == 4 and tuple(got.shape) == want.shape
        assert got.numpy().tobytes() == want.tobytes()
    assert pm.load_points(cloud).numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="npy"):
        pm.load_points(str(tmp_path / "map.pcd"))
    with pytest.raises(ValueError):
        pm.as_points(np.zeros((5, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        pm.as_points(np.zeros((5, 4), dtype=np.int32))
    pts = pm.as_points(cloud)
    keep = pm.keep_mask(pts).numpy()
    assert np.array_equal(keep, ref.kept(want)) and int((~keep).sum()) == ref.N_DROPPED_8X6
    ix = ref.build(cloud, ref.TILE)
    assert pm.tile_grid(pts, ref.TILE) == (ix["ox"], ix["oy"], 8, 6, len(cloud) - ref.N_DROPPED_8X6)
    assert (ix["ox"], ix["oy"], ix["dropped"]) == (-8.0, 4.0, ref.N_DROPPED_8X6)
    assert pm.tile_grid(pm.as_points(np.full((3, 4), np.nan, dtype=np.float32)), 2.0) == (0.0, 0.0, 0, 0, 0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "10", True):
        with pytest.raises(ValueError, match="TILE_M"):
            pm.tile_grid(pts, bad)


def test_size_refusals():
    pm = _pm()
    huge = np.broadcast_to(np.zeros((1, 4), dtype=np.float32), (1 << 31, 4))      # a view: no memory behind it
    with pytest.raises(ValueError, match="2\\^31"):
        pm.as_points(huge)
    with pytest.raises(ValueError, match="2\\^31"):
        pm.as_points(np.broadcast_to(np.zeros((4, 1), dtype=np.float32), (4, 1 << 31)))
    ok = pm.as_points(np.array([[0.0, 0.0, 0, 0], [4095.5, 4095.5, 0, 0]], dtype=np.float32))
    assert pm.tile_grid(ok, 1.0)[2:4] == (4096, 4096)                              # 2^24 tiles exactly
    over = pm.as_points(np.array([[0.0, 0.0, 0, 0], [4096.5, 4095.5, 0, 0]], dtype=np.float32))
    with pytest.raises(ValueError, match="2\\^24"):
        pm.tile_grid(over, 1.0)
    with pytest.raises(ValueError, match="2\\^24"):
        pm.tile_grid(pm.as_points(np.array([[0.0, 0.0, 0, 0], [3e38, -3e38, 0, 0]], dtype=np.float32)), 10.0)


def test_the_restatement_catches_a_wrong_evaluation():
    """A hand-worked index, then: an off-by-one in the last column of a run and an unstable order change the restated bytes."""
    pts = np.array([[5.0, 1.0, 0, 0], [1.0, 3.0, 0, 1], [5.5, 1.5, 0, 2], [np.nan, 0.0, 0, 3], [1.5, 1.0, 0, 4], [5.0, 1.0, 0, 5],
                    [2.0, 2.0, 0, 6]], dtype=np.float32)
    ix = ref.build(pts, 2.0)
    # origin (0, 0); tiles (ix, iy): 0 -> (2, 0), 1 -> (0, 1), 2 -> (2, 0), 4 -> (0, 0), 5 -> (2, 0), 6 -> (1, 1); cols = 2
    assert (ix["ox"], ix["oy"], ix["rows"], ix["cols"], ix["dropped"]) == (0.0, 0.0, 3, 2, 1)
    assert ix["keys"].tolist() == [4, 1, 4, -1, 0, 4, 3]
    assert ix["points"][:, 3].tolist() == [4, 1, 6, 0, 2, 5]
    assert ix["offsets"].tolist() == [0, 1, 2, 2, 3, 6, 6]
    assert ref.gather(ix, (1, 2, 0, 1))[:, 3].tolist() == [6, 0, 2, 5] and ref.count(ix, (1, 2, 0, 1)) == (4, 2)
    assert ref.gather(ix, (0, 2, 1, 1))[:, 3].tolist() == [1, 6] and ref.count(ix, (0, 2, 1, 1)) == (2, 2)
    big = ref.build(ref.cloud_8x6(), ref.TILE)
    rect = ref.RECTS["inside"]
    good = ref.gather(big, rect)
    assert good.tobytes() != ref.gather(big, rect, last_column_off_by_one=True).tobytes()
    p = ref.as_aos32(ref.cloud_8x6())
    k = ref.kept(p)
    idx = np.nonzero(k)[0]
    unstable = idx[::-1][np.argsort(big["keys"][idx[::-1]], kind="stable")]         # tiles in order, points inside a tile reversed
    assert np.array_equal(big["keys"][unstable], big["keys"][big["order"]])
    assert p[unstable].tobytes() != big["points"].tobytes()
    b0, b1 = big["offsets"][3 * 6 + 2], big["offsets"][3 * 6 + 3]                   # tile BIG: 3000 + the edge point + the 40 copies
    assert b1 - b0 == 3041 and np.all(np.diff(big["points"][b0:b1, 3]) > 0)         # the input's order inside the tile
    s0, s1 = big["offsets"][5 * 6 + 4], big["offsets"][5 * 6 + 5]
    assert s1 - s0 == 1
    empty = [int(big["offsets"][i * 6 + j + 1] - big["offsets"][i * 6 + j]) for i, j in ref.EMPTY]
    assert not any(empty)
