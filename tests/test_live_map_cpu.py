"""The live map's host side, without a GPU: the NumPy restatements against the reference-generated fixture, the window's geometry,
argument errors through the C ABI (nothing touches the device before the arguments are checked) and the configuration."""
import ctypes as C
import os

import numpy as np
import pytest

import _live_map_reference as lr

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "fill_black.npz")


def test_fill_black_restatement_equals_the_reference_fixture():
    g = np.load(GOLDEN)
    assert np.array_equal(g["label_colors"], lr.REF_COLORS)
    for name in ("a", "b"):
        img = g["img_" + name]
        assert img.shape == (40, 36, 3) and img.dtype == np.uint8
        got = lr.fill_black(img)
        assert got.shape == (38, 34, 3) and got.dtype == np.uint8
        assert np.array_equal(got, g["fill_black_" + name])
        # the fixture shows what "as written" means: pixels that were not black are rewritten too
        interior = img[1:-1, 1:-1]
        assert ((interior != got).any(axis=2) & (interior != 0).any(axis=2)).any()


def test_fill_edge_equals_the_reference_fixture_numpy_and_tensor():
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    g = np.load(GOLDEN)
    assert np.array_equal(lr.fill_edge(g["img_a"].copy()), g["fill_edge_a"])
    a = g["img_a"].copy()
    assert rr.fill_edge(a) is a and np.array_equal(a, g["fill_edge_a"])
    t = torch.from_numpy(g["img_a"].copy())
    assert rr.fill_edge(t) is t and np.array_equal(t.numpy(), g["fill_edge_a"])


def _sm(boundary=((100.0, 120.0), (800.0, 816.0)), res=0.1, size_m=(4.15, 3.35)):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = [list(boundary[0]), list(boundary[1])]
    cfg.MAPPING.RESOLUTION = res
    cfg.MAPPING.LIVE_MAP.SIZE_M = list(size_m)
    return SemanticMapping(cfg, device="cpu", logger=MyLogger("test", quiet=True))


def _pose_at_cell(sm, cx, cy):
    """a pose whose position lands at (cx, cy) cells of sm's grid"""
    from vision_semantic_segmentation_amd.utils import Pose
    x = sm.map_boundary[0][0] + cx * sm.resolution - lr.PCD_ORIGIN_OFFSET[0]
    y = sm.map_boundary[1][0] + cy * sm.resolution - lr.PCD_ORIGIN_OFFSET[1]
    return Pose((x, y, 0.0), (0.0, 0.0, 0.0, 1.0))


@pytest.mark.parametrize("cell,where", [((50.5, 20.25), "inside"), ((199.5, 159.5), "last cell"), ((-30.5, 400.5), "off the grid"),
                                       ((0.5, 0.5), "first cell")])
@pytest.mark.parametrize("size", [(41, 33), (40, 32), (1, 1), (7, 10)])
def test_window_geometry(cell, where, size):
    sm = _sm()
    assert (sm.map_height, sm.map_width) == (200, 160)
    pose = _pose_at_cell(sm, *cell)
    origin, got_size, (cx, cy) = sm.live_map_window(pose, size)
    want_origin, (wx, wy) = lr.window_of(pose.to_array(), sm.map_boundary, sm.resolution, size)
    assert origin == want_origin and got_size == size and (cx, cy) == (wx, wy)
    # the centre cell is the cell a point at the vehicle's position is mapped to: truncation towards zero (astype(int32))
    centre = (int(np.trunc(cx)), int(np.trunc(cy)))
    assert abs(cx - cell[0]) < 1e-6 and abs(cy - cell[1]) < 1e-6
    assert origin == (centre[0] - size[0] // 2, centre[1] - size[1] // 2)
    # odd sizes put the centre cell in the middle, even sizes one cell after it
    assert origin[0] + size[0] // 2 == centre[0] and origin[1] + size[1] // 2 == centre[1]


def test_window_size_from_config_metres():
    sm = _sm(size_m=(4.15, 3.35))
    _, size, _ = sm.live_map_window(_pose_at_cell(sm, 10.5, 10.5))
    assert size == (41, 33)
    sm = _sm(res=0.2, boundary=((100.0, 140.0), (800.0, 832.0)), size_m=(60.0, 60.0))
    assert sm.live_map_window(_pose_at_cell(sm, 10.5, 10.5))[1] == (300, 300)


def test_heading_and_car_block():
    from vision_semantic_segmentation_amd import renderer as rr
    from vision_semantic_segmentation_amd.mapping import pose_heading
    from vision_semantic_segmentation_amd.utils import Pose
    for deg in (0.0, 90.0, 37.0, 181.5, -63.0):
        a = np.deg2rad(deg)
        pose = Pose((1.0, 2.0, 3.0), (0.0, 0.0, float(np.sin(a / 2)), float(np.cos(a / 2))))
        c, s = pose_heading(pose)
        assert (c, s) == lr.heading(pose.to_array())
        assert abs(c - np.cos(a)) < 1e-12 and abs(s - np.sin(a)) < 1e-12
    assert rr.car_block(3.5, 4.25, 0.6, 0.8, 0.1) == lr.car_block(3.5, 4.25, 0.6, 0.8, 0.1) == (3.5, 4.25, 0.6, 0.8, -10.0, 30.0, -9.0, 9.0)


def _err():
    from vision_semantic_segmentation_amd import _lib
    return _lib.last_error()


def test_argument_errors_through_the_c_abi():
    """every case returns -1 with a message and never reaches the device (there is none here)"""
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(4096)                      # never dereferenced: the arguments are refused first
    col = (C.c_uint8 * 48)(*([7] * 48))
    th = (C.c_double * 16)(*([0.01] * 16))
    fp = (C.c_int32 * 5)(0, 3, 4, 2, 1)

    def live(map_=fake, dt=_lib.AVL_F64, hm=20, wm=20, c=5, colors=col, h=4, w=4, flags=0, thresholds=None, out=fake, fill=fp, nfill=5):
        return L.avl_live_map(map_, dt, hm, wm, c, colors, 0, 0, h, w, flags, None, thresholds, fill, nfill, None, None, out, None)

    assert live(map_=None) == -1 and "map is NULL" in _err()
    assert live(out=None) == -1 and "out is NULL" in _err()
    assert live(c=17) == -1 and "C = 17" in _err()
    assert live(c=0) == -1 and "C = 0" in _err()
    assert live(h=0) == -1 and "window 0 x 4" in _err()
    assert live(w=0) == -1 and "window 4 x 0" in _err()
    assert live(h=-3) == -1 and "window" in _err()
    assert live(flags=_lib.AVL_LIVE_THRESHOLDS) == -1 and "without thresholds_host" in _err()
    assert live(flags=_lib.AVL_LIVE_THRESHOLDS | _lib.AVL_LIVE_FILL, thresholds=None) == -1 and "thresholds_host" in _err()
    assert live(dt=_lib.AVL_F16) == -1 and "map dtype" in _err()
    assert live(colors=None) == -1 and "colors_host is NULL" in _err()
    assert live(flags=8) == -1 and "flags" in _err()
    assert live(hm=1, flags=_lib.AVL_LIVE_FILTER) == -1 and "reflects" in _err()
    assert live(hm=2, flags=_lib.AVL_LIVE_FILL) == -1 and "3 x 3" in _err()
    assert live(flags=_lib.AVL_LIVE_FILL, fill=(C.c_int32 * 5)(0, 3, 5, 2, 1)) == -1 and "fill priority[2] = 5" in _err()
    assert live(flags=_lib.AVL_LIVE_FILL, nfill=17) == -1 and "fill priority list of 17" in _err()

    def fill(img=fake, x=10, y=10, colors=col, n=5, prio=fp, nprio=5, out=fake):
        return L.avl_fill_black(img, x, y, colors, n, prio, nprio, out, None)

    assert fill(img=None) == -1 and "NULL" in _err()
    assert fill(out=None) == -1 and "NULL" in _err()
    assert fill(x=2) == -1 and "X < 3" in _err()
    assert fill(y=2) == -1 and "3 x 3" in _err()
    assert fill(n=17) == -1 and "17 colours" in _err()
    assert fill(n=0) == -1 and "0 colours" in _err()
    assert fill(colors=None) == -1 and "colors_host is NULL" in _err()
    assert fill(prio=None) == -1 and "priority list is NULL" in _err()
    assert fill(n=3) == -1 and "fill priority[1] = 3 with 3 colours" in _err()


def test_python_front_ends_refuse_bad_arguments_before_the_device():
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    m = torch.zeros((6, 6, 5), dtype=torch.float64)     # a CPU tensor: the library refuses before it would read it
    with pytest.raises(IndexError):
        rr.render_window(m, lr.REF_COLORS, (0, 0), (4, 4), thresholds=[0.01] * 4)
    with pytest.raises(ValueError, match="priority"):
        rr.render_window(m, lr.REF_COLORS, (0, 0), (4, 4), thresholds=[0.01] * 5, priority=[0, 1])
    with pytest.raises(ValueError, match="channel should have a color"):
        rr.render_window(m, lr.REF_COLORS[:4], (0, 0), (4, 4))
    with pytest.raises(ValueError, match="car_block"):
        rr.render_window(m, lr.REF_COLORS, (0, 0), (4, 4), car=(1.0, 2.0))
    with pytest.raises(RuntimeError, match="avl_live_map failed"):
        rr.render_window(m, lr.REF_COLORS, (0, 0), (0, 4), stream=0)
    with pytest.raises(RuntimeError, match="fill priority"):
        rr.render_window(m, lr.REF_COLORS, (0, 0), (4, 4), fill=True, fill_priority=[0, 9], stream=0)
    with pytest.raises(ValueError, match="uint8"):
        rr.fill_black(torch.zeros((5, 5, 3), dtype=torch.float32))


def test_config_defaults():
    from vision_semantic_segmentation_amd import get_cfg_defaults
    lm = get_cfg_defaults().MAPPING.LIVE_MAP
    assert dict(lm) == {"ENABLED": False, "SIZE_M": [60.0, 60.0], "EVERY": 1, "FILTER": True, "RENDER": "argmax", "PRIORITY": None,
                        "THRESHOLDS": None, "FILL_BLACK": False, "FILL_PRIORITY": [0, 3, 4, 2, 1], "DRAW_CAR": True,
                        "CAR_SIZE": [4.0, 1.8]}
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["MAPPING.LIVE_MAP.ENABLED", True, "MAPPING.LIVE_MAP.EVERY", 3])
    assert cfg.MAPPING.LIVE_MAP.ENABLED is True and cfg.MAPPING.LIVE_MAP.EVERY == 3


@pytest.mark.parametrize("enabled", [False, True])
def test_disabled_live_map_leaves_mappings_call_sequence_unchanged(enabled, monkeypatch):
    """ENABLED = False: mapping() and mapping_views() do what they did -- one fused frame call, nothing of the live path.
    ENABLED = True: the live step follows the grid update, once per call."""
    from vision_semantic_segmentation_amd import SemanticMapping
    sm = _sm()
    sm.live_cfg.ENABLED = enabled
    calls = []
    monkeypatch.setattr(SemanticMapping, "frame_device", lambda self, *a, **k: calls.append("frame_device"))
    monkeypatch.setattr(SemanticMapping, "frame_device_views", lambda self, *a, **k: calls.append("frame_device_views"))
    monkeypatch.setattr(SemanticMapping, "_live_map_step", lambda self, pose: calls.append("live"))
    monkeypatch.setattr(SemanticMapping, "live_map", lambda self, *a, **k: calls.append("live_map"))
    monkeypatch.setattr(SemanticMapping, "finish_run", lambda self, *a, **k: calls.append("finish_run"))
    sm.pcd, sm.pcd_frame_id = np.zeros((4, 3)), "velodyne"
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    sm.mapping(img, None, sm.cam1)
    sm.mapping_views([img, img], None, [sm.cam1, sm.cam6])
    sm.save_map_to_file = True
    sm.mapping(img, None, sm.cam1)
    live = ["live"] if enabled else []
    assert calls == ["frame_device"] + live + ["frame_device_views"] + live + ["frame_device"] + live + ["finish_run"]
    assert sm.live_map_image is None and sm.live_map_host is None


def test_the_mapped_pose_is_remembered_with_the_live_map_disabled(monkeypatch):
    """live_map(pose=None) uses the last pose mapped, whether or not ENABLED made mapping() render"""
    from vision_semantic_segmentation_amd import SemanticMapping
    sm = _sm()
    assert sm.live_cfg.ENABLED is False
    monkeypatch.setattr(SemanticMapping, "frame_device", lambda self, *a, **k: None)
    monkeypatch.setattr(SemanticMapping, "frame_device_views", lambda self, *a, **k: None)
    seen = []
    monkeypatch.setattr("vision_semantic_segmentation_amd.renderer.render_window",
                        lambda map, colors, origin, size, **kw: seen.append((origin, size)) or "image")
    monkeypatch.setattr(SemanticMapping, "map_dev", property(lambda self: None))
    with pytest.raises(RuntimeError, match="needs a pose"):
        sm.live_map()
    sm.pcd, sm.pcd_frame_id = np.zeros((4, 3)), "velodyne"
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    first, second = _pose_at_cell(sm, 50.5, 20.5), _pose_at_cell(sm, 70.5, 30.5)
    sm.mapping(img, first, sm.cam1)
    assert sm.live_map() == "image" and seen[-1] == ((30, 4), (41, 33))
    sm.mapping_views([img, img], second, [sm.cam1, sm.cam6])
    sm.mapping(img, None, sm.cam1)                      # a frame without a pose keeps the last one
    assert sm.live_map() == "image" and seen[-1] == ((50, 14), (41, 33)) and sm.live_map_origin == (50, 14)
