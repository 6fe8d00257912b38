"""The live cost map's host side, without a GPU: the NumPy twin's distance against a scalar loop, the inflation table, the
OccupancyGrid geometry, the configuration, and the argument errors of avl_cost_map through the built library (nothing touches the
device before the arguments are checked)."""
import ctypes as C
import math

import numpy as np
import pytest

import _cost_map_reference as cr
import _live_map_reference as lr


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("radius", range(6))
def test_twin_distance_equals_a_scalar_triple_loop(radius):
    rng = np.random.default_rng(radius)
    for h, w in ((1, 1), (1, 12), (12, 1), (5, 7), (12, 12)):
        for density in (0.0, 0.03, 0.3, 1.0):
            lethal = rng.random((h + 2 * radius, w + 2 * radius)) < density
            got, want = cr.distance2(lethal, radius), cr.distance2_scalar(lethal, radius)
            assert got.shape == (h, w) and np.array_equal(got, want)
            assert ((got == 0) == lethal[radius:radius + h, radius:radius + w]).all()
            assert ((got <= radius * radius) | (got == cr.FAR)).all()


def test_twin_disc_rim_and_rule():
    base = np.zeros((11 + 10, 11 + 10), dtype=np.int64)
    base[5 + 5, 5 + 5] = 100                                      # window cell (5, 5)
    table = np.arange(100, 100 - 26, -1)
    cost, d2 = cr.finish(base, 5, table)
    assert d2[5 + 3, 5 + 4] == 25 and d2[5 + 4, 5 + 4] == cr.FAR and d2[5, 5] == 0 and d2[5, 0] == 25
    assert cost[5 + 3, 5 + 4] == 75 and cost[5 + 4, 5 + 4] == 0 and cost[5, 5] == 100
    base[:] = -1
    base[10, 10] = 100
    base[10, 12] = 60
    table = np.array([100] + [7] * 9 + [0] * 16)                  # the table's tail is 0 before R * R
    cost, d2 = cr.finish(base, 5, table)
    assert cost[5, 5] == 100 and cost[5, 6] == 7 and cost[5, 7] == 60 and cost[8, 5] == 7 and cost[9, 5] == -1 and d2[9, 5] == 16
    assert cost[0, 0] == -1 and d2[0, 0] == cr.FAR


# ------------------------------------------------------------------------------------------------ inflation_table
def test_inflation_table():
    from vision_semantic_segmentation_amd import renderer as rr
    for r, res, ins, decay, mx in ((0, 0.2, 0.9, 3.0, 99), (7, 0.2, 0.9, 3.0, 99), (15, 0.1, 0.9, 3.0, 99), (32, 0.05, 0.45, 10.0, 99),
                                   (5, 0.5, 0.0, 1.0, 50), (9, 0.2, 5.0, 3.0, 99)):
        t = rr.inflation_table(r, res, ins, decay, mx)
        assert isinstance(t, np.ndarray) and t.dtype == np.uint8 and t.shape == (r * r + 1,)
        assert t[0] == 100 and (t[1:] >= 1).all() and (t[1:] <= mx).all()
        assert (np.diff(t.astype(np.int64)) <= 0).all()
        d = np.sqrt(np.arange(r * r + 1, dtype=np.float64)) * res
        assert (t[1:][d[1:] <= ins] == mx).all()                                    # the inscribed plateau
        assert (t[1:][d[1:] > ins + 1.0 / decay] < mx).all()                         # and it ends: a decay length out, mx / e at the most
    # pinned by hand: R = 3, 0.5 m cells, inscribed 0.6 m, decay 2 / m.  d2 = 1: 0.5 m, inside.  d2 = 4: 1.0 m,
    # 99 exp(-0.8) = 44.48 -> 44.  d2 = 9: 1.5 m, 99 exp(-1.8) = 16.36 -> 16.  d2 = 2: 0.7071 m, 99 exp(-0.21421) = 79.91 -> 80
    t = rr.inflation_table(3, 0.5, 0.6, 2.0)
    assert t[0] == 100 and t[1] == 99 and t[2] == 80 and t[4] == 44 and t[9] == 16
    assert t[4] == max(1, round(99 * math.exp(-2.0 * (1.0 - 0.6))))
    assert rr.inflation_table(32, 0.2, 0.9, 3.0)[-1] == 1                             # far out the floor is 1, not 0
    with pytest.raises(ValueError):
        rr.inflation_table(33, 0.2, 0.9, 3.0)


# ------------------------------------------------------------------------------------------------ geometry and configuration
def _sm(boundary=((100.0, 120.0), (800.0, 816.0)), res=0.1, **cost):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = [list(boundary[0]), list(boundary[1])]
    cfg.MAPPING.RESOLUTION = res
    cfg.MAPPING.COST_MAP.SIZE_M = [4.15, 3.35]
    for k, v in cost.items():
        cfg.MAPPING.COST_MAP[k] = v
    return SemanticMapping(cfg, device="cpu", logger=MyLogger("test", quiet=True))


def _pose_at_cell(sm, cx, cy):
    from vision_semantic_segmentation_amd.utils import Pose
    x = sm.map_boundary[0][0] + cx * sm.resolution - lr.PCD_ORIGIN_OFFSET[0]
    y = sm.map_boundary[1][0] + cy * sm.resolution - lr.PCD_ORIGIN_OFFSET[1]
    return Pose((x, y, 0.0), (0.0, 0.0, 0.0, 1.0))


@pytest.mark.parametrize("cell", [(50.5, 20.25), (199.5, 159.5), (-30.5, 400.5), (0.5, 0.5)])
@pytest.mark.parametrize("size", [None, (40, 32), (1, 1), (7, 10)])
def test_cost_map_info_puts_the_pose_where_live_map_window_puts_it(cell, size):
    from vision_semantic_segmentation_amd.utils import Pose
    sm = _sm()
    pose = _pose_at_cell(sm, *cell)
    info = sm.cost_map_info(pose, size)
    h, w = (41, 33) if size is None else size                     # COST_MAP.SIZE_M in cells
    origin, got_size, (cx, cy) = sm.live_map_window(pose, (h, w))
    assert got_size == (h, w)
    assert info["resolution"] == 0.1 and (info["width"], info["height"]) == (h, w)
    # a pose in the middle of the window's first cell is put into that cell (on the grid: live_map_window truncates towards zero)
    if origin[0] >= 0 and origin[1] >= 0:
        first = Pose((info["origin_x"] + 0.5 * 0.1, info["origin_y"] + 0.5 * 0.1, 0.0), (0.0, 0.0, 0.0, 1.0))
        assert sm.live_map_window(first, (1, 1))[0] == origin
    px, py = pose.to_array()[:2]
    assert abs((px - info["origin_x"]) / 0.1 - (cx - origin[0])) < 1e-6 and abs((py - info["origin_y"]) / 0.1 - (cy - origin[1])) < 1e-6
    assert abs(info["origin_x"] - (sm.map_boundary[0][0] + origin[0] * 0.1 - lr.PCD_ORIGIN_OFFSET[0])) < 1e-9
    with pytest.raises(RuntimeError, match="needs a pose"):
        sm.cost_map_info()
    with pytest.raises(RuntimeError, match="needs a pose"):
        sm.cost_map()


def test_config_defaults():
    from vision_semantic_segmentation_amd import get_cfg_defaults
    cm = get_cfg_defaults().MAPPING.COST_MAP
    assert dict(cm) == {"ENABLED": False, "SIZE_M": [60.0, 60.0], "EVERY": 1, "FILTER": True, "RENDER": "argmax", "PRIORITY": None,
                        "THRESHOLDS": None, "CLASS_COST": [0, 0, 0, 100, 100], "UNKNOWN_COST": -1, "INFLATION_RADIUS_M": 1.5,
                        "INSCRIBED_RADIUS_M": 0.9, "DECAY_PER_M": 3.0, "CLEAR_FOOTPRINT": True, "CAR_SIZE": [4.0, 1.8], "ORDER": "yx"}
    sm = _sm()
    assert sm.cost_map_image is None and sm.cost_map_host is None and sm.cost_map_origin is None
    par = _sm(res=0.2, boundary=((100.0, 140.0), (800.0, 832.0)), ENABLED=True)._cost_par
    assert par["radius_cells"] == 7 and par["inflation"].shape == (50,) and par["class_cost"] == [0, 0, 0, 100, 100]
    assert par["unknown_cost"] == -1 and par["order"] == "yx" and par["thresholds"] is None


def test_class_cost_and_radius_are_checked_at_construction():
    with pytest.raises(ValueError, match="CLASS_COST"):
        _sm(ENABLED=True, CLASS_COST=[0, 0, 100, 100])
    with pytest.raises(ValueError, match="INFLATION_RADIUS_M"):
        _sm(ENABLED=True, INFLATION_RADIUS_M=3.35)                # 33 cells of 0.1 m
    assert _sm(ENABLED=True, INFLATION_RADIUS_M=3.25)._cost_par["radius_cells"] == 32


@pytest.mark.parametrize("enabled", [False, True])
def test_cost_map_step_follows_the_grid_update_only_when_enabled(enabled, monkeypatch):
    from vision_semantic_segmentation_amd import SemanticMapping
    sm = _sm()
    sm.cost_cfg.ENABLED = enabled
    calls = []
    monkeypatch.setattr(SemanticMapping, "frame_device", lambda self, *a, **k: calls.append("frame_device"))
    monkeypatch.setattr(SemanticMapping, "frame_device_views", lambda self, *a, **k: calls.append("frame_device_views"))
    monkeypatch.setattr(SemanticMapping, "_cost_map_step", lambda self, pose: calls.append("cost"))
    sm.pcd, sm.pcd_frame_id = np.zeros((4, 3)), "velodyne"
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    sm.mapping(img, None, sm.cam1)
    sm.mapping_views([img, img], None, [sm.cam1, sm.cam6])
    cost = ["cost"] if enabled else []
    assert calls == ["frame_device"] + cost + ["frame_device_views"] + cost


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def _err():
    from vision_semantic_segmentation_amd import _lib
    return _lib.last_error()


def test_argument_errors_through_the_c_abi():
    """every case returns AVL_E_ARG with a message and never reaches the device (there is none here)"""
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(4096)                      # never dereferenced: the arguments are refused first
    th = (C.c_double * 16)(*([0.01] * 16))
    ok_cost = [0, 0, 0, 100, 100, -1]

    def table(r, edit=None):
        t = [100] + [max(99 - k, 1) for k in range(r * r)]
        if edit:
            t[edit[0]] = edit[1]
        return (C.c_uint8 * len(t))(*t)

    def cost(map_=fake, dt=_lib.AVL_F64, hm=20, wm=20, c=5, h=4, w=6, flags=0, thresholds=None, costs=ok_cost, r=2, infl="ok", out=fake,
             si=6, sj=1, d2=None, scratch=fake, nbytes=1 << 20):
        cc = None if costs is None else (C.c_int8 * len(costs))(*costs)
        infl = table(r if 0 <= r <= 32 else 0) if infl == "ok" else infl
        return L.avl_cost_map(map_, dt, hm, wm, c, 0, 0, h, w, flags, None, thresholds, cc, None, r, infl, out, si, sj, d2, scratch, nbytes, None)

    assert cost(flags=_lib.AVL_LIVE_FILL) == -1 and "AVL_LIVE_FILL" in _err()
    assert cost(flags=_lib.AVL_LIVE_FILL | _lib.AVL_LIVE_FILTER) == -1 and "AVL_LIVE_FILL" in _err()
    assert cost(flags=8) == -1 and "flags" in _err()
    assert cost(r=33) == -1 and "radius_cells = 33" in _err()
    assert cost(r=-1) == -1 and "radius_cells = -1" in _err()
    assert cost(infl=table(2, (0, 99))) == -1 and "infl_host[0] = 99" in _err()
    assert cost(infl=table(2, (3, 99))) == -1 and "infl_host[3] = 99 after 98" in _err()
    assert cost(infl=table(2, (1, 101))) == -1 and "may not increase" in _err()       # above 100 is above entry 0
    assert cost(costs=[0, 0, 101, 100, 100, -1]) == -1 and "cost_host[2] = 101" in _err()
    assert cost(costs=[0, 0, 0, 100, 100, -2]) == -1 and "cost_host[5] = -2" in _err()
    for si, sj in ((1, 1), (6, 0), (0, 1), (5, 1), (1, 3), (2, 3), (-6, 1), (6, -1)):                    # aliasing, zero or negative strides
        assert cost(si=si, sj=sj) == -1 and "stride" in _err(), (si, sj)
    assert cost(h=0) == -1 and "window 0 x 6" in _err()
    assert cost(w=0) == -1 and "window 4 x 0" in _err()
    assert cost(h=32769) == -1 and "window" in _err()
    assert cost(map_=None) == -1 and "map is NULL" in _err()
    assert cost(out=None) == -1 and "cost_out is NULL" in _err()
    assert cost(costs=None) == -1 and "cost_host is NULL" in _err()
    assert cost(infl=None) == -1 and "infl_host is NULL" in _err()
    assert cost(scratch=None) == -1 and "scratch is NULL" in _err()
    assert cost(c=17, costs=[0] * 18) == -1 and "C = 17" in _err()
    assert cost(dt=_lib.AVL_F16) == -1 and "map dtype" in _err()
    assert cost(flags=_lib.AVL_LIVE_THRESHOLDS) == -1 and "without thresholds_host" in _err()
    assert cost(hm=1, flags=_lib.AVL_LIVE_FILTER) == -1 and "reflects" in _err()
    assert cost(nbytes=(4 + 4) * 16 - 1) == -1 and "scratch of" in _err()
    # the scratch size: the window plus its ring, rows padded to 16 bytes; 0 for what the call refuses
    assert L.avl_cost_map_scratch_bytes(4, 6, 2) == 8 * 16
    assert L.avl_cost_map_scratch_bytes(600, 600, 15) == 630 * 640
    assert L.avl_cost_map_scratch_bytes(1, 1, 0) == 16
    assert (600 + 30) * (600 + 30) <= L.avl_cost_map_scratch_bytes(600, 600, 15) <= 1.03 * 630 * 630
    for h, w, r in ((0, 4, 1), (4, 0, 1), (4, 4, 33), (4, 4, -1), (32769, 4, 0)):
        assert L.avl_cost_map_scratch_bytes(h, w, r) == 0


def test_python_front_end_refuses_bad_arguments_before_the_device():
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    m = torch.zeros((6, 6, 5), dtype=torch.float64)     # a CPU tensor: refused before anything would read it
    with pytest.raises(ValueError, match="class costs"):
        rr.cost_window(m, (0, 0), (4, 4), [0, 0, 100])
    with pytest.raises(ValueError, match="order"):
        rr.cost_window(m, (0, 0), (4, 4), [0] * 5, order="zz")
    with pytest.raises(ValueError, match="radius_cells = 33"):
        rr.cost_window(m, (0, 0), (4, 4), [0] * 5, radius_cells=33, inflation=[100])
    with pytest.raises(ValueError, match="inflation table"):
        rr.cost_window(m, (0, 0), (4, 4), [0] * 5, radius_cells=2)
    with pytest.raises(ValueError, match="entries"):
        rr.cost_window(m, (0, 0), (4, 4), [0] * 5, radius_cells=2, inflation=[100, 50])
    with pytest.raises(ValueError, match="car_block"):
        rr.cost_window(m, (0, 0), (4, 4), [0] * 5, car=(1.0, 2.0))
    with pytest.raises(IndexError):
        rr.cost_window(m, (0, 0), (4, 4), [0] * 5, thresholds=[0.01] * 4)
    with pytest.raises(ValueError, match="out must be"):
        rr.cost_window(m, (0, 0), (4, 6), [0] * 5, order="yx", out=torch.zeros((4, 6), dtype=torch.int8))
    with pytest.raises(RuntimeError, match="avl_cost_map failed"):
        rr.cost_window(m, (0, 0), (0, 4), [0] * 5, stream=0)
    with pytest.raises(RuntimeError, match="cost_host"):
        rr.cost_window(m, (0, 0), (4, 4), [0, 0, 0, 0, 101], stream=0)
