"""The live cost map on the GPU (csrc/seg_costmap.hip) against its NumPy twin (tests/_cost_map_reference.py): the base pass alone
against the classes render_window colours; the distance and inflation pass on one-hot grids, where the class is beyond doubt; the two
output orders; the unknown rule; the ego footprint; SemanticMapping.cost_map on mapped fixture frames and on a scrolled window.
Everything is compared for equality: there is no tolerance."""
import os

import numpy as np
import pytest

import _cost_map_reference as cr
import _live_map_reference as lr
from test_gpu_live_map import (CLASS_COUNTS, DTYPES, HM, LIVE_BOUNDARY, WINDOWS, WM, _Cam, _ids, _map_frame, _pose7, make_grid,
                               window_args)
from test_gpu_render_parity import colors

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
RADII = [0, 1, 2, 3, 5, 7, 8, 15, 16, 31, 32]
TILE = (32, 64)                                            # k_cost_inflate's output tile


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the base pass alone
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("c", CLASS_COUNTS)
def test_base_cost_is_the_class_render_window_colours(c, dtype, cuda_device):
    """R = 0 and the injective cost[k] = k + 1, unknown = -1: the cost names the class"""
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    m = torch.from_numpy(np.array(make_grid(c, dtype))).to(cuda_device)
    before = m.clone()
    col = np.array(colors(c), dtype=np.uint8)
    cost_of = list(range(1, c + 1))
    seen = set()
    for filt in (False, True):
        for thr in (False, True):
            args = window_args(c, filt, thr, False)
            for origin, size in WINDOWS:
                picture = _np(rr.render_window(m, col, origin, size, **args))
                want = np.full(size, -1, dtype=np.int8)
                for k in range(c):
                    want[(picture == col[k]).all(axis=2)] = k + 1
                assert ((want > 0) == (picture != 0).any(axis=2)).all()
                got, d2 = rr.cost_window(m, origin, size, cost_of, -1, filter=filt, thresholds=args["thresholds"], priority=args["priority"],
                                         d2_out=True)
                assert got.is_cuda and got.dtype == torch.int8 and tuple(got.shape) == tuple(size) and d2.dtype == torch.uint16
                got = _np(got)
                assert np.array_equal(got, want), "window %s %s filter %d thresholds %d: %d cells differ" % (
                    origin, size, filt, thr, int((got != want).sum()))
                assert (_np(d2) == cr.FAR).all()           # nothing costs 100 here
                seen.update(np.unique(got).tolist())
    assert torch.equal(before.view(torch.uint8), m.view(torch.uint8)), "cost_window wrote to the grid"
    assert seen >= set(cost_of[:min(c, 5)]) | {-1}, seen
    # wholly outside: unknown everywhere, whatever unknown costs
    assert (_np(rr.cost_window(m, (200, 10), (8, 8), cost_of, 55)) == 55).all()


# ------------------------------------------------------------------------------------------------ 2. distance and inflation
C2 = 4
COSTS2 = [0, 100, 37, -1]                                  # class 1 is lethal, class 3 carries no information
SIZES = [((1, 1), (50, 40)), ((1, 70), (20, 5)), ((70, 1), (10, 33)), (TILE, (7, 3)), ((TILE[0] + 1, TILE[1] + 1), (-2, -3)),
         ((70, 131), (-9, -20))]


def _grid_of(cls, dtype=np.float64):
    """one-hot grid of the classes cls int [HM, WM]; -1 = an empty cell"""
    m = np.zeros((HM, WM, C2), dtype=dtype)
    ii, jj = np.nonzero(cls >= 0)
    m[ii, jj, cls[ii, jj]] = 1
    return m


def _plane(cls, origin, size, r):
    """the classes of the window and its ring of r cells, C2 where the grid has none"""
    h, w = size[0] + 2 * r, size[1] + 2 * r
    gi, gj = np.arange(h) + origin[0] - r, np.arange(w) + origin[1] - r
    vi, vj = (gi >= 0) & (gi < HM), (gj >= 0) & (gj < WM)
    out = np.full((h, w), C2, dtype=np.int64)
    if vi.any() and vj.any():
        sub = cls[np.ix_(gi[vi], gj[vj])]
        out[np.ix_(vi, vj)] = np.where(sub < 0, C2, sub)
    return out


def _check(m, cls, origin, size, r, table, costs=COSTS2, unknown=-1, car=None, what=""):
    from vision_semantic_segmentation_amd import renderer as rr
    cost, d2 = rr.cost_window(m, origin, size, costs, unknown, r, table, filter=False, car=car, d2_out=True)
    want_cost, want_d2 = cr.finish(cr.base_plane(_plane(cls, origin, size, r), origin, r, costs, unknown, car), r, table)
    cost, d2 = _np(cost), _np(d2)
    assert d2.dtype == np.uint16 and np.array_equal(d2, want_d2), "%s R %d window %s %s: %d clearances differ" % (
        what, r, origin, size, int((d2 != want_d2).sum()))
    assert cost.dtype == np.int8 and np.array_equal(cost, want_cost), "%s R %d window %s %s: %d costs differ" % (
        what, r, origin, size, int((cost != want_cost).sum()))
    return cost, d2


def _ring_only(origin, size, r, rng):
    """lethal cells in the ring of r cells outside the window and nowhere else"""
    gi, gj = np.arange(HM)[:, None], np.arange(WM)[None, :]
    near = (gi >= origin[0] - r) & (gi < origin[0] + size[0] + r) & (gj >= origin[1] - r) & (gj < origin[1] + size[1] + r)
    inside = (gi >= origin[0]) & (gi < origin[0] + size[0]) & (gj >= origin[1]) & (gj < origin[1] + size[1])
    return near & ~inside & (rng.random((HM, WM)) < 0.3)


@pytest.mark.parametrize("r", RADII)
def test_distance_and_inflation_equal_the_twin(r, cuda_device):
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    rng = np.random.default_rng(100 + r)
    table = rr.inflation_table(r, 0.25, 0.6, 1.0)
    dtype = np.float64 if r % 2 else np.float32
    hit = 0
    for size, origin in SIZES:
        background = rng.choice([-1, 0, 2, 3], size=(HM, WM))
        sets = {"none": np.zeros((HM, WM), dtype=bool), "all": np.ones((HM, WM), dtype=bool), "ring": _ring_only(origin, size, r, rng)}
        for density in (0.002, 0.05, 0.5):
            sets["%g" % density] = rng.random((HM, WM)) < density
        for name, lethal in sets.items():
            cls = np.where(lethal, 1, background)
            m = torch.from_numpy(_grid_of(cls, dtype)).to(cuda_device)
            before = m.clone()
            cost, d2 = _check(m, cls, origin, size, r, table, what=name)
            assert torch.equal(before, m), "cost_window wrote to the grid"
            if name == "ring" and r and lethal.any() and size != (1, 1):
                assert (cost < 100).all() and (d2 > 0).all()
                hit += int((d2 <= r * r).sum())
    assert hit > 0 or r == 0, "the ring's lethal cells reached no window"
    # everything off the grid is lethal and inflates into a window at the grid's edge
    solid = rng.choice([0, 2, 3], size=(HM, WM))
    m = torch.from_numpy(_grid_of(solid, dtype)).to(cuda_device)
    for size, origin in (((TILE[0] + 1, TILE[1] + 1), (-2, -3)), ((70, 131), (-9, -20)), ((1, 70), (95, 30)), ((5, 7), (40, 40))):
        cost, d2 = _check(m, solid, origin, size, r, table, unknown=100, what="off the grid is lethal")
        if size != (5, 7):
            assert (cost == 100).any()
            assert r == 0 or ((d2 > 0) & (d2 <= r * r)).any()


@pytest.mark.parametrize("r", RADII)
def test_one_lethal_cell_walked_around_a_probe(r, cuda_device):
    """One lethal cell at every offset of the (2R + 3)^2 square around the probe cell, in a grid that is free elsewhere; the window
    is two rows of 66 cells with the probe at (1, 40), so every lane and a second tile see the cell too.  The twin is evaluated once,
    for one lethal cell in a plane large enough to hold every relative position: the rule is invariant under translation."""
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    table = rr.inflation_table(r, 0.25, 0.6, 1.0)
    k = r + 1
    probe, origin, size = (48, 40), (47, 0), (2, 66)
    qh, qw = k + 1, probe[1] + k                            # the relative positions (cell - lethal cell) that occur
    base = np.zeros((2 * qh + 1 + 2 * r, 2 * qw + 1 + 2 * r), dtype=np.int64)
    base[qh + r, qw + r] = 100
    w_cost, w_d2 = cr.finish(base, r, table)
    cls = np.zeros((HM, WM), dtype=np.int64)
    m = torch.from_numpy(_grid_of(cls)).to(cuda_device)
    free, lethal = m[0, 0].clone(), torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=m.dtype, device=cuda_device)
    offsets = [(a, b) for a in range(-k, k + 1) for b in range(-k, k + 1)]
    cost = torch.empty((len(offsets),) + size, dtype=torch.int8, device=cuda_device)
    d2 = torch.empty((len(offsets),) + size, dtype=torch.uint16, device=cuda_device)
    for n, (a, b) in enumerate(offsets):
        m[probe[0] + a, probe[1] + b] = lethal
        rr.cost_window(m, origin, size, COSTS2, -1, r, table, filter=False, out=cost[n], d2_out=d2[n])
        m[probe[0] + a, probe[1] + b] = free
    cost, d2 = _np(cost), _np(d2)
    for n, (a, b) in enumerate(offsets):
        i0, j0 = qh + origin[0] - (probe[0] + a), qw + origin[1] - (probe[1] + b)
        assert np.array_equal(d2[n], w_d2[i0:i0 + 2, j0:j0 + 66]), (r, a, b)
        assert np.array_equal(cost[n], w_cost[i0:i0 + 2, j0:j0 + 66]), (r, a, b)
        q = a * a + b * b                                  # the probe itself: inside the disc or not
        assert d2[n, 1, 40] == (q if q <= r * r else cr.FAR) and cost[n, 1, 40] == (table[q] if q <= r * r else 0)
    if r == 5:                                             # the disc's rim
        assert d2[offsets.index((3, 4)), 1, 40] == 25 and d2[offsets.index((4, 4)), 1, 40] == cr.FAR
        assert d2[offsets.index((-5, 0)), 1, 40] == 25 and d2[offsets.index((0, 6)), 1, 40] == cr.FAR


# ------------------------------------------------------------------------------------------------ 3. the two orders
def test_order_yx_is_the_transpose_of_xy(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    rng = np.random.default_rng(3)
    cls = np.where(rng.random((HM, WM)) < 0.04, 1, rng.choice([-1, 0, 2, 3], size=(HM, WM)))
    m = torch.from_numpy(_grid_of(cls)).to(cuda_device)
    table = rr.inflation_table(5, 0.25, 0.6, 1.0)
    for size in ((1, 1), (1, 70), (70, 1), (31, 63), (33, 65), (2, 3), (70, 131)):
        for origin in ((5, 4), (-6, -7)):
            xy, d_xy = rr.cost_window(m, origin, size, COSTS2, -1, 5, table, filter=False, order="xy", d2_out=True)
            yx, d_yx = rr.cost_window(m, origin, size, COSTS2, -1, 5, table, filter=False, order="yx", d2_out=True)
            assert tuple(xy.shape) == size and tuple(yx.shape) == size[::-1] and yx.is_contiguous() and d_yx.is_contiguous()
            assert np.array_equal(_np(yx), _np(xy).T) and np.array_equal(_np(d_yx), _np(d_xy).T), (size, origin)
            _check(m, cls, origin, size, 5, table)
            given = torch.full(size[::-1], 77, dtype=torch.int8, device=cuda_device)
            assert rr.cost_window(m, origin, size, COSTS2, -1, 5, table, filter=False, order="yx", out=given) is given
            assert torch.equal(given, yx)


# ------------------------------------------------------------------------------------------------ 4. the unknown rule
def test_unknown_cells_inside_and_outside_the_inflation_radius(cuda_device):
    import torch
    cls = np.full((HM, WM), -1, dtype=np.int64)
    cls[40, 30] = 1                                        # the one lethal cell
    cls[40, 32] = 2                                        # a known cell at d2 = 4: keeps its 37 against the table's 7
    cls[44, 30] = 0                                        # a known free cell at d2 = 16, where the table is 0
    cls[30:36, 30] = 3                                     # a class that carries no information, beyond the radius
    m = torch.from_numpy(_grid_of(cls)).to(cuda_device)
    table = np.array([100] + [7] * 9 + [0] * 16, dtype=np.uint8)         # the tail is 0 before R * R = 25
    cost, d2 = _check(m, cls, (30, 20), (21, 21), 5, table)
    at = lambda gx, gy: (int(cost[gx - 30, gy - 20]), int(d2[gx - 30, gy - 20]))
    assert at(40, 30) == (100, 0) and at(40, 31) == (7, 1) and at(40, 32) == (37, 4) and at(43, 30) == (7, 9)
    assert at(44, 30) == (0, 16) and at(40, 34) == (-1, 16) and at(43, 34) == (-1, 25) and at(40, 36) == (-1, cr.FAR)
    assert at(35, 30) == (-1, 25) and at(34, 30) == (-1, cr.FAR)
    full = np.array([100] + [7] * 25, dtype=np.uint8)
    cost, d2 = _check(m, cls, (30, 20), (21, 21), 5, full)
    assert int(cost[13, 14]) == 7 and int(cost[14, 10]) == 7 and int(cost[5, 10]) == 7 and int(cost[4, 10]) == -1


# ------------------------------------------------------------------------------------------------ 5. the ego footprint
@pytest.mark.parametrize("yaw", [0.0, 30.0, 45.0, 90.0, 201.0])
def test_footprint_is_cleared_and_does_not_inflate(yaw, cuda_device):
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    cls = np.ones((HM, WM), dtype=np.int64)                 # a lethal grid underneath
    m = torch.from_numpy(_grid_of(cls)).to(cuda_device)
    table = rr.inflation_table(3, 0.2, 0.3, 2.0)
    c, s = lr.heading(_pose7(0.0, 0.0, yaw))
    for (cx, cy), origin, size in (((50.5, 36.5), (30, 20), (41, 33)), ((50.0, 36.0), (30, 20), (41, 33)), ((31.3, 50.8), (30, 20), (41, 33)),
                                   ((94.25, 70.5), (80, 54), (30, 40))):
        car = rr.car_block(cx, cy, c, s, 0.2)               # 20 x 9 cells
        cost, d2 = _check(m, cls, origin, size, 3, table, car=car, what="yaw %g" % yaw)
        mask = lr.car_mask(origin, size, car)
        on_grid = _plane(cls, origin, size, 0) == 1
        assert mask.any() and np.array_equal((d2 > 0) & on_grid, mask & on_grid)
        assert (cost[mask] < 100).all() and (cost[~mask & on_grid] == 100).all()
        deep = mask & (d2 == cr.FAR)                        # more than 3 cells from the rectangle's rim: nothing inflates into them
        if (cx, cy) == (50.5, 36.5):
            assert deep.any()
        assert (cost[deep] == 0).all()
    # off the grid too: the rectangle clears "unknown = lethal" cells beyond the last row
    car = rr.car_block(100.0, 40.0, c, s, 0.2)
    cost, d2 = _check(m, cls, (90, 20), (30, 40), 3, table, unknown=100, car=car, what="off the grid")
    assert (cost < 100).any()


# ------------------------------------------------------------------------------------------------ 6. SemanticMapping.cost_map
COST_SIZE_M = [20.6, 16.6]                                 # 41 x 33 cells of 0.5 m
CLASS_COST = [100, 20, 0, 100, 100]                        # the road is lethal too here: the fixture frames map mostly road


def _cost_sm(device, **cost):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils import Pose
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    g = np.load(os.path.join(GOLDEN, "mapping_W_world_pose_cam6.npz"))
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY, cfg.MAPPING.RESOLUTION = LIVE_BOUNDARY, 0.5
    cfg.MAPPING.PCD.USE_INTENSITY = bool(g["use_intensity"])
    cfg.MAPPING.COST_MAP.SIZE_M = COST_SIZE_M
    cfg.MAPPING.COST_MAP.CLASS_COST = CLASS_COST
    for k, v in cost.items():
        cfg.MAPPING.COST_MAP[k] = v
    sm = SemanticMapping(cfg, device=device, logger=MyLogger("test", quiet=True))
    sm.confusion_matrix = np.array(g["cm"])
    sm.pcd_frame_id = str(g["frame"])
    return sm, g, Pose.from_array(g["pose7"]), _Cam(g["P"])


def _expected_cost(sm, pose7, boundary, size=(41, 33), clear=True):
    """the twin on the grid as it is now: the existing GPU filter and renderer over the whole grid, then everything else in NumPy"""
    from vision_semantic_segmentation_amd import renderer as rr
    origin, (cx, cy) = lr.window_of(pose7, boundary, sm.resolution, size)
    whole = _np(rr.render_bev_map(rr.apply_filter(sm.map_dev).to(sm.map_dev.dtype), sm.label_colors))
    r = int(1.5 / sm.resolution)
    table = rr.inflation_table(r, sm.resolution, 0.9, 3.0)
    car = lr.car_block(cx, cy, *lr.heading(pose7), resolution=sm.resolution) if clear else None
    cost, d2 = cr.cost_map(whole, sm.label_colors, origin, size, list(sm.cost_cfg.CLASS_COST), -1, r, table, car)
    return origin, r, table, car, cost, d2


def test_cost_map_on_mapped_frames_equals_cost_window_and_the_twin(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    sm, g, pose, cam = _cost_sm(cuda_device)
    _map_frame(sm, g, pose, cam, 0)
    _map_frame(sm, g, pose, cam, 1)
    assert sm.cost_map_image is None and sm.cost_map_host is None          # ENABLED is off: mapping() computed nothing
    before = sm.map_dev.clone()
    origin, r, table, car, want, want_d2 = _expected_cost(sm, g["pose7"], LIVE_BOUNDARY)
    assert r == 3 and origin == (20, 4)
    got, d2 = sm.cost_map(d2=True)
    assert got.is_cuda and got.dtype == torch.int8 and tuple(got.shape) == (33, 41) and sm.cost_map_origin == origin
    assert np.array_equal(_np(got), want.T) and np.array_equal(_np(d2), want_d2.T)       # ORDER "yx"
    direct = rr.cost_window(sm.map_dev, origin, (41, 33), CLASS_COST, -1, r, table, car=rr.car_block(*car[:4], resolution=0.5), order="yx")
    assert torch.equal(direct, got)
    assert (want == 100).sum() > 20 and ((want > 0) & (want < 100)).sum() > 20 and (want == -1).any() and (want == 0).any()
    info = sm.cost_map_info()
    assert info == sm.cost_map_info(pose) and (info["width"], info["height"]) == (41, 33) and info["resolution"] == 0.5
    assert info["origin_x"] == LIVE_BOUNDARY[0][0] + 20 * 0.5 - lr.PCD_ORIGIN_OFFSET[0]
    sm.cost_cfg.ORDER, sm._cost_par = "xy", None
    sm.cost_cfg.CLEAR_FOOTPRINT = False
    _, _, _, _, want, _ = _expected_cost(sm, g["pose7"], LIVE_BOUNDARY, size=(12, 30), clear=False)
    out = torch.empty((12, 30), dtype=torch.int8, device=cuda_device)
    assert sm.cost_map(pose=pose, size_cells=(12, 30), out=out) is out and np.array_equal(_np(out), want)
    assert torch.equal(before, sm.map_dev), "cost_map changed the grid"


def test_enabled_cost_map_runs_every_second_frame_into_pinned_memory(cuda_device):
    import torch
    sm, g, pose, cam = _cost_sm(cuda_device, ENABLED=True, EVERY=2)
    images = []
    for k in range(4):
        _map_frame(sm, g, pose, cam, k)
        images.append(sm.cost_map_image)
        if k % 2 == 0:                                     # computed on this frame: the grid as it is now
            want = _expected_cost(sm, g["pose7"], LIVE_BOUNDARY)[4]
            assert np.array_equal(_np(sm.cost_map_image), want.T)
            torch.cuda.current_stream(cuda_device).synchronize()
            assert sm.cost_map_host.is_pinned() and sm.cost_map_host.dtype == torch.int8
            assert np.array_equal(sm.cost_map_host.numpy(), _np(sm.cost_map_image))
    assert images[0] is images[1] and images[2] is images[3] and images[1] is not images[2]
    assert not torch.equal(images[0], images[2])           # two more frames have been mapped in between
    assert sm.live_map_image is None                       # the live map stays off


# ------------------------------------------------------------------------------------------------ 7. scrolling
def test_cost_map_follows_a_scrolled_window(cuda_device):
    import _scroll_reference as ref
    from test_gpu_scroll import run_frames
    from vision_semantic_segmentation_amd import SemanticMapping, scroll as s
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    res, Hm, Wm = 0.25, 96, 64
    d = ref.Drive([(13.0, 9.0, 0.2), (30.5, -18.25, 0.6)], res=res, Hm=Hm, Wm=Wm, tile_m=4.0, range_max=12.0, n_points=1500, seed=9)
    d.anchor = (1300.0, 500.0)                             # integer metres: every boundary float is exact
    d.boundary = [[1300.0, 1300.0 + Hm * res], [500.0, 500.0 + Wm * res]]
    d.origins = ref.origins_of(d.poses, d.anchor, res, d.Ht, d.Wt, d.T, 1)
    cfg = d.cfg()
    cfg.MAPPING.COST_MAP.SIZE_M = [16.0, 12.0]             # 64 x 48 cells
    cfg.MAPPING.COST_MAP.CLASS_COST = CLASS_COST
    sm = SemanticMapping(cfg, device=cuda_device, logger=MyLogger("test", quiet=True))
    run_frames(sm, d, [0])
    first = sm.cost_map_info(d.poses[0])
    run_frames(sm, d, [1])
    O = d.origins[1][0]
    assert sm.scroll_origin == O and O != d.origins[0][0] and sm.scroll_count == 2
    boundary = s.window_boundary(d.anchor, O, Hm, Wm, res)
    assert boundary == sm.map_boundary
    pose7 = np.asarray(d.poses[1], dtype=np.float64)
    origin, r, table, car, want, want_d2 = _expected_cost(sm, pose7, boundary, size=(64, 48))
    got, d2 = sm.cost_map(d2=True)
    assert r == 6 and sm.cost_map_origin == origin and tuple(got.shape) == (48, 64)
    assert np.array_equal(_np(got), want.T) and np.array_equal(_np(d2), want_d2.T)
    assert (want >= 0).sum() > 100
    info = sm.cost_map_info()
    assert info["origin_x"] == boundary[0][0] + origin[0] * res - lr.PCD_ORIGIN_OFFSET[0]
    assert info["origin_y"] == boundary[1][0] + origin[1] * res - lr.PCD_ORIGIN_OFFSET[1]
    # the cost map moved with the vehicle in the map frame, to the cell, although the grid's cells were renumbered in between
    move = pose7[:2] - np.asarray(d.poses[0], dtype=np.float64)[:2]
    assert abs(move[0]) > 10 * res and abs(move[1]) > 10 * res
    assert abs((info["origin_x"] - first["origin_x"]) - move[0]) <= res and abs((info["origin_y"] - first["origin_y"]) - move[1]) <= res
