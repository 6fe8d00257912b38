"""The scrolling grid (MAPPING.SCROLL) on the GPU.

* k_tile_copy against the NumPy executor of _scroll_reference.py, byte for byte: the scroll tables of test_scroll_cpu.py (a 24 x 16
  window with T = 4 for layers of 40, 12, 8 and 4 bytes, each with its fill word; a 200 x 300 window with T = 100 and 40 bytes, whose
  4000-byte rows are no multiple of a wave's 1024 and whose tiles are split over workgroups), every buffer and the flags between
  guard strips of 0xAB that must survive, as must everything inside the buffers that no job names;
* the drive of _scroll_reference.main_drive through mapping_views with two cameras: site_map() and site_tiles() against the NumPy
  site on one big array, bit for bit (identity and log confusion matrix on f64, f32), the scroll count what next_origin dictates;
  test_scroll_cpu.py asserts that this drive scrolls on each axis, diagonally, jumps, re-enters stored tiles and adds to them;
* the same invariant once at RESOLUTION 0.1 with origins of several tiles;
* a scrolled instance against a fresh non-scrolling one with MAPPING.BOUNDARY = window_boundary(origin) and the window's content:
  frame_device_views, ground_fill_device, live_map and live_view give bit-equal grids and pictures;
* no scroll, nothing happens; there and back with the elevation layer; save_site / load_site."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _scroll_reference as ref

pytestmark = pytest.mark.gpu

SHIFTS = [(0, 1), (-1, 0), (1, -2), (6, 0), (9, -5)]
SMALL = [(40, 0), (12, 0), (8, 0), (4, 0x7FFFFFFF), (4, 0x80000000)]
GUARD = 256


# ------------------------------------------------------------------------------------------------ the kernel against the executor
def run_table_on_device(case, device):
    """-> ({key: bytes after the launch, guards included}, flags with guards): case.jobs through validate_jobs, encode_jobs and
    avl_tile_copy, every buffer of case.bufs between two guard strips of 0xAB"""
    import torch
    from vision_semantic_segmentation_amd import _lib, scroll as s
    n_flags = len(case.plan["leaving"])
    dev, extents = {}, {}
    for key, host in case.bufs.items():
        t = torch.full((GUARD + host.size + GUARD,), 0xAB, dtype=torch.uint8, device=device)
        t[GUARD:GUARD + host.size] = torch.from_numpy(host).to(device)
        dev[key] = t
        extents[key] = (t.data_ptr() + GUARD, int(host.size))
    s.validate_jobs(case.jobs, extents, case.T, case.bpc, n_flags)
    rec = np.zeros(len(case.jobs), dtype=s.JOB_DTYPE)
    s.encode_jobs(case.jobs, extents, rec)
    table = torch.from_numpy(rec.view(np.uint8)).to(device)
    flags = torch.full((16 + n_flags + 16,), -0x54545455, dtype=torch.int32, device=device)       # 0xABABABAB
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = _lib.lib().avl_tile_copy(C.c_void_p(table.data_ptr()), len(case.jobs), case.T, case.bpc, case.fill,
                                  C.c_void_p(flags.data_ptr() + 64), n_flags, C.c_void_p(stream))
    _lib.check(rc, "avl_tile_copy")
    torch.cuda.synchronize(device)
    return {k: t.cpu().numpy() for k, t in dev.items()}, flags.cpu().numpy()


def check_table(case, device):
    n_flags = len(case.plan["leaving"])
    got, got_flags = run_table_on_device(case, device)
    want_flags = ref.execute_jobs(case.jobs, case.bufs, case.T, case.bpc, case.fill, n_flags)     # writes case.bufs in place
    assert np.array_equal(case.bufs["new"].reshape(case.Hm, case.Wm, case.bpc),
                          case.site.view((case.new[0] * case.T, case.new[1] * case.T), case.Hm, case.Wm))
    for key, want in case.bufs.items():
        g = got[key]
        assert (g[:GUARD] == 0xAB).all() and (g[-GUARD:] == 0xAB).all(), "guard strip of %r written" % (key,)
        assert np.array_equal(g[GUARD:-GUARD], want), "%r: %d bytes differ" % (key, int((g[GUARD:-GUARD] != want).sum()))
    assert (got_flags[:16] == -0x54545455).all() and (got_flags[-16:] == -0x54545455).all(), "guard of the flags written"
    assert np.array_equal(got_flags[16:16 + n_flags], want_flags)
    assert np.array_equal(want_flags, case.want_flags()) and want_flags.sum() > 0
    return want_flags


@pytest.mark.parametrize("bpc,fill", SMALL, ids=["40", "12", "8", "4_max", "4_min"])
@pytest.mark.parametrize("shift", SHIFTS, ids=["%d_%d" % s for s in SHIFTS])
def test_tile_copy_small_window(shift, bpc, fill, cuda_device):
    flags = check_table(ref.TableCase(shift, bpc, fill, 4, 6, 4, 5, (2, -1)), cuda_device)
    assert 0 < flags.sum() < flags.size                             # some leaving tile is empty, some is not


@pytest.mark.parametrize("shift", SHIFTS, ids=["%d_%d" % s for s in SHIFTS])
def test_tile_copy_rows_of_4000_bytes(shift, cuda_device):
    check_table(ref.TableCase(shift, 40, 0, 100, 2, 3, 5, (2, -1)), cuda_device)


@pytest.mark.parametrize("bpc,fill", [(40, 0), (4, 0x7FFFFFFF)], ids=["40", "4_max"])
def test_tile_copy_ignores_the_fresh_word(bpc, fill, cuda_device):
    """struct avl_tile_job's last word is avl_tile_merge's: with 1 in every record the copy is the executor's, byte for byte"""
    from vision_semantic_segmentation_amd import scroll as s
    case = ref.TableCase((1, -2), bpc, fill, 4, 6, 4, 5, (2, -1))
    case.jobs = [j._replace(fresh=1) for j in case.jobs]
    rec = np.zeros(len(case.jobs), dtype=s.JOB_DTYPE)
    s.encode_jobs(case.jobs, case.extents, rec)
    assert (rec["fresh"] == 1).all()                                # the word reaches the device table
    check_table(case, cuda_device)


# ------------------------------------------------------------------------------------------------ the drive
_DRIVES = {}


def drive(name):
    if name not in _DRIVES:
        if name == "main":
            _DRIVES[name] = ref.main_drive()
        else:                                             # RESOLUTION 0.1: T = 20, a 120 x 80 window; origins of several tiles
            route = [(21.3, 13.1, 0.0), (23.3, 13.1, 0.4), (25.9, 15.2, 0.8), (29.3, 17.3, 1.0), (23.1, 11.0, math.pi)]
            _DRIVES[name] = ref.Drive(route, res=0.1, Hm=120, Wm=80, tile_m=2.0, range_max=7.0, n_points=1500, seed=4)
    return _DRIVES[name]


def make_sm(d, device, grid_dtype="f64", cm="identity", scroll=True, elevation=False, boundary=None):
    from vision_semantic_segmentation_amd import SemanticMapping, synthetic as syn
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    sm = SemanticMapping(d.cfg(grid_dtype, scroll, elevation, boundary), device=device, logger=MyLogger("test", quiet=True))
    if cm == "log":
        sm.confusion_matrix = syn.log_confusion(sm.map_depth)
    assert (sm.map_height, sm.map_width) == (d.Hm, d.Wm)
    return sm


def run_frames(sm, d, frames):
    import torch
    for k in frames:
        sm.pcd, sm.pcd_frame_id = d.clouds[k], "world"
        sm.mapping_views([torch.from_numpy(im).to(sm.device) for im in d.images[k]], d.poses[k], d.cams)


def check_site(sm, site, what=""):
    tiles = site.nonempty_tiles()
    assert sm.site_tiles() == sorted(tiles), what
    (i0, j0), want = site.region(tiles)
    origin, got = sm.site_map()
    got = got.cpu().numpy()
    assert origin == (i0, j0) and got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d of %d values differ, max |delta| %g" % (what, int((got != want).sum()), want.size, float(np.abs(got - want).max()))


@pytest.mark.parametrize("cm,grid_dtype", [("identity", "f64"), ("log", "f64"), ("log", "f32")], ids=["identity_f64", "log_f64", "log_f32"])
def test_drive_site_equals_the_numpy_site(cm, grid_dtype, cuda_device):
    d = drive("main")
    sm = make_sm(d, cuda_device, grid_dtype, cm)
    site = d.numpy_site(sm.confusion_matrix, np.float64 if grid_dtype == "f64" else np.float32)
    prev = (0, 0)
    for k in range(len(d.poses)):
        before = sm.last_scroll
        run_frames(sm, d, [k])
        origin, moved = d.origins[k]
        assert sm.scroll_origin == origin, k
        if moved:
            assert sm.last_scroll["shift"] == ((origin[0] - prev[0]) // d.T, (origin[1] - prev[1]) // d.T)
            assert sm.last_scroll["entering"] == sm.last_scroll["loaded"] + sm.last_scroll["filled"]
        else:
            assert sm.last_scroll is before
        prev = origin
    assert sm.scroll_count == sum(1 for _, moved in d.origins if moved) >= 5
    assert sm.map_boundary == ref.window_boundary(d.anchor, d.origins[-1][0], d.Hm, d.Wm, d.res)
    check_site(sm, site, "%s %s" % (cm, grid_dtype))
    # a rectangle that cuts through window, store and nothing
    (i0, j0), got = sm.site_map(rect=(-5, -2, -4, 1))
    assert (i0, j0) == (-5 * d.T, -4 * d.T)
    pad = ref.BigSite((-8, d.tile_rect[1], -8, d.tile_rect[3]), d.T, (5,), site.big.dtype)
    pad.view((site.I, site.J), *site.big.shape[:2])[...] = site.big
    assert np.array_equal(got.cpu().numpy(), pad.big[3 * d.T:7 * d.T, 4 * d.T:10 * d.T])


def test_drive_at_resolution_0_1(cuda_device):
    d = drive("fine")
    assert sum(1 for _, moved in d.origins if moved) >= 3 and all(abs(o[0]) >= 3 * d.T for o, _ in d.origins)
    sm = make_sm(d, cuda_device, "f64", "log")
    site = d.numpy_site(sm.confusion_matrix)
    run_frames(sm, d, range(len(d.poses)))
    assert sm.scroll_count == sum(1 for _, moved in d.origins if moved)
    check_site(sm, site, "resolution 0.1")


# ------------------------------------------------------------------------------------------------ a scrolled instance equals a fresh one
def test_scrolled_instance_equals_a_fresh_one_with_that_boundary(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import scroll as s
    res, Hm, Wm = 0.25, 96, 64
    route = [(13.0, 9.0, 0.2), (30.5, -18.25, 0.6)]
    d = ref.Drive(route, res=res, Hm=Hm, Wm=Wm, tile_m=4.0, range_max=12.0, n_points=1500, seed=9)
    d.anchor = (1300.0, 500.0)                                                    # integer metres: every boundary float is exact
    d.boundary = [[1300.0, 1300.0 + Hm * res], [500.0, 500.0 + Wm * res]]
    d.origins = ref.origins_of(d.poses, d.anchor, res, d.Ht, d.Wt, d.T, 1)
    cfg = d.cfg()
    cfg.MAPPING.GROUND_FILL.ENABLED = False
    cfg.MAPPING.GROUND_FILL.SIZE_M = [22.0, 14.0]          # the cameras see the ground from 5.4 m ahead of the sensor on
    cfg.MAPPING.GROUND_FILL.RANGE_MAX = 12.0
    cfg.MAPPING.LIVE_MAP.SIZE_M = [16.0, 12.0]
    cfg.MAPPING.LIVE_VIEW.SIZE_PX = [72, 56]
    from vision_semantic_segmentation_amd import SemanticMapping
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    a = SemanticMapping(cfg, device=cuda_device, logger=MyLogger("test", quiet=True))
    run_frames(a, d, [0, 1])
    O = d.origins[1][0]
    assert a.scroll_origin == O and a.scroll_count == 2 and O != d.origins[0][0]
    boundary = s.window_boundary(d.anchor, O, Hm, Wm, res)
    assert boundary == a.map_boundary and all(float(v) == float(int(v * 4) / 4.0) for row in boundary for v in row)
    cfg_b = cfg.clone()
    cfg_b.MAPPING.SCROLL.ENABLED = False
    cfg_b.MAPPING.BOUNDARY = boundary
    b = SemanticMapping(cfg_b, device=cuda_device, logger=MyLogger("test", quiet=True))
    assert b._scroll is None and (b.map_height, b.map_width) == (Hm, Wm)
    b.map = a.map
    pose = d.poses[1]
    plane = [0.01, -0.02, 1.0, 1.9]
    labels = [torch.from_numpy(np.random.default_rng(k).integers(0, 19, (24, 32), dtype=np.uint8)).to(cuda_device) for k in range(2)]
    for sm in (a, b):
        sm.pcd_frame_id = "world"
        sm.frame_device_views(d.clouds[1], "world", torch.stack(labels), pose, d.cams, src_kind="classmap", image_size=(d.IMG_H, d.IMG_W))
    assert torch.equal(a.map_dev, b.map_dev) and int((a.map_dev != 0).sum()) > 100
    for sm in (a, b):
        sm.set_ground_plane(plane)
        sm.ground_fill_device(labels, pose, d.cams, grid_frame_id="world", src_kind="classmap", image_size=(d.IMG_H, d.IMG_W))
    assert int(a.last_filled.sum()) > 0 and torch.equal(a.last_filled, b.last_filled)
    assert torch.equal(a.map_dev, b.map_dev)
    assert a.live_map_window(pose) == b.live_map_window(pose)
    assert torch.equal(a.live_map(pose), b.live_map(pose)) and int(a.live_map(pose).sum()) > 0
    assert torch.equal(a.live_view(pose), b.live_view(pose)) and np.array_equal(a.live_view_matrix_last, b.live_view_matrix_last)
    assert np.array_equal(a.height_plane(pose, "world"), b.height_plane(pose, "world"))


# ------------------------------------------------------------------------------------------------ no scroll, nothing happens
def test_no_scroll_nothing_happens(cuda_device):
    import torch
    d = drive("main")
    sm = make_sm(d, cuda_device)
    run_frames(sm, d, [0])
    assert sm.scroll_count == 1
    tensor, last, store = sm.map_dev, sm.last_scroll, sm._scroll
    slabs, directory = store.n_slabs, dict(store.directory)
    for k in (1, 0, 1):                                                           # inside the hysteresis band
        assert d.origins[1][0] == d.origins[0][0]
        run_frames(sm, d, [k])
    assert sm.scroll_count == 1 and sm.map_dev is tensor and sm.last_scroll is last
    assert store.n_slabs == slabs and store.directory == directory
    assert sm.scroll_to(ref.yaw_pose(float("nan"), 0.0, 0.0)) is False and sm.scroll_count == 1
    plain = make_sm(d, cuda_device, scroll=False, boundary=ref.window_boundary(d.anchor, d.origins[0][0], d.Hm, d.Wm, d.res))
    assert plain._scroll is None and plain.scroll_cfg.ENABLED is False
    for k in (0, 1, 0, 1):
        run_frames(plain, d, [k])
    assert torch.equal(sm.map_dev, plain.map_dev) and int((plain.map_dev != 0).sum()) > 100
    assert plain.scroll_count == 0 and plain.last_scroll is None and plain.scroll_origin == (0, 0)
    assert plain._grid.map is plain.map_dev


# ------------------------------------------------------------------------------------------------ there and back
def test_there_and_back_with_the_elevation_layer(cuda_device):
    import torch
    d = drive("main")
    sm = make_sm(d, cuda_device, cm="log", elevation=True)
    sm.set_ground_plane([0.0, 0.0, 1.0, 1.9])
    run_frames(sm, d, [0, 1])
    T = d.T
    home = sm.scroll_origin
    layers = [sm.map_dev.clone()] + [t.clone() for t in sm.elevation_layer()]
    assert int(layers[2].sum()) > 0, "the frames put nothing into the elevation layer"
    assert sm.scroll_to(ref.yaw_pose(-1.5 + 2 * d.tile_m, 1.0 + 2 * d.tile_m, 0.0)) is True
    assert sm.scroll_origin == (home[0] + 2 * T, home[1] + 2 * T) and sm.last_scroll["shift"] == (2, 2)
    away = [sm.map_dev] + list(sm.elevation_layer())
    empty = [0, 0, 0, 2 ** 31 - 1, -2 ** 31]
    for before, now, e in zip(layers, away, empty):
        assert torch.equal(now[:d.Hm - 2 * T, :d.Wm - 2 * T], before[2 * T:, 2 * T:])      # the content sits at the shifted offset
        entered = torch.ones((d.Hm, d.Wm), dtype=torch.bool, device=cuda_device)
        entered[:d.Hm - 2 * T, :d.Wm - 2 * T] = False
        assert bool((now[entered] == e).all())                                              # what entered is empty
    assert sm.scroll_to(ref.yaw_pose(-1.5, 1.0, 0.0)) is True and sm.scroll_origin == home
    assert sm.last_scroll["loaded"] > 0 and sm.last_scroll["shift"] == (-2, -2)
    for before, now in zip(layers, [sm.map_dev] + list(sm.elevation_layer())):
        assert torch.equal(now.view(torch.uint8), before.view(torch.uint8))
    assert sm.site_tiles("elevation") and set(sm.site_tiles("elevation")) <= set(sm.site_tiles())
    (i0, j0), elev = sm.site_map(layer="elevation")
    assert len(elev) == 4 and elev[0].dtype == torch.int64 and int(elev[1].sum()) == int(layers[2].sum())


# ------------------------------------------------------------------------------------------------ save and load
def test_save_and_load_site(tmp_path, cuda_device):
    d = drive("main")
    half = 8
    assert d.origins[half][1]                 # frame `half` scrolls, so a fresh run's first call takes the same origin
    whole = make_sm(d, cuda_device, cm="log")
    run_frames(whole, d, range(half))
    path = os.path.join(str(tmp_path), "site.npz")
    whole.save_site(path)
    run_frames(whole, d, range(half, len(d.poses)))
    fresh = make_sm(d, cuda_device, cm="log")
    fresh.load_site(path)
    assert fresh.scroll_origin == (0, 0) and not bool(fresh.map_dev.any())
    site_half = d.numpy_site(whole.confusion_matrix, frames=range(half))
    check_site(fresh, site_half, "loaded")
    run_frames(fresh, d, range(half, len(d.poses)))
    check_site(fresh, d.numpy_site(whole.confusion_matrix), "continued after load")
    o1, m1 = whole.site_map()
    o2, m2 = fresh.site_map()
    assert o1 == o2 and np.array_equal(m1.cpu().numpy(), m2.cpu().numpy())
    other = ref.Drive(ref.ROUTE[:2], res=0.5, Hm=48, Wm=32, tile_m=8.0)
    with pytest.raises(ValueError, match="site file has T = 8"):
        make_sm(other, cuda_device).load_site(path)
