"""The site overview on the GPU: k_site_overview and SemanticMapping.site_overview against the NumPy twin of
_site_overview_reference.py, the reduced grid as bit patterns and the picture byte for byte.

* the kernel alone through the C ABI, both outputs between guard strips of 0xAB that must survive: a rectangle of 3 x 4 tiles with
  two tiles absent, the others in a window buffer (one of its tiles masked out although its bytes are garbage) and in the slabs of a
  pool, so both pitches stand in one table; payloads of both signs with -0.0; T = 8 and T = 20 at every k that divides them, f64 and
  f32; T = 100 at k = 10, 25 and 100 (rows of 4000 bytes, chunks that start off a 16-byte bound, a strip of 400 KB that takes ten
  stages); C = 1, 8, 9, 16 (both branches of numpy_row_sum); the thresholds renderer with a priority; one tile row wider than a stage
  (T = 320, C = 16, f64, k = 320); 1600 tiles, more than the launch splits by pixel rows; n_tiles = 0.
* through the API: the drives of test_gpu_scroll.py (identity f64, log f64, log f32) -- after the last frame and once right after a
  scroll, site_overview(k, reduced=True) is the twin of the NumPy site for every k that divides T; site_overview(1) is
  render_bev_map(site_map()[1]); site_map() and scroll_count are what they were.  A rectangle larger than the site, one that cuts
  through it, the thresholds renderer, an empty site, `out`, the automatic k, finish_run's site_map.png."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _scroll_reference as ref
import _site_overview_reference as ov
from _site_overview_reference import run_kernel

pytestmark = pytest.mark.gpu

def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def divisors(T):
    return [k for k in range(1, T + 1) if T % k == 0]


# ------------------------------------------------------------------------------------------------ the kernel against the executor
def check_case(case, k, device, thresholds=None, priority=None):
    want_R, want_pic = ov.execute_sources(case.table, case.bufs, case.T, case.C, case.dtype, case.nh, case.nw, k, ov.COLORS[:case.C],
                                          thresholds, priority)
    pic, R = run_kernel(case.table, case.bufs, case.T, case.C, case.dtype, case.nh, case.nw, k, device, thresholds, priority)
    assert R.shape == want_R.shape and pic.shape == want_pic.shape
    assert np.array_equal(bits(R), bits(want_R)), "%d of %d values of R differ" % (int((bits(R) != bits(want_R)).sum()), R.size)
    assert np.array_equal(pic, want_pic), "%d pixels differ" % int((pic != want_pic).any(axis=2).sum())
    P = case.T // k
    for r, c in case.absent:                                             # an absent tile: black and +0
        assert not pic[r * P:(r + 1) * P, c * P:(c + 1) * P].any() and not bits(R[r * P:(r + 1) * P, c * P:(c + 1) * P]).any()
    assert len(np.unique(pic.reshape(-1, 3), axis=0)) >= min(3, case.C + 1)
    return pic, R


_CASES = {}


def table_case(T, Cn, dtype):
    key = (T, Cn, np.dtype(dtype).name)
    if key not in _CASES:
        _CASES[key] = ov.TableCase(T, Cn, dtype)
    return _CASES[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("T,k", [(8, k) for k in divisors(8)] + [(20, k) for k in divisors(20)], ids=lambda v: str(v))
def test_kernel_every_k(T, k, dtype, cuda_device):
    case = table_case(T, 5, dtype)
    pic, R = check_case(case, k, cuda_device)
    if k == 1:                                                           # a cell's -0.0 arrives as +0, and a pixel of -0.0 is black
        assert np.signbit(case.full).any() and not np.signbit(R[case.full == 0]).any()
        picture_only, none = run_kernel(case.table, case.bufs, T, 5, dtype, 3, 4, k, cuda_device, reduced=False)
        assert none is None and np.array_equal(picture_only, pic)


@pytest.mark.parametrize("k", [10, 25, 100])
def test_kernel_rows_of_4000_bytes(k, cuda_device):
    check_case(table_case(100, 5, np.float64), k, cuda_device)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("Cn", [1, 8, 9, 16])
def test_kernel_class_counts(Cn, dtype, cuda_device):
    check_case(table_case(8, Cn, dtype), 2, cuda_device)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_kernel_thresholds_with_a_priority(dtype, cuda_device):
    case = table_case(8, 5, dtype)
    th, pr = [0.3, 0.01, 0.2, 0.05, 0.6], [3, 0, 4, 2, 1]
    pic, _ = check_case(case, 4, cuda_device, th, pr)
    plain, _ = check_case(case, 4, cuda_device)
    other, _ = check_case(case, 4, cuda_device, th, [0, 1, 2, 3, 4])
    assert (pic != plain).any() and (pic != other).any()                # neither the arg-max picture nor the trivial priority's


def test_kernel_a_tile_row_wider_than_a_stage(cuda_device):
    """T = 320, C = 16, f64, k = 320: one pixel's part of one tile row is 40960 bytes, more than a stage holds, so the row is walked in
    two column parts; one tile in a buffer of the window's pitch, one in a slab"""
    from vision_semantic_segmentation_amd import scroll as s
    T, Cn = 320, 16
    rng = np.random.default_rng(5)
    full = ov.payload(rng, (T, 2 * T, Cn), np.float64)
    bufs = [full.reshape(-1).view(np.uint8).copy(), np.ascontiguousarray(full[:, T:]).reshape(-1).view(np.uint8).copy()]
    table = s.overview_sources((0, 0, 0, 1), T, Cn * 8, 2 * T, (0, 0), np.array([[True, False]]), [(0, 1)], [0], 1)
    assert [int(p) for p in table["pitch"]] == [2 * T * Cn * 8, T * Cn * 8]
    want_R, want_pic = ov.overview(full, T, ov.COLORS)
    pic, R = run_kernel(table, bufs, T, Cn, np.float64, 1, 2, T, cuda_device)
    assert np.array_equal(bits(R), bits(want_R)) and np.array_equal(pic, want_pic) and pic.any(axis=2).all()


def test_kernel_more_tiles_than_the_launch_splits(cuda_device):
    """40 x 40 tiles of T = 8 at k = 1: a workgroup takes more than one pixel row of its tile"""
    from vision_semantic_segmentation_amd import scroll as s
    T, Cn, n = 8, 5, 40
    rng = np.random.default_rng(6)
    full = ov.payload(rng, (n * T, n * T, Cn), np.float32)
    mask = rng.random((n, n)) < 0.9
    bufs = [full.reshape(-1).view(np.uint8).copy()]
    for i, j in zip(*np.nonzero(~mask)):
        full[i * T:(i + 1) * T, j * T:(j + 1) * T] = 0.0
    table = s.overview_sources((0, n - 1, 0, n - 1), T, Cn * 4, n * T, (0, 0), mask, [], [], 1)
    assert 1400 < len(table) == int(mask.sum()) < 1600
    for k in (1, 2):
        want_R, want_pic = ov.overview(full, k, ov.COLORS[:Cn])
        pic, R = run_kernel(table, bufs, T, Cn, np.float32, n, n, k, cuda_device)
        assert np.array_equal(bits(R), bits(want_R)) and np.array_equal(pic, want_pic)


def test_kernel_no_tiles(cuda_device):
    case = table_case(8, 5, np.float64)
    pic, R = run_kernel(case.table[:0], case.bufs, 8, 5, np.float64, 3, 4, 2, cuda_device, n_tiles=0)
    assert not pic.any() and not bits(R).any()


# ------------------------------------------------------------------------------------------------ the drives
_DRIVES, _SITES = {}, {}


def drive(name):
    if name not in _DRIVES:
        if name == "main":
            _DRIVES[name] = ref.main_drive()
        else:                                             # test_gpu_scroll.py's drive at RESOLUTION 0.1: T = 20, a 120 x 80 window
            route = [(21.3, 13.1, 0.0), (23.3, 13.1, 0.4), (25.9, 15.2, 0.8), (29.3, 17.3, 1.0), (23.1, 11.0, math.pi)]
            _DRIVES[name] = ref.Drive(route, res=0.1, Hm=120, Wm=80, tile_m=2.0, range_max=7.0, n_points=1500, seed=4)
    return _DRIVES[name]


def numpy_site(name, cm_name, cm, grid_dtype, n_frames):
    key = (name, cm_name, grid_dtype, n_frames)
    if key not in _SITES:
        _SITES[key] = drive(name).numpy_site(cm, np.float64 if grid_dtype == "f64" else np.float32, frames=range(n_frames))
    return _SITES[key]


def make_sm(d, device, grid_dtype="f64", cm="identity", overview=None):
    from vision_semantic_segmentation_amd import SemanticMapping, synthetic as syn
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = d.cfg(grid_dtype)
    for name, value in (overview or {}).items():
        setattr(cfg.MAPPING.SITE_OVERVIEW, name, value)
    sm = SemanticMapping(cfg, device=device, logger=MyLogger("test", quiet=True))
    if cm == "log":
        sm.confusion_matrix = syn.log_confusion(sm.map_depth)
    return sm


def run_frames(sm, d, frames):
    import torch
    for k in frames:
        sm.pcd, sm.pcd_frame_id = d.clouds[k], "world"
        sm.mapping_views([torch.from_numpy(im).to(sm.device) for im in d.images[k]], d.poses[k], d.cams)


def check_overviews(sm, d, site, what):
    """every k that divides T against the twin of the NumPy site; k = 1 against render_bev_map(site_map()); nothing moved"""
    import torch
    from vision_semantic_segmentation_amd.renderer import render_bev_map
    tiles = site.nonempty_tiles()
    (i0, j0), full = site.region(tiles)
    count = sm.scroll_count
    origin_before, map_before = sm.site_map()
    assert origin_before == (i0, j0) and np.array_equal(bits(map_before.cpu().numpy()), bits(full)), what
    for k in divisors(d.T):
        origin, pic, R = sm.site_overview(k, reduced=True)
        want_R, want_pic = ov.overview(full, k, np.asarray(sm.label_colors))
        assert origin == (i0, j0) and tuple(pic.shape) == want_pic.shape and tuple(R.shape) == want_R.shape, (what, k)
        assert pic.dtype == torch.uint8 and R.dtype == map_before.dtype
        R = R.cpu().numpy()
        assert np.array_equal(bits(R), bits(want_R)), "%s k = %d: %d of %d values of R differ" % (what, k, int((bits(R) != bits(want_R)).sum()), R.size)
        assert np.array_equal(pic.cpu().numpy(), want_pic), (what, k)
        assert sm.last_site_overview == {"rect": (i0 // d.T, i0 // d.T + full.shape[0] // d.T - 1, j0 // d.T, j0 // d.T + full.shape[1] // d.T - 1),
                                         "cells_per_pixel": k, "tiles": len(tiles)}
        if k == 1:
            assert torch.equal(pic, render_bev_map(map_before, sm.label_colors))
            assert len(np.unique(want_pic.reshape(-1, 3), axis=0)) >= 3
    origin_after, map_after = sm.site_map()
    assert origin_after == origin_before and torch.equal(map_after.view(torch.uint8), map_before.view(torch.uint8))
    assert sm.scroll_count == count
    return full


@pytest.mark.parametrize("cm,grid_dtype", [("identity", "f64"), ("log", "f64"), ("log", "f32")], ids=["identity_f64", "log_f64", "log_f32"])
@pytest.mark.parametrize("name", ["main", "fine"])
def test_drive_overview_equals_the_twin(name, cm, grid_dtype, cuda_device):
    d = drive(name)
    sm = make_sm(d, cuda_device, grid_dtype, cm)
    mid = max(k for k in range(1, len(d.poses) - 1) if d.origins[k][1])             # the last frame but the final one that scrolls
    run_frames(sm, d, range(mid + 1))
    assert sm.scroll_origin == d.origins[mid][0] and sm._scroll.pending is not None  # right after a scroll: its flags are not retired yet
    first = sm.site_overview(1)[1]                                                   # the overview retires them itself
    assert sm._scroll.pending is None and first.any()
    check_overviews(sm, d, numpy_site(name, cm, sm.confusion_matrix, grid_dtype, mid + 1), "%s %s %s mid-drive" % (name, cm, grid_dtype))
    run_frames(sm, d, range(mid + 1, len(d.poses)))
    site = numpy_site(name, cm, sm.confusion_matrix, grid_dtype, len(d.poses))
    full = check_overviews(sm, d, site, "%s %s %s" % (name, cm, grid_dtype))
    if name == "fine" or cm != "log":
        return
    # a rectangle larger than the site: black borders; one that cuts through window, store and nothing
    T = d.T
    tiles = site.nonempty_tiles()
    ti0, ti1 = min(t[0] for t in tiles), max(t[0] for t in tiles)
    tj0, tj1 = min(t[1] for t in tiles), max(t[1] for t in tiles)
    pad = np.zeros((full.shape[0] + 5 * T, full.shape[1] + 4 * T, full.shape[2]), dtype=full.dtype)
    pad[2 * T:2 * T + full.shape[0], 3 * T:3 * T + full.shape[1]] = full
    k = 4
    origin, pic, R = sm.site_overview(k, rect=(ti0 - 2, ti1 + 3, tj0 - 3, tj1 + 1), reduced=True)
    want_R, want_pic = ov.overview(pad, k, np.asarray(sm.label_colors))
    assert origin == ((ti0 - 2) * T, (tj0 - 3) * T)
    assert np.array_equal(bits(R.cpu().numpy()), bits(want_R)) and np.array_equal(pic.cpu().numpy(), want_pic)
    P = T // k
    assert not want_pic[:2 * P].any() and not want_pic[:, :3 * P].any() and not want_pic[-3 * P:].any() and not want_pic[:, -P:].any()
    origin, pic, R = sm.site_overview(2, rect=(ti0 - 1, ti0 + 3, tj0 + 1, tj0 + 2), reduced=True)
    want_R, want_pic = ov.overview(pad[T:6 * T, 4 * T:6 * T], 2, np.asarray(sm.label_colors))
    assert origin == ((ti0 - 1) * T, (tj0 + 1) * T) and want_pic.any()
    assert np.array_equal(bits(R.cpu().numpy()), bits(want_R)) and np.array_equal(pic.cpu().numpy(), want_pic)
    # the thresholds renderer with a priority, into a tensor of the caller's
    import torch
    th, pr = [0.3, 0.01, 0.2, 0.05, 0.6], [3, 0, 4, 2, 1]
    out = torch.full((full.shape[0] // 2, full.shape[1] // 2, 3), 0xAB, dtype=torch.uint8, device=cuda_device)
    origin, pic = sm.site_overview(2, thresholds=th, priority=pr, out=out)
    assert pic is out and np.array_equal(out.cpu().numpy(), ov.overview(full, 2, np.asarray(sm.label_colors), th, pr)[1])
    with pytest.raises(ValueError, match="out must be"):
        sm.site_overview(4, out=out)
    with pytest.raises(ValueError, match="does not divide"):
        sm.site_overview(3)
    # cells_per_pixel from the configuration: 0 = the smallest k whose picture fits MAX_SIDE_PX
    sm.cfg.MAPPING.SITE_OVERVIEW.MAX_SIDE_PX = max(full.shape[:2]) // 2 - 1
    assert tuple(sm.site_overview()[1].shape[:2]) == (full.shape[0] // 4, full.shape[1] // 4) and sm.last_site_overview["cells_per_pixel"] == 4
    sm.cfg.MAPPING.SITE_OVERVIEW.CELLS_PER_PIXEL = 8
    assert sm.last_site_overview["cells_per_pixel"] == 4 and sm.site_overview()[1].shape[0] == full.shape[0] // 8


def test_overview_of_a_loaded_site(tmp_path, cuda_device):
    """after load_site the window holds nothing and every tile comes from the store"""
    d = drive("main")
    sm = make_sm(d, cuda_device, "f64", "log")
    run_frames(sm, d, range(8))
    path = os.path.join(str(tmp_path), "site.npz")
    sm.save_site(path)
    fresh = make_sm(d, cuda_device, "f64", "log")
    fresh.load_site(path)
    assert not fresh._scroll.window_valid
    site = numpy_site("main", "log", sm.confusion_matrix, "f64", 8)
    (i0, j0), full = site.region(site.nonempty_tiles())
    for one in (sm, fresh):
        origin, pic, R = one.site_overview(4, reduced=True)
        want_R, want_pic = ov.overview(full, 4, np.asarray(one.label_colors))
        assert origin == (i0, j0) and np.array_equal(bits(R.cpu().numpy()), bits(want_R)) and np.array_equal(pic.cpu().numpy(), want_pic)
    assert fresh.last_site_overview["tiles"] == len(site.nonempty_tiles())


def test_an_empty_site_and_a_map_that_does_not_scroll(cuda_device):
    d = drive("main")
    sm = make_sm(d, cuda_device)
    origin, pic, R = sm.site_overview(2, reduced=True)
    assert origin == (0, 0) and tuple(pic.shape) == (0, 0, 3) and tuple(R.shape) == (0, 0, 5)
    assert sm._scroll.tables == [None, None]                                           # nothing was uploaded or launched
    from vision_semantic_segmentation_amd import SemanticMapping
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = d.cfg()
    cfg.MAPPING.SCROLL.ENABLED = False
    with pytest.raises(RuntimeError, match="MAPPING.SCROLL.ENABLED is False"):
        SemanticMapping(cfg, device=cuda_device, logger=MyLogger("test", quiet=True)).site_overview(2)


# ------------------------------------------------------------------------------------------------ finish_run
def read_picture(folder, stem):
    """the RGB picture finish_run wrote as ``stem``.png (channel 0 stored as blue) or, without PIL, ``stem``.npy"""
    png, npy = os.path.join(folder, stem + ".png"), os.path.join(folder, stem + ".npy")
    if os.path.exists(png):
        from PIL import Image
        return np.asarray(Image.open(png))[:, :, ::-1]
    return np.load(npy)


def test_finish_run_writes_site_map(tmp_path, cuda_device):
    d = drive("main")
    folders, maps = {}, {}
    for enabled in (False, True):
        sm = make_sm(d, cuda_device, "f64", "log", overview={"ENABLED": enabled, "CELLS_PER_PIXEL": 2})
        run_frames(sm, d, range(8))
        assert sm.scroll_count >= 3
        want = sm.site_overview(2)[1].cpu().numpy() if enabled else None
        folders[enabled] = str(tmp_path / ("on" if enabled else "off"))
        maps[enabled] = sm.finish_run(folders[enabled])
        names = sorted(os.listdir(folders[enabled]))
        if enabled:
            assert [n for n in names if n.startswith("site_map.")] in (["site_map.png"], ["site_map.npy"])
            got = read_picture(folders[enabled], "site_map")
            assert np.array_equal(got, want) and len(np.unique(want.reshape(-1, 3), axis=0)) >= 3
            assert want.shape[0] > d.Hm // 2 or want.shape[1] > d.Wm // 2                # the site outgrew the window
        else:
            assert not [n for n in names if n.startswith("site_map")] and sm.last_site_overview is None
    assert np.array_equal(maps[False], maps[True])
    assert sorted(n for n in os.listdir(folders[True]) if not n.startswith("site_map")) == sorted(os.listdir(folders[False]))
    for n in os.listdir(folders[False]):
        with open(os.path.join(folders[False], n), "rb") as a, open(os.path.join(folders[True], n), "rb") as b:
            assert a.read() == b.read(), n
