"""Height-aware mapping on the GPU (csrc/mapping.hip: k_fused_vote_height, k_views_vote_height, k_point_heights, k_elevation_mean)
against the NumPy restatement of the rule (tests/_height_reference.py).

Heights are compared bit for bit.  Grids are compared bit for bit with what the PLAIN calls do with the cloud from which the
reference's gated (and, with MAPPING.OCCLUSION, culled) points were removed, padded back to n with points that project nowhere so
that the same vote / apply path runs; the path is asserted.  The reference is fed the slack the GPU returns, after that was checked
against its own (bit for bit without a transform, to one ulp with one).  The layer's integer arrays are compared exactly.  Scenes
are tiny (96 x 64 and 97 x 61 pixels, 1 .. 3000 points, grids of 64 x 64 and 50 x 30 cells): all six vote / apply paths run."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import _height_reference as ref
import _occlusion_reference as occ
from oracle import mapping_oracle as mo

pytestmark = pytest.mark.gpu

# (grid, n, the path avl_fused_frame_path gives), as tests/test_gpu_occlusion.py derives them
FRAME_CASES = [("g64", 3000, 2), ("g64", 257, 3), ("g64", 63, 3), ("g64", 1, 3),
               ("g50x30", 3000, 1), ("g50x30", 257, 1), ("g50x30", 63, 1), ("g50x30", 11, 0), ("g50x30", 1, 0)]
VIEWS_CASES = [("g64", 257, 4), ("g64", 3000, 5), ("g50x30", 257, 4), ("g50x30", 3000, 5)]
# (map dtype, USE_INTENSITY, semantic source, cloud format, frame of the cloud, occlusion (s, R, rel, abs) or None)
VARIANTS = {"f64_int_rgb_soa64_velodyne": ("f64", True, "rgb", "soa64", "velodyne", None),
            "f32_noint_cls_aos32_world": ("f32", False, "classmap", "aos32", "world", None),
            "f64_int_logits_soa64_velodyne": ("f64", True, "logits", "soa64", "velodyne", None),
            "f32_int_rgb_aos32_velodyne_occl": ("f32", True, "rgb", "aos32", "velodyne", (4, 1, 0.1, 1.0)),
            "f64_noint_logits_soa64_world_occl": ("f64", False, "logits", "soa64", "world", (7, 0, 0.1, 1.0))}
NOWHERE = {"velodyne": np.array([-1.0, 0.0, 0.0, 0.0])}      # behind the sensor: no candidate of any view
SCENES = ref.scenes()


class Cam(object):
    def __init__(self, P):
        self.P = P


def nowhere(frame_id):
    if frame_id not in NOWHERE:
        T = np.linalg.inv(ref.origin_to_velodyne(ref.POSE7))
        NOWHERE[frame_id] = np.append(np.matmul(T, np.array([-1.0, 0.0, 0.0, 1.0]))[:3], 0.0)
    return NOWHERE[frame_id]


def cloud_as(pcd, fmt):
    """(what goes to the GPU, the float64 [4, n] cloud the oracle sees)"""
    if fmt == "soa64":
        return pcd, pcd
    aos = np.ascontiguousarray(pcd.T.astype(np.float32))
    return aos, np.ascontiguousarray(aos.T.astype(np.float64))


def removed(gpu_cloud, drop, frame_id):
    """the cloud without the points of ``drop``, padded back to n with points that project nowhere (same layout and dtype)"""
    keep = ~drop
    if gpu_cloud.shape[0] == 4 and gpu_cloud.dtype == np.float64:
        out = np.tile(nowhere(frame_id).reshape(4, 1), (1, gpu_cloud.shape[1]))
        out[:, :int(keep.sum())] = gpu_cloud[:, keep]
        return out
    out = np.tile(nowhere(frame_id).astype(np.float32), (gpu_cloud.shape[0], 1))
    out[:int(keep.sum())] = gpu_cloud[keep]
    return out


def make_sm(sc, device, dtype="f64", gate=False, elev=False, occl=None, colours=None):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults, synthetic as syn
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = sc.boundary
    cfg.MAPPING.RESOLUTION = sc.res
    cfg.MAPPING.PCD.USE_INTENSITY = sc.use_intensity
    cfg.MAPPING.GRID_DTYPE = dtype
    if colours is not None:
        cfg.LABEL_COLORS = [list(c) for c in colours]
    if gate:
        cfg.MAPPING.HEIGHT_GATE.ENABLED = True
        cfg.MAPPING.HEIGHT_GATE.MIN_M, cfg.MAPPING.HEIGHT_GATE.MAX_M, cfg.MAPPING.HEIGHT_GATE.SLOPE = list(sc.min_m), list(sc.max_m), sc.slope
    if elev:
        cfg.MAPPING.ELEVATION.ENABLED = True
    if occl is not None:
        cfg.MAPPING.OCCLUSION.ENABLED = True
        cfg.MAPPING.OCCLUSION.CELL_PX, cfg.MAPPING.OCCLUSION.RADIUS, cfg.MAPPING.OCCLUSION.REL_TOL, cfg.MAPPING.OCCLUSION.ABS_TOL = occl
    sm = SemanticMapping(cfg, device=device, logger=MyLogger("test", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    assert (sm.map_height, sm.map_width) == (sc.Hm, sc.Wm)
    if gate:
        sm.set_ground_plane(sc.plane)
    return sm


def device_sources(sc, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(s)).to(device) for s in sc.sources]


def frame_path(sm, n, V=1):
    from vision_semantic_segmentation_amd import _lib
    g = sm.grid
    g.ensure_capacity(n)
    gs = g.struct()
    return _lib.lib().avl_fused_frame_views_path(C.byref(gs), n, V, sm._bonus_classes())


def run_frame(sm, sc, cloud, src, v=0):
    sm.frame_device(cloud, sc.frame_id, src, sc.pose7, Cam(sc.Ps[v]), src_kind=sc.kind, image_size=(sc.h, sc.w))


def run_views(sm, sc, cloud, srcs):
    sm.frame_device_views(cloud, sc.frame_id, srcs, sc.pose7, [Cam(P) for P in sc.Ps], src_kind=sc.kind, image_size=(sc.h, sc.w))


def same_grid(a, b, what):
    import torch
    assert a.map_dev.dtype == b.map_dev.dtype
    assert torch.equal(a.map_dev, b.map_dev), "%s: %d values differ" % (what, int((a.map_dev != b.map_dev).sum()))
    for sm in (a, b):
        assert not bool(sm.grid.cell_mask.any()) and not bool(sm.grid.counter[4:].any()), "%s: scratch not cleared" % what


def gpu_heights(sm, sc, gpu_cloud):
    """point_heights_device -> the GPU's slack, after h was compared bit for bit and s bit for bit (no transform) or to one ulp"""
    h, s = sm.point_heights_device(gpu_cloud, sc.frame_id, sc.pose7, plane=sc.plane)
    h, s = h.cpu().numpy(), s.cpu().numpy()
    assert tuple(sm.height_plane(sc.pose7, sc.frame_id, sc.plane)) == sc.plane_n()
    want_h, want_s = sc.heights(), sc.slacks()
    assert np.array_equal(h, want_h, equal_nan=True), "%d heights differ" % int((h != want_h).sum())
    if sc.frame_id == "velodyne":
        assert np.array_equal(s, want_s, equal_nan=True)
    else:
        assert (np.abs(s - want_s) <= np.spacing(np.abs(want_s))).all(), "slack off by %g ulp" % float((np.abs(s - want_s) / np.spacing(np.abs(want_s))).max())
    return s


def gpu_culled(sm, sc, gpu_cloud, par):
    """bool [V, n]: visibility_device's culled candidates, after they were compared with the occlusion rule fed the GPU's keys"""
    if par is None:
        return None
    state, key = sm.visibility_device(gpu_cloud, sc.frame_id, sc.pose7, [Cam(P) for P in sc.Ps], (sc.h, sc.w), return_keys=True)
    state, key = state.cpu().numpy(), key.cpu().numpy()
    want = np.stack([pr.states(key=key[v], s=par[0], R=par[1], rel=par[2], abs_=par[3]) for v, pr in enumerate(sc.projs)])
    assert np.array_equal(state, want)
    return want == 2


def scene_for(grid, n, seed, V, variant, size):
    dtype, intensity, kind, fmt, frame_id, par = VARIANTS[variant]
    sc = ref.Scene("case", grid, size, n, seed, V, kind, frame_id, use_intensity=intensity)
    gpu_cloud, host_cloud = cloud_as(sc.pcd, fmt)
    return sc.see(host_cloud), gpu_cloud, dtype, par


# ---------------------------------------------------------------------------------------------------------------- 1. heights
@pytest.mark.parametrize("fmt", ["soa64", "aos32"])
@pytest.mark.parametrize("sc", SCENES, ids=[sc.name for sc in SCENES])
def test_point_heights_equal_the_rule(sc, fmt, cuda_device):
    gpu_cloud, host_cloud = cloud_as(sc.pcd, fmt)
    seen = copy.copy(sc).see(host_cloud)
    sm = make_sm(seen, cuda_device)
    assert not sm.height_gate_enabled()                         # point_heights_device works with the option off
    gpu_heights(sm, seen, gpu_cloud)


def test_point_heights_of_non_finite_points_are_nan(cuda_device):
    sc = SCENES[6]
    pcd = sc.pcd.copy()
    pcd[0, 0], pcd[1, 1], pcd[2, 2] = np.nan, np.inf, -np.inf
    seen = copy.copy(sc).see(pcd)
    sm = make_sm(seen, cuda_device)
    h, s = sm.point_heights_device(pcd, sc.frame_id, sc.pose7, plane=sc.plane)
    h, s = h.cpu().numpy(), s.cpu().numpy()
    assert np.isnan(h[:3]).all() and np.isnan(s[:3]).all() and np.isfinite(h[3:]).all() and np.isfinite(s[3:]).all()
    assert np.array_equal(h, seen.heights(), equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- 2. fused frame
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case", FRAME_CASES, ids=["%s_n%d_p%d" % c for c in FRAME_CASES])
def test_gated_frame_equals_the_plain_frame_on_the_filtered_cloud(case, variant, cuda_device):
    grid, n, path = case
    sc, gpu_cloud, dtype, par = scene_for(grid, n, 11 + n, 1, variant, ref.SIZES[n % 2])
    src = device_sources(sc, cuda_device)[0]
    gated = make_sm(sc, cuda_device, dtype, gate=True, occl=par)
    plain = make_sm(sc, cuda_device, dtype)
    assert frame_path(gated, n) == path and frame_path(plain, n) == path
    s = gpu_heights(gated, sc, gpu_cloud)
    culled = gpu_culled(gated, sc, gpu_cloud, par)
    before = sc.bits_before(culled)
    after = sc.bits_after(before, s=s)
    assert ((after == 0) | (after == before)).all()             # one class per pixel: a point votes as before or not at all
    out = (before[0] != 0) & (after[0] == 0)
    run_frame(gated, sc, gpu_cloud, src)
    assert gated.last_gated.cpu().tolist() == [int(out.sum())]
    drop = out if culled is None else out | culled[0]
    run_frame(plain, sc, removed(gpu_cloud, drop, sc.frame_id), src)
    same_grid(gated, plain, "gated frame vs plain frame on the filtered cloud")
    if n == 3000:
        assert out.sum() >= 30 and int(gated.map_dev.count_nonzero()) > 20
        ungated = make_sm(sc, cuda_device, dtype, occl=par)
        run_frame(ungated, sc, gpu_cloud, src)
        assert not bool((ungated.map_dev == gated.map_dev).all()), "the gate changed nothing: the case tests nothing"


# ---------------------------------------------------------------------------------------------------------------- 3. views
@pytest.mark.parametrize("variant", ["f64_int_rgb_soa64_velodyne", "f32_noint_cls_aos32_world", "f64_noint_logits_soa64_world_occl"])
@pytest.mark.parametrize("V", [2, 3])
@pytest.mark.parametrize("case", VIEWS_CASES, ids=["%s_n%d_p%d" % c for c in VIEWS_CASES])
def test_gated_views_equal_sequential_plain_frames_on_filtered_clouds(case, V, variant, cuda_device):
    grid, n, path = case
    sc, gpu_cloud, dtype, par = scene_for(grid, n, 23 + n, V, variant, ref.SIZES[V % 2])
    srcs = device_sources(sc, cuda_device)
    fused = make_sm(sc, cuda_device, dtype, gate=True, occl=par)
    plain = make_sm(sc, cuda_device, dtype)
    assert frame_path(fused, n, V) == path
    s = gpu_heights(fused, sc, gpu_cloud)
    culled = gpu_culled(fused, sc, gpu_cloud, par)
    before = sc.bits_before(culled)
    after = sc.bits_after(before, s=s)
    assert ((after == 0) | (after == before)).all()
    run_views(fused, sc, gpu_cloud, srcs)
    assert fused.last_gated.cpu().tolist() == sc.gated_counts(before, after)
    for v in range(V):
        drop = (before[v] != 0) & (after[v] == 0)
        drop = drop if culled is None else drop | culled[v]
        run_frame(plain, sc, removed(gpu_cloud, drop, sc.frame_id), srcs[v], v)
    same_grid(fused, plain, "gated views vs plain frames on the per-view filtered clouds")
    if n == 3000:
        assert int(fused.map_dev.count_nonzero()) > 20 and all(c > 20 for c in sc.gated_counts(before, after))


def test_more_views_than_one_call_takes_are_gated_call_by_call(cuda_device):
    sc = ref.Scene("five", "g64", ref.SIZES[1], 3000, 5, 5, "classmap")
    srcs = device_sources(sc, cuda_device)
    many = make_sm(sc, cuda_device, gate=True, elev=True)
    before = sc.bits_before()
    after = sc.bits_after(before, s=gpu_heights(many, sc, sc.pcd))
    run_views(many, sc, sc.pcd, srcs)
    assert many.last_gated.cpu().tolist() == sc.gated_counts(before, after)
    plain = make_sm(sc, cuda_device)
    layer = ref.empty_layer(sc.Hm, sc.Wm)
    for v in range(5):
        run_frame(plain, sc, removed(sc.pcd, (before[v] != 0) & (after[v] == 0), sc.frame_id), srcs[v], v)
        layer = sc.layer_after(after[v:v + 1], layer)           # the fall-back's layer takes a point once per call
    same_grid(many, plain, "five gated views vs plain frames")
    for got, want in zip(many.elevation_layer(), layer):
        assert np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- 4. the apply's order, exact bounds
def test_two_labels_that_share_red_and_green_are_gated_apart(cuda_device):
    """a "road" pixel votes road and, with this palette, sidewalk; the sidewalk's band reaches 1.5 m, so a shrub point keeps only
    the sidewalk bit.  No plain call on a filtered cloud does that: the grid is compared with the reference's own apply."""
    colours = [list(c) for c in mo.LABEL_COLORS]
    colours[4] = [colours[0][0], colours[0][1], 99]
    for grid, n in [("g64", 3000), ("g64", 257), ("g50x30", 3000), ("g50x30", 11)]:
        sc = ref.Scene("shared", grid, ref.SIZES[0], n, 31 + n, 1, "rgb", colours=colours, max_m=[0.5, 0.5, 0.5, math.inf, 1.5])
        sm = make_sm(sc, cuda_device, gate=True, colours=colours)
        before = sc.bits_before()
        after = sc.bits_after(before, s=gpu_heights(sm, sc, sc.pcd))
        if n == 3000:
            both = (before[0] & 0x11) == 0x11
            assert both.sum() > 50 and (both & ((after[0] & 0x11) == 0x10)).sum() > 5
        run_frame(sm, sc, sc.pcd, device_sources(sc, cuda_device)[0])
        assert sm.last_gated.cpu().tolist() == sc.gated_counts(before, after)
        assert np.array_equal(sm.map, sc.grid_after(after, sm.confusion_matrix))


@pytest.mark.parametrize("grid", sorted(ref.GRIDS))
def test_bounds_are_inclusive_to_the_last_bit(grid, cuda_device):
    sc, keep = ref.exact_scene(grid)
    sm = make_sm(sc, cuda_device, gate=True)
    s = gpu_heights(sm, sc, sc.pcd)
    assert not s.any()
    before = sc.bits_before()
    after = sc.bits_after(before, s=s)
    assert np.array_equal(after[0] != 0, keep) and (before[0] != 0).all()
    run_frame(sm, sc, sc.pcd, device_sources(sc, cuda_device)[0])
    assert sm.last_gated.cpu().tolist() == [int((~keep).sum())]
    assert np.array_equal(sm.map, sc.grid_after(after, sm.confusion_matrix))
    wide = copy.copy(sc)
    wide.min_m, wide.max_m = [-math.inf] * 5, [math.inf] * 5
    sm = make_sm(wide, cuda_device, gate=True)
    run_frame(sm, wide, sc.pcd, device_sources(sc, cuda_device)[0])
    assert sm.last_gated.cpu().tolist() == [0] and np.array_equal(sm.map, sc.grid_after(before, sm.confusion_matrix))


# ---------------------------------------------------------------------------------------------------------------- 5. elevation
@pytest.mark.parametrize("gate", [True, False], ids=["gated", "ungated"])
@pytest.mark.parametrize("case", [("g64", 3000, 1, "velodyne"), ("g64", 257, 1, "world"), ("g50x30", 3000, 3, "velodyne"), ("g50x30", 11, 1, "velodyne"),
                                  ("g64", 3000, 3, "world"), ("g64", 257, 2, "velodyne")], ids=lambda c: "%s_n%d_V%d_%s" % c)
def test_elevation_layer_after_three_frames(case, gate, cuda_device):
    import torch
    grid, n, V, frame_id = case
    sm, layer, frames = None, ref.empty_layer(*ref.GRIDS[grid][:2]), []
    for f in range(3):
        sc = ref.Scene("frame%d" % f, grid, ref.SIZES[f % 2], n, 50 + 7 * f + n, V, "rgb", frame_id)
        sm = make_sm(sc, cuda_device, gate=gate, elev=True) if sm is None else sm
        before = sc.bits_before()
        kept = sc.bits_after(before, s=gpu_heights(sm, sc, sc.pcd)) if gate else before
        layer = sc.layer_after(kept, layer)
        frames.append((sc, device_sources(sc, cuda_device)))
        (run_views if V > 1 else lambda m, c, p, s: run_frame(m, c, p, s[0]))(sm, sc, sc.pcd, frames[-1][1])
        if V > 1 and n == 3000:
            assert (((kept & 0xffff & ref.ELEV_CLASSES) != 0).sum(axis=0) == V).any()     # a point every view sees: counted once
    got = [t.cpu().numpy() for t in sm.elevation_layer()]
    assert [g.dtype for g in got] == [np.int64, np.int32, np.int32, np.int32]
    for g, want, what in zip(got, layer, ("sum", "cnt", "min", "max")):
        assert np.array_equal(g, want), "%s: %d cells differ" % (what, int((g != want).sum()))
    if n == 3000:
        assert int((got[1] > 1).sum()) > 20 and int(got[1].sum()) > 300
    mean = sm.elevation_device()
    assert mean.dtype == torch.float32 and tuple(mean.shape) == tuple(ref.GRIDS[grid][:2])
    assert np.array_equal(mean.cpu().numpy(), ref.elevation_mean(layer), equal_nan=True)
    # a permutation of every cloud leaves the layer as it is, and the grid
    other = make_sm(frames[0][0], cuda_device, gate=gate, elev=True)
    for f, (sc, srcs) in enumerate(frames):
        perm = np.random.default_rng(f).permutation(n)
        (run_views if V > 1 else lambda m, c, p, s: run_frame(m, c, p, s[0]))(other, sc, np.ascontiguousarray(sc.pcd[:, perm]), srcs)
    for a, b in zip(other.elevation_layer(), sm.elevation_layer()):
        assert torch.equal(a, b)
    same_grid(other, sm, "permuted clouds")
    sm.reset_elevation()
    for t, v in zip(sm.elevation_layer(), ref.EMPTY):
        assert bool((t == v).all())
    assert bool(torch.isnan(sm.elevation_device()).all())


# ---------------------------------------------------------------------------------------------------------------- 6. options off, routing
@pytest.mark.parametrize("sc", [s for s in SCENES if s.n in (11, 3000)], ids=lambda s: s.name)
def test_with_both_options_off_nothing_changes_and_elevation_alone_leaves_the_grid(sc, cuda_device):
    cfg = dict(range_max=ref.RANGE_MAX, T_velodyne_to_baselink=mo.velodyne_to_baselink(), boundary=sc.boundary, resolution=sc.res,
               label_names=mo.LABELS_NAMES, label_colors=mo.LABEL_COLORS, confusion_matrix=None, use_pcd_intensity=True)
    src = device_sources(sc, cuda_device)[0]
    off = make_sm(sc, cuda_device)
    run_frame(off, sc, sc.pcd, src)
    cfg["confusion_matrix"] = off.confusion_matrix
    want = mo.mapping_frame(np.zeros((sc.Hm, sc.Wm, 5)), sc.pcd, sc.frame_id, sc.sources[0], sc.pose7, sc.Ps[0], cfg)
    assert np.array_equal(off.map, want)
    assert off.last_gated is None and off._elevation is None    # nothing of the feature was touched
    elev = make_sm(sc, cuda_device, elev=True)
    run_frame(elev, sc, sc.pcd, src)
    same_grid(elev, off, "elevation alone vs the plain frame")
    assert elev.last_gated is None and int(elev.elevation_layer()[1].sum()) == int(((sc.bits_before()[0] & ref.ELEV_CLASSES) != 0).sum())


def test_the_gate_waits_for_a_plane_in_mapping_and_raises_in_frame_device(cuda_device):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    sc = SCENES[8]
    assert sc.frame_id == "velodyne" and sc.n == 3000
    src = device_sources(sc, cuda_device)[0]
    sm = make_sm(sc, cuda_device, gate=True)
    sm.ground_plane = None
    with pytest.raises(RuntimeError, match="ground plane"):
        run_frame(sm, sc, sc.pcd, src)
    sm.pcd, sm.pcd_frame_id = sc.pcd, "velodyne"
    sm.mapping(src, None, Cam(sc.Ps[0]))
    plain = make_sm(sc, cuda_device)
    run_frame(plain, sc, sc.pcd, src)
    same_grid(sm, plain, "mapping() without a plane vs the plain frame")
    assert sm.last_gated is None
    sm.set_ground_plane(sc.plane)
    sm.mapping(src, None, Cam(sc.Ps[0]))
    before = sc.bits_before()
    after = sc.bits_after(before)
    assert sm.last_gated.cpu().tolist() == sc.gated_counts(before, after) and sm.last_gated.item() > 30
    sm.mapping_views([src], None, [Cam(sc.Ps[0])])
    assert sm.last_gated.cpu().tolist() == sc.gated_counts(before, after)
    for key, bad in [("MAX_M", [0.5, 0.5]), ("MIN_M", ["low"] * 5)]:
        cfg = get_cfg_defaults()
        cfg.MAPPING.HEIGHT_GATE.ENABLED = True
        cfg.MAPPING.HEIGHT_GATE[key] = bad
        with pytest.raises(ValueError, match="HEIGHT_GATE"):
            SemanticMapping(cfg, device=cuda_device)
    cfg = get_cfg_defaults()
    cfg.MAPPING.ELEVATION.ENABLED = True
    cfg.MAPPING.ELEVATION.CLASSES = ["kerb"]
    with pytest.raises(ValueError, match="kerb"):
        SemanticMapping(cfg, device=cuda_device)
