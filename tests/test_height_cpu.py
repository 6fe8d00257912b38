"""Height-aware mapping without a GPU: that the NumPy reference (tests/_height_reference.py) is the oracle's plain frame when the gate
is wide open, that the shared scenes can tell the rule of include/avl_hip.h (struct avl_height) from its likely mis-implementations
and gate a fair share of every larger cloud -- all asserted on the reference alone -- and the host side: configuration parsing, the
ctypes mirror of struct avl_height and the argument checks, which run before any GPU call."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import _height_reference as ref
from oracle import mapping_oracle as mo

SCENES = ref.scenes()
BIG = [sc for sc in SCENES if sc.n >= 257]
CM = np.log(np.full((5, 5), 0.05) + 0.75 * np.eye(5))


def _oracle_grid(sc):
    grid = np.zeros((sc.Hm, sc.Wm, 5))
    cfg = dict(range_max=ref.RANGE_MAX, T_velodyne_to_baselink=mo.velodyne_to_baselink(), boundary=sc.boundary, resolution=sc.res,
               label_names=mo.LABELS_NAMES, label_colors=mo.LABEL_COLORS, confusion_matrix=CM, use_pcd_intensity=sc.use_intensity)
    return mo.mapping_frame(grid, sc.pcd, sc.frame_id, sc.sources[0], sc.pose7, sc.Ps[0], cfg)


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_scenes_have_the_sizes_the_suite_relies_on():
    assert sorted({sc.n for sc in SCENES}) == [1, 11, 63, 257, 3000]
    assert {(sc.w, sc.h) for sc in SCENES} == {(96, 64), (97, 61)} and {sc.grid for sc in SCENES} == {"g64", "g50x30"}
    assert {sc.frame_id for sc in SCENES} == {"velodyne", "world"}
    n = ref.normalise(ref.PLANE)
    assert abs(math.sqrt(n[0] ** 2 + n[1] ** 2 + n[2] ** 2) - 1.0) < 1e-15 and n[2] > 0 and ref.PLANE[2] != n[2]
    assert ref.normalise([0.0, 0.0, -2.0, 4.0]) == (0.0, 0.0, 1.0, -2.0)


@pytest.mark.parametrize("sc", BIG, ids=[sc.name for sc in BIG])
def test_a_wide_open_gate_gives_the_oracles_plain_grid(sc):
    before = sc.bits_before()
    wide = ref.gate(before[0], sc.heights(), sc.slacks(), [-math.inf] * 5, [math.inf] * 5)
    assert np.array_equal(wide, before[0])
    want = _oracle_grid(sc)
    assert np.array_equal(sc.grid_after(before, CM), want) and np.count_nonzero(want) > 20


@pytest.mark.parametrize("sc", BIG, ids=[sc.name for sc in BIG])
def test_larger_scenes_gate_and_keep_a_fair_share_of_every_bounded_class(sc):
    before = sc.bits_before()[0]
    after = sc.bits_after()[0]
    voting = int((before != 0).sum())
    gated = int(((before != 0) & (after == 0)).sum())
    assert voting >= 40, (sc.name, voting)
    assert gated >= 0.10 * voting and voting - gated >= 0.10 * voting, (sc.name, voting, gated)
    assert np.isin(after, [0]).sum() + (after == before).sum() >= after.size     # one class per pixel: a point keeps all or nothing
    for i in range(5):
        had, has = (before >> i) & 1, (after >> i) & 1
        if math.isfinite(ref.MAX_M[i]) or math.isfinite(ref.MIN_M[i]):
            assert (had & ~has).any() and has.any(), (sc.name, i, int(had.sum()), int(has.sum()))
    veg = (before >> 3) & 1                                     # unbounded above: only the points below the ground go
    assert ((veg == 1) & (after == 0) & (sc.heights() > 0)).sum() == 0


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_changes_the_result_on_some_scene(mutant):
    hit = []
    for sc in BIG + ref.view_scenes() + [ref.exact_scene()[0]]:
        if mutant == "velodyne_plane_on_world_cloud" and sc.frame_id == "velodyne":
            continue
        before = sc.bits_before()
        good = sc.bits_after(before)
        if mutant == "elevation_per_view":
            a, b = sc.layer_after(good), sc.layer_after(good, mutant=mutant)
            changed = any(not np.array_equal(x, y) for x, y in zip(a, b))
        else:
            changed = not np.array_equal(good, sc.bits_after(before, mutant=mutant))
        if changed:
            hit.append(sc.name)
    assert hit, "no scene can tell the rule from its mutant %s" % mutant


def test_exact_boundary_cases_on_the_reference():
    sc, keep = ref.exact_scene()
    h = sc.heights()
    assert h[0] == 0.5 and h[1] == 0.5 + 2.0 ** -52 and h[2] == -0.5 and h[3] == -0.5 - 2.0 ** -51 and h[4] == 0.0
    before = sc.bits_before()
    assert (before[0] == 1).all()                               # every point is a candidate on the grid whose pixel says "road"
    after = sc.bits_after(before)
    assert np.array_equal(after[0] != 0, keep)
    assert sc.gated_counts(before, after) == [int((~keep).sum())]
    inf_sc = ref.Scene("inf", "g64", ref.SIZES[0], 8, 0, plane=ref.EXACT_PLANE, min_m=[-math.inf] * 5, max_m=[math.inf] * 5, slope=0.0,
                       cloud=sc.pcd, sources=sc.sources)
    assert (inf_sc.bits_after()[0] == 1).all()


def test_the_layer_counts_a_point_once_however_many_views_see_it():
    for sc in ref.view_scenes():
        after = sc.bits_after()
        seen = ((after & 0xffff & ref.ELEV_CLASSES) != 0).sum(axis=0)
        assert (seen >= 2).any(), sc.name                       # some point votes a ground class in two views
        layer = sc.layer_after(after)
        assert int(layer[1].sum()) == int((seen >= 1).sum())
        assert (layer[2][layer[1] > 0] <= layer[3][layer[1] > 0]).all()
        assert (layer[2][layer[1] == 0] == ref.EMPTY[2]).all() and (layer[3][layer[1] == 0] == ref.EMPTY[3]).all()
        mean = ref.elevation_mean(layer)
        assert np.isnan(mean[layer[1] == 0]).all() and np.isfinite(mean[layer[1] > 0]).all()


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_config_defaults():
    from vision_semantic_segmentation_amd.config import get_cfg_defaults
    m = get_cfg_defaults().MAPPING
    assert m.HEIGHT_GATE.ENABLED is False and m.ELEVATION.ENABLED is False
    assert m.HEIGHT_GATE.MIN_M == -0.5 and list(m.HEIGHT_GATE.MAX_M) == [0.5, 0.5, 0.5, math.inf, 0.5] and m.HEIGHT_GATE.SLOPE == 0.02
    assert list(m.ELEVATION.CLASSES) == ["road", "crosswalk", "lane", "sidewalk"] and m.ELEVATION.QUANTUM_M == 0.001


def _stub(cfg):
    from vision_semantic_segmentation_amd.mapping import SemanticMapping
    stub = types.SimpleNamespace(height_gate_cfg=cfg.MAPPING.HEIGHT_GATE, elevation_cfg=cfg.MAPPING.ELEVATION,
                                 label_names=list(cfg.LABELS_NAMES), ground_plane=None)
    stub._per_label = lambda v, what: SemanticMapping._per_label(stub, v, what)
    return stub


def test_bounds_and_class_names_are_parsed_at_construction():
    from vision_semantic_segmentation_amd.config import get_cfg_defaults
    from vision_semantic_segmentation_amd.mapping import SemanticMapping
    cfg = get_cfg_defaults()
    stub = _stub(cfg)
    lo, hi, slope = SemanticMapping._parse_height_gate(stub)
    assert lo.tolist() == [-0.5] * 5 and hi.tolist() == [0.5, 0.5, 0.5, math.inf, 0.5] and slope == 0.02
    assert SemanticMapping._parse_elevation(stub) == (0b10111, 0.001)
    for key, bad, match in [("MAX_M", [0.5, 0.5], "2 entries"), ("MIN_M", [0.0] * 6, "6 entries"), ("MAX_M", [0.5, 0.5, "x", 1, 1], "numbers"),
                            ("MIN_M", float("nan"), "NaN"), ("MIN_M", 1.0, "exceeds"), ("SLOPE", -0.1, "SLOPE"), ("SLOPE", float("nan"), "SLOPE"),
                            ("SLOPE", float("inf"), "SLOPE")]:
        cfg = get_cfg_defaults()
        cfg.MAPPING.HEIGHT_GATE[key] = bad
        with pytest.raises(ValueError, match=match):
            SemanticMapping._parse_height_gate(_stub(cfg))
    for key, bad, match in [("CLASSES", ["road", "pavement"], "pavement"), ("QUANTUM_M", 0.0, "QUANTUM_M"), ("QUANTUM_M", float("inf"), "QUANTUM_M")]:
        cfg = get_cfg_defaults()
        cfg.MAPPING.ELEVATION[key] = bad
        with pytest.raises(ValueError, match=match):
            SemanticMapping._parse_elevation(_stub(cfg))


def test_height_plane_is_the_normalised_plane_in_the_grids_frame():
    from vision_semantic_segmentation_amd.config import get_cfg_defaults
    from vision_semantic_segmentation_amd.mapping import SemanticMapping, origin_to_velodyne, velodyne_to_baselink
    stub = _stub(get_cfg_defaults())
    stub._origin_to_velodyne = lambda pose: origin_to_velodyne(pose, velodyne_to_baselink())
    stub._plane_in_grid_frame = lambda plane, pose, frame: SemanticMapping._plane_in_grid_frame(stub, plane, pose, frame)
    with pytest.raises(RuntimeError, match="ground plane"):
        SemanticMapping.height_plane(stub, None, "velodyne")
    stub.ground_plane = np.array(ref.PLANE)
    assert tuple(SemanticMapping.height_plane(stub, None, "velodyne")) == ref.normalise(ref.PLANE)
    assert tuple(SemanticMapping.height_plane(stub, ref.POSE7, "world")) == ref.plane_in_cloud_frame(ref.PLANE, "world", ref.POSE7)
    assert tuple(SemanticMapping.height_plane(stub, None, "velodyne", [0, 0, -2.0, 4.0])) == (0.0, 0.0, 1.0, -2.0)
    with pytest.raises(ValueError, match="vertical"):
        SemanticMapping.height_plane(stub, None, "velodyne", [1.0, 0.0, 0.0, 1.0])
    assert SemanticMapping._gate_if_plane(types.SimpleNamespace(height_gate_enabled=lambda: True, ground_plane=None)) == {"_gate": False}
    assert SemanticMapping._gate_if_plane(types.SimpleNamespace(height_gate_enabled=lambda: False, ground_plane=None)) == {}
    assert SemanticMapping._gate_if_plane(types.SimpleNamespace(height_gate_enabled=lambda: True, ground_plane=np.ones(4))) == {}


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _frame(L, g, ht, pts, n=4, cm=True, image=None):
    from vision_semantic_segmentation_amd import _lib
    P = (C.c_double * 12)(*([1.0] * 12))
    src = (C.c_void_p * 1)(pts if image is None else image)
    colours = (C.c_uint8 * 15)(*[v for c in mo.LABEL_COLORS for v in c])
    cmh = (C.c_double * 25)(*([0.0] * 25))
    rc = L.avl_fused_frame_views_height(C.byref(g), pts, n, _lib.AVL_F64, 8, 8 * n, 1, P, None, 100.0, _lib.AVL_SRC_RGB, src, 8, 8, 8, 8, None,
                                        colours, cmh if cm else None, 0, None, None, C.byref(ht) if ht is not None else None, None)
    return rc, _lib.last_error()


def test_argument_errors_return_before_any_gpu_work():
    """every refusal of the new entry points comes from the host: no GPU is needed to see it.  The pointers are host memory that no
    kernel ever sees, since every call below is refused"""
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.AvlHeight) == 8 + 32 + 128 + 128 + 8 + 8 + 8 + 8 + 32
    buf = np.zeros(4096, dtype=np.uint8)
    ptr = (buf.ctypes.data + 63) // 64 * 64
    g = _lib.AvlGrid()
    g.map, g.map_dtype, g.Hm, g.Wm, g.C = ptr, _lib.AVL_F64, 4, 4, 5
    g.resolution = 0.5
    g.cell_mask, g.touched, g.touched_cap, g.counter, g.counter_len = ptr, ptr, 1 << 20, ptr, 256

    def height(**kw):
        ht = _lib.AvlHeight()
        ht.gate = 1
        ht.plane[:] = [0.0, 0.0, 1.0, 2.0]
        ht.min_m[:5] = [-0.5] * 5
        ht.max_m[:5] = [0.5] * 5
        ht.slope, ht.quantum = 0.02, 0.001
        for k, v in kw.items():
            if isinstance(v, tuple):
                arr = getattr(ht, k)
                arr[v[0]] = v[1]
            else:
                setattr(ht, k, v)
        return ht

    rc, msg = _frame(L, g, None, ptr)
    assert rc == -1 and "avl_height is NULL" in msg
    rc, msg = _frame(L, g, height(), None, image=ptr)
    assert rc == -1 and "pts is NULL" in msg                                   # what the plain calls refuse
    rc, msg = _frame(L, g, height(), ptr, cm=False)
    assert rc == -1 and "cm_host is NULL" in msg
    for kw, match in [(dict(plane=(0, math.nan)), "plane coefficient 0"), (dict(plane=(3, math.inf)), "plane coefficient 3"),
                      (dict(plane=(2, 0.0)), "c > 0"), (dict(plane=(2, -1.0)), "c > 0"), (dict(min_m=(1, math.nan)), "class 1 is a NaN"),
                      (dict(max_m=(4, math.nan)), "class 4 is a NaN"), (dict(min_m=(2, 0.75)), "class 2: min"), (dict(slope=-0.01), "slope"),
                      (dict(slope=math.nan), "slope"), (dict(gate=2), "gate = 2"), (dict(gated=ptr + 2), "gated counts"),
                      (dict(elev_sum=ptr), "1 of its 4"), (dict(elev_sum=ptr, elev_cnt=ptr, elev_max=ptr), "3 of its 4"),
                      (dict(elev_classes=1, quantum=0.0), "quantum"), (dict(elev_classes=1, quantum=math.inf), "quantum"),
                      (dict(elev_classes=1, quantum=-1.0), "quantum"), (dict(elev_classes=1 << 5), "beyond C"),
                      (dict(elev_sum=ptr + 4, elev_cnt=ptr, elev_min=ptr, elev_max=ptr, elev_classes=1), "8-byte"),
                      (dict(elev_sum=ptr, elev_cnt=ptr + 2, elev_min=ptr, elev_max=ptr, elev_classes=1), "4-byte")]:
        rc, msg = _frame(L, g, height(**kw), ptr)
        assert rc == -1 and match in msg, (kw, msg)
    # bounds of classes the grid does not have, and a gate that is off, are not read
    g.C = 2
    rc, msg = _frame(L, g, height(min_m=(3, math.nan), gate=0, slope=-1.0), None, image=ptr)
    assert rc == -1 and "pts is NULL" in msg
    g.C = 5

    ht = height()
    assert L.avl_point_heights(None, 5, _lib.AVL_F64, 8, 40, None, C.byref(ht), ptr, ptr, None) == -1 and "pts is NULL" in _lib.last_error()
    assert L.avl_point_heights(ptr, 5, _lib.AVL_F64, 8, 40, None, None, ptr, ptr, None) == -1 and "avl_height is NULL" in _lib.last_error()
    assert L.avl_point_heights(ptr, 5, _lib.AVL_F64, 8, 40, None, C.byref(height(plane=(2, 0.0))), ptr, ptr, None) == -1
    assert L.avl_point_heights(ptr, 5, _lib.AVL_F64, 8, 40, None, C.byref(height(slope=math.nan)), ptr, ptr, None) == -1
    assert L.avl_point_heights(ptr, 5, _lib.AVL_F64, 8, 40, None, C.byref(ht), None, ptr, None) == -1 and "NULL" in _lib.last_error()
    assert L.avl_point_heights(ptr, 5, _lib.AVL_F64, 8, 40, None, C.byref(ht), ptr + 4, ptr, None) == -1 and "8-byte" in _lib.last_error()
    assert L.avl_point_heights(ptr, 0, _lib.AVL_F64, 8, 8, None, C.byref(ht), None, None, None) == 0          # an empty cloud: nothing to do
    assert L.avl_elevation_mean(ptr, ptr, 16, 0.0, ptr, None) == -1 and "quantum" in _lib.last_error()
    assert L.avl_elevation_mean(ptr, ptr, 16, math.nan, ptr, None) == -1
    assert L.avl_elevation_mean(None, ptr, 16, 0.001, ptr, None) == -1 and "NULL" in _lib.last_error()
    assert L.avl_elevation_mean(ptr + 4, ptr, 16, 0.001, ptr, None) == -1 and "8-byte" in _lib.last_error()
    assert L.avl_elevation_mean(ptr, ptr, -1, 0.001, ptr, None) == -1
    assert L.avl_elevation_reset(ptr, None, ptr, ptr, 16, None) == -1 and "NULL" in _lib.last_error()
    assert L.avl_elevation_reset(ptr, ptr, ptr + 2, ptr, 16, None) == -1 and "4-byte" in _lib.last_error()
    assert L.avl_elevation_reset(None, None, None, None, 0, None) == 0
