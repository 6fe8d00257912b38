"""The ground fill's reference and cases (tests/_ground_fill_reference.py) checked without a GPU: the premise of the rule's
equivalence (every virtual point lands in its own cell), the share of candidates, the properties the cases claim, the power of the
cases against likely mis-implementations (MUTANTS), plane_to_frame and the configuration."""
import types

import numpy as np
import pytest

import _ground_fill_reference as ref
from oracle import mapping_oracle as mo

CASES = ref.cases()
IDS = [c["name"] for c in CASES]
_EXPECTED = {}


def expected(case, dtype=np.float64):
    """the reference's result for a case, computed once: (grid0, grid, counts, stats)"""
    key = (case["name"], np.dtype(dtype).name)
    if key not in _EXPECTED:
        stats = {}
        grid0 = ref.seeded_grid(case, dtype)
        grid, counts = ref.expected(case, grid0, stats=stats)
        _EXPECTED[key] = (grid0, grid, counts, stats)
    return _EXPECTED[key]


def test_the_case_names_are_distinct_and_cover_the_list():
    assert len(set(IDS)) == len(IDS)
    kinds = {(c["kind"], len(c["P"])) for c in CASES}
    assert {(k, v) for k in ("classmap", "rgb", "logits") for v in (1, 3)} <= kinds
    assert {c["frame"] for c in CASES} == {"velodyne", "world"}
    assert {c["C"] for c in CASES} == {5, 16} and any(len(c["P"]) == 4 and c["C"] == 16 for c in CASES)
    assert any(c["window"] == ((45, 30), (37, 41)) for c in CASES) and any(c["window"][0][0] < 0 for c in CASES)
    assert any(c["weight"] == 0.5 for c in CASES) and any(tuple(c["plane"][:2]) == (0.03, -0.02) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_virtual_point_lands_in_its_own_cell(case):
    pcd, i, j = ref.virtual_cloud(case)
    pix, on = mo.cell_indices(pcd, case["boundary"], case["res"], case["Hm"], case["Wm"])
    assert on.all() and np.array_equal(pix[0], i) and np.array_equal(pix[1], j)
    (x0, y0), (h, w) = case["window"]
    assert len(i) == (min(x0 + h, case["Hm"]) - max(x0, 0)) * (min(y0 + w, case["Wm"]) - max(y0, 0))
    assert np.isfinite(pcd).all()


@pytest.mark.parametrize("geometry", [([[-100.0, 100.0], [-100.0, 100.0]], 0.1), ([[0.0, 70.0], [-10.0, 10.0]], 0.1),
                                      ([[-3.3, 17.77], [1.01, 9.2]], 0.07), ([[-100.0, 100.0], [-100.0, 100.0]], 0.3)],
                         ids=["2000x2000", "700x200", "odd_0.07", "default_0.3"])
def test_cell_centres_land_in_their_own_cells_on_other_grids(geometry):
    boundary, res = geometry
    Hm, Wm = mo.map_dims(boundary, res)
    case = dict(boundary=boundary, res=res, Hm=Hm, Wm=Wm, window=((0, 0), (Hm, Wm)), frame="velodyne", plane=np.array(ref.GROUND))
    pcd, i, j = ref.virtual_cloud(case)
    pix, on = mo.cell_indices(pcd, boundary, res, Hm, Wm)
    assert on.all() and np.array_equal(pix[0], i) and np.array_equal(pix[1], j)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_candidate_share_and_claimed_properties(case):
    _, grid, counts, st = expected(case)
    share = st["candidates"] / st["cells"]
    print("%s: %d of %d cells are candidates (%.0f %%), filled %s, culled %s, abstained %s, range cut %d, masked votes %d, empty %d" % (
        case["name"], st["candidates"], st["cells"], 100 * share, counts["filled"], counts["culled"], counts["abstained"],
        st["range_cut"], st["masked_votes"], st["empty"]))
    assert 0.10 <= share <= 0.90
    assert all(f > 0 for f in counts["filled"])
    assert st["range_cut"] >= 1                                   # a cell in the image, within the cloud's range, beyond the fill's
    assert st["masked_votes"] >= 1                                # a vote for a class that CLASSES leaves out
    if len(case["P"]) > 1:
        assert st["multi"] >= 1                                   # a cell that takes the votes of several views
    if case["occl"] is not None:
        assert st["culled"] >= 1 and st["empty"] >= 1
    if case["kind"] == "logits" and case["min_margin"] > 0:
        assert sum(counts["abstained"]) >= 1
    if case["kind"] == "logits" and case["min_margin"] == 0:
        assert sum(counts["abstained"]) == 0


def test_the_gate_cases_differ_only_in_the_gate():
    g0, g3 = (expected(c)[1] for c in CASES if c["name"] in ("gate_0", "gate_0.3"))
    assert not np.array_equal(g0, g3)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_direct_apply_equals_the_oracles_update_map(case):
    """the mutants are applied to cells by index (apply_direct, rule 5 written out): without a mutant that is what the oracle's
    update_map does with the virtual cloud, for both map types"""
    for dtype in (np.float64, np.float32):
        grid0, grid, counts, _ = expected(case, dtype)
        direct, direct_counts = ref.expected(case, grid0, direct=True)
        assert direct.dtype == grid.dtype and np.array_equal(direct, grid) and direct_counts == counts
        assert not np.array_equal(grid, grid0)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_changes_the_grid_of_some_case(mutant):
    hit = []
    for case in CASES:
        if mutant == "empty_culls" and case["occl"] is None:
            continue
        if mutant == "plane_not_in_grid_frame" and case["frame"] == "velodyne":
            continue
        dtype = np.float32 if mutant == "round_once" else np.float64
        grid0, grid, _, _ = expected(case, dtype)
        if not np.array_equal(ref.expected(case, grid0, mutant=mutant)[0], grid):
            hit.append(case["name"])
    assert hit, "no case can tell the rule from its mutant %s" % mutant


# ---------------------------------------------------------------------------------------------------------------- plane_to_frame
def test_plane_to_frame_against_points_moved_by_the_inverse_transform():
    from vision_semantic_segmentation_amd.ground_plane import plane_coefficients, plane_tilt_deg, plane_to_frame
    from vision_semantic_segmentation_amd.plane_3d import Plane3D
    rng = np.random.default_rng(0)
    T = np.linalg.inv(np.matmul(mo.transform_from_pose(ref.WORLD_POSE), mo.velodyne_to_baselink()))      # world -> velodyne
    for plane in (Plane3D(0.03, -0.02, 1.0, 2.0), [0.1, 0.2, -0.9, 1.5], np.array(ref.GROUND)):
        a, b, c, d = plane_coefficients(plane)
        xy = rng.uniform(-30, 30, (2, 50))
        on_plane = np.stack([xy[0], xy[1], -(a * xy[0] + b * xy[1] + d) / c, np.ones(50)])            # velodyne frame
        moved = np.matmul(np.linalg.inv(T), on_plane)                                                   # the same points in the world
        got = plane_to_frame(plane, T)
        assert got.shape == (4,) and got.dtype == np.float64
        assert np.abs(np.matmul(got, moved)).max() < 1e-9
        assert np.array_equal(got, np.matmul(np.array([a, b, c, d]), T))
        assert np.array_equal(plane_to_frame(plane, None), np.array([a, b, c, d]))
    assert np.array_equal(ref.plane_in_grid_frame(dict(frame="world", pose7=ref.WORLD_POSE, plane=np.array(ref.TILTED))),
                          plane_to_frame(ref.TILTED, T))
    assert plane_tilt_deg([0, 0, -2, 1]) == 0.0 and abs(plane_tilt_deg([1, 0, 1, 0]) - 45.0) < 1e-12
    assert np.isnan(plane_tilt_deg([0, 0, 0, 1]))
    res = types.SimpleNamespace(plane=Plane3D(0, 0, 1, 2))
    assert plane_coefficients(res).tolist() == [0.0, 0.0, 1.0, 2.0]
    for bad in ([1, 2, 3], None, types.SimpleNamespace(plane=None)):
        with pytest.raises(ValueError):
            plane_coefficients(bad)


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_config_defaults():
    from vision_semantic_segmentation_amd.config import get_cfg_defaults
    gf = get_cfg_defaults().MAPPING.GROUND_FILL
    assert gf.ENABLED is False
    assert list(gf.SIZE_M) == [60, 60] and gf.RANGE_MAX == 30.0 and gf.WEIGHT == 1.0 and gf.MAX_TILT_DEG == 30
    assert list(gf.CLASSES) == ["road", "crosswalk", "lane", "sidewalk"]


def test_class_names_and_planes_are_checked_on_the_host():
    from vision_semantic_segmentation_amd.config import get_cfg_defaults
    from vision_semantic_segmentation_amd.mapping import SemanticMapping
    cfg = get_cfg_defaults()
    stub = types.SimpleNamespace(ground_fill_cfg=cfg.MAPPING.GROUND_FILL, label_names=list(cfg.LABELS_NAMES), ground_plane=None)
    assert SemanticMapping._ground_fill_class_mask(stub) == 0b10111                # vegetation, class 3, stays out
    assert SemanticMapping.ground_fill_enabled(stub) is False
    cfg.MAPPING.GROUND_FILL.CLASSES = ["road", "pavement"]
    with pytest.raises(ValueError, match="pavement"):
        SemanticMapping._ground_fill_class_mask(stub)
    SemanticMapping.set_ground_plane(stub, [0.0, 0.0, 1.0, 2.0])
    assert stub.ground_plane.tolist() == [0.0, 0.0, 1.0, 2.0]
    stub.set_ground_plane = lambda p: SemanticMapping.set_ground_plane(stub, p)
    SemanticMapping.plane_callback(stub, types.SimpleNamespace(coef=[0.0, 0.1, 1.0, 1.9]))
    assert stub.ground_plane.tolist() == [0.0, 0.1, 1.0, 1.9]
    with pytest.raises(ValueError, match="finite"):
        SemanticMapping.set_ground_plane(stub, [0.0, float("nan"), 1.0, 2.0])


def test_argument_errors_return_before_any_gpu_work():
    """the new entry points refuse bad arguments on the host: no GPU is needed to see it"""
    import ctypes as C
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    assert L.avl_ground_fill_views(None, None, 1, None, None, 1, None, 4, 4, 8, 8, None, None, None, None, None) == -1
    assert L.avl_ground_fill_views_logits(None, None, 1, None, None, None, 8, 8, None, None, None, None) == -1
    assert "avl_point_logits is NULL" in _lib.last_error()
    assert L.avl_occlusion_depth(None, 5, 1, 8, 40, 1, None, None, 100.0, 8, 8, None, None) == -1 and "pts is NULL" in _lib.last_error()
    assert C.sizeof(_lib.AvlGroundFill) == 72
