"""The dense ground fill on the GPU (csrc/mapping.hip: k_ground_fill; avl_ground_fill_views, avl_ground_fill_views_logits,
avl_occlusion_depth) against the NumPy restatement of the rule (tests/_ground_fill_reference.py) and against the vote kernels.

Every grid comparison is of every byte (np.array_equal), for f64 and f32 maps, from a seeded non-zero grid.  The shapes are the
smallest at which the kernel can still go wrong: a 96 x 80 grid at 0.25 m (30 workgroups), projection images of 64 x 48 and 97 x 61
pixels, class maps of half that size, logits of 12 x 16 x 19 with rows of 19 and 24 floats, a 37 x 41 window (a tail wave), a window
that hangs over two edges of the grid, 1 to 5 views and 5 and 16 map classes."""
import ctypes as C

import numpy as np
import pytest

import _ground_fill_reference as ref
import _occlusion_reference as occ
from oracle import mapping_oracle as mo

pytestmark = pytest.mark.gpu

CASES = ref.cases()
IDS = [c["name"] for c in CASES]
DTYPES = {"f64": np.float64, "f32": np.float32}
_EXPECTED = {}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def expected(case, dtype):
    """the reference's (grid0, grid, counts) of a case, computed once and never changed"""
    key = (case["name"], dtype)
    if key not in _EXPECTED:
        grid0 = ref.seeded_grid(case, DTYPES[dtype])
        grid, counts = ref.expected(case, grid0)
        _EXPECTED[key] = (grid0, grid, counts)
    return _EXPECTED[key]


class Cam(object):
    def __init__(self, P):
        self.P = P


def make_sm(case, device, dtype, enabled=False, classes=None, cloud_range=ref.CLOUD_RANGE):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = get_cfg_defaults()
    cfg.LABELS = list(range(case["C"])) if case["C"] != 5 else cfg.LABELS
    cfg.LABELS_NAMES = list(case["names"])
    cfg.LABEL_COLORS = [list(c) for c in case["colours"]]
    cfg.MAPPING.BOUNDARY = case["boundary"]
    cfg.MAPPING.RESOLUTION = case["res"]
    cfg.MAPPING.GRID_DTYPE = dtype
    cfg.MAPPING.PCD.USE_INTENSITY = False
    cfg.MAPPING.PCD.RANGE_MAX = cloud_range
    gf = cfg.MAPPING.GROUND_FILL
    gf.ENABLED, gf.RANGE_MAX, gf.WEIGHT = enabled, case["range_max"], case["weight"]
    gf.CLASSES = list(case["classes"] if classes is None else classes)
    if case["occl"] is not None:
        o = cfg.MAPPING.OCCLUSION
        o.ENABLED, o.CELL_PX, o.RADIUS, o.REL_TOL, o.ABS_TOL = True, case["occl"]["s"], case["occl"]["R"], case["occl"]["rel"], case["occl"]["abs_"]
    sm = SemanticMapping(cfg, device=device, logger=MyLogger("test", quiet=True))
    sm.confusion_matrix = case["cm"]
    sm.min_margin = case["min_margin"]
    assert (sm.map_height, sm.map_width, sm.map_depth) == (case["Hm"], case["Wm"], case["C"])
    return sm


def dev_sources(case, device):
    """the case's sources on the device; logits keep their row stride"""
    import torch
    out = []
    for src in case["sources"]:
        if case["kind"] == "logits":
            base = src.base if src.base is not None and src.base.ndim == src.ndim else src
            out.append(torch.from_numpy(np.ascontiguousarray(base)).to(device)[..., :src.shape[-1]])
        else:
            out.append(torch.from_numpy(np.ascontiguousarray(src)).to(device))
    return out


def pose_of(case):
    from vision_semantic_segmentation_amd.utils import Pose
    return None if case["pose7"] is None else Pose.from_array(case["pose7"])


def fill(sm, case, device, sources=None, **kw):
    args = dict(plane=case["plane"], grid_frame_id=case["frame"], src_kind=case["kind"], image_size=(case["img_h"], case["img_w"]),
                net_size=case["net"], net_palette=case["palette"], window=case["window"], pcd=case["cloud"], pcd_frame_id=case["frame"])
    args.update(kw)
    sm.ground_fill_device(dev_sources(case, device) if sources is None else sources, pose_of(case), [Cam(P) for P in case["P"]], **args)


def check_counts(sm, case, counts):
    assert sm.last_filled.cpu().tolist() == counts["filled"]
    if case["occl"] is not None:
        assert sm.last_culled.cpu().tolist() == counts["culled"]
    if case["kind"] == "logits":
        assert sm.last_abstained.cpu().tolist() == counts["abstained"]


# ---------------------------------------------------------------------------------------------------------------- 1, 3, 4: against the reference
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_fill_equals_the_reference(case, dtype, cuda_device):
    grid0, grid, counts = expected(case, dtype)
    sm = make_sm(case, cuda_device, dtype)
    sm.map = grid0
    fill(sm, case, cuda_device)
    got = sm.map
    print("%s %s: filled %s culled %s abstained %s, %d values differ" % (case["name"], dtype, sm.last_filled.cpu().tolist(),
          None if sm.last_culled is None else sm.last_culled.cpu().tolist(),
          None if sm.last_abstained is None else sm.last_abstained.cpu().tolist(), int((got != grid).sum())))
    assert got.dtype == grid.dtype and np.array_equal(got, grid)
    check_counts(sm, case, counts)
    assert not bool(sm.grid.cell_mask.any()) and not bool(sm.grid.counter.any())          # the fill never touches the scratch


def test_the_walls_shadow_is_empty_and_the_rest_is_filled(cuda_device):
    case = by_name("wall_classmap")
    grid0, _, _ = expected(case, "f64")
    sm = make_sm(case, cuda_device, "f64")
    sm.map = grid0
    fill(sm, case, cuda_device)
    changed = (sm.map != grid0).any(axis=2)
    pcd, _, _ = ref.virtual_cloud(case)
    x, y = pcd[0].reshape(case["Hm"], case["Wm"]), pcd[1].reshape(case["Hm"], case["Wm"])
    shadow = (x > 12.5) & (x < 20.0) & (np.abs(y) < 0.2 * x)             # behind the wall at x = 10, |y| < 3
    near = (x > 3.0) & (x < 5.5) & (np.abs(y) < 1.5)                      # in front of the post and the wall
    assert shadow.sum() > 500 and not changed[shadow].any()
    assert changed[near].sum() >= 0.9 * near.sum()
    plain = make_sm(dict(case, occl=None), cuda_device, "f64")            # without culling the shadow takes the wall's labels
    plain.map = grid0
    fill(plain, case, cuda_device)
    assert (plain.map != grid0).any(axis=2)[shadow].sum() > 100


def test_occlusion_depth_alone_gives_the_reference_buffer(cuda_device):
    from vision_semantic_segmentation_amd import _lib
    case = by_name("wall_classmap")
    sm = make_sm(case, cuda_device, "f64")
    V, w, h, s = len(case["P"]), case["img_w"], case["img_h"], case["occl"]["s"]
    o = sm._occlusion(V, h, w)
    sm.last_culled.fill_(5)
    view, T, _, P, stream = sm._frame_args(case["cloud"], "velodyne", None, np.stack(case["P"]), grid=False)
    _lib.check(_lib.lib().avl_occlusion_depth(*view, V, P, T, ref.CLOUD_RANGE, w, h, C.byref(o), stream), "avl_occlusion_depth")
    Hc, Wc = -(-h // s), -(-w // s)
    got = sm._occl_depth[(V, Hc, Wc)].cpu().numpy().view(np.uint32).reshape(V, Hc, Wc)
    for v in range(V):
        want = ref.real_depth(case, v)
        assert np.array_equal(got[v], want), "view %d: %d words differ" % (v, int((got[v] != want).sum()))
        assert (want != occ.EMPTY).sum() > 20 and (want == occ.EMPTY).sum() > 20
    assert sm.last_culled.cpu().tolist() == [0] * V                       # the call resets the counts with the buffer
    empty = np.zeros((4, 0))
    view, T, _, P, stream = sm._frame_args(empty, "velodyne", None, np.stack(case["P"]), grid=False)
    _lib.check(_lib.lib().avl_occlusion_depth(*view, V, P, T, ref.CLOUD_RANGE, w, h, C.byref(o), stream), "avl_occlusion_depth")
    assert bool((sm._occl_depth[(V, Hc, Wc)] == -1).all())               # an empty cloud leaves every cell empty


# ---------------------------------------------------------------------------------------------------------------- 2: against existing code
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["classmap_3views", "logits_3views", "world_classmap_3views", "gate_0.3"])
def test_the_fill_equals_frame_device_views_on_the_virtual_cloud(name, dtype, cuda_device):
    """needs no reference: the vote kernels map the window's cell centres, put on the plane, as a cloud.  USE_INTENSITY off, a full
    class mask and one range for both."""
    case = by_name(name)
    grid0 = ref.seeded_grid(case, DTYPES[dtype])
    a = make_sm(case, cuda_device, dtype, classes=case["names"])
    b = make_sm(case, cuda_device, dtype, classes=case["names"], cloud_range=case["range_max"])
    a.map, b.map = grid0, grid0
    srcs = dev_sources(case, cuda_device)
    fill(a, case, cuda_device, sources=srcs)
    pcd, _, _ = ref.virtual_cloud(case)
    b.frame_device_views(pcd, case["frame"], srcs, pose_of(case), [Cam(P) for P in case["P"]], src_kind=case["kind"],
                         image_size=(case["img_h"], case["img_w"]), net_size=case["net"], net_palette=case["palette"])
    assert np.array_equal(a.map, b.map) and not np.array_equal(a.map, grid0)
    if case["kind"] == "logits":
        assert a.last_abstained.cpu().tolist() == b.last_abstained.cpu().tolist()


# ---------------------------------------------------------------------------------------------------------------- 5: scratch contract
def oracle_frame(grid, case, pcd, v):
    cfg = dict(range_max=ref.CLOUD_RANGE, boundary=case["boundary"], resolution=case["res"], label_names=case["names"],
               label_colors=case["colours"], confusion_matrix=case["cm"], use_pcd_intensity=False)
    return mo.mapping_frame(grid, pcd, "velodyne", ref.colour_image(case, v), None, case["P"][v], cfg)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fill_frame_fill_on_one_grid(dtype, cuda_device):
    case = by_name("classmap_3views")
    cloud = occ.make_cloud(78, 2000)
    grid0, step1, _ = expected(case, dtype)
    want = oracle_frame(np.array(step1, copy=True), case, cloud, 0)
    want, _ = ref.expected(case, want)
    sm = make_sm(case, cuda_device, dtype)
    sm.map = grid0
    srcs = dev_sources(case, cuda_device)
    fill(sm, case, cuda_device, sources=srcs)
    sm.frame_device(cloud, "velodyne", srcs[0], None, Cam(case["P"][0]), src_kind="classmap", image_size=(case["img_h"], case["img_w"]))
    assert not bool(sm.grid.cell_mask.any()) and not bool(sm.grid.counter[4:].any())
    fill(sm, case, cuda_device, sources=srcs)
    assert np.array_equal(sm.map, want)
    assert not bool(sm.grid.cell_mask.any()) and not bool(sm.grid.counter[4:].any())


def test_the_fill_works_without_the_grids_scratch(cuda_device):
    case = by_name("rgb_3views")
    grid0, grid, counts = expected(case, "f64")
    sm = make_sm(case, cuda_device, "f64")
    sm.map = grid0
    full = sm.grid.struct

    def map_only(map_tensor=None):
        g = full(map_tensor)
        g.cell_mask = g.touched = g.counter = None
        g.touched_cap = g.counter_len = 0
        return g
    sm.grid.struct = map_only
    fill(sm, case, cuda_device)
    assert np.array_equal(sm.map, grid)
    check_counts(sm, case, counts)


# ---------------------------------------------------------------------------------------------------------------- 6: refusals
def raw_args(sm, case, device):
    """what ground_fill_device hands avl_ground_fill_views for a class-map case, as a dict that a test may break"""
    import torch
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.mapping import _dbl
    V = len(case["P"])
    srcs = dev_sources(case, device)
    gf = _lib.AvlGroundFill()
    (gf.x0, gf.y0), (gf.h, gf.w) = case["window"]
    gf.plane[:] = [float(v) for v in case["plane"]]
    gf.range_max, gf.class_mask = case["range_max"], 0x1f
    filled = torch.full((V,), 7, dtype=torch.int32, device=device)
    gf.filled = filled.data_ptr()
    return dict(g=sm.grid.struct(), gf=gf, n_views=V, P=_dbl(np.stack(case["P"])), T=None, kind=_lib.AVL_SRC_CLASSMAP,
                src=(C.c_void_p * V)(*[t.data_ptr() for t in srcs]), sw=case["img_w"] // 2, sh=case["img_h"] // 2, iw=case["img_w"],
                ih=case["img_h"], lut=sm._lut_host(case["palette"]), colors=sm._colors_host(), cm=_dbl(case["cm"]), occl=None,
                keep=(srcs, filled))


def raw_call(a):
    from vision_semantic_segmentation_amd import _lib
    g = C.byref(a["g"]) if a["g"] is not None else None
    gf = C.byref(a["gf"]) if a["gf"] is not None else None
    occl = C.byref(a["occl"]) if a["occl"] is not None else None
    rc = _lib.lib().avl_ground_fill_views(g, gf, a["n_views"], a["P"], a["T"], a["kind"], a["src"], a["sw"], a["sh"], a["iw"], a["ih"],
                                          a["lut"], a["colors"], a["cm"], occl, None)
    return rc, _lib.last_error()


def test_bad_arguments_are_refused_and_change_nothing(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import _lib
    case = by_name("classmap_3views")
    grid0, grid, counts = expected(case, "f64")
    sm = make_sm(case, cuda_device, "f64")
    sm.map = grid0

    def broken(change):
        a = raw_args(sm, case, cuda_device)
        change(a)
        rc, msg = raw_call(a)
        torch.cuda.synchronize()
        assert rc == -1, msg
        assert a["keep"][1].cpu().tolist() == [7] * a["keep"][1].numel()           # not even the counts were reset
        return msg

    def put(key, value):
        return lambda a: a.__setitem__(key, value)

    def gf_field(name, value):
        return lambda a: setattr(a["gf"], name, value)

    def plane(k, value):
        return lambda a: a["gf"].plane.__setitem__(k, value)

    assert "NULL" in broken(put("g", None))
    assert "NULL" in broken(put("gf", None))
    assert "NULL" in broken(lambda a: setattr(a["g"], "map", None))
    assert "n_views" in broken(put("n_views", 0))
    assert "n_views" in broken(put("n_views", 5))
    assert "window" in broken(gf_field("h", -1))
    assert "window" in broken(gf_field("w", -1))
    assert "2^31" in broken(lambda a: (setattr(a["gf"], "h", 70000), setattr(a["gf"], "w", 70000)))
    for k in range(4):
        assert "plane" in broken(plane(k, float("nan")))
        assert "plane" in broken(plane(k, float("inf")))
    assert "c = 0" in broken(plane(2, 0.0))
    for bad in (float("nan"), 0.0, -1.0):
        assert "range_max" in broken(gf_field("range_max", bad))
    assert "P_host" in broken(put("P", None))
    assert "cm_host" in broken(put("cm", None))
    assert "lut_host" in broken(put("lut", None))
    assert "src_kind" in broken(put("kind", 7))
    assert "NULL" in broken(lambda a: a["src"].__setitem__(1, None))
    assert "RGB source" in broken(put("kind", _lib.AVL_SRC_RGB))
    assert "aligned" in broken(lambda a: setattr(a["gf"], "filled", a["gf"].filled + 2))
    wall_sm = make_sm(by_name("wall_classmap"), cuda_device, "f64")
    o = wall_sm._occlusion(3, case["img_h"], case["img_w"])
    o.cell_px = 0
    assert "cell_px" in broken(put("occl", o))
    rc = _lib.lib().avl_ground_fill_views_logits(C.byref(sm.grid.struct()), C.byref(raw_args(sm, case, cuda_device)["gf"]), 1, None, None, None,
                                                 64, 48, None, None, None, None)
    assert rc == -1 and "avl_point_logits is NULL" in _lib.last_error()
    assert np.array_equal(sm.map, grid0)

    # a window wholly off the grid succeeds, resets the counts and launches nothing
    for window in (((case["Hm"], 0), (5, 5)), ((0, -9), (5, 9)), ((3, 3), (0, 7))):
        a = raw_args(sm, case, cuda_device)
        (a["gf"].x0, a["gf"].y0), (a["gf"].h, a["gf"].w) = window
        rc, msg = raw_call(a)
        assert rc == 0, msg
        assert a["keep"][1].cpu().tolist() == [0, 0, 0]
    sm._map_host = None
    assert np.array_equal(sm.map, grid0)
    a = raw_args(sm, case, cuda_device)                                             # and the arguments as they stand do fill
    a["gf"].class_mask = ref.class_mask(case)
    assert raw_call(a)[0] == 0 and a["keep"][1].cpu().tolist() == counts["filled"]
    sm._map_host = None
    assert np.array_equal(sm.map, grid)


def test_python_refusals(cuda_device):
    case = by_name("classmap_1view")
    sm = make_sm(case, cuda_device, "f64")
    with pytest.raises(RuntimeError, match="ground plane"):
        fill(sm, case, cuda_device, plane=None)
    with pytest.raises(ValueError, match="tilted"):
        fill(sm, case, cuda_device, plane=[1.0, 0.0, 0.5, 2.0])
    with pytest.raises(ValueError, match="tilted"):
        fill(sm, case, cuda_device, plane=[0.0, 0.0, 0.0, 2.0])
    sm.ground_fill_cfg.CLASSES = ["road", "pavement"]
    with pytest.raises(ValueError, match="pavement"):
        fill(sm, case, cuda_device)
    assert not bool(sm.map_dev.any())


# ---------------------------------------------------------------------------------------------------------------- 7: wiring
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mapping_and_mapping_views_run_the_fill_after_the_frame(dtype, cuda_device):
    case = by_name("rgb_3views")
    cloud = occ.make_cloud(79, 2000)
    cams = [Cam(P) for P in case["P"]]
    images = [np.ascontiguousarray(s) for s in case["sources"]]
    grid0 = ref.seeded_grid(case, DTYPES[dtype])
    on, off, steps = make_sm(case, cuda_device, dtype, enabled=True), make_sm(case, cuda_device, dtype), make_sm(case, cuda_device, dtype)
    for sm in (on, off, steps):
        sm.map = grid0
        sm.pcd, sm.pcd_frame_id = cloud, "velodyne"
    on.mapping_views(images, None, cams)                                  # no plane yet: the frame alone
    off.mapping_views(images, None, cams)
    assert np.array_equal(on.map, off.map) and on.last_filled is None
    on.set_ground_plane(case["plane"])
    off.set_ground_plane(case["plane"])                                   # a plane without ENABLED changes nothing
    on.mapping_views(images, None, cams)
    off.mapping_views(images, None, cams)
    srcs = dev_sources(case, cuda_device)
    for _ in range(2):
        steps.frame_device_views(cloud, "velodyne", srcs, None, cams, src_kind="rgb")
    want_off = np.array(steps.map, copy=True)
    steps.ground_fill_device(srcs, None, cams, plane=case["plane"], grid_frame_id="velodyne", src_kind="rgb")     # the default window
    assert np.array_equal(on.map, steps.map) and on.last_filled.cpu().tolist() == steps.last_filled.cpu().tolist()
    assert np.array_equal(off.map, want_off) and off.last_filled is None and not np.array_equal(on.map, off.map)
    oracle = np.array(grid0, copy=True)                                  # ENABLED False is the parent's behaviour: the oracle's frames
    for _ in range(2):
        for v in range(3):
            oracle_frame(oracle, case, cloud, v)
    assert np.array_equal(off.map, oracle)
    on.mapping(images[1], None, cams[1])
    steps.set_ground_plane(case["plane"])
    steps.frame_device(cloud, "velodyne", srcs[1], None, cams[1], src_kind="rgb")
    steps.ground_fill_device(srcs[1], None, cams[1], src_kind="rgb")     # one camera, one tensor, the plane last set, the cloud's frame
    assert np.array_equal(on.map, steps.map) and on.last_filled.numel() == 1
    assert on.last_filled.cpu().tolist() == steps.last_filled.cpu().tolist()
