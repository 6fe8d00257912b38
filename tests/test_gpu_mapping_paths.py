"""Every vote / apply path of avl_fused_frame (include/avl_hip.h, avl_fused_frame_path), for both semantic sources and both
grid types, against the NumPy oracle run on a grid of the same dtype: bit for bit after every frame.

The path a case means to run is asserted before each frame, so a change of the selection rule cannot silently move a case onto
another path.  Label sets go through the config as a user would set them (LABELS_NAMES / LABEL_COLORS): class counts 1 to 16,
two lane classes (byte-mask bonus bits 6 and 7, 32-bit bonus bits 16 and 31), two classes that differ only in blue (a point
votes for both: blue is ignored) and a class whose colour never occurs.  Half the points carry intensities on and
next to the lane bonus edges (2.0 and 14.0 give no bonus, 1.999 and 14.001 do, NaN does not)."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IMG_H, IMG_W = 480, 640
SMALL_H, SMALL_W = 133, 167          # class-map source: a non-integer nearest upscale to the image size

_ROAD, _CROSS, _LANE, _SIDEWALK, _VEG = [128, 64, 128], [140, 140, 200], [255, 255, 255], [244, 35, 232], [107, 142, 35]


def _palette_rg_distinct():
    """the 16 palette colours with distinct (R, G), first occurrence of each"""
    from oracle.mapping_oracle import PALETTE_19
    out, seen = [], set()
    for c in PALETTE_19:
        if (c[0], c[1]) not in seen:
            seen.add((c[0], c[1]))
            out.append(list(c))
    assert len(out) == 16
    return out


LABEL_SETS = {
    "c5": (["road", "crosswalk", "lane", "vegetation", "sidewalk"], [_ROAD, _CROSS, _LANE, _VEG, _SIDEWALK]),
    # 6 classes + 2 lane bonus bits = all 8 bits of the byte mask
    "c6_two_lanes": (["road", "crosswalk", "lane", "vegetation", "sidewalk", "lane"], [_ROAD, _CROSS, _LANE, _VEG, _SIDEWALK, [220, 220, 0]]),
    # 7 + 2 = 9 bits: the 32-bit mask only
    "c7_two_lanes": (["road", "crosswalk", "lane", "vegetation", "sidewalk", "lane", "building"],
                     [_ROAD, _CROSS, _LANE, _VEG, _SIDEWALK, [220, 220, 0], [70, 70, 70]]),
    # 16 classes, lanes at 0 and 15: bonus bits 16 and 31 of the 32-bit mask
    "c16_lanes_0_15": (["lane"] + ["c%d" % i for i in range(1, 15)] + ["lane"], _palette_rg_distinct()),
    "c1_lane": (["lane"], [_LANE]),
    # classes 0 and 1 share R and G (blue differs): a road point votes for both; class 3's colour never occurs
    "blue_differs_and_absent": (["road", "road_blue", "lane", "never", "sidewalk"], [_ROAD, [128, 64, 7], _LANE, [1, 2, 3], _SIDEWALK]),
}

# (id, path, Hm, Wm, resolution, label set, points of the three frames: n, n shifted, another n)
CASES = [
    ("p3_1000_c5", 3, 1000, 1000, 0.25, "c5", (30000, 12000)),
    ("p3_1000_c6_two_lanes", 3, 1000, 1000, 0.25, "c6_two_lanes", (30000, 12000)),
    ("p3_1000_c1_lane", 3, 1000, 1000, 0.25, "c1_lane", (30000, 12000)),
    ("p2_160_c5", 2, 160, 160, 0.5, "c5", (20000, 40000)),
    ("p2_160_c6_two_lanes", 2, 160, 160, 0.5, "c6_two_lanes", (20000, 40000)),
    ("p2_160_blue_absent", 2, 160, 160, 0.5, "blue_differs_and_absent", (20000, 40000)),
    ("p1_1002_c5", 1, 1002, 1002, 0.25, "c5", (30000, 12000)),               # cells % 16 == 4: no byte mask
    ("p1_160_c7_two_lanes", 1, 160, 160, 0.5, "c7_two_lanes", (20000, 40000)),
    ("p1_160_c16", 1, 160, 160, 0.5, "c16_lanes_0_15", (20000, 40000)),
    ("p0_999x1001_c5", 0, 999, 1001, 0.25, "c5", (30000, 12000)),             # odd cell count: no sweep
    ("p0_1000_c7_two_lanes", 0, 1000, 1000, 0.25, "c7_two_lanes", (6000, 3000)),  # 9 bits, n * 128 < cells
    ("p0_1002_blue_absent", 0, 1002, 1002, 0.25, "blue_differs_and_absent", (5000, 3000)),
    ("p0_201x199_c16", 0, 201, 199, 0.5, "c16_lanes_0_15", (20000, 8000)),
]


def _boundary(Hm, Wm, res):
    from oracle import mapping_oracle as mo
    ox, oy = mo.PCD_ORIGIN_OFFSET[0], mo.PCD_ORIGIN_OFFSET[1]
    return [[ox - Hm * res / 2, ox + Hm * res / 2], [oy - Wm * res / 2, oy + Wm * res / 2]]


def make_sm(label_set, Hm, Wm, res, grid_dtype, device):
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults, synthetic as syn
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    names, colors = LABEL_SETS[label_set]
    cfg = get_cfg_defaults()
    cfg.LABELS = list(range(len(names)))
    cfg.LABELS_NAMES = list(names)
    cfg.LABEL_COLORS = [list(c) for c in colors]
    cfg.MAPPING.BOUNDARY = _boundary(Hm, Wm, res)
    cfg.MAPPING.RESOLUTION = res
    cfg.MAPPING.PCD.USE_INTENSITY = True
    cfg.MAPPING.GRID_DTYPE = grid_dtype
    sm = SemanticMapping(cfg, device=device, logger=MyLogger("test", quiet=True))
    sm.confusion_matrix = syn.log_confusion(len(names))
    assert (sm.map_height, sm.map_width, sm.map_depth) == (Hm, Wm, len(names))
    return sm


def oracle_cfg(sm):
    return dict(range_max=sm.pcd_range_max, boundary=sm.map_boundary, resolution=sm.resolution, label_names=list(sm.label_names),
                label_colors=np.asarray(sm.label_colors), confusion_matrix=sm.confusion_matrix, use_pcd_intensity=True)


def frame_path(sm, n):
    """the path avl_fused_frame will take for n points on this grid (frame_device sizes the scratch the same way first)"""
    from vision_semantic_segmentation_amd import _lib
    g = sm.grid
    g.ensure_capacity(n)
    gs = g.struct()
    return _lib.lib().avl_fused_frame_path(C.byref(gs), n, sm._bonus_classes())


EDGE_INTENSITIES = np.array([2.0, 14.0, 1.999, 14.001, np.nan, np.nextafter(2.0, 0.0), np.nextafter(14.0, 99.0)])


def cloud(rng, n, cam):
    from vision_semantic_segmentation_amd import synthetic as syn
    pcd = syn.make_cloud(rng, n, cam.K, cam.R, cam.t, IMG_W, IMG_H)
    k = np.arange(0, n, 2)
    pcd[3, k] = EDGE_INTENSITIES[(k // 2) % EDGE_INTENSITIES.size]
    return pcd


class Scene(object):
    """camera, semantic source on the device and the colour image the oracle projects onto"""

    def __init__(self, rng, src_kind, device):
        import torch
        from oracle import mapping_oracle as mo
        from vision_semantic_segmentation_amd import synthetic as syn
        from vision_semantic_segmentation_amd.camera import camera_setup_1
        self.cam = camera_setup_1().scaled(IMG_W / 1920.0, IMG_H / 1440.0)
        self.src_kind = src_kind
        if src_kind == "rgb":
            self.image = syn.colorize(syn.make_label_map(rng, IMG_H, IMG_W, tile=9))
            self.src = torch.from_numpy(self.image).to(device)
        else:
            small = syn.make_label_map(rng, SMALL_H, SMALL_W, tile=3)
            self.image = mo.semantic_image_from_labels(small, IMG_H, IMG_W)
            self.src = torch.from_numpy(small).to(device)

    def run(self, sm, pcd):
        sm.frame_device(pcd, "velodyne", self.src, None, self.cam, src_kind=self.src_kind, image_size=(IMG_H, IMG_W))


def check_frame(sm, scene, grid, pcd, want_path, what):
    from oracle import mapping_oracle as mo
    n = pcd.shape[1]
    got_path = frame_path(sm, n)
    assert got_path == want_path, "%s: n = %d takes path %d, not %d" % (what, n, got_path, want_path)
    scene.run(sm, pcd)
    mo.mapping_frame(grid, pcd, "velodyne", scene.image, None, scene.cam.P, oracle_cfg(sm))
    got = sm.map
    assert got.dtype == grid.dtype
    assert np.array_equal(got, grid), "%s: %d of %d values differ" % (what, int((got != grid).sum()), grid.size)
    assert not bool(sm.grid.cell_mask.any()), "%s: vote mask not cleared" % what
    assert not bool(sm.grid.counter[4:].any()), "%s: list cursors / tickets not back to zero" % what


@pytest.mark.parametrize("grid_dtype", ["f64", "f32"])
@pytest.mark.parametrize("src_kind", ["rgb", "classmap"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_frame_path_matches_oracle(case, src_kind, grid_dtype, cuda_device):
    name, path, Hm, Wm, res, label_set, (n1, n3) = case
    rng = np.random.default_rng(zlib.crc32(("%s/%s/%s" % (name, src_kind, grid_dtype)).encode()))
    sm = make_sm(label_set, Hm, Wm, res, grid_dtype, cuda_device)
    scene = Scene(rng, src_kind, cuda_device)
    grid = np.zeros((Hm, Wm, sm.map_depth), dtype=np.float64 if grid_dtype == "f64" else np.float32)
    pcd = cloud(rng, n1, scene.cam)
    check_frame(sm, scene, grid, pcd, path, "frame 1")
    assert np.count_nonzero(grid) > 100
    pcd2 = pcd.copy()
    pcd2[0:2] += 0.37
    check_frame(sm, scene, grid, pcd2, path, "frame 2 (shifted)")
    check_frame(sm, scene, grid, cloud(rng, n3, scene.cam), path, "frame 3 (n = %d)" % n3)


@pytest.mark.parametrize("grid_dtype", ["f64", "f32"])
@pytest.mark.parametrize("seq", [
    ("c5", 200, 200, 0.5, ((10000, 3), (25000, 2), (10000, 3), (20000, 3))),   # 2n > cells switches to the sweep and back
    ("c5", 1002, 1002, 0.25, ((5000, 0), (30000, 1), (5000, 0))),              # n * 128 >= cells switches to the sweep and back
    ("c16_lanes_0_15", 160, 160, 0.5, ((150, 0), (20000, 1), (150, 0))),
], ids=["3_2_3_3", "0_1_0", "c16_0_1_0"])
def test_consecutive_frames_on_different_paths(seq, grid_dtype, cuda_device):
    """One grid, frames whose sizes move the frame from path to path: the scratch each path leaves behind (byte or 32-bit mask,
    list cursors) must be what the next path expects."""
    label_set, Hm, Wm, res, frames = seq
    rng = np.random.default_rng(Hm * 7 + len(frames))
    sm = make_sm(label_set, Hm, Wm, res, grid_dtype, cuda_device)
    scene = Scene(rng, "rgb", cuda_device)
    grid = np.zeros((Hm, Wm, sm.map_depth), dtype=np.float64 if grid_dtype == "f64" else np.float32)
    for k, (n, path) in enumerate(frames):
        check_frame(sm, scene, grid, cloud(rng, n, scene.cam), path, "frame %d" % (k + 1))
    assert np.count_nonzero(grid) > 100


@pytest.mark.parametrize("np_dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("label_set", sorted(LABEL_SETS))
def test_update_map_numpy_grid_label_sets(label_set, np_dtype, cuda_device):
    """update_map on a NumPy grid (the reference's calling convention: avl_vote_points + avl_grid_apply on the touched rows) with
    every label set, float64 and float32 arrays, two accumulating updates: bit for bit against the oracle on the same dtype."""
    from oracle import mapping_oracle as mo
    rng = np.random.default_rng(len(label_set) * 31 + (np_dtype == np.float32))
    sm = make_sm(label_set, 400, 400, 0.25, "f64", cuda_device)
    scene = Scene(rng, "rgb", cuda_device)
    grid = np.zeros((400, 400, sm.map_depth), dtype=np_dtype)
    want = grid.copy()
    oc = oracle_cfg(sm)
    for k in range(2):
        pcd = cloud(rng, 20000, scene.cam)
        mp, lab = sm.project_pcd(pcd, "velodyne", scene.image, None, scene.cam)
        assert sm.update_map(grid, mp, lab) is grid
        assert grid.dtype == np_dtype
        mo.update_map(want, mp, lab, oc["boundary"], oc["resolution"], oc["label_names"], oc["label_colors"], oc["confusion_matrix"], True)
        assert np.array_equal(grid, want), "update %d: %d values differ" % (k + 1, int((grid != want).sum()))
    assert np.count_nonzero(want) > 100
