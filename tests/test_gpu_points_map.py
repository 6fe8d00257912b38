"""The points map on the GPU (csrc/seg_pointsmap.hip: k_tile_keys, k_points_map_gather; points_map.py; SemanticMapping with
MAPPING.POINTS_MAP.SOURCE = "index") against the NumPy restatement of tests/_points_map_reference.py, byte for byte, and -- the
point of it -- a frame on the gathered cloud against the same frame on the whole map, bit for bit.

The clouds are the smallest that reach every branch: about 5600 points in 8 x 6 tiles of 4 m with empty tiles (the first and the
last of a rectangle's row, a whole row of it), a tile of one point, a tile of 3041 points (a run over several workgroups that ends off
a boundary), points on tile edges, NaN and infinite fields; 70 rows of 1 m tiles (the scan of the run lengths crosses a wave); 1200
rows of 0.05 m tiles (more than one launch takes)."""
import numpy as np
import pytest

import _points_map_reference as ref

pytestmark = pytest.mark.gpu

CLOUDS = {"8x6": (ref.cloud_8x6, ref.TILE), "rows70": (ref.cloud_rows70, 1.0), "tall": (ref.cloud_tall, 0.05)}
IMG = (96, 128)
# the vehicle's poses of the frame tests (x, y, z, yaw, pitch, roll): the first window lies inside the index, the others are clipped
POSES = [ref.pose_from(2.0, 14.0, 0.0, 0.1, 0.02, -0.01), ref.pose_from(20.0, 9.0, 0.1, 2.5, -0.02, 0.03), ref.pose_from(-6.0, 26.0, 0.0, -0.8, 0.0, 0.02)]
_CACHE = {}


def indices(name, device):
    """(the restatement's index, the PointsMapIndex) of a cloud, built once"""
    from vision_semantic_segmentation_amd.points_map import PointsMapIndex
    if name not in _CACHE:
        make, tile_m = CLOUDS[name]
        cloud = make()
        _CACHE[name] = (ref.build(cloud, tile_m), PointsMapIndex(cloud, tile_m, device, keep_keys=True), cloud)
    return _CACHE[name]


def make_sm(device, source="index", radius=0.0, occlusion=False, log_cm=False):
    from oracle import mapping_oracle as mo
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults, synthetic as syn
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = get_cfg_defaults()
    ox, oy = mo.PCD_ORIGIN_OFFSET[:2]
    cfg.MAPPING.BOUNDARY = [[ox - 12.0, ox + 28.0], [oy - 4.0, oy + 36.0]]       # world x -12 .. 28, y -4 .. 36: the index and a margin
    cfg.MAPPING.RESOLUTION = 0.2
    cfg.MAPPING.PCD.RANGE_MAX = ref.RANGE_MAX
    cfg.MAPPING.POINTS_MAP.SOURCE = source
    cfg.MAPPING.POINTS_MAP.TILE_M = ref.TILE
    cfg.MAPPING.POINTS_MAP.RADIUS_M = radius
    cfg.MAPPING.OCCLUSION.ENABLED = occlusion
    cfg.MAPPING.OCCLUSION.CELL_PX, cfg.MAPPING.OCCLUSION.REL_TOL, cfg.MAPPING.OCCLUSION.ABS_TOL = 4, 0.1, 1.0   # the default 8 px cell is a twelfth of this image's height
    sm =SemanticMapping(cfg, device=device, logger=MyLogger("test", quiet=True))
    assert (sm.map_height, sm.map_width, sm.map_depth, sm.grid_dtype) == (200, 200, 5, "f64")
    if log_cm:
        sm.confusion_matrix = syn.log_confusion(5)
    return sm


def cams():
    from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6
    return [c.scaled(IMG[1] / 1920.0, IMG[0] / 1440.0) for c in (camera_setup_1(), camera_setup_6())]


def class_maps(device, n=1):
    import torch
    from vision_semantic_segmentation_amd import synthetic as syn
    rng = np.random.default_rng(3)
    ids = np.array([2, 1, 8, 10, 3, 0], dtype=np.uint8)            # the five map classes and one the map does not hold
    return [torch.from_numpy(ids[syn.make_label_map(rng, IMG[0], IMG[1], num_classes=6, tile=7)]).to(device) for _ in range(n)]


@pytest.mark.parametrize("name", list(CLOUDS))
def test_keys_offsets_and_sorted_cloud_equal_the_restatement(name, cuda_device):
    want, got, cloud = indices(name, cuda_device)
    assert (got.ox, got.oy, got.rows, got.cols, got.tile_m, got.dropped) == (want["ox"], want["oy"], want["rows"], want["cols"], want["tile_m"],
                                                                             want["dropped"])
    assert got.keys.dtype.itemsize == 4 and got.keys.cpu().numpy().tobytes() == want["keys"].tobytes()
    assert got.offsets.cpu().numpy().tobytes() == want["offsets"].tobytes() == got.offsets_host.tobytes()
    pts = got.points.cpu().numpy()
    assert pts.dtype == np.float32 and pts.shape == want["points"].shape and pts.tobytes() == want["points"].tobytes()
    assert len(got) == len(cloud) - want["dropped"] and got.points.data_ptr() % 16 == 0
    if name == "8x6":
        assert (got.rows, got.cols, got.dropped) == (8, 6, ref.N_DROPPED_8X6)
    if name == "tall":
        assert got.rows > 1024


def test_an_index_built_from_the_other_layout_and_dtype_is_the_same(cuda_device):
    from vision_semantic_segmentation_amd.points_map import PointsMapIndex
    want, got, cloud = indices("8x6", cuda_device)
    import torch
    other = PointsMapIndex(torch.from_numpy(np.ascontiguousarray(cloud.T.astype(np.float64))).to(cuda_device), ref.TILE, cuda_device)
    assert other.points.cpu().numpy().tobytes() == want["points"].tobytes() and other.offsets_host.tobytes() == want["offsets"].tobytes()
    # the keys are kept on request only: the index holds the sorted cloud and the offsets
    assert other.keys is None and other.device_bytes() == 16 * len(other) + 4 * (8 * 6 + 1)
    assert got.device_bytes() == other.device_bytes() + 4 * len(cloud)
    empty = PointsMapIndex(np.full((5, 4), np.nan, dtype=np.float32), 3.0, cuda_device)
    assert (empty.rows, empty.cols, empty.dropped, len(empty)) == (0, 0, 5, 0) and empty.offsets_host.tolist() == [0]


def _rects(name, ix):
    if name == "8x6":
        return [ref.clip(r, ix["rows"], ix["cols"]) for r in ref.RECTS.values()] + [(3, 3, 2, 2), (0, 7, 2, 2)]
    if name == "rows70":
        return [(0, 69, 0, 2), (0, 69, 1, 1), (3, 66, 0, 1), (63, 64, 0, 2)]
    return [(0, ix["rows"] - 1, 0, ix["cols"] - 1), (100, 1150, 1, 1), (0, 1023, 0, 1), (0, 1024, 0, 0)]


@pytest.mark.parametrize("name", list(CLOUDS))
def test_the_gathered_cloud_equals_the_restatement_and_the_rest_of_dst_is_untouched(name, cuda_device):
    import torch
    from vision_semantic_segmentation_amd import points_map as pm
    want, got, _ = indices(name, cuda_device)
    cap = len(got) + 300
    sizes = []
    for rect in _rects(name, want):
        expect = ref.gather(want, rect)
        m = len(expect)
        assert pm.window_count(got.offsets_host, got.rows, got.cols, rect) == ref.count(want, rect) and ref.count(want, rect)[0] == m
        dst = torch.full((cap * 16,), 0xAB, dtype=torch.uint8, device=cuda_device).view(torch.float32).view(cap, 4)
        pm.gather(got, rect, dst)
        out = dst.cpu().numpy()
        assert out[:m].tobytes() == expect.tobytes(), rect
        assert (out[m:].view(np.uint8) == 0xAB).all(), rect
        sizes.append(m)
        if m:
            exact = torch.full((m * 16,), 0xAB, dtype=torch.uint8, device=cuda_device).view(torch.float32).view(m, 4)
            pm.gather(got, rect, exact)                                     # a dst of exactly M points
            assert exact.cpu().numpy().tobytes() == expect.tobytes()
            with pytest.raises(RuntimeError, match="dst holds"):
                pm.gather(got, rect, dst[:m - 1])
    if name == "8x6":
        assert 0 in sizes and 1 in sizes and len(got) in sizes and 3041 in sizes
    with pytest.raises(RuntimeError, match="leaves"):
        pm.gather(got, (0, got.rows, 0, 0), torch.empty((cap, 4), dtype=torch.float32, device=cuda_device))


def test_reduced_map_device_crops_the_restatements_window_and_reuses_it(cuda_device):
    """reduced_map_device for poses and both window modes: the restatement's rectangle, its bytes and last_reduced.  A second call
    with the same rectangle launches nothing (reused, the same buffer and bytes); a pose one tile further gives new bytes."""
    want, got, _ = indices("8x6", cuda_device)
    camlist = cams()
    seen = set()
    for radius in (0.0, 5.0):
        sm = make_sm(cuda_device, radius=radius)
        sm.points_map_index = got
        for pose in POSES + [ref.pose_from(60.0, 60.0), ref.pose_from(11.0, 17.0, 0.0, 1.2)]:
            for cl in (camlist[:1], camlist):
                rect = ref.window(want, pose, cl, IMG[0], IMG[1], ref.RANGE_MAX, radius, 1.0)
                expect = ref.gather(want, rect)
                before = sm._reduced_rect
                cloud = sm.reduced_map_device(pose, cl, IMG)
                assert tuple(cloud.shape) == (len(expect), 4) and cloud.cpu().numpy().tobytes() == expect.tobytes()
                lr = sm.last_reduced
                assert lr["points"] == len(expect) and lr["rect"] == rect and lr["reused"] == (rect == before)
                assert lr["rows"] == ref.count(want, rect)[1] and lr["tiles"] == max(rect[1] - rect[0] + 1, 0) * max(rect[3] - rect[2] + 1, 0)
                seen.add((len(expect) == 0, lr["reused"]))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    sm = make_sm(cuda_device, radius=5.0)
    sm.points_map_index = got
    first = sm.reduced_map_device(POSES[0])                    # the vehicle's own cameras, their own image size: the square needs neither
    kept, ptr = first.cpu().numpy().copy(), first.data_ptr()
    assert sm.last_reduced["reused"] is False and len(kept) > 100
    again = sm.reduced_map_device(ref.pose_from(2.01, 14.0, 0.0, 0.1))
    assert sm.last_reduced["reused"] is True and again.data_ptr() == ptr and again.cpu().numpy().tobytes() == kept.tobytes()
    moved = sm.reduced_map_device(ref.pose_from(2.0 + ref.TILE, 14.0, 0.0, 0.1))
    assert sm.last_reduced["reused"] is False and moved.cpu().numpy().tobytes() != kept.tobytes()
    # the reuse is per stream: on another stream the gather runs again (the cloud is ordered on the stream asked for), then reuses there
    import torch
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    other = sm.reduced_map_device(ref.pose_from(2.0 + ref.TILE, 14.0, 0.0, 0.1), stream=side.cuda_stream)
    assert sm.last_reduced["reused"] is False
    side.synchronize()
    assert other.cpu().numpy().tobytes() == ref.gather(want, sm.last_reduced["rect"]).tobytes()
    sm.reduced_map_device(ref.pose_from(2.0 + ref.TILE, 14.0, 0.0, 0.1), stream=side.cuda_stream)
    assert sm.last_reduced["reused"] is True
    no_index = make_sm(cuda_device)
    with pytest.raises(RuntimeError, match="no points map is loaded"):
        no_index.reduced_map_device(POSES[0], camlist, IMG)
    with pytest.raises(ValueError, match="pose"):
        sm.reduced_map_device(None, camlist, IMG)


def _frame(sm, cloud, pose, variant, device):
    """one frame of `variant` on `cloud` (a world cloud); the sources are the same for every caller"""
    import torch
    camlist = cams()
    if variant == "logits":
        rng = np.random.default_rng(8)
        logits = torch.from_numpy(rng.normal(0.0, 2.0, (IMG[0] // 2, IMG[1] // 2, 19)).astype(np.float32)).to(device)
        sm.frame_device(cloud, "world", logits, pose, camlist[0], src_kind="logits", image_size=IMG)
    elif variant == "views":
        sm.frame_device_views(cloud, "world", class_maps(device, 2), pose, camlist, src_kind="classmap", image_size=IMG)
    else:
        sm.frame_device(cloud, "world", class_maps(device)[0], pose, camlist[0], src_kind="classmap", image_size=IMG)


@pytest.mark.parametrize("variant", ["identity_cm", "log_cm", "occlusion", "logits", "views"])
def test_a_frame_on_the_gathered_cloud_equals_the_frame_on_the_whole_map(variant, cuda_device):
    """Three poses accumulate into one 200 x 200 x 5 f64 grid twice: from reduced_map_device's cloud and from the whole sorted cloud.
    The grids are bit-equal although every gathered cloud is a proper part of the map."""
    want, got, _ = indices("8x6", cuda_device)
    kw = dict(occlusion=variant == "occlusion", log_cm=variant != "identity_cm")
    part, whole = make_sm(cuda_device, **kw), make_sm(cuda_device, source="topic", **kw)
    part.points_map_index = got
    camlist = cams()[:2 if variant == "views" else 1]
    rects = []
    for pose in POSES:
        cloud = part.reduced_map_device(pose, camlist, IMG)
        assert 0 < len(cloud) < len(got)
        rects.append(part.last_reduced["rect"])
        _frame(part, cloud, pose, variant, cuda_device)
        _frame(whole, got.points, pose, variant, cuda_device)
    assert len(set(rects)) >= 2                                # (two cameras' windows of the first two poses are one rectangle: a reused buffer)
    a, b = part.map, whole.map
    touched = int(np.any(b != 0, axis=2).sum())
    print("%s: %d cells touched, rectangles %s" % (variant, touched, rects))
    assert touched > 50                                        # the comparison is over real votes (a guard on the scene, not on the code)
    if variant == "occlusion":
        assert int(part.last_culled.sum()) > 0 and part.last_culled.cpu().tolist() == whole.last_culled.cpu().tolist()
    assert a.tobytes() == b.tobytes()


def test_a_radius_smaller_than_the_frustum_gives_the_crops_grid_not_the_whole_maps(cuda_device):
    """RADIUS_M = 5 cuts voters off: the grid equals a frame on the restatement's crop and differs from the whole map's -- the
    comparison above can tell the two apart."""
    import torch
    want, got, _ = indices("8x6", cuda_device)
    part, crop, whole = make_sm(cuda_device, radius=5.0, log_cm=True), make_sm(cuda_device, source="topic", log_cm=True), make_sm(cuda_device, source="topic", log_cm=True)
    part.points_map_index = got
    camlist = cams()[:1]
    for pose in POSES:
        _frame(part, part.reduced_map_device(pose, camlist, IMG), pose, "log_cm", cuda_device)
        rect = ref.window(want, pose, camlist, IMG[0], IMG[1], ref.RANGE_MAX, 5.0, 1.0)
        _frame(crop, torch.from_numpy(ref.gather(want, rect)).to(cuda_device), pose, "log_cm", cuda_device)
        _frame(whole, got.points, pose, "log_cm", cuda_device)
    assert part.map.tobytes() == crop.map.tobytes()
    assert part.map.tobytes() != whole.map.tobytes()


def test_mapping_with_the_index_equals_the_whole_map_and_never_reads_pcd(cuda_device, tmp_path):
    """mapping() and mapping_views() with SOURCE = "index", the map loaded from MAPPING.POINTS_MAP.PATH and no ROS: the grid of
    mapping() on the whole sorted cloud, and self.pcd is never read."""
    import torch
    from oracle import mapping_oracle as mo
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults, synthetic as syn
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    want, got, cloud = indices("8x6", cuda_device)

    class NoPcd(SemanticMapping):
        pcd = property(lambda self: (_ for _ in ()).throw(AssertionError("self.pcd was read")), lambda self, v: None)

    path = str(tmp_path / "site.npy")
    np.save(path, np.ascontiguousarray(cloud.T))
    cfg = get_cfg_defaults()
    ox, oy = mo.PCD_ORIGIN_OFFSET[:2]
    cfg.MAPPING.BOUNDARY = [[ox - 12.0, ox + 28.0], [oy - 4.0, oy + 36.0]]
    cfg.MAPPING.RESOLUTION = 0.2
    cfg.MAPPING.PCD.RANGE_MAX = ref.RANGE_MAX
    cfg.MAPPING.POINTS_MAP.SOURCE, cfg.MAPPING.POINTS_MAP.PATH, cfg.MAPPING.POINTS_MAP.TILE_M = "index", path, ref.TILE
    sm = NoPcd(cfg, device=cuda_device, logger=MyLogger("test", quiet=True))
    assert sm.points_map_index.points.cpu().numpy().tobytes() == want["points"].tobytes()
    whole = make_sm(cuda_device, source="topic")
    whole.pcd, whole.pcd_frame_id = got.points, "world"
    sm.confusion_matrix = whole.confusion_matrix = syn.log_confusion(5)
    camlist = cams()
    rng = np.random.default_rng(4)
    ids = np.array([2, 1, 8, 10, 3, 0], dtype=np.uint8)
    images = [syn.colorize(ids[syn.make_label_map(rng, IMG[0], IMG[1], num_classes=6, tile=7)]) for _ in range(2)]
    for pose in POSES:
        sm.mapping(images[0], pose, camlist[0])
        whole.mapping(images[0], pose, camlist[0])
        assert sm.last_reduced["points"] < len(got)
    sm.mapping_views(images, POSES[0], camlist)
    whole.mapping_views(images, POSES[0], camlist)
    assert sm.frames_mapped == whole.frames_mapped == 5
    assert int(np.any(whole.map != 0, axis=2).sum()) > 100
    assert sm.map.tobytes() == whole.map.tobytes()
    assert isinstance(sm.last_reduced["points"], int) and torch.is_tensor(sm._reduced_buf)
    # estimate_ground_plane in index mode: the plane of the crop of the vehicle's own cameras around the pose
    from vision_semantic_segmentation_amd.ground_plane import estimate_ground_plane_device
    got_plane = sm.estimate_ground_plane(POSES[0], hypotheses=64).host()
    rect = ref.window(want, POSES[0], [sm.cam1, sm.cam6], 1440, 1920, ref.RANGE_MAX, 0.0, 1.0)
    assert sm.last_reduced["rect"] == rect
    crop = torch.from_numpy(ref.gather(want, rect)).to(cuda_device)
    direct = estimate_ground_plane_device(crop, T=sm._origin_to_velodyne(POSES[0]), device=cuda_device, hypotheses=64).host()
    assert got_plane.used > 100 and got_plane.words.tobytes() == direct.words.tobytes()
