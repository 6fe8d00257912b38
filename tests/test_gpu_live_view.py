"""The heading-up live view on the GPU (k_live_view, csrc/seg_livemap.hip): renderer.render_view against the NumPy restatement
tests/_live_view_reference.py, which samples the whole-grid live picture -- the project's own filter and renderers over the whole
grid, the restated fill_black -- through the matrix in float64.  EVERY byte of every picture is compared: no tolerance, no pixel
left out.  The cases are vr.gpu_cases(); tests/test_live_view_cpu.py shows what they contain and that they tell the definition
from wrong versions of it."""
import functools

import numpy as np
import pytest

import _live_map_reference as lr
import _live_view_reference as vr
from test_gpu_live_map import LIVE_BOUNDARY, _live_sm, _map_frame

pytestmark = pytest.mark.gpu

CASES = {case["name"]: case for case in vr.gpu_cases()}


@functools.lru_cache(maxsize=None)
def grid_dev(c, dtype):
    import torch
    return torch.from_numpy(np.array(vr.make_grid(c, dtype))).cuda()


@functools.lru_cache(maxsize=None)
def rendered_whole_grid(c, dtype, filt, thr):
    """the chain's first two stages over the WHOLE grid with the functions the repository already has, on the GPU"""
    from vision_semantic_segmentation_amd import renderer as rr
    t = grid_dev(c, dtype)
    f = rr.apply_filter(t).to(t.dtype) if filt else t
    r = (rr.render_bev_map_with_thresholds(f, vr.colors(c), vr.render_priority(c), vr.thresholds(c)) if thr
         else rr.render_bev_map(f, vr.colors(c)))
    out = r.cpu().numpy()
    out.setflags(write=False)
    return out


def view_args(case):
    c = case["c"]
    return dict(filter=case["filt"], thresholds=vr.thresholds(c) if case["thr"] else None,
                priority=vr.render_priority(c) if case["thr"] else None, fill=case["fill"], fill_priority=vr.fill_priority(c),
                car=case["car"])


def check(case):
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    c = case["c"]
    want = vr.compose_view(rendered_whole_grid(c, case["dtype"], case["filt"], case["thr"]), case["m"], vr.SIZE,
                           label_colors=np.array(vr.colors(c)), **vr.case_kwargs(case))
    got = rr.render_view(grid_dev(c, case["dtype"]), vr.colors(c), case["m"], vr.SIZE, **view_args(case))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == vr.SIZE + (3,)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "%s: %d pixels differ" % (case["name"], int((got != want).any(axis=2).sum()))
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_translation_equals_the_live_map(dtype, cuda_device):
    """M = [[1, 0, x0], [0, 1, y0]]: avl_live_map's window byte for byte, the fill, its ring and the car included"""
    from vision_semantic_segmentation_amd import renderer as rr
    case = CASES["identity %s" % np.dtype(dtype).name]
    got = check(case)
    kw = view_args(case)
    window = rr.render_window(grid_dev(5, dtype), vr.colors(5), case["geometry"]["origin"], vr.SIZE, **kw)
    assert np.array_equal(got, window.cpu().numpy())
    assert (got == [255, 0, 0]).all(axis=2).sum() > 50


@pytest.mark.parametrize("k", vr.SCALES)
@pytest.mark.parametrize("deg", list(vr.HEADINGS))
def test_headings_and_scales(deg, k, cuda_device):
    check(CASES["heading %g k %g" % (deg, k)])


@pytest.mark.parametrize("deg", [30.0, 45.0])
def test_every_setting_at_one_cell_per_pixel(deg, cuda_device):
    """filter on / off x arg-max / thresholds x fill on / off x car on / off"""
    for case in vr.cross_cases(deg):
        check(case)


@pytest.mark.parametrize("name", ["heading 30 k 1 float32", "heading 30 k 1 C 3"])
def test_float32_grid_and_three_classes(name, cuda_device):
    check(CASES[name])


def test_the_largest_admitted_matrix_and_the_first_refused(cuda_device):
    """|M00| + |M01| = |M10| + |M11| = 2.875 exactly at 45 degrees, with the fill (the widest footprint the kernel's LDS box holds);
    one step of each entry further and the host refuses"""
    from vision_semantic_segmentation_amd import renderer as rr
    case = CASES["largest admitted matrix"]
    m = case["m"]
    assert abs(m[0, 0]) + abs(m[0, 1]) == vr.MAX_SPAN and abs(m[1, 0]) + abs(m[1, 1]) == vr.MAX_SPAN and case["fill"]
    check(case)
    for row in (0, 1):
        over = m.copy()
        over[row, :2] = np.nextafter(m[row, :2], np.sign(m[row, :2]) * 4.0)
        assert abs(over[row, 0]) + abs(over[row, 1]) == np.nextafter(vr.MAX_SPAN, 4.0)
        with pytest.raises(RuntimeError, match=r"avl_live_view failed.*\|M%d0\| \+ \|M%d1\|.*limit is 2.875" % (row, row)):
            rr.render_view(grid_dev(5, np.float64), vr.colors(5), over, vr.SIZE, **view_args(case))


def test_singular_and_far_matrices_are_legal_and_the_grid_is_only_read(cuda_device):
    """a zero 2 x 2 part paints one cell everywhere; offsets far beyond any grid give black; NumPy in gives NumPy out"""
    import torch
    from vision_semantic_segmentation_amd import renderer as rr
    t = grid_dev(5, np.float64)
    before = t.clone()
    rendered = rendered_whole_grid(5, np.float64, True, False)
    for m in (np.array([[0.0, 0.0, 50.5], [0.0, 0.0, 30.2]]), np.array([[0.0, 0.0, 50.5], [0.0, 1.0, 30.2]]),
              np.array([[0.7, -0.7, 1e300], [0.7, 0.7, 10.0]]), np.array([[1.0, 0.0, -3e9], [0.0, 1.0, 4e18]]),
              np.array([[-2.0, 0.5, 130.0], [0.25, 2.5, -70.0]])):
        want = vr.compose_view(rendered, m, (40, 70), fill=True, label_colors=lr.REF_COLORS)
        got = rr.render_view(t, vr.colors(5), m, (40, 70), fill=True)
        assert np.array_equal(got.cpu().numpy(), want), m
    assert (want != 0).any(), "the sheared view shows nothing"
    assert torch.equal(before.view(torch.uint8), t.view(torch.uint8)), "render_view wrote to the grid"
    case = CASES["heading 30 k 1"]
    host = rr.render_view(np.array(vr.make_grid(5, np.float64)), vr.colors(5), case["m"], vr.SIZE, **view_args(case))
    assert isinstance(host, np.ndarray) and np.array_equal(host, check(case))
    out = torch.empty(vr.SIZE + (3,), dtype=torch.uint8, device=cuda_device)
    assert rr.render_view(t, vr.colors(5), case["m"], vr.SIZE, out=out, **view_args(case)) is out and np.array_equal(out.cpu().numpy(), host)


# ------------------------------------------------------------------------------------------------ SemanticMapping
VIEW = dict(SIZE_PX=[45, 52], METRES_PER_PIXEL=0.4, ANCHOR=[0.7, 0.5])           # 0.8 cells of 0.5 m per pixel


def _view_sm(device, **live):
    sm, g, pose, cam = _live_sm(device, **live)
    for k, v in VIEW.items():
        sm.live_view_cfg[k] = v
    return sm, g, pose, cam


def _expected_view(sm, pose7, fill=False, car=True):
    """the restatement's picture of the grid as it is now, for `pose7`"""
    from vision_semantic_segmentation_amd import renderer as rr
    _, (cx, cy) = lr.window_of(pose7, LIVE_BOUNDARY, 0.5, (1, 1))
    m = vr.view_matrix((cx, cy), lr.heading(pose7), 0.4 / 0.5, VIEW["SIZE_PX"], VIEW["ANCHOR"])
    smooth = rr.apply_filter(sm.map_dev).to(sm.map_dev.dtype)
    whole = rr.render_bev_map(smooth, sm.label_colors).cpu().numpy()
    block = lr.car_block(cx, cy, *lr.heading(pose7), resolution=0.5) if car else None
    return m, vr.compose_view(whole, m, tuple(VIEW["SIZE_PX"]), fill, np.array(sm.label_colors), lr.REF_PRIORITY, block)


def test_live_view_of_a_general_pose_equals_the_restatement(cuda_device):
    import torch
    from vision_semantic_segmentation_amd.utils import Pose
    sm, g, pose, cam = _view_sm(cuda_device)
    _map_frame(sm, g, pose, cam, 0)
    _map_frame(sm, g, pose, cam, 1)
    before = sm.map_dev.clone()
    pose7 = np.array(g["pose7"], dtype=np.float64)
    pose7[3:7] = (0.12, -0.07, 0.61, 0.78)                 # a general quaternion, not normalised
    m, want = _expected_view(sm, pose7)
    got = sm.live_view(Pose.from_array(pose7))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (45, 52, 3)
    assert sm.live_view_matrix_last.tobytes() == m.tobytes()
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want == [255, 0, 0]).all(axis=2).any(), "no car in the view"
    assert int(((want != 0).any(axis=2) & ~(want == [255, 0, 0]).all(axis=2)).sum()) > 50, "the view shows hardly any mapped cell"
    sm.live_cfg.FILL_BLACK, sm.live_cfg.DRAW_CAR = True, False
    assert np.array_equal(sm.live_view(Pose.from_array(pose7)).cpu().numpy(), _expected_view(sm, pose7, fill=True, car=False)[1])
    assert np.array_equal(sm.live_view().cpu().numpy(), _expected_view(sm, np.array(g["pose7"]), fill=True, car=False)[1])   # the last pose mapped
    assert torch.equal(before, sm.map_dev), "live_view changed the grid"


def test_heading_up_mapping_leaves_the_view_in_pinned_memory_and_the_grid_alone(cuda_device):
    import torch
    sm, g, pose, cam = _view_sm(cuda_device, ENABLED=True)
    sm.live_view_cfg.HEADING_UP = True
    plain, _, _, _ = _view_sm(cuda_device)                 # the same frames without the live step
    for k in range(2):
        _map_frame(sm, g, pose, cam, k)
        _map_frame(plain, g, pose, cam, k)
        m, want = _expected_view(sm, np.array(g["pose7"]))
        sm.live_map_ready.synchronize()
        assert sm.live_map_host.is_pinned() and np.array_equal(sm.live_map_host.numpy(), want)
        assert np.array_equal(sm.live_map_image.cpu().numpy(), want)
        assert sm.live_view_matrix_last.tobytes() == m.tobytes() and sm.live_map_origin is None
    assert torch.equal(sm.map_dev, plain.map_dev), "the live step changed the grid"
