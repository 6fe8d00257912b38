"""Points labelled from interpolated logits on the GPU (csrc/mapping.hip: the logits instantiations of k_fused_vote and k_views_vote,
k_point_labels) against the NumPy float32 restatement of the rule (tests/_point_logits_reference.py).

States are compared point by point and margins bit for bit.  Grids are compared bit for bit with what the PLAIN class-map call does
on the same cloud when it is fed the reference's full label map (255 where the pixel abstains), on the grids, clouds and path table
of tests/test_gpu_occlusion.py (all four single-view paths and both views paths; the path is asserted).  The logits are tiny (9 x 13
and 1 x 7 pixels) and the clouds hold at most 3000 points."""
import numpy as np
import pytest

import _occlusion_reference as occ
import _point_logits_reference as ref
from test_gpu_occlusion import FRAME_CASES, VIEWS_CASES, WORLD_POSE, Cam, cams, cloud_as, frame_path, make_sm, same_grid

pytestmark = pytest.mark.gpu

H_, W_, K_ = 9, 13, 19                       # the logits of the grid tests ...
NET = (33, 50)                               # ... interpolated to the network's input ...
IMG = (66, 100)                              # ... which stands for a camera image of twice the size
FAVOUR = 1.5                                 # added to the logits of the classes the map holds, so that most points vote


def dev_logits(arr, device):
    """a float32 [.., K] host view (possibly of wider rows) on the device with the same strides"""
    import torch
    base = arr.base if arr.base is not None and arr.base.ndim == arr.ndim else arr
    t = torch.from_numpy(np.ascontiguousarray(base)).to(device)
    return t[..., :arr.shape[-1]]


def pinhole(img_hw):
    h, w = img_hw
    return occ.pinhole_P(w, h, f=0.6 * w)


_CLOUDS = {}


def cloud_variants(sm):
    """[(id, what goes to the GPU, the float64 cloud the oracle sees, frame id, pose, pose7)]: SoA f64 and AoS f32, in the velodyne
    frame and in the world frame with a pose"""
    from vision_semantic_segmentation_amd.utils import Pose
    if "v" not in _CLOUDS:
        vel = occ.make_cloud(301, 3000)
        world = vel.copy()
        world[0:3] = (np.linalg.inv(sm._origin_to_velodyne(Pose.from_array(WORLD_POSE))) @ np.vstack([vel[0:3], np.ones((1, vel.shape[1]))]))[0:3]
        _CLOUDS["v"] = []
        for fmt in ("soa64", "aos32"):
            for name, pcd, frame, pose7 in (("vel", vel, "velodyne", None), ("world", world, "world", WORLD_POSE)):
                gpu, host = cloud_as(pcd, fmt)
                _CLOUDS["v"].append(("%s_%s" % (fmt, name), gpu, host, frame, pose7))
    return [(i, g, h, f, None if p7 is None else Pose.from_array(p7), p7) for i, g, h, f, p7 in _CLOUDS["v"]]


_PROJ = {}


def projection(cid, host, P, img_hw, frame, pose7):
    key = (cid, img_hw, P.tobytes())
    if key not in _PROJ:
        _PROJ[key] = occ.Projection(host, P, img_hw[1], img_hw[0], frame_id=frame, pose7=pose7)
    return _PROJ[key]


# ---------------------------------------------------------------------------------------------------------------- 1. states and margins
STATE_CASES = [(name, K, extra, kind) for name in ref.SHAPES for K in ref.KS for extra in (0, 3) for kind in ("normal", "quantised")]


@pytest.mark.parametrize("name,K,extra,kind", STATE_CASES, ids=["%s_K%d_ld+%d_%s" % c for c in STATE_CASES])
def test_point_labels_equal_the_rule(name, K, extra, kind, cuda_device):
    (h, w), net, images = ref.SHAPES[name]
    logits = ref.make_logits(13 * K + h + extra, h, w, K, kind, ld=K + extra)
    t = dev_logits(logits, cuda_device)
    assert tuple(t.shape) == (h, w, K) and t.stride(1) == K + extra
    sm = make_sm("g64", cuda_device)
    abstained_any, ties = 0, 0
    for img in images:
        cam = Cam(pinhole(img))
        for cid, gpu, host, frame, pose, pose7 in cloud_variants(sm):
            pr = projection(cid, host, cam.P, img, frame, pose7)
            assert pr.cand.sum() > 40, (name, img, cid)
            for gate in (0.0, 0.3):
                sm.min_margin = gate
                state, margin = sm.point_labels_device(gpu, frame, pose, cam, t, img, net_size=net)
                assert tuple(state.shape) == (1, 3000) and tuple(margin.shape) == (1, 3000)
                want_s, want_m = ref.point_states(pr, logits, net[0], net[1], gate)
                assert np.array_equal(state[0].cpu().numpy(), want_s), (img, cid, gate, int((state[0].cpu().numpy() != want_s).sum()))
                got_m = margin[0].cpu().numpy()
                assert np.array_equal(got_m.view(np.uint32), want_m.view(np.uint32)) or np.array_equal(got_m, want_m, equal_nan=True)
                assert sm.last_abstained.cpu().tolist() == [int((want_s == 254).sum())]
                abstained_any += int((want_s == 254).sum())
                ties += int((want_m[pr.cand] == 0).sum())
    assert abstained_any > 0
    if kind == "quantised" and net == (h, w):
        assert ties > 0                                      # exact ties occur where the weights are 0 and 1


def test_point_labels_of_several_views_and_more_than_one_call_takes(cuda_device):
    import torch
    V = 5
    camlist = cams(IMG[1], IMG[0], V)
    logits = [ref.make_logits(40 + v, H_, W_, K_) for v in range(V)]
    t = torch.stack([dev_logits(z, cuda_device) for z in logits])
    pcd = occ.make_cloud(17, 3000)
    sm = make_sm("g64", cuda_device)
    sm.min_margin = 0.25
    state, margin = sm.point_labels_device(pcd, "velodyne", None, camlist, t, IMG, net_size=NET)
    for v in range(V):
        pr = occ.Projection(pcd, camlist[v].P, IMG[1], IMG[0])
        want_s, want_m = ref.point_states(pr, logits[v], NET[0], NET[1], 0.25)
        assert np.array_equal(state[v].cpu().numpy(), want_s) and np.array_equal(margin[v].cpu().numpy(), want_m, equal_nan=True)
        assert int(sm.last_abstained[v]) == int((want_s == 254).sum()) > 0


def test_nan_and_infinite_logits(cuda_device):
    logits = np.ascontiguousarray(ref.make_logits(3, H_, W_, K_))
    logits[2, 3, 5] = np.nan
    logits[2, 4, 7] = np.nan
    logits[5, 5, 2] = np.inf
    logits[5, 6, 2] = np.inf
    logits[6, 9, :] = -np.inf
    t = dev_logits(logits, cuda_device)
    sm = make_sm("g64", cuda_device)
    cam = Cam(pinhole(IMG))
    pcd = occ.make_cloud(19, 3000)
    pr = occ.Projection(pcd, cam.P, IMG[1], IMG[0])
    for gate in (0.0, 0.5, float("inf")):
        sm.min_margin = gate
        state, margin = sm.point_labels_device(pcd, "velodyne", None, cam, t, IMG, net_size=NET)
        want_s, want_m = ref.point_states(pr, logits, NET[0], NET[1], gate)
        assert np.array_equal(state[0].cpu().numpy(), want_s) and np.array_equal(margin[0].cpu().numpy(), want_m, equal_nan=True)
    assert np.isnan(want_m[pr.cand]).sum() > 5 and (want_s[pr.cand][np.isnan(want_m[pr.cand])] < 254).all()       # a NaN margin votes


# ---------------------------------------------------------------------------------------------------------------- 2. grids
def label_map(logits, gate, device):
    import torch
    return torch.from_numpy(ref.full_labels(logits, NET[0], NET[1], gate)).to(device)


def gates_for(logits_list, projs):
    """0, about the median reference margin of the first view's candidates, and one candidate's exact margin"""
    _, m = ref.point_states(projs[0], logits_list[0], NET[0], NET[1], 0.0)
    mc = np.sort(m[projs[0].cand])
    if len(mc) == 0:
        return [0.0, 0.3, 0.1]
    positive = mc[mc > 0]
    return [0.0, float(np.median(mc)), float(positive[len(positive) // 3]) if len(positive) else 0.1]


def expect_abstained(projs, logits_list, host, grid, gate):
    from test_gpu_occlusion import GRIDS
    on = occ.on_grid(host, *GRIDS[grid])
    return [int(((ref.point_states(pr, z, NET[0], NET[1], gate)[0] == 254) & on).sum()) for pr, z in zip(projs, logits_list)]


@pytest.mark.parametrize("intensity", [True, False], ids=["int", "noint"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", FRAME_CASES, ids=["%s_n%d_p%d" % c for c in FRAME_CASES])
def test_frame_from_logits_equals_the_classmap_frame_on_the_reference_labels(case, dtype, intensity, cuda_device):
    grid, n, path = case
    fmt = "soa64" if dtype == "f64" else "aos32"
    cam = Cam(pinhole(IMG))
    logits = ref.make_logits(n + 5, H_, W_, K_, favour=FAVOUR)
    t = dev_logits(logits, cuda_device)
    lg, cm = make_sm(grid, cuda_device, dtype, intensity), make_sm(grid, cuda_device, dtype, intensity)
    assert frame_path(lg, n) == path and frame_path(cm, n) == path
    clouds = [cloud_as(occ.make_cloud(500 + n + i, n), fmt) for i in range(3)]
    projs = [occ.Projection(host, cam.P, IMG[1], IMG[0]) for _, host in clouds]
    withheld = 0
    for gate in gates_for([logits], projs[:1]):
        lg.min_margin = gate
        labels = label_map(logits, gate, cuda_device)
        for (gpu, host), pr in zip(clouds, projs):
            lg.frame_device(gpu, "velodyne", t, None, cam, src_kind="logits", image_size=IMG, net_size=NET)
            cm.frame_device(gpu, "velodyne", labels, None, cam, src_kind="classmap", image_size=IMG)
            same_grid(lg, cm, "gate %g" % gate)
            want = expect_abstained([pr], [logits], host, grid, gate)
            assert lg.last_abstained.cpu().tolist() == want, gate
            withheld += want[0]
    assert lg.frames_mapped == 9
    if n == 3000:
        assert withheld > 100 and int(lg.map_dev.count_nonzero()) > 20


@pytest.mark.parametrize("intensity", [True, False], ids=["int", "noint"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", VIEWS_CASES, ids=["%s_n%d_p%d" % c for c in VIEWS_CASES])
def test_views_from_logits_equal_the_classmap_views_on_the_reference_labels(case, dtype, intensity, cuda_device):
    import torch
    grid, n, path = case
    V = 3
    fmt = "soa64" if dtype == "f64" else "aos32"
    camlist = cams(IMG[1], IMG[0], V)
    logits = [ref.make_logits(n + 50 + v, H_, W_, K_, favour=FAVOUR) for v in range(V)]
    t = torch.stack([dev_logits(z, cuda_device) for z in logits])
    lg, cm = make_sm(grid, cuda_device, dtype, intensity), make_sm(grid, cuda_device, dtype, intensity)
    assert frame_path(lg, n, V) == path
    clouds = [cloud_as(occ.make_cloud(600 + n + i, n), fmt) for i in range(3)]
    projs = [[occ.Projection(host, c.P, IMG[1], IMG[0]) for c in camlist] for _, host in clouds]
    withheld = 0
    for gate in gates_for(logits, projs[0]):
        lg.min_margin = gate
        labels = torch.stack([label_map(z, gate, cuda_device) for z in logits])
        for (gpu, host), prs in zip(clouds, projs):
            lg.frame_device_views(gpu, "velodyne", t, None, camlist, src_kind="logits", image_size=IMG, net_size=NET)
            cm.frame_device_views(gpu, "velodyne", labels, None, camlist, src_kind="classmap", image_size=IMG)
            same_grid(lg, cm, "gate %g" % gate)
            want = expect_abstained(prs, logits, host, grid, gate)
            assert lg.last_abstained.cpu().tolist() == want, gate
            withheld += sum(want)
    if n == 3000:
        assert withheld > 100 and int(lg.map_dev.count_nonzero()) > 20


# ---------------------------------------------------------------------------------------------------------------- 3. views
@pytest.mark.parametrize("V", [2, 3, 4, 5])
@pytest.mark.parametrize("case", [("g64", 257), ("g64", 3000)], ids=lambda c: "%s_n%d" % c)
def test_views_equal_single_calls_in_view_order(case, V, cuda_device):
    """V = 2..4: one fused call; V = 5: more views than one call takes, mapped by sequential single-view calls"""
    import torch
    grid, n = case
    camlist = cams(IMG[1], IMG[0], V)
    logits = [ref.make_logits(70 + v, H_, W_, K_, favour=FAVOUR) for v in range(V)]
    t = torch.stack([dev_logits(z, cuda_device) for z in logits])
    pcd = occ.make_cloud(700 + n, n)
    fused, seq = make_sm(grid, cuda_device), make_sm(grid, cuda_device)
    fused.min_margin = seq.min_margin = 0.3
    fused.frame_device_views(pcd, "velodyne", t, None, camlist, src_kind="logits", image_size=IMG, net_size=NET)
    counts = []
    for v in range(V):
        seq.frame_device(pcd, "velodyne", t[v], None, camlist[v], src_kind="logits", image_size=IMG, net_size=NET)
        counts += seq.last_abstained.cpu().tolist()
    same_grid(fused, seq, "%d views" % V)
    assert fused.last_abstained.cpu().tolist() == counts and fused.frames_mapped == V
    if n == 3000:
        assert sum(counts) > 50 and int(fused.map_dev.count_nonzero()) > 20
    # a list of views is the tensor
    again = make_sm(grid, cuda_device)
    again.min_margin = 0.3
    again.frame_device_views(pcd, "velodyne", [t[v] for v in range(V)], None, camlist, src_kind="logits", image_size=IMG, net_size=NET)
    same_grid(again, fused, "list of views")


# ---------------------------------------------------------------------------------------------------------------- 4. occlusion
@pytest.mark.parametrize("case", [("g64", 3000, 1), ("g64", 257, 1), ("g50x30", 3000, 1), ("g50x30", 11, 1), ("g64", 257, 3), ("g64", 3000, 3),
                                  ("g50x30", 3000, 3), ("g64", 3000, 5)], ids=lambda c: "%s_n%d_V%d" % c)
def test_occlusion_composes_with_the_logits_source(case, cuda_device):
    import torch
    grid, n, V = case
    par = dict(CELL_PX=4, RADIUS=1, REL_TOL=0.1, ABS_TOL=1.0)
    camlist = cams(IMG[1], IMG[0], V)
    logits = [ref.make_logits(80 + v, H_, W_, K_, favour=FAVOUR) for v in range(V)]
    t = torch.stack([dev_logits(z, cuda_device) for z in logits])
    gate = 0.3
    labels = torch.stack([label_map(z, gate, cuda_device) for z in logits])
    pcd = occ.make_cloud(800 + n, n)
    lg, cm, plain = make_sm(grid, cuda_device, occl=par), make_sm(grid, cuda_device, occl=par), make_sm(grid, cuda_device)
    lg.min_margin = plain.min_margin = gate
    if V == 1:
        lg.frame_device(pcd, "velodyne", t[0], None, camlist[0], src_kind="logits", image_size=IMG, net_size=NET)
        cm.frame_device(pcd, "velodyne", labels[0], None, camlist[0], src_kind="classmap", image_size=IMG)
        plain.frame_device(pcd, "velodyne", t[0], None, camlist[0], src_kind="logits", image_size=IMG, net_size=NET)
    else:
        lg.frame_device_views(pcd, "velodyne", t, None, camlist, src_kind="logits", image_size=IMG, net_size=NET)
        cm.frame_device_views(pcd, "velodyne", labels, None, camlist, src_kind="classmap", image_size=IMG)
        plain.frame_device_views(pcd, "velodyne", t, None, camlist, src_kind="logits", image_size=IMG, net_size=NET)
    same_grid(lg, cm, "occlusion on")
    assert lg.last_culled.cpu().tolist() == cm.last_culled.cpu().tolist() and len(lg.last_culled) == V
    # a culled candidate is not evaluated: it is no abstention
    state = cm.visibility_device(pcd, "velodyne", None, camlist, IMG).cpu().numpy()
    from test_gpu_occlusion import GRIDS
    on = occ.on_grid(pcd, *GRIDS[grid])
    want = []
    for v in range(V):
        s, _ = ref.point_states(occ.Projection(pcd, camlist[v].P, IMG[1], IMG[0]), logits[v], NET[0], NET[1], gate)
        want.append(int(((s == 254) & on & (state[v] == 1)).sum()))
    assert lg.last_abstained.cpu().tolist() == want
    if n == 3000:
        assert sum(lg.last_culled.cpu().tolist()) > 50
        assert not torch.equal(lg.map_dev, plain.map_dev), "culling changed nothing: the case tests nothing"


# ---------------------------------------------------------------------------------------------------------------- 5. the full-resolution kernel
@pytest.mark.parametrize("name,K", [(name, K) for name in ref.SHAPES for K in ref.KS], ids=lambda v: str(v))
def test_states_equal_the_full_resolution_kernels_labels_but_for_near_ties(name, K, cuda_device):
    """seg_head.hip's k_full_res_eval evaluates the same interpolation at every pixel (it may contract multiply-adds): its labels,
    sampled at the points' pixels, are the states wherever the reference's margin exceeds 16 * 2^-24 * max|corner logit|"""
    import torch
    from vision_semantic_segmentation_amd import seg_head
    (h, w), net, images = ref.SHAPES[name]
    logits = np.ascontiguousarray(ref.make_logits(900 + K + h, h, w, K))
    t = dev_logits(logits, cuda_device)
    full = torch.empty(net, dtype=torch.uint8, device=cuda_device)
    seg_head.full_res_eval(t, net[0], net[1], labels_out=full)
    full = full.cpu().numpy()
    sm = make_sm("g64", cuda_device)
    pcd = occ.make_cloud(23, 3000)
    differ = total = 0
    for img in images:
        cam = Cam(pinhole(img))
        pr = occ.Projection(pcd, cam.P, img[1], img[0])
        state, margin = sm.point_labels_device(pcd, "velodyne", None, cam, t, img, net_size=net)
        state, margin = state[0].cpu().numpy(), margin[0].cpu().numpy()
        ny, nx = ref.point_pixels(pr, net[0], net[1])
        c = pr.cand
        bad = c & (state != full[ny, nx])
        bound = ref.near_tie_bound(logits, net[0], net[1], ny, nx)
        assert (margin[bad].astype(np.float64) <= bound[bad]).all(), (margin[bad], bound[bad])
        differ, total = differ + int(bad.sum()), total + int(c.sum())
    print("%s K=%d: %d of %d candidates differ from the full-resolution kernel's labels" % (name, K, differ, total))
    assert total > 100 and differ <= 0.01 * total


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def test_a_networks_logits_feed_the_mapper(cuda_device):
    import torch
    from vision_semantic_segmentation_amd.network import SegNet, random_state_dict
    h, w = 64, 96
    net = SegNet(random_state_dict(0), h, w, precision="f32", device=cuda_device)
    img = np.random.default_rng(5).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    net.forward(torch.from_numpy(img).to(cuda_device))
    t = net.logits
    assert t.dtype == torch.float32 and t.dim() == 3 and int(t.shape[2]) == 19
    logits = t.cpu().numpy()
    cam = Cam(pinhole((h, w)))
    pcd = occ.make_cloud(29, 3000)
    pr = occ.Projection(pcd, cam.P, w, h)
    _, m = ref.point_states(pr, logits, h, w, 0.0)
    gate = float(np.median(m[pr.cand]))
    lg, cm = make_sm("g64", cuda_device), make_sm("g64", cuda_device)
    lg.min_margin = gate
    lg.frame_device(pcd, "velodyne", t, None, cam, src_kind="logits", image_size=(h, w))           # net_size defaults to image_size
    labels = torch.from_numpy(ref.full_labels(logits, h, w, gate)).to(cuda_device)
    cm.frame_device(pcd, "velodyne", labels, None, cam, src_kind="classmap", image_size=(h, w))
    same_grid(lg, cm, "a network's logits")
    state, margin = lg.point_labels_device(pcd, "velodyne", None, cam, t, (h, w))
    want_s, want_m = ref.point_states(pr, logits, h, w, gate)
    assert np.array_equal(state[0].cpu().numpy(), want_s) and np.array_equal(margin[0].cpu().numpy(), want_m, equal_nan=True)
    assert 0 < (want_s == 254).sum() < pr.cand.sum()


def test_raw_frame_logits_are_the_plans_logits(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import SemanticSegmentation
    from vision_semantic_segmentation_amd.config import get_network_cfg_defaults
    cfg = get_network_cfg_defaults()
    cfg.MODEL.PRECISION = "f32"
    seg = SemanticSegmentation(cfg, device=cuda_device)
    frames = np.random.default_rng(7).integers(0, 256, size=(2, 64, 96, 3), dtype=np.uint8)
    labels = seg.segmentation_device_raw(frames[0]).clone()
    lg = seg.logits_device_raw(frames[0])
    assert lg.dtype == torch.float32 and tuple(lg.shape) == tuple(labels.shape) + (19,)
    assert torch.equal(lg.argmax(2).to(torch.uint8), labels)
    assert lg.data_ptr() == seg.net_for(64, 96, raw_frame=(64, 96)).logits.data_ptr()               # the plan's buffer: no extra pass
    batch = seg.logits_device_raw_batch(frames)
    assert tuple(batch.shape) == (2,) + tuple(lg.shape)
    assert torch.equal(batch[0], seg.logits_device_raw(frames[0])) and torch.equal(batch.argmax(3).to(torch.uint8), seg.segmentation_device_raw_batch(frames))
    assert tuple(seg.logits_device_raw_batch(frames[:1]).shape) == (1,) + tuple(lg.shape)
