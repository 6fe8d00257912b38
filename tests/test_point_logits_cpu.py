"""The logits rule (struct avl_point_logits in include/avl_hip.h) without a GPU: its NumPy restatement (tests/_point_logits_reference.py)
against torch's bilinear interpolation on the CPU and against hand-worked pixels, and the host side of the feature -- the argument
checks of the three entry points through the built library (an empty cloud returns before any GPU work), the ctypes struct, the
configuration key and the shape and dtype checks of the src_kind="logits" source."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _occlusion_reference as occ
import _point_logits_reference as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32 = np.float32
CASES = [(name, K, kind) for name in ref.SHAPES for K in ref.KS for kind in ("normal", "quantised")]


# ---------------------------------------------------------------------------------------------------------------- against torch
@pytest.mark.parametrize("name,K,kind", CASES, ids=["%s_K%d_%s" % c for c in CASES])
def test_reference_equals_torch_interpolate_argmax_but_for_near_ties(name, K, kind):
    import torch
    import torch.nn.functional as F
    (h, w), (net_h, net_w), _ = ref.SHAPES[name]
    logits = ref.make_logits(7 * K + h, h, w, K, kind)
    x = torch.from_numpy(np.ascontiguousarray(logits)).permute(2, 0, 1).unsqueeze(0)
    want = F.interpolate(x, size=(net_h, net_w), mode="bilinear", align_corners=True).argmax(1)[0].numpy()
    got = ref.full_labels(logits, net_h, net_w, 0.0)
    assert got.dtype == np.uint8 and got.shape == (net_h, net_w) and int(got.max()) < K
    margins = ref.full_margins(logits, net_h, net_w)
    ny, nx = np.divmod(np.arange(net_h * net_w), net_w)
    bound = ref.near_tie_bound(logits, net_h, net_w, ny, nx).reshape(net_h, net_w)
    differ = got != want
    print("%s K=%d %s: %d of %d pixels differ from torch, largest margin among them %g" % (
        name, K, kind, int(differ.sum()), differ.size, float(margins[differ].max()) if differ.any() else 0.0))
    assert (margins[differ].astype(np.float64) <= bound[differ]).all()
    assert differ.mean() <= 0.01                              # the inputs are fit to tell the two apart


# ---------------------------------------------------------------------------------------------------------------- hand-worked pixels
def two_by_two(K=3):
    z = np.zeros((2, 2, K), dtype=np.float32)
    z[0, 0], z[0, 1], z[1, 0], z[1, 1] = [1, 0, -1][:K], [0, 2, -1][:K], [3, 0, -1][:K], [0, 0, 4][:K]
    return z


def test_the_corners_and_the_last_row_and_column():
    z = two_by_two()
    lab = ref.full_labels(z, 3, 3, 0.0)
    # the four corners of the 3 x 3 output are the four source pixels; its centre is their mean (1, .5, .5); the edges' middles the
    # means of two: (.5, 1, -1), (2, 0, -1), (0, 1, 1.5) and, in the last row, (1.5, 0, 1.5) -- a tie, which the first index wins
    assert lab.tolist() == [[0, 1, 1], [0, 0, 2], [0, 0, 2]]
    m = ref.full_margins(z, 3, 3)
    assert m[0, 0] == 1 and m[0, 2] == 2 and m[2, 0] == 3 and m[2, 2] == 4 and m[1, 1] == 0.5
    assert m[0, 1] == 0.5 and m[1, 0] == 2 and m[2, 1] == 0 and m[1, 2] == 0.5
    # the last row and column: y1 == y0 and x1 == x0 there, with weights (1, 0): the value is the source pixel's, bit for bit
    zz = ref.interpolate(z, 3, 3, np.array([2, 2, 0]), np.array([2, 0, 2]))
    assert np.array_equal(zz, np.stack([z[1, 1], z[1, 0], z[0, 1]]))


def test_one_source_row():
    logits = ref.make_logits(3, 1, 7, 5)
    zz = ref.interpolate(logits, 5, 29, np.array([0, 2, 4, 4]), np.array([0, 14, 28, 7]))
    assert np.array_equal(zz[0], logits[0, 0]) and np.array_equal(zz[2], logits[0, 6])
    # every output row reads the one source row: sy = 0
    lab = ref.full_labels(logits, 5, 29, 0.0)
    assert (lab == lab[0]).all()
    sx = F32(6) / F32(28)
    fx = sx * F32(14)
    x0 = int(fx)
    lx = fx - F32(x0)
    hx = F32(1) - lx
    want = F32(1) * (hx * logits[0, x0] + lx * logits[0, x0 + 1]) + F32(0) * (hx * logits[0, x0] + lx * logits[0, x0 + 1])
    assert np.array_equal(zz[1], want)


def test_net_size_equal_to_the_logits_size_copies_them():
    logits = ref.make_logits(5, 9, 13, 19)
    ny, nx = np.divmod(np.arange(9 * 13), 13)
    assert np.array_equal(ref.interpolate(logits, 9, 13, ny, nx).reshape(9, 13, 19), logits)      # every weight is 0 or 1
    assert np.array_equal(ref.full_labels(logits, 9, 13, 0.0), logits.argmax(2).astype(np.uint8))


def test_a_constant_image_ties_everywhere():
    logits = np.full((9, 13, 5), 0.75, dtype=np.float32)
    assert not ref.full_labels(logits, 33, 50, 0.0).any()                      # all tie: the first index wins
    assert not ref.full_margins(logits, 33, 50).any()
    assert (ref.full_labels(logits, 33, 50, 1e-30) == 255).all()              # and any positive gate makes every pixel abstain


def test_a_nan_logit_is_maximal_and_votes():
    z = two_by_two()
    z[0, 0, 1] = np.nan
    lab, m = ref.full_labels(z, 3, 3, 1e30), ref.full_margins(z, 3, 3)
    # the NaN reaches every pixel that reads (0, 0) with a weight -- also with weight 0 (0 * NaN): everything but the last row and
    # column of corners... which here read (0, 0) with weight 0 as well, except where x0 = x1 = 1 and y0 = y1 = 1
    assert lab[0, 0] == 1 and np.isnan(m[0, 0])
    assert lab[1, 1] == 1 and np.isnan(m[1, 1])
    assert lab[2, 2] == 255 and m[2, 2] == 4                                   # (1, 1) alone: 4 < 1e30 abstains
    assert (lab[np.isnan(m)] == 1).all()                                       # a NaN margin votes whatever the gate
    # two NaNs: the first one wins
    z[0, 0, 0] = np.nan
    assert ref.full_labels(z, 3, 3, 0.0)[0, 0] == 0
    # K = 1: margin +inf, never abstains
    one = ref.make_logits(1, 2, 2, 1)
    assert np.isposinf(ref.full_margins(one, 3, 3)).all() and not ref.full_labels(one, 3, 3, 1e30).any()


def test_a_margin_equal_to_the_gate_votes_and_the_next_float_abstains():
    logits = ref.make_logits(9, 9, 13, 19)
    m = ref.full_margins(logits, 33, 50)
    lab0 = ref.full_labels(logits, 33, 50, 0.0)
    assert not (lab0 == 255).any()                                             # a gate of 0 gates nothing
    gate = np.sort(m.ravel())[m.size // 2]                                      # one pixel's own margin, about the median
    assert gate.dtype == np.float32 and gate > 0 and (m == gate).any()
    lab = ref.full_labels(logits, 33, 50, gate)
    assert np.array_equal(lab == 255, m < gate) and np.array_equal(lab[m >= gate], lab0[m >= gate])
    up = np.nextafter(gate, F32(np.inf))
    lab = ref.full_labels(logits, 33, 50, up)
    assert (lab[m == gate] == 255).all() and int((lab == 255).sum()) == int((m <= gate).sum())


def test_point_states_follow_the_projection():
    w, h = 100, 66
    pcd = occ.make_cloud(3, 3000)
    pr = occ.Projection(pcd, occ.pinhole_P(w, h), w, h)
    logits = ref.make_logits(11, 9, 13, 19)
    gate = 0.4
    state, margin = ref.point_states(pr, logits, 33, 50, gate)
    full, fm = ref.full_labels(logits, 33, 50, gate), ref.full_margins(logits, 33, 50)
    assert (state[~pr.cand] == 255).all() and not margin[~pr.cand].any() and pr.cand.sum() > 500
    c = np.nonzero(pr.cand)[0]
    ny, nx = pr.iy[c] * 33 // 66, pr.ix[c] * 50 // 100                        # the nearest rule at an integer factor of 2
    assert np.array_equal(np.where(state[c] == 254, 255, state[c]), full[ny, nx]) and np.array_equal(margin[c], fm[ny, nx])
    assert 0 < (state[c] == 254).sum() < len(c)


# ---------------------------------------------------------------------------------------------------------------- the host side
def test_configuration_key_and_its_validation():
    from vision_semantic_segmentation_amd import get_cfg_defaults
    from vision_semantic_segmentation_amd.mapping import confidence_min_margin
    cfg = get_cfg_defaults()
    assert dict(cfg.MAPPING.CONFIDENCE) == dict(MIN_MARGIN=0.0)
    assert confidence_min_margin(cfg) == 0.0
    for good in (0, 0.5, 3, np.float32(0.25), float("inf")):
        cfg.MAPPING.CONFIDENCE.MIN_MARGIN = good
        assert confidence_min_margin(cfg) == float(good)
    for bad in (-0.1, float("nan"), "0.5", None, True, [0.5]):
        cfg.MAPPING.CONFIDENCE.MIN_MARGIN = bad
        with pytest.raises(ValueError, match="MIN_MARGIN"):
            confidence_min_margin(cfg)


def test_ctypes_struct_is_the_c_struct(tmp_path):
    """size and the offset of every field, in order, from a host program compiled against include/avl_hip.h"""
    from vision_semantic_segmentation_amd._lib import AVL_MAX_VIEWS, AvlPointLogits
    names = [name for name, _ in AvlPointLogits._fields_]
    assert names == ["logits", "h", "w", "K", "ld", "net_h", "net_w", "min_margin", "abstained"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "avl_hip.h"\nint main(void) {\n'
                   '    printf("%zu %d", sizeof(avl_point_logits), AVL_MAX_VIEWS);\n'
                   + "".join('    printf(" %%zu", offsetof(avl_point_logits, %s));\n' % n for n in names) + "    return 0;\n}\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(AvlPointLogits), AVL_MAX_VIEWS] + [getattr(AvlPointLogits, n).offset for n in names]


FAKE = 0x7f0000700000                      # 16-byte aligned, never dereferenced: every call below returns before any GPU work


def _pl(n_views=4, **kw):
    from vision_semantic_segmentation_amd import _lib
    p = _lib.AvlPointLogits()
    for v in range(n_views):
        p.logits[v] = FAKE + 0x10000 * v
    p.h, p.w, p.K, p.ld, p.net_h, p.net_w, p.min_margin, p.abstained = 9, 13, 19, 19, 33, 50, 0.0, None
    for k, v in kw.items():
        if k.startswith("logits"):
            p.logits[int(k[6:])] = v
        else:
            setattr(p, k, v)
    return p


def _grid(**kw):
    from vision_semantic_segmentation_amd import _lib
    g = _lib.AvlGrid()
    g.map, g.touched, g.counter, g.cell_mask = 0x7f0000200000, 0x7f0000300000, 0x7f0000400000, 0x7f0000100000
    g.map_dtype, g.Hm, g.Wm, g.C = _lib.AVL_F64, 64, 64, 5
    g.off_x, g.off_y, g.b00, g.b10, g.resolution = 1369.0496826171875, 562.84814453125, 1377.0, 546.0, 0.5
    g.touched_cap, g.counter_len = 1 << 20, 256
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _calls(p, n_views=2, grid=None, occl=None, pts=0x7f0000500000, P=True, lut=True, cm=True, img=(100, 66), bonus=1 << 2, dtype=None):
    """the three entry points on an EMPTY cloud (n = 0 returns after validation, before any HIP call) -> {name: (rc, message)}"""
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    g = _grid() if grid is None else grid
    Pm = (C.c_double * 48)() if P else None
    lut_, cm_ = (C.c_uint32 * 256)() if lut else None, (C.c_double * 256)() if cm else None
    pp = C.byref(p) if p is not None else None
    oc = C.byref(occl) if occl is not None else None
    head = (C.byref(g), pts, 0, _lib.AVL_F32 if dtype is None else dtype, 16, 4)
    out = {}
    rc = L.avl_fused_frame_logits(*head, Pm, None, 100.0, pp, img[0], img[1], lut_, cm_, bonus, oc, None)
    out["avl_fused_frame_logits"] = (rc, _lib.last_error())
    rc = L.avl_fused_frame_views_logits(*head, n_views, Pm, None, 100.0, pp, img[0], img[1], lut_, cm_, bonus, oc, None)
    out["avl_fused_frame_views_logits"] = (rc, _lib.last_error())
    rc = L.avl_point_labels(*head[1:], n_views, Pm, None, 100.0, img[0], img[1], pp, None, None, None)
    out["avl_point_labels"] = (rc, _lib.last_error())
    return out


def test_valid_arguments_map_the_empty_cloud():
    from vision_semantic_segmentation_amd import _lib
    for V in (1, 2, 4):
        for name, (rc, msg) in _calls(_pl(), n_views=V).items():
            assert rc == 0, (name, V, msg)
    o = _lib.AvlOcclusion()
    o.cell_px, o.radius, o.rel_tol, o.abs_tol, o.depth, o.depth_words, o.culled = 8, 1, 0.05, 0.5, FAKE, 1 << 20, None
    for name, (rc, msg) in _calls(_pl(), occl=o).items():
        assert rc == 0, (name, msg)
    assert _calls(_pl(K=1, ld=1))["avl_point_labels"][0] == 0 and _calls(_pl(K=254, ld=254))["avl_point_labels"][0] == 0


BAD = [
    ("logits_null", dict(logits0=None), "logits are NULL"),
    ("logits_misaligned", dict(logits0=FAKE + 2), "not 4-byte aligned"),
    ("K_0", dict(K=0), "K = 0"),
    ("K_255", dict(K=255, ld=255), "K = 255"),
    ("ld_below_K", dict(ld=18), "ld = 18 < K = 19"),
    ("h_0", dict(h=0), "pixels"),
    ("w_neg", dict(w=-3), "pixels"),
    ("net_h_0", dict(net_h=0), "net size"),
    ("net_w_neg", dict(net_w=-1), "net size"),
    ("margin_neg", dict(min_margin=-0.5), "min_margin"),
    ("margin_nan", dict(min_margin=float("nan")), "min_margin"),
    ("abstained_misaligned", dict(abstained=FAKE + 1), "abstained"),
]


@pytest.mark.parametrize("kw,msg", [b[1:] for b in BAD], ids=[b[0] for b in BAD])
def test_bad_logits_arguments_are_refused_without_a_gpu(kw, msg):
    for name, (rc, err) in _calls(_pl(**kw)).items():
        assert rc == -1, (name, rc, err)
        assert msg in err, (name, err)


def test_null_struct_view_counts_and_a_view_out_of_use():
    from vision_semantic_segmentation_amd import _lib
    for name, (rc, err) in _calls(None).items():
        assert rc == -1 and "avl_point_logits is NULL" in err, (name, err)
    for V, msg in ((0, "at least one view"), (-1, "at least one view"), (5, "exceeds the limit")):
        res = _calls(_pl(), n_views=V)
        assert res["avl_fused_frame_logits"][0] == 0
        for name in ("avl_fused_frame_views_logits", "avl_point_labels"):
            assert res[name][0] == -1 and msg in res[name][1], (name, V, res[name])
    # only the views in use need logits: the single-view call reads logits[0] alone, two views read two
    res = _calls(_pl(logits1=None), n_views=2)
    assert res["avl_fused_frame_logits"][0] == 0
    assert res["avl_fused_frame_views_logits"][0] == -1 and "view 1" in res["avl_fused_frame_views_logits"][1]
    assert res["avl_point_labels"][0] == -1 and "view 1" in res["avl_point_labels"][1]
    assert all(rc == 0 for rc, _ in _calls(_pl(logits2=None, logits3=FAKE + 1), n_views=2).values())
    assert _lib.AVL_LABEL_ABSTAINED == ref.ABSTAINED and _lib.AVL_LABEL_NONE == ref.NONE


def test_what_the_plain_calls_refuse_is_refused():
    from vision_semantic_segmentation_amd import _lib
    frame = ("avl_fused_frame_logits", "avl_fused_frame_views_logits")
    every = frame + ("avl_point_labels",)
    for kw, names, msg in [(dict(pts=None), (), ""),                                            # an empty cloud needs no points
                           (dict(P=False), every, "P_host is NULL"),
                           (dict(img=(0, 66)), every, "image size"),
                           (dict(dtype=7), every, "point dtype"),
                           (dict(lut=False), frame, "lut_host is NULL"),
                           (dict(cm=False), frame, "cm_host is NULL"),
                           (dict(grid=_grid(C=0)), frame, "grid"),
                           (dict(grid=_grid(map=None)), frame, "NULL members"),
                           (dict(grid=_grid(resolution=0.0)), frame, "resolution"),
                           (dict(bonus=1 << 5), frame, "bonus_classes")]:
        for name, (rc, err) in _calls(_pl(), **kw).items():
            if name in names:
                assert rc == -1 and msg in err, (kw, name, err)
            else:
                assert rc == 0, (kw, name, err)
    # more vote bits than a view's byte holds: refused for two views, fine for one
    res = _calls(_pl(), grid=_grid(C=8), bonus=1)
    assert res["avl_fused_frame_logits"][0] == 0 and res["avl_point_labels"][0] == 0
    assert res["avl_fused_frame_views_logits"][0] == -1 and "vote bits" in res["avl_fused_frame_views_logits"][1]
    # a bad avl_occlusion is refused as avl_fused_frame_occl refuses it; avl_point_labels takes none
    o = _lib.AvlOcclusion()
    o.cell_px, o.radius, o.rel_tol, o.abs_tol, o.depth, o.depth_words, o.culled = 0, 1, 0.05, 0.5, FAKE, 1 << 20, None
    res = _calls(_pl(), occl=o)
    for name in frame:
        assert res[name][0] == -1 and "cell_px = 0" in res[name][1]
    assert res["avl_point_labels"][0] == 0


def test_logits_source_shape_and_dtype_errors():
    import torch
    from vision_semantic_segmentation_amd.mapping import logits_views
    ok = torch.zeros((9, 13, 19), dtype=torch.float32)
    with pytest.raises(ValueError, match="CUDA"):                      # everything else about it is right
        logits_views(ok)
    with pytest.raises(ValueError, match="float32"):
        logits_views(ok.double())
    with pytest.raises(ValueError, match="float32"):
        logits_views(ok.to(torch.uint8))
    with pytest.raises(ValueError, match=r"\[h', w', K\]"):
        logits_views(ok[0])
    with pytest.raises(ValueError, match=r"\[h', w', K\]"):
        logits_views(ok.unsqueeze(0))                                  # a batch for one camera
    with pytest.raises(ValueError, match=r"\[h', w', K\]"):
        logits_views(np.zeros((9, 13, 19), dtype=np.float32))
    with pytest.raises(ValueError, match="1..254"):
        logits_views(torch.zeros((2, 2, 255), dtype=torch.float32))
    with pytest.raises(ValueError, match="strides"):
        logits_views(ok.permute(1, 0, 2))                              # rows of pixels that do not follow each other
    with pytest.raises(ValueError, match="strides"):
        logits_views(torch.zeros((19, 9, 13), dtype=torch.float32).permute(1, 2, 0))      # NCHW planes seen as NHWC
    with pytest.raises(ValueError, match="3 logits views"):
        logits_views(torch.zeros((2, 9, 13, 19), dtype=torch.float32), 3)
    with pytest.raises(ValueError, match="3 logits views"):
        logits_views(ok, 3)
    with pytest.raises(ValueError, match="2 semantic sources for 3 cameras"):
        logits_views([ok, ok], 3)
    with pytest.raises(ValueError, match="one shape"):
        logits_views([ok, torch.zeros((9, 13, 5), dtype=torch.float32)], 2)
    with pytest.raises(ValueError, match="one shape"):
        logits_views([ok, torch.zeros((9, 13, 22), dtype=torch.float32)[:, :, :19]], 2)    # one shape, two row strides
    with pytest.raises(ValueError, match="CUDA"):
        logits_views(torch.zeros((2, 9, 13, 19), dtype=torch.float32), 2)
    with pytest.raises(ValueError, match="CUDA"):                      # the first K columns of wider rows are a valid source
        logits_views(torch.zeros((9, 13, 22), dtype=torch.float32)[:, :, :19])
