"""Occlusion culling without a GPU: that the shared scenes (tests/_occlusion_reference.py) can tell the rule of include/avl_hip.h from
its likely mis-implementations, the properties the rule has by construction -- both asserted on the NumPy reference alone -- and the
host side: configuration keys, the ctypes mirror of struct avl_occlusion, avl_occlusion_depth_words and the argument checks, which
run before any GPU call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _occlusion_reference as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCENES = ref.scenes()
BIG = [sc for sc in SCENES if sc[3] == 3000]
GRID = (64, 64, 0.5)                      # the first grid of tests/test_gpu_occlusion.py


def _proj(sc):
    _, w, h, _, pcd, P = sc
    return ref.Projection(pcd, P, w, h)


@pytest.fixture(scope="module")
def big():
    """(scene, projection, states at the defaults) of the 3000-point scenes, computed once"""
    out = []
    for sc in BIG:
        pr = _proj(sc)
        out.append((sc, pr, pr.states()))
    return out


# ---------------------------------------------------------------------------------------------------------------- the scenes test something
def test_scenes_have_the_sizes_the_suite_relies_on():
    assert [(sc[1], sc[2], sc[3]) for sc in SCENES] == [(w, h, n) for (w, h) in [(96, 64), (97, 61)] for n in [1, 63, 257, 3000]]
    for _, w, h, n, pcd, P in SCENES:
        assert pcd.shape == (4, n) and pcd.dtype == np.float64 and P.shape == (3, 4)
    assert 97 % 8 and 61 % 8 and 97 % 7 and 61 % 7          # partial last cells at s = 8 and s = 7


def test_large_scenes_cull_and_keep_at_least_five_percent(big):
    for sc, pr, st in big:
        cand = int(pr.cand.sum())
        assert cand >= 1500, sc[0]
        assert (st == 2).sum() >= 0.05 * cand and (st == 1).sum() >= 0.05 * cand, (sc[0], cand, int((st == 2).sum()))
        assert np.array_equal(st != 0, pr.cand)


def test_a_culled_and_a_kept_point_share_a_depth_cell(big):
    for sc, pr, st in big:
        cell = (pr.iy // 8) * 1000 + pr.ix // 8
        assert np.intersect1d(cell[st == 2], cell[st == 1]).size > 0, sc[0]


def test_some_point_is_culled_only_through_a_neighbour_cell(big):
    for sc, pr, st in big:
        r0 = pr.states(R=0)
        assert ((r0 == 1) & (st == 2)).any(), sc[0]
        assert not ((r0 == 2) & (st == 1)).any(), sc[0]      # a larger neighbourhood only lowers m


def test_neighbourhoods_are_clipped_on_all_four_borders(big):
    for sc, pr, st in big:
        Wc, Hc = -(-pr.img_w // 8), -(-pr.img_h // 8)
        cx, cy = pr.ix[pr.cand] // 8, pr.iy[pr.cand] // 8
        assert (cx == 0).any() and (cx == Wc - 1).any() and (cy == 0).any() and (cy == Hc - 1).any(), sc[0]


def test_an_off_grid_candidate_hides_an_on_grid_point(big):
    for sc, pr, st in big:
        on = ref.on_grid(sc[4], *GRID)
        assert (pr.cand & ~on).any() and (pr.cand & on).any()
        without = ref.visibility(pr.ix, pr.iy, pr.cand & on, pr.key32(), pr.img_w, pr.img_h, 8, 1, 0.05, 0.5)
        assert (on & (st == 2) & (without == 1)).any(), sc[0]


MUTANT_PARS = [dict(), dict(rel=0.0, abs_=0.0), dict(s=7, R=2, rel=0.2, abs_=0.0), dict(s=1, R=1, rel=0.0, abs_=0.25)]


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_each_reference_mutant_changes_the_culled_set(mutant, big):
    changed = []
    for sc, pr, _ in big:
        for par in MUTANT_PARS:
            good = pr.states(**par)
            bad = pr.states(mutant=mutant, src_size=(pr.img_w // 2, pr.img_h // 2), **par)
            if not np.array_equal(good == 2, bad == 2):
                changed.append((sc[0], par))
    assert changed, "no scene tells the rule from the mutant %s" % mutant


# ---------------------------------------------------------------------------------------------------------------- properties of the rule
PARS = [dict(), dict(s=7, R=2, rel=0.0, abs_=0.0), dict(s=1, R=0, rel=0.1, abs_=0.1)]


@pytest.mark.parametrize("sc", SCENES, ids=[sc[0] for sc in SCENES])
def test_permuting_the_cloud_permutes_the_states(sc):
    _, w, h, n, pcd, P = sc
    perm = np.random.default_rng(n).permutation(n)
    for par in PARS:
        assert np.array_equal(ref.Projection(pcd[:, perm], P, w, h).states(**par), _proj(sc).states(**par)[perm])


@pytest.mark.parametrize("sc", SCENES, ids=[sc[0] for sc in SCENES])
def test_a_huge_abs_tol_culls_nothing(sc):
    pr = _proj(sc)
    for par in PARS:
        assert np.array_equal(pr.states(**dict(par, abs_=1e30)), pr.cand.astype(np.uint8))


@pytest.mark.parametrize("sc", SCENES, ids=[sc[0] for sc in SCENES])
def test_zero_tolerances_keep_exactly_the_neighbourhood_minima(sc):
    pr = _proj(sc)
    key = pr.key32()
    for s, R in [(8, 1), (7, 2), (8, 0)]:
        st = pr.states(s=s, R=R, rel=0.0, abs_=0.0)
        depth, valid = ref.depth_buffer(np.where(pr.cand, pr.ix, 0), np.where(pr.cand, pr.iy, 0), pr.cand, key, pr.img_w, pr.img_h, s)
        assert np.array_equal(valid, pr.cand)               # every candidate of these scenes has a finite positive key
        Hc, Wc = depth.shape
        for i in np.nonzero(pr.cand)[0]:
            cx, cy = pr.ix[i] // s, pr.iy[i] // s
            m = min(int(depth[y, x]) for y in range(max(cy - R, 0), min(cy + R, Hc - 1) + 1) for x in range(max(cx - R, 0), min(cx + R, Wc - 1) + 1))
            assert (st[i] == 1) == (int(key[i:i + 1].view(np.uint32)[0]) == m)


def test_one_pixel_cells_without_radius_cull_only_points_that_share_a_pixel(big):
    for sc, pr, _ in big:
        st = pr.states(s=1, R=0, rel=0.0, abs_=0.0)
        key = pr.key32()
        pix = pr.iy.astype(np.int64) * pr.img_w + pr.ix
        assert (st == 2).any(), sc[0]
        for i in np.nonzero(st == 2)[0]:
            mates = pr.cand & (pix == pix[i])
            assert mates.sum() >= 2 and key[mates].min() < key[i]
        alone = pr.cand & (np.bincount(pix[pr.cand], minlength=pr.img_w * pr.img_h)[np.where(pr.cand, pix, 0)] == 1)
        assert not (st[alone] == 2).any()


# ---------------------------------------------------------------------------------------------------------------- the host side
def test_configuration_keys_and_defaults():
    from vision_semantic_segmentation_amd import get_cfg_defaults
    oc = get_cfg_defaults().MAPPING.OCCLUSION
    assert dict(oc) == dict(ENABLED=False, CELL_PX=8, RADIUS=1, REL_TOL=0.05, ABS_TOL=0.5)
    assert oc.ENABLED is False
    assert ref.DEFAULTS == dict(s=oc.CELL_PX, R=oc.RADIUS, rel=oc.REL_TOL, abs_=oc.ABS_TOL)


def test_ctypes_struct_is_the_c_struct(tmp_path):
    """size and the offset of every field, in order, from a host program compiled against include/avl_hip.h"""
    from vision_semantic_segmentation_amd._lib import AvlOcclusion
    names = [name for name, _ in AvlOcclusion._fields_]
    assert names == ["cell_px", "radius", "rel_tol", "abs_tol", "depth", "depth_words", "culled"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "avl_hip.h"\nint main(void) {\n    printf("%zu", sizeof(avl_occlusion));\n'
                   + "".join('    printf(" %%zu", offsetof(avl_occlusion, %s));\n' % n for n in names) + "    return 0;\n}\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(AvlOcclusion)] + [getattr(AvlOcclusion, n).offset for n in names]


def test_depth_words():
    from vision_semantic_segmentation_amd import _lib
    f = _lib.lib().avl_occlusion_depth_words
    for (w, h) in ref.SIZES + [(1920, 1440)]:
        for s in (1, 7, 8, 64):
            for V in (1, 2, 3, 4):
                assert f(w, h, s, V) == V * (-(-h // s)) * (-(-w // s))
    assert f(96, 64, 8, 1) == 96 and f(97, 61, 8, 3) == 3 * 8 * 13 and f(97, 61, 7, 2) == 2 * 9 * 14
    assert f(96, 64, 0, 1) == 0 and f(96, 64, 65, 1) == 0 and f(0, 64, 8, 1) == 0 and f(96, 64, 8, 0) == 0


FAKE = 0x7f0000700000                      # 16-byte aligned, never dereferenced: every call below returns before any GPU work


def _occl(**kw):
    from vision_semantic_segmentation_amd import _lib
    o = _lib.AvlOcclusion()
    o.cell_px, o.radius, o.rel_tol, o.abs_tol = 8, 1, 0.05, 0.5
    o.depth, o.depth_words, o.culled = FAKE, 96, None
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _grid():
    from vision_semantic_segmentation_amd import _lib
    g = _lib.AvlGrid()
    g.map, g.touched, g.counter, g.cell_mask = 0x7f0000200000, 0x7f0000300000, 0x7f0000400000, 0x7f0000100000
    g.map_dtype, g.Hm, g.Wm, g.C = _lib.AVL_F64, 64, 64, 5
    g.off_x, g.off_y, g.b00, g.b10, g.resolution = 1369.0496826171875, 562.84814453125, 1377.0, 546.0, 0.5
    g.touched_cap, g.counter_len = 1 << 20, 256
    return g


def _calls(o, n_views_for_visibility=1):
    """the three culling entry points on an EMPTY cloud (n = 0 returns after validation, before any HIP call) -> [(name, rc, message)]"""
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    g = _grid()
    P = (C.c_double * 48)()
    lut, colors, cm = (C.c_uint32 * 256)(), (C.c_uint8 * 48)(), (C.c_double * 256)()
    op = C.byref(o) if o is not None else None
    head = (C.byref(g), 0x7f0000500000, 0, _lib.AVL_F32, 16, 4)
    tail = (96, 64, 96, 64, lut, colors, cm, 1 << 2, op, None)
    out = []
    rc = L.avl_fused_frame_occl(*head, P, None, 100.0, _lib.AVL_SRC_CLASSMAP, 0x7f0000600000, *tail)
    out.append(("avl_fused_frame_occl", rc, _lib.last_error()))
    src = (C.c_void_p * 2)(0x7f0000600000, 0x7f0000610000)
    rc = L.avl_fused_frame_views_occl(*head, 2, P, None, 100.0, _lib.AVL_SRC_CLASSMAP, src, *tail)
    out.append(("avl_fused_frame_views_occl", rc, _lib.last_error()))
    rc = L.avl_occlusion_visibility(0x7f0000500000, 0, _lib.AVL_F32, 16, 4, n_views_for_visibility, P, None, 100.0, 96, 64, op, None, None, None)
    out.append(("avl_occlusion_visibility", rc, _lib.last_error()))
    return out


def test_valid_arguments_map_the_empty_cloud():
    for name, rc, msg in _calls(_occl(depth_words=192)):
        assert rc == 0, (name, msg)


BAD = [
    ("cell_px_0", dict(cell_px=0), "cell_px = 0"),
    ("cell_px_65", dict(cell_px=65), "cell_px = 65"),
    ("radius_neg", dict(radius=-1), "radius = -1"),
    ("radius_3", dict(radius=3), "radius = 3"),
    ("rel_tol_neg", dict(rel_tol=-0.01), "rel_tol"),
    ("rel_tol_nan", dict(rel_tol=float("nan")), "rel_tol"),
    ("abs_tol_neg", dict(abs_tol=-1.0), "abs_tol"),
    ("abs_tol_nan", dict(abs_tol=float("nan")), "abs_tol"),
    ("depth_null", dict(depth=None), "depth scratch is NULL"),
    ("depth_short", dict(depth_words=95), "95 words"),            # one view of 96 x 64 at s = 8 needs 96
    ("depth_misaligned", dict(depth=FAKE + 2), "aligned"),
]


@pytest.mark.parametrize("kw,msg", [b[1:] for b in BAD], ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_without_a_gpu(kw, msg):
    for name, rc, err in _calls(_occl(**dict(dict(depth_words=192), **kw))):
        assert rc == -1, (name, rc, err)
        assert msg in err, (name, err)


def test_null_struct_two_views_scratch_and_view_count():
    for name, rc, err in _calls(None):
        assert rc == -1 and "occl is NULL" in err, (name, err)
    # 96 words hold one view, not two
    res = {name: (rc, err) for name, rc, err in _calls(_occl(depth_words=96))}
    assert res["avl_fused_frame_occl"][0] == 0 and res["avl_occlusion_visibility"][0] == 0
    assert res["avl_fused_frame_views_occl"][0] == -1 and "192 needed" in res["avl_fused_frame_views_occl"][1]
    name, rc, err = _calls(_occl(depth_words=1 << 20), n_views_for_visibility=5)[2]
    assert rc == -1 and "exceeds the limit" in err
