"""The cases of test_gpu_pool_resample_exact.py, checked without a GPU (tests/_pool_resample_operands.py): every case builds with its
operand conditions asserted while it does (max-pool: >= 10 % negative outputs, no +0.0, the split premise hi + lo exact and canonical,
>= 5 % of the windows decided by lo; bilinear: float32 evaluation == float64, F.interpolate in float64 gives the same, >= 20 % rounded
outputs and ties in both directions where the weights are fractions; one-side split depthwise: the bound, ties, dropping lo changes >= 30 %
of the f16 outputs; split stem: the kernel's own split returns (xh, xl), float32 == float64, >= 20 % of the lo values round); the
library accepts every case's op; what the device reads holds the poison where the op must not read; the coordinate rule stays under the
derived bar of the tolerance test while the contracted coordinate exceeds it in more than a tenth of the elements; and the comparison has
teeth: each deliberate mistake changes at least one byte of the expected buffers of every case it applies to.  The mistake table is
printed (run with -s to see it)."""
import pytest
import torch

import _pool_resample_operands as M
from test_fused_mixed_operands_cpu import _create

_ALL = [(fam, c) for fam, t in M.FAMILIES.items() for c in t[0]]


def _fid(p):
    fam, c = p
    return "%s-%s" % (fam, M.FAMILIES[fam][1](c))


def test_the_cases_are_the_shapes_at_which_these_kernels_can_go_wrong():
    assert M.MP_SHAPES == [(1, 1, 8, 1, 0), (2, 2, 8, 1, 0), (7, 9, 24, 1, 0), (8, 10, 64, 3, 0), (35, 67, 64, 2, 8)]
    assert {c.prec for c in M.MP_CASES} == {"f32", "bf16", "f16"} and len(M.MP_CASES) == 15
    assert {(c.H, c.W) for c in M.MP_SPLIT_CASES} == {(1, 1), (2, 2), (7, 9), (8, 10), (35, 67)} and len(M.MP_SPLIT_CASES) == 20
    assert {c.C for c in M.MP_SPLIT_CASES} == {8, 64} and {c.B for c in M.MP_SPLIT_CASES} == {1, 3}
    assert [s[:4] for s in M.BL_SIZES] == [(5, 9, 9, 17), (3, 5, 9, 17), (9, 17, 5, 9), (2, 2, 2, 2), (1, 1, 4, 7), (1, 6, 5, 6), (4, 6, 1, 1), (9, 3, 33, 9)]
    assert M.BL_SIZES[-1][5] == 3 and {s[4] for s in M.BL_SIZES} == {8, 64} and len(M.BL_CASES) == 6 * 8
    for h, w, OH, OW, _, _ in M.BL_SIZES:                      # the scale is a power of two (or 0): every weight is exact
        for n, m in ((h, OH), (w, OW)):
            s = (n - 1) / (m - 1) if m > 1 else 0.0
            assert s == 0 or torch.log2(torch.tensor(s)).item() % 1 == 0
    assert M.BL_TOL_SIZES == [(3, 266, 5, 1080), (266, 3, 1080, 5), (17, 30, 68, 120)] and {c.form for c in M.BL_TOL_CASES} == {"f32", "split"}
    assert M.DW_SHAPES == [(9, 9, 64, 1, 1, True, 1), (19, 27, 128, 2, 2, False, 2), (8, 30, 64, 12, 12, True, 1), (11, 13, 64, 1, 0, False, 1)]
    assert [(c.fmt, c.H, c.W, c.B) for c in M.ST_CASES] == [("f32", 33, 47, 1), ("f32", 7, 250, 1), ("f32", 224, 9, 1), ("f32", 37, 53, 2),
                                                            ("u8", 33, 47, 1), ("u8", 7, 250, 1)]


@pytest.mark.parametrize("p", _ALL, ids=_fid)
def test_case_builds_and_is_accepted(p):
    fam, c = p
    _, cid, _, _, want, stored, dev, make_op = M.FAMILIES[fam]
    bufs, _ = want(c)
    assert M.same(stored(c), bufs)
    d = dev(c)
    for k, t in bufs.items():                                  # the fill around the output slice
        assert bool((t[-M.TAIL:] == M.FILL).all()) and bool((t[:, :M.OUT_OFF] == M.FILL).all()) and bool((t[:, t.shape[1] - M.OUT_PAD + M.OUT_OFF:] == M.FILL).all())
    ptr = {k: (1 << 20) << i for i, k in enumerate(list(d) + list(bufs))}
    op = make_op(c, ptr)
    assert _create(op) == 0, cid(c)
    assert op.out_ld > op.out_c and (op.out - ptr["out"]) > 0
    if fam != "stem_split":                                    # the poison: past the last image, and in the columns outside the slice
        poisoned = torch.isposinf if fam == "maxpool" else torch.isnan
        for k in ("in", "in_lo"):
            if k in d:
                t = d[k]
                live = torch.isfinite(t.float())
                assert bool(poisoned(t[-M.TAIL:].float()).all()) and int(live.sum()) == (t.shape[0] - M.TAIL) * op.in_c and bool(poisoned(t.float())[~live].all())
        assert op.in_ld > op.in_c or fam == "maxpool"
    elif c.fmt == "f32":
        assert bool(torch.isnan(d["in"][-M.TAIL:]).all()) and d["in"].numel() == c.B * 3 * c.H * c.W + M.TAIL


def test_split_ops_reach_the_split_kernels():
    """the launch layer's branches, restated: a depthwise 3x3 with exactly one side split is k_dwconv_split; a stem with w_layout 1 and
    w_split 1 is the split MFMA stem and asks for out_lo; a max-pool takes both sides split or none"""
    ptr = lambda names: {k: (1 << 20) << i for i, k in enumerate(names)}
    c = M.DW_CASES[0]
    for c in M.DW_CASES:
        op = M.dw_make_op(c, ptr(list(M.dw_device_inputs(c)) + list(M.dw_want(c)[0])))
        assert (op.in_lo is None) != (op.out_lo is None) and op.ksize == 3 and not op.out_mx
    c = M.MP_SPLIT_CASES[4]
    op = M.mp_make_op(c, ptr(["in", "in_lo", "out", "out_lo"]))
    assert _create(op) == 0
    op.out_lo = None
    assert _create(op) != 0
    c = M.ST_CASES[0]
    op = M.st_make_op(c, ptr(["in", "weight", "bias", "out", "out_lo"]))
    assert op.w_layout == 1 and op.w_split == 1 and _create(op) == 0


def test_the_stem_weights_reach_the_device_as_two_independent_arrays():
    from vision_semantic_segmentation_amd.network import pack_stem_mfma
    for c in (M.ST_CASES[0], M.ST_CASES[4]):
        o, d = M.st_operands(c), M.st_device_inputs(c)
        n = d["weight"].numel() // 2
        assert torch.equal(d["weight"][:n].double(), pack_stem_mfma(o["Wh"])) and torch.equal(d["weight"][n:].double(), pack_stem_mfma(o["Wl"]))
        assert bool((o["Wl"] != 0).any()) and not torch.equal(o["Wh"] != 0, o["Wl"] != 0)
    o = M.st_operands(M.ST_CASES[4])                           # one-hot: half the channels through Wh alone, half through Wl alone
    nz = lambda w: (w != 0).reshape(64, -1).sum(dim=1)
    assert torch.equal(nz(o["Wh"]) + nz(o["Wl"]), torch.ones(64, dtype=torch.long)) and int(nz(o["Wl"]).sum()) == 32


@pytest.mark.parametrize("c", M.BL_TOL_CASES, ids=M.bl_id)
def test_the_coordinate_rule_meets_the_derived_bar_and_a_contracted_coordinate_does_not(c):
    """bar = 8 u max|four corners| (+ 2^-22 |ref| for the split pair): the stated rule evaluated in float32 stays under it everywhere, the
    coordinate with scale * dst - corner as one fused operation exceeds it in more than 10 % of the elements"""
    ref, bar = M.bl_tolerance(c)
    cm = M.corner_max(M.bl_value(M.bl_operands(c)), c.OH, c.OW)
    fig = {}
    for mode in ("rule", "contracted"):
        err = (M.bl_host_float32(c, mode) - ref).abs()
        fig[mode] = (float((err / (M.U * cm)).max()), float((err > bar).double().mean()))
        print("%s %-10s worst %.2f u max|corner|, over the bar in %.1f %% of the elements" % (M.bl_id(c), mode, fig[mode][0], 100 * fig[mode][1]))
    assert fig["rule"][1] == 0.0
    assert fig["contracted"][1] > 0.10
    if c.form == "f32":
        assert fig["rule"][0] <= 3.0


def test_every_mistake_changes_a_byte_of_every_case_it_applies_to():
    lines = []
    for fam, (cases, cid, muts, applicable, want, stored, _, _) in M.FAMILIES.items():
        for mut in muts:
            counts = [(cid(c), M.changed_bytes(stored(c, mut), want(c)[0])) for c in cases if applicable(c, mut)]
            assert counts, (fam, mut, "applies to no case")
            lines.append("%-13s %-26s cases %2d  bytes changed: least %7d (%s), all cases %8d" % (
                fam, mut, len(counts), min(n for _, n in counts), min(counts, key=lambda t: t[1])[0], sum(n for _, n in counts)))
            for name, n in counts:
                assert n > 0, (fam, mut, name, "changes no expected byte")
    print("\n" + "\n".join(lines))
    assert len(lines) == len(M.MP_MUTATIONS) + len(M.BL_MUTATIONS) + len(M.DW_MUTATIONS) + len(M.ST_MUTATIONS) == 6 + 6 + 5 + 7


def test_a_mistake_that_cannot_show_is_stated_as_such():
    """where applicable() says no, the reason is a property of the case, shown here: the mistake leaves every byte as it is"""
    for c, mut in ((M.MPCase("f16", 2, 2, 8, 1, 0), "window_from_2oy"), (M.MPCase("split", 1, 1, 64, 1, 0), "hi_only")):
        assert not M.mp_applicable(c, mut) and M.same(M.mp_stored(c, mut), M.mp_want(c)[0])
    for c, mut in ((M.BLCase("f16", 1, 6, 5, 6, 64, 1), "scale_in_over_out"), (M.BLCase("in_lo", 9, 17, 5, 9, 8, 1), "drop_in_lo"),
                   (M.BLCase("out_lo", 9, 17, 5, 9, 8, 1), "out_lo_truncated")):
        assert not M.bl_applicable(c, mut) and M.same(M.bl_stored(c, mut), M.bl_want(c)[0])
