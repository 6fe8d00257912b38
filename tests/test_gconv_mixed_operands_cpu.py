"""The cases of test_gpu_gconv_mixed_exact.py, checked without a GPU (tests/_gconv_mixed_operands.py): every case builds with all the
operand conditions asserted while it does (the FP4 operands survive the host quantiser and the shipped weight packer, the exactness
bound, float32 == float64, >= 20 % rounded outputs, ties in both directions, a populated lo plane, distinct scale bytes); the library
accepts every case's op; a host evaluation of what the DEVICE reads (decoded fragments and bundles) reproduces every expected buffer;
every case reaches the (WS, XS, NJ) and the tiles per workgroup it names at 256 CUs; and the comparison has teeth: for one case per
form each subtly wrong host result changes at least one stored byte."""
import ctypes as C

import pytest
import torch

import _gconv_mixed_operands as M


def _create(op):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    rc = _lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan))
    if rc == 0:
        _lib.lib().avl_seg_plan_destroy(plan)
    return rc


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_case_builds_and_the_evaluator_reproduces_every_buffer(c):
    v, bufs = M.want(c)
    g = M.geometry(c)
    assert v.shape == (g["m"], c.C) and g["rows"] > g["m"]                  # rows past M exist: their fill is compared
    assert bufs["out"].shape == (g["rows"], c.C) and bool((bufs["out"][g["m"]:] == M.FILL).all())
    assert M.has_lo(c) or bool((bufs["out_lo"] == M.FILL).all())
    assert M.has_mx(c) or bool((bufs["out_mx"] == M.FILL_BYTE).all())
    assert M.same(M.evaluate(c), bufs)


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_case_is_accepted_and_reaches_the_instantiation_it_names(c):
    """pick_th restates the launcher's choice: the claim (NJ, tiles per workgroup) holds at 256 CUs, and avl_seg_plan_create accepts the op
    (placeholder pointers: no GPU)"""
    assert M.accepted(c)
    t = M.pick_th(c, 256)
    assert (t["nj"], t["tpw"]) == (c.nj, c.tpw), (M.case_id(c), t)
    assert _create(M.shape_op(c)) == 0


def test_cases_cover_the_forms_shapes_and_instantiations():
    reached = {(c.ws, c.xs, c.nj) for c in M.CASES}
    # every instantiation of k_gconv_mfma<f16, 1 | 2, NJ, XS> but <f16, 1, 1, true> (below)
    assert reached == {(2, False, 1), (2, False, 2), (1, False, 1), (1, False, 2), (1, False, 4), (1, True, 2)}
    forms = {(c.ws, c.xs, c.in_lo, c.form) for c in M.CASES}
    assert {(2, False, il, f) for il in (False, True) for f in M.FORMS} <= forms
    assert {(1, False, False, f) for f in M.FORMS} <= forms and (1, True, False, "lo") in forms
    for ws, xs in ((2, False), (1, False), (1, True)):
        sel = [c for c in M.CASES if (c.ws, c.xs) == (ws, xs)]
        assert any(c.s == 1 and c.d == 1 and M.geometry(c)["oh"] % (2 * c.nj) and c.W % 32 for c in sel)        # ragged in both directions
        assert any(c.s == 1 and c.d == 2 for c in sel) and any(c.s == 1 and c.d == 4 for c in sel)               # the comb
        long = [c for c in sel if M.pick_th(c)["tpw"] >= 3]
        assert long and all(M.walk_crosses_columns(M.pick_th(c)) and M.pick_th(c)["nj"] >= 2 for c in long)      # both buffers reused, late_stage
    assert any(c.ws == 2 and c.s == 2 and c.nj == 1 for c in M.CASES)
    assert any(c.ws == 1 and not c.xs and (c.s, c.d) == (2, 1) and c.nj == 2 for c in M.CASES)
    assert any(c.ws == 1 and (c.s, c.d) == (2, 2) and c.nj == 1 for c in M.CASES)
    batched = [c for c in M.CASES if c.B > 1]
    assert batched and all(c.ws == 2 and (c.H * c.W) % 256 and (M.geometry(c)["m"] // c.B) % 256 for c in batched)
    assert {c.in_lo for c in batched} == {False, True}
    assert {c.C for c in M.CASES if c.ws == 2} == {256, 512, 1024} and {c.C for c in M.CASES if c.ws == 1} >= {128, 256, 512, 1024}


def test_the_two_row_tile_with_a_split_input_is_unreachable():
    """k_gconv_mfma<f16, 1, 1, true> is instantiated, but no accepted op launches it: at stride 2 two split-input tiles of even two rows do
    not fit 160 KB (refused at plan creation), and at stride 1 the four-row tile always fits (dilation > 1 combs: tap distance 1)"""
    for d in (1, 2, 4):
        c = M.Case(1, True, False, "lo", 1, 23, 45, 256, 2, d, 1, 1)
        assert not M.accepted(c) and _create(M.shape_op(c)) != 0
        for C_ in (128, 1024):
            for hw in ((3, 3), (23, 45), (300, 700)):
                assert M.pick_th(M.Case(1, True, False, "lo", 1, hw[0], hw[1], C_, 1, d, 0, 0))["th"] == 4
    # MX at stride 2 with dilation 2 is refused as well
    c = M.Case(2, False, True, "mx_f32lo", 1, 23, 45, 256, 2, 2, 1, 1)
    assert not M.accepted(c) and _create(M.shape_op(c)) != 0


def _one_per_form():
    seen, out = set(), []
    for c in M.CASES:
        k = (c.ws, c.xs, c.in_lo, c.form, c.bias)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _one_per_form(), ids=M.case_id)
def test_mutations_are_caught(c):
    """each deliberately wrong host evaluation differs from the expectation in at least one stored byte; the one that provably cannot on
    integer biases (Q4(lo) from the other source: v - out has at most seven significant bits there, exact in f16) is asserted to change
    nothing on those cases and to be caught, in both directions, on M.FRAC_CASES"""
    _, bufs = M.want(c)
    n = 0
    for mut in M.MUTATIONS:
        if not M.applicable(c, mut):
            continue
        if M.invisible(c, mut):
            assert M.same(M.evaluate(c, mut), bufs), (M.case_id(c), mut)
            continue
        assert not M.same(M.evaluate(c, mut), bufs), (M.case_id(c), mut)
        n += 1
    assert n >= 6


def test_every_mutation_applies_somewhere():
    cases = _one_per_form()
    assert all(any(M.applicable(c, m) and not M.invisible(c, m) for c in cases) for m in M.MUTATIONS)
    # the source of Q4(lo): visible where the form says fp32 and where it says the f16 plane
    assert {c.form for c in M.FRAC_CASES} == {"mx_f32lo", "mx_lo"}
    for c in M.FRAC_CASES:
        v, bufs = M.want(c)
        lo32 = v - v.to(torch.float16).double()
        assert bool((lo32.to(torch.float16).double() != lo32).any())


def test_a_wrong_last_row_lands_in_the_fill_only():
    """the "rows past M" mutation leaves the live rows as they are: only the comparison of the fill catches it"""
    c = M.CASES[0]
    _, bufs = M.want(c)
    m = M.geometry(c)["m"]
    bad = M.evaluate(c, "last_row_past_m")
    assert torch.equal(bad["out"][:m], bufs["out"][:m]) and not torch.equal(bad["out"][m:], bufs["out"][m:])
    assert not torch.equal(bad["out_mx"], bufs["out_mx"])
