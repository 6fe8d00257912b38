"""The operands of test_gpu_exact_ops.py, checked without a GPU (tests/_exact_operands.py builds them and asserts, while it does,
that the float32 and float64 host evaluations agree, that every expected output is finite, that >= 20 % of the 16-bit outputs
round and that exact ties round in both directions), and the teeth of the comparison: for one case of each op a subtly wrong host
result -- another rounding rule, one product dropped, two taps swapped, a K block skipped in the last row tile, the residual
added after the ReLU -- is not torch.equal to the expected tensor."""
import pytest
import torch
import torch.nn.functional as F

import _exact_operands as X

PRECS = ["f32", "bf16", "f16"]


@pytest.mark.parametrize("case", X.GEMM_CASES + [X.GEMM_RING256], ids=str)
def test_gemm_operands(case):
    for prec in PRECS:
        c = X.gemm_case(case, prec)
        assert c["want"].shape == (case[0], case[2])


@pytest.mark.parametrize("case", X.GEMM_ARGMAX, ids=str)
def test_classifier_operands_hold_ties(case):
    c = X.gemm_case(case, "f16")
    assert c["tied_rows"] > 0 and c["want"].dtype == torch.float32


@pytest.mark.parametrize("case", X.CONV3X3_CASES, ids=str)
def test_dense_conv_operands(case):
    H, W, cg, G, s, d = case
    for prec in PRECS:
        X.conv_case(H, W, cg * G, G, 3, s, d, d, prec)
    X.conv_split_case(H, W, cg * G, G, s, d, True)


def test_dense_conv_split_operands_without_lo_plane():
    for (H, W, cg, G, s, d), with_lo in X.CONV3X3_SPLIT:
        if not with_lo:
            X.conv_split_case(H, W, cg * G, G, s, d, False)


def test_grouped_and_depthwise_operands():
    for H, W, cg, s, d in X.GCONV_MFMA_CASES:
        for prec in ("bf16", "f16"):
            X.conv_case(H, W, 32 * cg, 32, 3, s, d, d, prec)
    for cg in X.GCONV_DIRECT_CG:
        for H, W, s, d in X.GCONV_DIRECT_SHAPES:
            for prec in PRECS:
                X.conv_case(H, W, 16 * cg, 16, 3, s, d, d, prec)
    for H, W, Cc, d, pad, relu in X.DW3_CASES:
        for prec in PRECS:
            X.conv_case(H, W, Cc, Cc, 3, 1, pad, d, prec, relu=relu)
    for ks in X.DWK_KS:
        for H, W, Cc, batch in X.DWK_SHAPES:
            for prec in PRECS:
                X.conv_case(H, W, Cc, Cc, ks, 1, 0, 1, prec, relu=bool(ks & 1), batch=batch)


@pytest.mark.parametrize("hw", X.STEM_SIZES, ids=str)
def test_stem_operands(hw):
    for prec in PRECS:
        for fmt in ("f32", "u8"):
            X.stem_case(hw[0], hw[1], fmt, "direct", prec)
            if prec != "f32":
                X.stem_case(hw[0], hw[1], fmt, "mfma", prec)


def test_dwpw_operands():
    for H, W, K, N, d, pad, relu in X.DWPW_CASES:
        for prec in ("bf16", "f16"):
            X.dwpw_case(H, W, K, N, d, pad, prec, relu)


def test_the_evaluator_is_the_convolution():
    """the im2col evaluator against F.conv2d in float64: dense, grouped, depthwise, strided, dilated past the image"""
    for H, W, Cc, G, k, s, pad, d in ((9, 14, 64, 1, 3, 1, 2, 2), (11, 17, 64, 16, 3, 2, 2, 2), (5, 7, 64, 64, 3, 1, 12, 12), (13, 9, 64, 64, 5, 1, 0, 1)):
        c = X.conv_case(H, W, Cc, G, k, s, pad, d, "f32", tag=1)
        cg = Cc // G
        w = c["W4"].reshape(Cc, k, k, cg).permute(0, 3, 1, 2).double()
        ref = F.relu(F.conv2d(c["x"].permute(0, 3, 1, 2).double(), w, c["bias"].double(), stride=s, padding=pad, dilation=d, groups=G))
        assert torch.equal(ref[0].permute(1, 2, 0).reshape(-1, Cc), c["v"])


def _teeth_cases():
    return {
        "gemm": X.gemm_case((777, 2048, 512, True, True, "slices"), "bf16"),
        "gemm_f16": X.gemm_case((777, 256, 128, True, False, None), "f16"),
        "conv3x3": X.conv_case(13, 21, 256, 1, 3, 1, 2, 2, "f16"),
        "gconv_mfma": X.conv_case(23, 45, 256, 32, 3, 2, 2, 2, "bf16"),
        "gconv_direct": X.conv_case(13, 21, 64, 16, 3, 1, 1, 1, "f16"),
        "dwconv3": X.conv_case(17, 23, 128, 128, 3, 1, 12, 12, "bf16", relu=False),
        "dwconv_k": X.conv_case(13, 29, 64, 64, 5, 1, 0, 1, "f16"),
        "stem": X.stem_case(33, 47, "f32", "mfma", "bf16"),
        "stem_u8": X.stem_case(33, 47, "u8", "mfma", "f16"),
        "dwpw": X.dwpw_case(19, 27, 128, 256, 12, 12, "f16", True),
    }


def test_every_mutation_is_caught():
    caught = {m: 0 for m in X.MUTATIONS}
    for name, c in _teeth_cases().items():
        assert torch.equal(X.evaluate(c), c["want"]), name                      # the evaluator reproduces the expected tensor ...
        for mut in X.MUTATIONS:
            if X.applicable(c, mut):
                assert not torch.equal(X.evaluate(c, mut), c["want"]), (name, mut)      # ... and no mutation of it does
                caught[mut] += 1
    assert all(caught.values()), caught
    # the depthwise stage of the fused op: two swapped taps
    a, b = X.dwpw_case(19, 27, 128, 256, 12, 12, "f16", True), X.dwpw_case(19, 27, 128, 256, 12, 12, "f16", True, dw_mut="swap_taps")
    assert not torch.equal(a["want"], b["want"])


def test_rounding_mutations_differ_only_where_they_should():
    v = torch.tensor([257.0, 259.0, -257.0, -259.0, 258.0, 300.5], dtype=torch.float64)
    assert X.round_toward_zero(v, "bf16").tolist() == [256.0, 258.0, -256.0, -258.0, 258.0, 300.0]
    assert X.round_half_away(v, "bf16").tolist() == [258.0, 260.0, -258.0, -260.0, 258.0, 300.0]
    assert v.to(torch.bfloat16).tolist() == [256.0, 260.0, -256.0, -260.0, 258.0, 300.0]
    v = torch.tensor([2049.0, 2051.0, -2049.0, -2051.0, 2050.0], dtype=torch.float64)
    assert X.round_toward_zero(v, "f16").tolist() == [2048.0, 2050.0, -2048.0, -2050.0, 2050.0]
    assert X.round_half_away(v, "f16").tolist() == [2050.0, 2052.0, -2050.0, -2052.0, 2050.0]
    assert v.to(torch.float16).tolist() == [2048.0, 2052.0, -2048.0, -2052.0, 2050.0]


# ------------------------------------------------------------------------- the ring GEMM's EXT forms (tests/_ring_ext_operands.py)
import _ring_ext_operands as R  # noqa: E402


@pytest.mark.parametrize("c", R.SMALL_CASES + R.MULTI_TILE_CASES, ids=R.case_id)
def test_ring_ext_operands(c):
    """every case: the exactness bound, float32 product == float64 product, >= 20 % of the outputs round, ties in both directions,
    non-zero lo planes (R.want asserts them); sentinels survive outside the written slices"""
    g = R.geometry(c)
    v, bufs = R.want(c, check64=True)
    assert v.shape == (g["M"], c.N)
    assert bool((bufs["out"][:, g["M"]:] == R.FILL).all()) and bool((bufs["out"][:, :, :R.COL] == R.FILL).all())
    assert bool((bufs["out"][:, :, R.COL + g["n1"]:] == R.FILL).all()) and bool((bufs["out2"][:, g["M"]:] == R.FILL).all())
    assert bool((bufs["out"][1] == R.FILL).all()) != bool(c.lo1) and bool((bufs["out2"][1] == R.FILL).all()) != bool(c.lo2)
    assert bool((bufs["out2"][0] == R.FILL).all()) != bool(c.n_split)
    a = R.device_input(c)
    rows = R.row_map(c)
    assert bool(torch.isfinite(a[:, rows, :R.K].float()).all()) and int(torch.isfinite(a.float()).sum()) == a.shape[0] * g["M"] * R.K


_HOST = torch.zeros(1 << 12, dtype=torch.uint8)
_PTR = (_HOST.data_ptr() + 255) // 256 * 256        # host memory: validation and the route look at values and alignment only


@pytest.mark.parametrize("c", R.SMALL_CASES + R.MULTI_TILE_CASES, ids=R.case_id)
def test_ring_ext_case_runs_the_instantiation_the_table_names(c):
    """the library's route for the case's op (placeholder pointers: no GPU) is the row of R.INSTANTIATION the case claims, on the
    256-row tiles of the ring kernel, and avl_seg_plan_create accepts that op"""
    import ctypes as C
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp, gemm_route
    op = R.shape_op(c, _PTR)
    r = gemm_route(op)
    assert R.instantiation(r) == R.INSTANTIATION[(c.mode, R.claimed_variant(c))]
    assert R.variant(c) == R.claimed_variant(c)
    bn = {2: 128, 3: 256}[R.claimed_variant(c)]
    assert (r["tile_m"], r["tile_n"], r["launches"]) == (256, bn, 1)
    assert R.tiles(c) == ((R.geometry(c)["M"] + 255) // 256, (c.N + bn - 1) // bn) and r["workgroups"] == min(256, r["m_tiles"] * r["n_tiles"])
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan)), "avl_seg_plan_create")
    _lib.lib().avl_seg_plan_destroy(plan)


def test_ring_ext_cases_reach_what_they_claim():
    """all eight EXT instantiations among the small cases of each form; every multi-tile case has more tiles than the grid's cap"""
    for cases in (R.SMALL_STRIDED, R.SMALL_TWIN, R.SMALL_BOTH):
        assert {(c.mode, R.variant(c)) for c in cases} == set(R.INSTANTIATION)
    assert {(c.mode, R.variant(c)) for c in R.MULTI_TILE_CASES} == set(R.INSTANTIATION)
    for c in R.MULTI_TILE_CASES:
        mt, nt = R.tiles(c)
        assert mt in (86, 171) and mt * nt > 256 and R.geometry(c)["M"] % 256 != 0, R.case_id(c)
        assert (256 % nt != 0) == (c.N != 512)
        if c.s > 1:
            assert (R.geometry(c)["M"] // c.B) % 256 != 0          # the image boundary falls inside a row tile
    assert any(c.s == 3 and c.B == 2 and c.extra and c.ih % 3 and c.iw % 3 for c in R.SMALL_STRIDED)
    assert any(c.n_split and c.s > 1 for c in R.MULTI_TILE_CASES)
    assert any(R.tiles(c)[0] * R.tiles(c)[1] > 512 and c.n_split for c in R.MULTI_TILE_CASES)      # every workgroup walks two tiles


@pytest.mark.parametrize("c", [R.SMALL_STRIDED[6], R.SMALL_STRIDED[8], R.SMALL_TWIN[6], R.SMALL_TWIN[9], R.SMALL_BOTH[6], R.SMALL_BOTH[7],
                               R.SMALL_BOTH[0], R.MULTI_TILE_CASES[12]], ids=R.case_id)
def test_ring_ext_mutations_are_caught(c):
    """each deliberately wrong host evaluation differs from the expectation in at least one stored element"""
    _, bufs = R.want(c)
    assert R.same(R.stored(c, R.exact_v(c)), bufs)
    n = 0
    for mut in R.MUTATIONS:
        if R.applicable(c, mut):
            assert not R.same(R.mutated(c, mut), bufs), (R.case_id(c), mut)
            n += 1
    assert n >= 2


def test_ring_ext_every_mutation_applies_somewhere():
    cases = [R.SMALL_STRIDED[8], R.SMALL_TWIN[6], R.SMALL_BOTH[6]]
    assert all(any(R.applicable(c, m) for c in cases) for m in R.MUTATIONS)
    assert all(R.applicable(R.SMALL_BOTH[6], m) for m in R.MUTATIONS)
