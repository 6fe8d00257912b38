"""The cases of test_gpu_fused_mixed_exact.py, checked without a GPU (tests/_fused_mixed_operands.py): every case builds with all the
operand conditions asserted while it does (the exactness bound and float32 == float64 at every stage, >= 20 % rounded hi values, ties in
both directions in the output split and in an intermediate split, populated lo tiles and lo planes, tied class maxima); what the device
reads decodes back to the independent hi and lo matrices, and the splice helpers reproduce the shipped packers' bytes on coupled
weights; the library accepts every case's op and the host restatement of its dispatch names the kernel the case claims; the case lists
cover every reachable instantiation and shape class; and the comparison has teeth: each subtly wrong host evaluation changes at least
one stored byte of at least one case per kernel family it applies to."""
import ctypes as C

import pytest
import torch

import _fused_mixed_operands as M


def _create(op):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    plan = C.c_void_p()
    rc = _lib.lib().avl_seg_plan_create((AvlSegOp * 1)(op), 1, C.byref(plan))
    if rc == 0:
        _lib.lib().avl_seg_plan_destroy(plan)
    return rc


class _Placeholder(dict):
    """a distinct aligned address per buffer name: what the library's validation looks at (no GPU)"""
    def __missing__(self, key):
        self[key] = 1 << 20 << len(self)
        return self[key]


# ------------------------------------------------------------------------------------------------------------------ DWPW
@pytest.mark.parametrize("c", M.DW_CASES, ids=M.dw_id)
def test_dwpw_case_builds_is_accepted_and_names_its_kernel(c):
    r, bufs = M.want_dw(c)
    g = M.dw_geometry(c)
    bm = c.B * g["m"]
    assert r["y"].shape == (bm, c.N) and g["rows"] > bm and g["rows_in"] > c.B * c.H * c.W          # rows past M exist: their fill is compared
    assert M.same(M.dw_evaluate(c), bufs)
    if c.kernel == "cls":
        assert bufs["logits"].shape == (g["rows"], c.ncls) and bool((bufs["logits"][bm:] == M.FILL_LOGIT).all()) and bool((bufs["labels"][bm:] == M.FILL_LABEL).all())
        assert torch.equal(bufs["labels"][:bm].long(), torch.argmax(bufs["logits"][:bm], dim=1)) or c.order == "hole"
    else:
        assert bool((bufs["out"][bm:] == M.FILL).all()) and (c.olo or bool((bufs["out_lo"] == M.FILL).all()))
        if c.slices:
            assert bool((bufs["out"][:, :g["out_off"]] == M.FILL).all()) and bool((bufs["out"][:, g["out_off"] + c.N:] == M.FILL).all())
    if c.order == "hole":
        live = M.dw_live_rows(c)
        assert 0 < int((~live).sum()) < bm and bool((bufs["out"][:bm][~live] == M.FILL).all())
    op = M.make_dw_op(c, _Placeholder())
    assert _create(op) == 0
    assert M.dw_dispatch(op.w_split, bool(op.in_lo), bool(op.out_f32)) == c.kernel


@pytest.mark.parametrize("c", [c for c in M.DW_CASES if c.K <= 512 and c.order != "hole"][::3], ids=M.dw_id)
def test_dwpw_device_inputs_hold_the_independent_matrices(c):
    o, d, g = M.dw_operands(c), M.dw_device_inputs(c), M.dw_geometry(c)
    w = d["weight"].reshape(g["np"], g["nk"], 2, 64)
    assert torch.equal(w[:, :, 0].reshape(g["np"], c.K).float(), o["Wh"]) and torch.equal(w[:, :, 1].reshape(g["np"], c.K).float(), o["Wl"])
    n_in = c.B * c.H * c.W
    cols = slice(g["in_off"], g["in_off"] + c.K)
    assert torch.equal(d["x"][0, :n_in, cols].float(), o["xh"].reshape(n_in, c.K))
    if o["xl"] is not None:
        xl = d["x"][1, :n_in, cols].float()
        assert torch.equal(xl, o["xl"].reshape(n_in, c.K)) and float((xl != 0).float().mean()) > 0.8
        assert not torch.equal(xl.double(), (o["xh"].double() - o["xh"].to(torch.float16).double()).reshape(n_in, c.K))      # no remainder of x_hi (which is exact)
    if c.kernel != "w2":
        p = d["params"][:g["nk"] * 640].view(torch.float32).reshape(g["nk"], 8, 10, 8)
        assert torch.equal(p[:, :, :9].permute(0, 1, 3, 2).reshape(c.K, 9), o["w1"]) and torch.equal(p[:, :, 9].reshape(c.K), o["b1"])
        if g["nk"] > 1:
            assert not torch.equal(p[0], p[1])                                  # the parameters differ per K-step: a stale ring slot shows
    assert torch.equal(d["params"][-g["mtiles"]:], M.dw_order(c))


def test_splice_helpers_address_the_shipped_layouts():
    """fed the two halves of a coupled split, the helpers give the shipped packers' bytes"""
    from vision_semantic_segmentation_amd.network import pack_bottleneck, pack_split_rows, split_f16
    g = torch.Generator().manual_seed(5)
    w = torch.randn((256, 192), generator=g, dtype=torch.float64)
    hi, lo = split_f16(w)
    assert bool((lo != 0).any())
    assert torch.equal(M.splice_rows(pack_split_rows(hi.double(), 2), pack_split_rows(lo.double(), 2)).view(torch.int16), pack_split_rows(w, 2).view(torch.int16))
    for cin, ds in ((64, True), (256, False)):
        ws = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((128, cin), (128, 4, 3, 3), (256, 128), (256, cin))]
        if not ds:
            ws[3] = None
        his, los = zip(*[(None, None) if t is None else tuple(p.double() for p in split_f16(t)) for t in ws])
        for a, b, ref in zip(pack_bottleneck(*his, 32), pack_bottleneck(*los, 32), pack_bottleneck(*ws, 32)):
            assert torch.equal(M.splice_fragments(a, b).view(torch.int16), ref.view(torch.int16))


def test_dwpw_cases_cover_the_kernels_and_shapes():
    by = {k: [c for c in M.DW_CASES if c.kernel == k] for k in M.DW_KERNELS}
    assert all(by.values())
    from _exact_operands import DWPW_CASES
    assert {(c.H, c.W, c.K, c.N, c.dil, c.pad) for c in by["w2"]} == {t[:6] for t in DWPW_CASES}
    x = by["x"]
    assert {64, 128, 512, 2048} <= {c.K for c in x} and any(c.K == 2048 and c.pad == c.dil == 24 for c in x) and any(c.N == 512 for c in x)
    assert any(M.dw_geometry(c)["m"] % 128 and M.dw_geometry(c)["mtiles"] % 8 and M.dw_geometry(c)["mtiles"] > 8 for c in x)
    assert any(c.slices for c in x) and any(c.B == 2 and (c.H * c.W) % 128 for c in x)
    xs = by["xs"]
    assert {c.layout for c in xs} == {0, 1} and {(c.pad, c.dil) for c in xs} >= {(0, 1), (12, 12), (1, 1)}
    assert any(c.layout and M.dw_geometry(c)["oh"] % 8 and M.dw_geometry(c)["ow"] % 16 for c in xs) and any(c.layout and M.dw_geometry(c)["ow"] <= 16 for c in xs)
    assert any(not c.layout and M.dw_geometry(c)["ow"] < 128 for c in xs)
    assert {64, 320, 512} <= {c.K for c in xs} and {64, 512} <= {c.N for c in xs} and any(c.B == 2 for c in xs)
    assert {"tile", "block", "rev", "hole"} <= {c.order for c in xs}
    cl = by["cls"]
    assert {c.ncls for c in cl} == {1, 5, 19, 32} and {c.layout for c in cl} == {0, 1} and {64, 512} <= {c.K for c in cl}
    assert any(c.B == 2 for c in cl) and any(c.allneg for c in cl)
    assert any(not c.olo for c in by["w2"] + x + xs)


# a few small cases per kernel family: together every mutation applies to each family it can
_DW_TEETH = [c for c in M.DW_CASES if c in (
    M.DCase("w2", 1, 9, 9, 64, 48, 2, 2), M.DCase("x", 1, 12, 21, 512, 256, 1, 1), M.DCase("x", 2, 12, 21, 128, 256, 2, 2),
    M.DCase("xs", 1, 14, 23, 320, 256, 1, 0), M.DCase("xs", 1, 16, 16, 64, 512, 1, 1, 1, "block"), M.DCase("xs", 1, 21, 40, 128, 256, 1, 0, 1, "block"),
    M.DCase("cls", 1, 14, 23, 512, 256, 1, 0, 0, "tile", 19), M.DCase("cls", 1, 21, 40, 64, 256, 1, 0, 1, "block", 5, allneg=True))]


@pytest.mark.parametrize("c", _DW_TEETH, ids=M.dw_id)
def test_dwpw_mutations_are_caught(c):
    _, bufs = M.want_dw(c)
    n = 0
    for mut in M.DW_MUTATIONS:
        if M.dw_applicable(c, mut):
            assert not M.same(M.dw_evaluate(c, mut), bufs), (M.dw_id(c), mut)
            n += 1
    assert n >= 8


def test_every_dwpw_mutation_applies_to_every_family_it_can():
    assert len(_DW_TEETH) == 8
    for k in M.DW_KERNELS:
        sel = [c for c in _DW_TEETH if c.kernel == k]
        possible = [m for m in M.DW_MUTATIONS if any(M.dw_applicable(c, m) for c in M.DW_CASES if c.kernel == k)]
        assert all(any(M.dw_applicable(c, m) for c in sel) for m in possible), k
    assert all(any(M.dw_applicable(c, m) for c in _DW_TEETH) for m in M.DW_MUTATIONS)


def test_a_row_written_past_m_lands_in_the_fill_only():
    for c, ev, key, m in ((_DW_TEETH[1], M.dw_evaluate, "out", None), (M.BN_CASES[1], M.bn_evaluate, "out", None)):
        good, bad = ev(c), ev(c, "row_past_m")
        m = c.B * (M.dw_geometry(c)["m"] if isinstance(c, M.DCase) else M.bn_geometry(c)["m"])
        assert torch.equal(bad[key][:m], good[key][:m]) and not torch.equal(bad[key][m:], good[key][m:])


# ------------------------------------------------------------------------------------------------------------ bottleneck
@pytest.mark.parametrize("c", M.BN_CASES, ids=M.bn_id)
def test_bottleneck_case_builds_is_accepted_and_names_its_kernel(c):
    r, bufs = M.want_bn(c)
    g = M.bn_geometry(c)
    bm = c.B * g["m"]
    assert r["y"].shape == (bm, M.COUT) and g["rows"] > bm
    assert bool((bufs["out"][bm:] == M.FILL).all()) and (c.olo or bool((bufs["out_lo"] == M.FILL).all()))
    if c.slices:
        assert bool((bufs["out"][:, :g["out_off"]] == M.FILL).all()) and bool((bufs["out"][:, g["out_off"] + M.COUT:] == M.FILL).all())
    if (c.H, c.W) != M.BN_MANY:
        assert M.same(M.bn_evaluate(c), bufs)
    else:
        assert g["tiles"] == 510 and g["tpw"] == 2
    op = M.make_bn_op(c, _Placeholder())
    assert _create(op) == 0
    assert M.bn_dispatch(op.in_c, op.w_split, bool(op.in_lo), bool(op.out_lo)) == (c.cin, c.cin == 64, bool(c.t1lo), bool(c.xlo), bool(c.olo))


def _unfrag(p, rows, k):
    """the inverse of the packer's MFMA fragment order: [rows / 16][k / 32][hi, lo][lane 64][8] -> (hi, lo) float32 [rows][k]"""
    f = p.reshape(rows // 16, k // 32, 2, 4, 16, 8).permute(2, 0, 4, 1, 3, 5).reshape(2, rows, k)
    return f[0].float(), f[1].float()


@pytest.mark.parametrize("c", [M.BN_CASES[1], M.BN_CASES[15]], ids=M.bn_id)
def test_bottleneck_device_inputs_hold_the_independent_matrices(c):
    o, d = M.bn_ops_of(c), M.bn_device_inputs(c)
    hi, lo = _unfrag(d["p1"], M.WIDTH, c.cin)
    assert torch.equal(hi, o["W1h"]) and torch.equal(lo, o["W1l"]) and bool((lo != 0).any())
    hi, lo = _unfrag(d["p2"], M.WIDTH, 160)                    # dense 16-channel windows: [out][tap 10][in 16]
    for got, w in ((hi, o["W2h"]), (lo, o["W2l"])):
        dense = got.reshape(M.WIDTH, 10, 16)
        co = torch.arange(M.WIDTH)
        back = torch.stack([dense[co, :9, (co % 16) // 4 * 4 + ci] for ci in range(4)], dim=1)
        assert torch.equal(back.reshape(M.WIDTH, 4, 3, 3), w) and float(dense.abs().sum()) == float(w.abs().sum())
    ks3 = (M.WIDTH + (c.cin if c.cin == 64 else 0)) // 32
    p3 = d["p3"].reshape(8, ks3, 2, 2, 64, 8).permute(0, 2, 1, 3, 4, 5).reshape(-1)                  # [wave][nj][ks][hi, lo][lane][8]
    hi, lo = _unfrag(p3, M.COUT, ks3 * 32)
    i = torch.arange(16)
    rows = torch.cat([32 * wv + (i >> 2) * 8 + nj * 4 + (i & 3) for wv in range(8) for nj in range(2)])
    want_hi = torch.cat([o["W3h"]] + ([o["Wdh"]] if c.cin == 64 else []), dim=1)[rows]
    want_lo = torch.cat([o["W3l"]] + ([o["Wdl"]] if c.cin == 64 else []), dim=1)[rows]
    assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo)
    bm = c.B * c.H * c.W
    g = M.bn_geometry(c)
    cols = slice(g["in_off"], g["in_off"] + c.cin)
    assert torch.equal(d["x"][0, :bm, cols].float(), o["xh"].reshape(bm, c.cin))
    if c.xlo:
        assert torch.equal(d["x"][1, :bm, cols].float(), o["xl"].reshape(bm, c.cin)) and float((o["xl"] != 0).float().mean()) > 0.8


def test_bottleneck_cases_cover_the_instantiations_and_shapes():
    inst = {(c.cin, c.t1lo, c.xlo, c.olo) for c in M.BN_CASES}
    assert inst == {(64, t, False, o) for t in (False, True) for o in (False, True)} | {(256, False, x, o) for x in (False, True) for o in (False, True)}
    assert len({M.bn_kernel(c) for c in M.BN_CASES}) == 8
    shapes = {(c.B, c.H, c.W) for c in M.BN_CASES}
    assert {(1, 8, 16), (1, 23, 45), (1, 1, 1), (1, 3, 200), (1, 70, 5), (2, 23, 45), (1, *M.BN_MANY)} <= shapes
    for cin in (64, 256):
        sel = [c for c in M.BN_CASES if c.cin == cin]
        assert any(c.slices for c in sel) and any(c.B == 2 for c in sel) and any((c.H, c.W) == M.BN_MANY for c in sel)
    assert all(c.xlo for c in M.BN_CASES if c.cin == 256 and (c.B == 2 or (c.H, c.W) == M.BN_MANY))          # the independent x_lo plane where tiles are walked


_BN_TEETH = [M.BCase(64, True, False, True, 2, 23, 45), M.BCase(64, False, False, False, 1, 23, 45), M.BCase(256, False, True, True, 2, 23, 45),
             M.BCase(256, False, False, False, 1, 70, 5)]


@pytest.mark.parametrize("c", _BN_TEETH, ids=M.bn_id)
def test_bottleneck_mutations_are_caught(c):
    assert c in M.BN_CASES
    _, bufs = M.want_bn(c)
    n = 0
    for mut in M.BN_MUTATIONS:
        if M.bn_applicable(c, mut):
            assert not M.same(M.bn_evaluate(c, mut), bufs), (M.bn_id(c), mut)
            n += 1
    assert n >= 14


def test_every_bottleneck_mutation_applies_somewhere():
    assert all(any(M.bn_applicable(c, m) for c in _BN_TEETH) for m in M.BN_MUTATIONS)
    for cin in (64, 256):
        possible = [m for m in M.BN_MUTATIONS if any(M.bn_applicable(c, m) for c in M.BN_CASES if c.cin == cin)]
        assert all(any(M.bn_applicable(c, m) for c in _BN_TEETH if c.cin == cin) for m in possible)
