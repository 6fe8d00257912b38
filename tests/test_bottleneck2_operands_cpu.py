"""The cases of test_gpu_bottleneck2_exact.py, checked without a GPU (tests/_bottleneck2_operands.py): every case builds with all the
operand conditions asserted while it does (the exactness bound and float32 == float64 at every stage, >= 20 % rounded hi values, ties in
both directions in the output split and in the t2 split, a populated t2l tile, lo32 and Q4(lo) plane, spread scale bytes, a column
clamped as a whole); the library accepts every case's op, and in_c = 512 is restated as reaching k_bottleneck_w256; what the device
reads decodes back to the independent matrices, and the splice helper reproduces the shipped packer's bytes at width 256; the overflow
case flags the four tiles around its pixel; and the comparison has teeth: each subtly wrong host evaluation changes at least one stored
byte of every case it applies to.  The 270 x 240 case builds and is accepted here, but takes no part in the mutation matrix (its
reference takes four seconds per mutation; its operands come from the same generator as the seven smaller shapes)."""
import pytest
import torch

import _bottleneck2_operands as M
from test_fused_mixed_operands_cpu import _create, _Placeholder, _unfrag

_SMALL = [c for c in M.CASES if (c.H, c.W) != M.MANY]


def test_the_cases_are_the_shapes_at_which_the_kernel_can_go_wrong():
    shapes = [(c.B, c.H, c.W) for c in M.CASES if not c.frac]
    assert shapes == [(1, 1, 1), (1, 4, 16), (1, 5, 17), (1, 70, 5), (1, 3, 200), (1, 23, 45), (2, 23, 45), (1, 270, 240)]
    assert [c for c in M.CASES if c.frac] == [M.B2Case(1, 5, 17, True)]
    g = M.geometry(M.B2Case(1, *M.MANY))
    assert g["tiles"] == 1020 and g["tpw"] == 4
    for c in M.CASES:
        g = M.geometry(c)
        assert g["rows"] > g["bm"] and g["rows"] % 256 == 0                    # rows past M exist; the scale slabs' stride is not B H W


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_case_builds_is_accepted_and_reaches_the_layer2_kernel(c):
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes, mx_quant_fp4
    r, bufs = M.want(c)
    g = M.geometry(c)
    bm, rows = g["bm"], g["rows"]
    assert r["y"].shape == (bm, M.COUT) and bufs["out"].shape == (rows, M.COUT) and bufs["out_mx"].shape == (2, mx_bundle_bytes(rows, M.COUT))
    assert bool((bufs["out"][bm:] == M.FILL).all())
    hi = bufs["out"][:bm].double()
    for half, t in ((0, hi), (1, r["y"] - hi)):                                   # byte for byte what mx_quant_fp4 gives for out and for lo32
        q, s = M.unbundle(c, bufs["out_mx"], half)
        eq, es = mx_quant_fp4(t)
        assert torch.equal(q[:bm], eq) and torch.equal(s[:, :bm], es)
        assert bool((q[bm:] == M.FILL_BYTE).all()) and bool((s[:, bm:] == M.FILL_BYTE).all())
    if (c.H, c.W) != M.MANY:
        assert M.same(M.evaluate(c), bufs)
    op = M.make_op(c, _Placeholder())
    assert _create(op) == 0
    assert op.in_c == 512 and M.dispatch(op.in_c) == M.KERNEL


def test_the_library_takes_the_512_channel_branch_for_these_ops():
    """in_c = 512 is what selects k_bottleneck_w256 (launch_bottleneck, validate_bottleneck): the same op without its MX trunk, with a lo
    plane or with layer1's channel count is refused"""
    c = M.CASES[2]
    assert _create(M.make_op(c, _Placeholder())) == 0
    for change in (dict(in_mx=0), dict(out_mx=0), dict(mx_flags=0), dict(in_lo=1 << 12), dict(in_c=256, in_ld=256), dict(w_split=1)):
        op = M.make_op(c, _Placeholder())
        for k, v in change.items():
            setattr(op, k, v)
        assert _create(op) != 0, change


@pytest.mark.parametrize("c", [M.CASES[2], M.CASES[6]], ids=M.case_id)
def test_device_inputs_hold_the_independent_matrices(c):
    from vision_semantic_segmentation_amd.network import mx_dequant_fp4
    o, d, g = M.operands(c), M.device_inputs(c), M.geometry(c)
    bm, rows = g["bm"], g["rows"]
    hi, lo = _unfrag(d["p1"], M.WIDTH, M.CIN)
    assert torch.equal(hi, o["W1h"]) and torch.equal(lo, o["W1l"]) and bool((lo != 0).any()) and not torch.equal(hi, lo)
    hi, lo = _unfrag(d["p2"], M.WIDTH, 160)                    # dense 16-channel windows: [out][tap 10][in 16]
    for got, w in ((hi, o["W2h"]), (lo, o["W2l"])):
        dense = got.reshape(M.WIDTH, 10, 16)
        co = torch.arange(M.WIDTH)
        back = torch.stack([dense[co, :9, (co % 16) // M.CG * M.CG + ci] for ci in range(M.CG)], dim=1)
        assert torch.equal(back.reshape(M.WIDTH, M.CG, 3, 3), w) and float(dense.abs().sum()) == float(w.abs().sum())
        assert bool((dense[:, 9] == 0).all()) and bool((w[:, :, 2, 2] != 0).any())                      # the tenth tap slot: zeros, tap 8 itself is not
    p3 = d["p3"].reshape(8, 8, 4, 2, 64, 8).permute(0, 2, 1, 3, 4, 5).reshape(-1)                         # [wave][nj][ks][hi, lo][lane][8]
    hi, lo = _unfrag(p3, M.COUT, M.WIDTH)
    i = torch.arange(16)
    perm = torch.cat([64 * wv + (i >> 2) * 16 + nj * 4 + (i & 3) for wv in range(8) for nj in range(4)])
    assert torch.equal(hi, o["W3h"][perm]) and torch.equal(lo, o["W3l"][perm])
    assert torch.equal(d["bias"], torch.cat([o["b1"], o["b2"], o["b3"]]))
    # the input: hi plane, NaN past the last pixel; x_lo only as the lo half of in_mx, on the FP4 grid, no remainder of x_hi
    assert torch.equal(d["x"][:bm].float(), o["xh"]) and bool(torch.isnan(d["x"][bm:]).all())
    q, s = d["in_mx"][1, :rows * 256].view(rows, 256), d["in_mx"][1, rows * 256:].view(2, rows, 8)
    assert torch.equal(mx_dequant_fp4(q[:bm], s[:, :bm]), o["xl"].double())
    assert bool((q[bm:] == M.IN_FILL_BYTE).all()) and bool((s[:, bm:] == M.IN_FILL_BYTE).all())
    assert float((o["xl"] != 0).float().mean()) > 0.8 and bool((o["xh"].to(torch.float16).float() == o["xh"]).all())
    live = s[:, :bm]
    assert len(torch.unique(live)) >= 3 and bool((live[:, :, 1:] != live[:, :, :-1]).any()) and bool((live[:, 1:] != live[:, :-1]).any())
    qh, sh = d["in_mx"][0, :rows * 256].view(rows, 256), d["in_mx"][0, rows * 256:].view(2, rows, 8)
    assert float(mx_dequant_fp4(qh, sh).abs().min()) == 6.0 * 2 ** 13                                   # the half the kernel must not read


def test_splice_reproduces_the_shipped_packer_at_width_256():
    """fed the two halves of a coupled split, splice_fragments gives pack_bottleneck's bytes (32 groups of 8, 512 -> 256 -> 512)"""
    from vision_semantic_segmentation_amd.network import pack_bottleneck, split_f16
    g = torch.Generator().manual_seed(6)
    ws = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((M.WIDTH, M.CIN), (M.WIDTH, M.CG, 3, 3), (M.COUT, M.WIDTH))]
    his, los = zip(*[tuple(p.double() for p in split_f16(t)) for t in ws])
    assert all(bool((t != 0).any()) for t in los)
    for a, b, ref in zip(pack_bottleneck(*his, None, M.GROUPS), pack_bottleneck(*los, None, M.GROUPS), pack_bottleneck(*ws, None, M.GROUPS)):
        assert torch.equal(M.splice_fragments(a, b).view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("c", _SMALL, ids=M.case_id)
def test_mutations_are_caught(c):
    _, bufs = M.want(c)
    n = 0
    for mut in M.MUTATIONS:
        if not M.applicable(c, mut):
            continue
        if M.invisible(c, mut):
            assert M.same(M.evaluate(c, mut), bufs), (M.case_id(c), mut, "claimed invisible")
        else:
            assert not M.same(M.evaluate(c, mut), bufs), (M.case_id(c), mut)
            n += 1
    assert n >= 20


def test_every_mutation_applies_and_shows_somewhere():
    assert len(M.MUTATIONS) == 24
    for mut in M.MUTATIONS:
        assert any(M.applicable(c, mut) and not M.invisible(c, mut) for c in _SMALL), mut
    big = M.B2Case(1, *M.MANY)
    assert all(M.applicable(big, m) for m in M.MUTATIONS if m != "batch_halo")


def test_a_row_written_past_m_lands_in_the_fill_only():
    c = M.CASES[5]
    bm = M.geometry(c)["bm"]
    good, bad = M.evaluate(c), M.evaluate(c, "row_past_m")
    assert torch.equal(bad["out"][:bm], good["out"][:bm]) and not torch.equal(bad["out"][bm:], good["out"][bm:])
    for half in (0, 1):
        (q0, s0), (q1, s1) = M.unbundle(c, good["out_mx"], half), M.unbundle(c, bad["out_mx"], half)
        assert torch.equal(q0[:bm], q1[:bm]) and torch.equal(s0[:, :bm], s1[:, :bm]) and not torch.equal(q0[bm:], q1[bm:]) and not torch.equal(s0[:, bm:], s1[:, bm:])


def test_the_overflow_case_flags_the_four_tiles_around_its_pixel():
    c = M.B2Case(1, *M.MANY)
    g = M.geometry(c)
    n, py, px = M.overflow_pixel(c)
    assert py % M.TH == 0 and px % M.TW == 0 and 0 < py < c.H and 0 < px < c.W          # the corner where four tiles meet
    f = M.flagged_tiles(c)
    ty, tx = py // M.TH, px // M.TW
    assert f.nonzero().tolist() == [[n, ty - 1, tx - 1], [n, ty - 1, tx], [n, ty, tx - 1], [n, ty, tx]]
    assert int(M.flagged_rows(c).sum()) == 4 * M.TH * M.TW
    for t in (f[n].reshape(-1).nonzero().reshape(-1)).tolist():                         # at 256 CUs: neither first nor last of its workgroup
        assert t >= 256 and t + 256 < g["tiles"]
    d, base = M.overflow_inputs(c), M.device_inputs(c)
    row = (n * c.H + py) * c.W + px
    changed = (d["x"].view(torch.int16) != base["x"].view(torch.int16)).any(dim=1).nonzero().reshape(-1).tolist()
    assert changed == [row] and all(torch.equal(d[k], base[k]) for k in d if k != "x")
    assert float(d["x"][row].abs().max()) == 2048.0
