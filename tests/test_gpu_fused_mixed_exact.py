"""The two fusions of the default "mixed" plan that keep a split intermediate in LDS -- AVL_OP_DWPW in its mixed forms (k_dwpw<f16, 2>,
k_dwpw_x, k_dwpw_xs<false>, k_dwpw_xs<true>: csrc/seg_dwpw.hip) and AVL_OP_BOTTLENECK of layer1 (the eight k_bottleneck<CIN, DS, T1LO,
XLO, OLO>: csrc/seg_bottleneck.hip) -- each op ALONE through avl_seg_plan_* on exactly computable operands: every buffer the op owns
(hi plane, lo plane, fp32 logits, labels, with the fill around them) is compared for equality with the exact result rounded once.

Why.  test_gpu_mixed.py and test_gpu_bottleneck.py see these kernels through bars relative to max|ref| (6e-6, 4 * 2^-11 / sqrt(K), 3e-6,
3e-4, 1.5 * 2^-11) on Gaussian operands with coupled hi / lo weights.  Such a bar cannot see a wrong value on a few small outputs, a lo
plane that is no proper remainder, the rounding mode of a hi / lo split, one tap missing on one image edge, depthwise parameters of a
K-step used four steps late, or an element stored where nothing should be; DESIGN.md quotes what each deliberate mistake costs under those
bars.  Both kernels carry hand-counted `s_waitcnt vmcnt(N)` next to LDS-DMA: a stale tile gives plausible numbers that only equality sees.

tests/_fused_mixed_operands.py builds the cases (its docstring states what the kernels compute and the operand design: independent hi and
lo weight matrices spliced through the shipped packers, biases beyond 2048 on a quarter of the intermediate's channels so that the in-LDS
lo tiles are populated, everything a multiple of 1/8 below 2^24 units); tests/test_fused_mixed_operands_cpu.py checks every condition, the
dispatch claims and the teeth of the comparison without a GPU.

Which kernel a case reaches: every case names it, and the test checks the name against the host restatement of launch_dwpw's /
launch_bottleneck's dispatch on the op it is about to run.  All four DWPW kernels and all eight layer1 instantiations are reached
(profiles/fused_exact/ has the kernel trace).  The two 270 x 240 bottleneck cases need more tiles than the device has CUs: the test derives
the tiles per workgroup from multi_processor_count and FAILS below two (the cross-tile X prefetch, both X slots of the DS form).

Hardware observation (MI355X): every case was bit-equal on the first run; no expected value had to mirror an instruction beyond what the
operand module's docstring states (v_fma_mix / v_cvt_pk_f16_f32 / v_fma_mixlo_f16 round to nearest even, the f16 MFMA accumulates these
sums exactly).

No tolerance anywhere: bit equality."""
import pytest

import _fused_mixed_operands as M

pytestmark = pytest.mark.gpu


def _differences(case, name, got, want, live_rows, width):
    """which elements differ and by how much: the pattern tells an indexing bug from a rounding rule from a missing pass"""
    import torch
    a, b = (got.view(torch.int16), want.view(torch.int16)) if got.dtype == torch.float16 else (got, want)
    a, b, g2, w2 = (t.reshape(t.shape[0], -1) for t in (a, b, got, want))
    bad = (a != b).nonzero()
    rows, cols = bad[:, 0], bad[:, 1]
    diff = (g2.double() - w2.double()).abs()
    first = [(tuple(i.tolist()), float(g2[tuple(i)]), float(w2[tuple(i)])) for i in bad[:6]]
    return "%s %s: %d of %d differ (%d in rows past M = %d), max |diff| %g, rows %d..%d (image rows of %d: y %d..%d), columns %d..%d, first (index, got, want): %s" % (
        case, name, bad.shape[0], b.numel(), int((rows >= live_rows).sum()), live_rows, float(diff[torch.isfinite(diff)].max()), int(rows.min()), int(rows.max()),
        width, int(rows.min()) // width, int(rows.max()) // width, int(cols.min()), int(cols.max()), first)


def _compare(case, got, want, live_rows, width):
    import torch
    assert got.keys() == want.keys()
    wrong = [_differences(case, k, got[k], want[k], live_rows, width) for k in got
             if not torch.equal(got[k].view(torch.int16) if got[k].dtype == torch.float16 else got[k], want[k].view(torch.int16) if want[k].dtype == torch.float16 else want[k])]
    assert not wrong, "\n".join(wrong)
    assert M.same(got, want)


@pytest.mark.parametrize("c", M.DW_CASES, ids=M.dw_id)
def test_fused_depthwise_pointwise_mixed_exact(c, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    _, want = M.want_dw(c)
    g = M.dw_geometry(c)
    d = {k: v.to(cuda_device) for k, v in M.dw_device_inputs(c).items()}
    ptr = {"in": d["x"][0].data_ptr(), "in_lo": d["x"][1].data_ptr(), "weight": d["weight"].data_ptr(), "bias": d["bias"].data_ptr(), "params": d["params"].data_ptr()}
    if c.kernel == "cls":
        got = {"logits": torch.full((g["rows"], c.ncls), M.FILL_LOGIT, dtype=torch.float32, device=cuda_device),
               "labels": torch.full((g["rows"],), M.FILL_LABEL, dtype=torch.uint8, device=cuda_device)}
        ptr.update(wc=d["wc"].data_ptr(), bc=d["bc"].data_ptr(), logits=got["logits"].data_ptr(), labels=got["labels"].data_ptr())
    else:
        got = {k: torch.full((g["rows"], g["out_ld"]), M.FILL, dtype=torch.float16, device=cuda_device) for k in ("out", "out_lo")}
        ptr.update(out=got["out"].data_ptr(), out_lo=got["out_lo"].data_ptr())
    op = M.make_dw_op(c, ptr)
    assert M.dw_dispatch(op.w_split, bool(op.in_lo), bool(op.out_f32)) == c.kernel, "%s no longer reaches %s" % (M.dw_id(c), M.DW_KERNELS[c.kernel])
    _run_plan([op])
    _compare(M.dw_id(c), {k: v.cpu() for k, v in got.items()}, want, c.B * g["m"], g["ow"])


@pytest.mark.parametrize("c", M.BN_CASES, ids=M.bn_id)
def test_fused_bottleneck_mixed_exact(c, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    g = M.bn_geometry(c, torch.cuda.get_device_properties(cuda_device).multi_processor_count)
    if (c.H, c.W) == M.BN_MANY:
        assert g["tpw"] >= 2, "%s: %d tiles give %d per workgroup on this device: the case needs at least two" % (M.bn_id(c), g["tiles"], g["tpw"])
    _, want = M.want_bn(c)
    d = {k: v.to(cuda_device) for k, v in M.bn_device_inputs(c).items()}
    got = {k: torch.full((g["rows"], g["out_ld"]), M.FILL, dtype=torch.float16, device=cuda_device) for k in ("out", "out_lo")}
    ptr = {"in": d["x"][0].data_ptr(), "in_lo": d["x"][1].data_ptr(), "p1": d["p1"].data_ptr(), "p2": d["p2"].data_ptr(), "p3": d["p3"].data_ptr(),
           "bias": d["bias"].data_ptr(), "out": got["out"].data_ptr(), "out_lo": got["out_lo"].data_ptr()}
    op = M.make_bn_op(c, ptr)
    assert M.bn_dispatch(op.in_c, op.w_split, bool(op.in_lo), bool(op.out_lo)) == (c.cin, c.cin == 64, bool(c.t1lo), bool(c.xlo), bool(c.olo)), \
        "%s no longer reaches %s" % (M.bn_id(c), M.bn_kernel(c))
    _run_plan([op])
    _compare(M.bn_id(c), {k: v.cpu() for k, v in got.items()}, want, c.B * g["m"], c.W)
