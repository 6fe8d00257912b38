"""AVL_OP_MAXPOOL, AVL_OP_BILINEAR, the one-side split AVL_OP_DWCONV (k_dwconv_split) and the split AVL_OP_STEM (k_stem_mfma<f16, false,
true, F32IN>), each ALONE through avl_seg_plan_* on exactly computable operands: every output buffer -- a column slice of a wider buffer
with rows past the last pixel, all filled with a sentinel -- is compared for equality, as int16 / int32, with the exact result rounded
once.  The inputs carry NaN (max-pool: +Inf, which fmaxf does not drop) in the columns and rows the op must not read.

Why.  These kernels sit between the GEMMs and convolutions of every plan and were seen only through Gaussian operands and bars relative
to max|ref|: a max-pool fed post-ReLU values cannot tell 0 padding from -Inf, the split pool and the split stem were compared as
hi + lo at 3e-6 (a dropped Wl.xh pass, a truncated lo plane or an independent maximum of the two planes sits under it), and the lo plane
of a split depthwise input contributes less than the f16 bar it was held to.  tests/_pool_resample_operands.py builds the cases (its
docstring states what each kernel computes and the operand design); tests/test_pool_resample_operands_cpu.py checks every operand
condition and that each deliberate mistake changes an expected byte.

One test has a tolerance: the bilinear coordinate rule at scales that are no power of two, against float64 interpolation with the
coordinate of the stated rule (f = float32(float32(scale) * float32(dst)), corner int(f), weight f - corner).  The bar is derived, per
element: 8 * 2^-24 * max|four corners| (hx and hy carry one rounding each; the five-operation lerp gives gamma_5, with or without FMA),
plus 2^-22 |ref| for a split output pair, compared as hi + lo.  A coordinate contracted into one FMA exceeds it in 10 % .. 66 % of the
elements (CPU test)."""
import pytest

import _pool_resample_operands as M
from test_gpu_exact_ops import _same

pytestmark = pytest.mark.gpu


def _run(fam, c, dev):
    """the case's op alone -> {"out"[, "out_lo"]} on the host, whole buffers"""
    import torch
    from test_gpu_ops import _run_plan
    _, cid, _, _, want, _, inputs, make_op = M.FAMILIES[fam]
    bufs, _ = want(c)
    d = {k: v.to(dev) for k, v in inputs(c).items()}
    got = {k: torch.full(t.shape, M.FILL, dtype=t.dtype, device=dev) for k, t in bufs.items()}
    ptr = {k: v.data_ptr() for k, v in list(d.items()) + list(got.items())}
    _run_plan([make_op(c, ptr)])
    return {k: v.cpu() for k, v in got.items()}, bufs


def _check(fam, c, dev):
    got, want = _run(fam, c, dev)
    cid = M.FAMILIES[fam][1](c)
    for k in want:                                             # the values first (the report then names them), then the bit patterns (-0.0)
        _same(got[k], want[k], "%s %s %s" % (fam, cid, k))
        _same(M.bits(got[k]), M.bits(want[k]), "%s %s %s as integers" % (fam, cid, k))
    assert M.same(got, want)


@pytest.mark.parametrize("c", M.MP_CASES + M.MP_SPLIT_CASES, ids=M.mp_id)
def test_maxpool_exact(c, cuda_device):
    """values of both signs with whole windows negative and some -0.0; split: the output pair is the pair of the window's float64 arg-max"""
    _check("maxpool", c, cuda_device)


@pytest.mark.parametrize("c", M.BL_CASES, ids=M.bl_id)
def test_bilinear_exact(c, cuda_device):
    """power-of-two scales: every weight is exact and the result is the exact value rounded once, in every plane combination"""
    _check("bilinear", c, cuda_device)


@pytest.mark.parametrize("c", M.DW_CASES, ids=M.dw_id)
def test_depthwise_one_side_split_exact(c, cuda_device):
    _check("dwconv_split", c, cuda_device)


@pytest.mark.parametrize("c", M.ST_CASES, ids=M.st_id)
def test_split_stem_exact(c, cuda_device):
    """fp32 planes: acc = Wh.xh + Wl.xh + Wh.xl on independent hi and lo weights; uint8: one-hot weights, the kernel's table mirrored"""
    _check("stem_split", c, cuda_device)


@pytest.mark.parametrize("c", M.BL_TOL_CASES, ids=M.bl_id)
def test_bilinear_coordinate_rule(c, cuda_device):
    """Gaussian inputs at 266 -> 1080 and 17 -> 68; |got - ref| <= 8 * 2^-24 * max|four corners| (+ 2^-22 |ref| for the split pair) per element"""
    import torch
    got, _ = _run_tol(c, cuda_device)
    ref, bar = M.bl_tolerance(c)
    err = (got - ref).abs()
    cm = M.corner_max(M.bl_value(M.bl_operands(c)), c.OH, c.OW)
    over = err > bar
    print("%s: worst %.2f u max|corner|, over the bar in %d of %d elements (%.1f %%)" % (
        M.bl_id(c), float((err / (M.U * cm)).max()), int(over.sum()), over.numel(), 100 * float(over.double().mean())))
    assert bool(torch.isfinite(got).all())
    assert not bool(over.any()), "%s: %d of %d elements over the bar, worst %.2f u max|corner|" % (
        M.bl_id(c), int(over.sum()), over.numel(), float((err / (M.U * cm)).max()))


def _run_tol(c, dev):
    """-> (the output as float64 [B][OH][OW][C], hi + lo for the split form; the raw buffers); the fill around the slice is asserted here"""
    import torch
    from test_gpu_ops import _run_plan
    dt = M._dtype(M.bl_prec(c))
    d = {k: v.to(dev) for k, v in M.bl_device_inputs(c).items()}
    rows = c.B * c.OH * c.OW
    got = {k: torch.full((rows + M.TAIL, c.C + M.OUT_PAD), M.FILL, dtype=dt, device=dev) for k in (("out", "out_lo") if c.form == "split" else ("out",))}
    _run_plan([M.bl_make_op(c, {k: v.data_ptr() for k, v in list(d.items()) + list(got.items())})])
    got = {k: v.cpu() for k, v in got.items()}
    total = 0.0
    for t in got.values():
        assert bool((t[rows:] == M.FILL).all()) and bool((t[:, :M.OUT_OFF] == M.FILL).all()) and bool((t[:, M.OUT_OFF + c.C:] == M.FILL).all())
        total = total + t[:rows, M.OUT_OFF:M.OUT_OFF + c.C].double()
    return total.reshape(c.B, c.OH, c.OW, c.C), got
