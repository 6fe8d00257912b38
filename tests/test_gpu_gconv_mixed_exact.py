"""The split and MX forms of the grouped 3x3 on the matrix cores (k_gconv_mfma<f16, 1 | 2, NJ, XS>, csrc/seg_gconv_mfma.hip), each op
ALONE through avl_seg_plan_* on exactly computable operands: every byte the op may write -- the hi plane, the lo plane, both FP4
planes of out_mx and both scale slabs, with the fill around them -- is compared for equality with the float64 result rounded once.

Why.  test_gpu_mixed.py::test_mx_grouped_conv sees the WS = 2 form through a bar of 0.3 * 2^-11 of max|ref| on Gaussian operands: a
whole missing FP4 correction pass clears it by a factor of 1.4 .. 1.7 only, one wrong tap or an un-zeroed halo sits ON it, and a wrong
scale byte of one tap group or one window's scale select passes.  The split forms (test_split_grouped_conv, test_gpu_fullsplit.py)
compare hi + lo on coupled operands: neither the hi / lo split, nor the rounding of the hi plane, nor which weight block meets which
input plane is pinned.  The same weakness was removed for the GEMMs (test_gpu_gemm_exact.py) and for WS = 0 (test_gpu_exact_ops.py).

tests/_gconv_mixed_operands.py builds the cases (its docstring has the operand design: decoupled matrices per term, per-block scale
factors of {1/2, 1, 2}, w_mx spliced through the shipped packer, the exactness bound, the bias, the expected buffers);
tests/test_gconv_mixed_operands_cpu.py checks every condition and the teeth of the comparison without a GPU.

Which instantiation a case reaches.  There is no route query for this op: _gconv_mixed_operands.pick_th restates the launcher's
gconv_pick_th, every case names its (WS, XS, NJ) and its tiles per workgroup, and the test re-checks the claim with the device's
multi_processor_count before it runs -- it FAILS if a case no longer reaches what it names.  Reached here:
    k_gconv_mfma<f16, 2, 1>         MX at stride 2 (two four-row MX tiles do not fit 160 KB)
    k_gconv_mfma<f16, 2, 2>         MX at stride 1, plain and combed (dilation 2, 4), a walk of three tiles, a batch of two
    k_gconv_mfma<f16, 1, 1>         split weights at stride 2 with dilation 2
    k_gconv_mfma<f16, 1, 2>         split weights: stride 1, stride 2, comb, a walk of three tiles
    k_gconv_mfma<f16, 1, 4>         split weights on the eight-row tile (97 x 33 at C = 1024, and the dilation-4 comb at 19 x 67)
    k_gconv_mfma<f16, 1, 2, true>   split weights and a split input: plain, combed, a walk of three tiles
k_gconv_mfma<f16, 1, 1, true> (split input on the two-row tile) is instantiated but UNREACHABLE: at stride 2 two split-input tiles of
even two rows exceed 160 KB and validate_gconv_mfma refuses the op, at stride 1 the four-row tile always fits (dilation > 1 combs, tap
distance 1) and the two-row tile is taken only when nothing else fits (test_the_two_row_tile_with_a_split_input_is_unreachable).
k_gconv_mfma<f16, 2, 4> is not instantiated.

Three further cases (M.FRAC_CASES) carry biases with a 2^-10 part, still exact in fp32: only there does it show in the bytes whether
the Q4(lo) half was quantised from the fp32 difference (AVL_MX_OUT_LO) or from the stored f16 lo plane (out_lo).

Hardware observation (MI355X): v_mfma_scale_f32_16x16x128_f8f6f4 accumulates this kernel's K layout (four taps x 32 channels per
instruction, the third instruction three quarters zero) exactly, into the accumulator the f16 MFMAs use: every case is bit-equal to
the host's result rounded once to nearest even, and the epilogue's quantiser agrees with network.mx_quant_fp4 byte for byte
(DESIGN.md, section 4).  The file takes about five seconds.

No tolerance anywhere: bit equality."""
import pytest

import _gconv_mixed_operands as M

pytestmark = pytest.mark.gpu


def _differences(c, name, got, want):
    """which elements differ and by how much: the pattern tells an indexing bug from a rounding rule from a scale mix-up"""
    import torch
    g = M.geometry(c)
    a, b = (got.view(torch.int16), want.view(torch.int16)) if got.dtype == torch.float16 else (got, want)
    bad = (a != b).nonzero()
    past = int((bad[:, -2] >= g["m"]).sum()) if bad.shape[1] >= 2 else 0
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]]
    rows, cols = bad[:, -2], bad[:, -1]
    diff = (got.double() - want.double()).abs()
    return "%s %s: %d of %d differ (%d in rows past M = %d), max |diff| %g, rows %d..%d (image rows of %d: y %d..%d), columns %d..%d, first (index, got, want): %s" % (
        M.case_id(c), name, bad.shape[0], b.numel(), past, g["m"], float(diff[torch.isfinite(diff)].max()) if bad.shape[0] else 0.0,
        int(rows.min()), int(rows.max()), g["ow"], int(rows.min()) % (g["oh"] * g["ow"]) // g["ow"], int(rows.max()) % (g["oh"] * g["ow"]) // g["ow"],
        int(cols.min()), int(cols.max()), first)


def _views(c, bufs):
    """the buffers as named 2-d / 3-d pieces: planes, FP4 planes and scale slabs of both halves"""
    g = M.geometry(c)
    rows, C = g["rows"], c.C
    v = {"out": bufs["out"], "out_lo": bufs["out_lo"]}
    if C % 256 == 0:
        for half, part in ((0, "hi"), (1, "lo")):
            b = bufs["out_mx"][half]
            v["out_mx Q4(%s) plane" % part] = b[:rows * (C // 2)].view(rows, C // 2)
            v["out_mx Q4(%s) scales [slab][row][8]" % part] = b[rows * (C // 2):].view(C // 256, rows, 8)
    return v


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_grouped_conv_mixed_exact(c, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes
    t = M.pick_th(c, torch.cuda.get_device_properties(cuda_device).multi_processor_count)
    assert (t["nj"], t["tpw"]) == (c.nj, c.tpw), "%s no longer reaches what it names on this device: %s" % (M.case_id(c), t)
    assert c.tpw < 3 or M.walk_crosses_columns(t)
    _, want = M.want(c)
    g = M.geometry(c)
    d = {k: v.to(cuda_device) for k, v in M.device_inputs(c).items()}
    f16 = torch.float16
    got = {"out": torch.full((g["rows"], c.C), M.FILL, dtype=f16, device=cuda_device),
           "out_lo": torch.full((g["rows"], c.C), M.FILL, dtype=f16, device=cuda_device),
           "out_mx": torch.full((2, mx_bundle_bytes(g["rows"], c.C) if c.C % 256 == 0 else 0), M.FILL_BYTE, dtype=torch.uint8, device=cuda_device)}
    ptr = {"in": d["planes"][0].data_ptr(), "in_lo": d["planes"][1].data_ptr(), "weight": d["weight"].data_ptr(), "bias": d["bias"].data_ptr(),
           "out": got["out"].data_ptr(), "out_lo": got["out_lo"].data_ptr(), "out_mx": got["out_mx"].data_ptr()}
    if c.ws == 2:
        ptr["w_mx"], ptr["in_mx"] = d["w_mx"].data_ptr(), d["in_mx"].data_ptr()
    _run_plan([M.make_op(c, ptr)])
    got = {k: v.cpu() for k, v in got.items()}
    gv, wv = _views(c, got), _views(c, want)
    wrong = [_differences(c, name, gv[name], wv[name]) for name in gv if not torch.equal(
        gv[name].view(torch.int16) if gv[name].dtype == f16 else gv[name], wv[name].view(torch.int16) if wv[name].dtype == f16 else wv[name])]
    assert not wrong, "\n".join(wrong)
    assert M.same(got, want)
