"""The ring GEMM's EXT instantiations (strided input rows, a second destination, both in one op) run ALONE through avl_seg_plan_* on
exactly computable operands: every byte of both destinations' two planes is compared with the float64 result rounded once.

tests/_ring_ext_operands.py builds the cases (its docstring has the operand design; tests/test_exact_operands_cpu.py checks the
operand conditions and that the comparison has teeth, without a GPU).  What differs from tests/test_gpu_fused_passes.py: the
reference is the host's float64 product, not another GPU kernel, and the multi-tile cases have more tiles than the grid's 256
workgroups, so workgroups walk a second tile (in two cases every workgroup does) -- the hand-over `pt += nwg; set_tile(pt)` in
issue_part, the per-tile choice of destination in the epilogue and init_acc(t + nwg) all run, with the destination CHANGING
between a workgroup's consecutive tiles wherever 256 % ntiles != 0.

"strided + second destination in one op" (validate_gemm admits it) is tested here as working.

No tolerance anywhere: bit equality."""
import ctypes as C

import pytest

import _ring_ext_operands as R

pytestmark = pytest.mark.gpu

REPEATS = 80        # the race screen's relaunches (test_ring_gemm_with_residual_repeats_under_load's count)


def _plan(c, cuda_device, fill=R.FILL, bias=None, more_ops=()):
    """-> (plan handle, the two destination buffers on the device, whatever must stay alive); fill = the sentinel around the
    output, bias = another bias vector, more_ops = ops appended to the plan"""
    import torch
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp, gemm_route
    g = R.geometry(c)
    nsub = R.MODES[c.mode][1]
    a = R.device_input(c).to(cuda_device)
    w, b = (t.to(cuda_device) for t in R.device_weights(c, bias))
    dt = a.dtype
    out = torch.full((2, g["out_rows"], g["ld1"]), fill, dtype=dt, device=cuda_device)
    out2 = torch.full((2, g["out_rows"], g["ld2"]), fill, dtype=dt, device=cuda_device)
    op = R.shape_op(c, 16)
    op.in_, op.weight, op.bias = a[0].data_ptr(), w.data_ptr(), b.data_ptr()
    if nsub == 3:
        op.in_lo = a[1].data_ptr()
    op.out = out[0, :, R.COL:].data_ptr()
    if c.lo1:
        op.out_lo = out[1, :, R.COL:].data_ptr()
    if c.n_split:
        op.out2, op.out2_ld, op.n_split = out2[0].data_ptr(), g["ld2"], c.n_split
        if c.lo2:
            op.out2_lo = out2[1].data_ptr()
    # the kernel the case is here for, asked of the library for the very op that runs (the table: R.INSTANTIATION)
    assert R.instantiation(gemm_route(op)) == R.INSTANTIATION[(c.mode, R.claimed_variant(c))], R.case_id(c)
    ops = [op] + list(more_ops)
    plan = C.c_void_p()
    _lib.check(_lib.lib().avl_seg_plan_create((AvlSegOp * len(ops))(*ops), len(ops), C.byref(plan)), "avl_seg_plan_create")
    return plan, {"out": out, "out2": out2}, (a, w, b)


def _check(c, got, want, what=""):
    import torch
    g = R.geometry(c)
    for name in ("out", "out2"):
        for p, plane in enumerate(("hi", "lo")):
            a, b = got[name][p].cpu().view(torch.int16), want[name][p].view(torch.int16)
            if not torch.equal(a, b):
                bad = (a != b).nonzero()
                rows_past_m = int((bad[:, 0] >= g["M"]).sum())
                raise AssertionError("%s%s, %s %s plane: %d elements differ (%d of them in rows past M = %d), first at row %d column %d: got %r, want %r" % (
                    what, R.case_id(c), name, plane, bad.shape[0], rows_past_m, g["M"], int(bad[0, 0]), int(bad[0, 1]),
                    float(got[name][p][bad[0, 0], bad[0, 1]]), float(want[name][p][bad[0, 0], bad[0, 1]])))


def _run_case(c, cuda_device, repeats=0):
    import torch
    from vision_semantic_segmentation_amd import _lib
    _, want = R.want(c)
    plan, got, keep = _plan(c, cuda_device)
    try:
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().avl_seg_plan_run(plan, s), "avl_seg_plan_run")
        torch.cuda.synchronize()
        _check(c, got, want)                                   # the FIRST launch against the exact expectation
        if repeats:
            first = {k: v.clone() for k, v in got.items()}
            snaps = [{k: torch.empty_like(v) for k, v in got.items()} for _ in range(4)]
            for i in range(repeats):                            # back to back, copies in between: the same bytes every time
                _lib.lib().avl_seg_plan_run(plan, s)
                for k in got:
                    snaps[i % 4][k].copy_(got[k])
                if i % 4 == 3:
                    torch.cuda.synchronize()
                    for sn in snaps:
                        for k in got:
                            assert torch.equal(sn[k].view(torch.int16), first[k].view(torch.int16)), \
                                "%s: %s of launch ~%d differs from the first one" % (R.case_id(c), k, i)
    finally:
        _lib.lib().avl_seg_plan_destroy(plan)
    del keep


# Which instantiation a case reaches: k_gemm_ring<R.INSTANTIATION[(mode, R.variant(case))]> (_plan asserts it on the op that runs):
#   f16   wl2  k_gemm_ring<f16,  4, 2, 4, 3, 1, 0, 3, true>        f16   wl3  k_gemm_ring<f16,  2, 4, 8, 2, 1, 0, 2, true>
#   bf16  wl2  k_gemm_ring<bf16, 4, 2, 4, 3, 1, 0, 3, true>        bf16  wl3  k_gemm_ring<bf16, 2, 4, 8, 2, 1, 0, 2, true>
#   w2    wl2  k_gemm_ring<f16,  4, 2, 4, 3, 2, 1, 3, true>        w2    wl3  k_gemm_ring<f16,  2, 4, 8, 3, 2, 1, 2, true>  (AST = 2)
#   split wl2  k_gemm_ring<f16,  4, 2, 4, 3, 3, 1, 3, true>        split wl3  k_gemm_ring<f16,  2, 4, 8, 2, 3, 1, 2, true>
# (wl2 = 256 x 128 tiles, wl3 = 256 x 256; w2 = NSUB 2, split = NSUB 3.)  Each list below holds all eight
# (test_ring_ext_cases_reach_what_they_claim asserts it); the case id names mode and w_layout.
@pytest.mark.parametrize("c", R.SMALL_STRIDED, ids=R.case_id)
def test_strided_rows_exact(c, cuda_device):
    """reference: the float64 product over the sub-sampled pixels x[img, ::s, ::s]; the skipped pixels hold NaN"""
    _run_case(c, cuda_device)


@pytest.mark.parametrize("c", R.SMALL_TWIN, ids=R.case_id)
def test_second_destination_exact(c, cuda_device):
    """columns [0, n_split) in out, the rest in out2, with out2_lo set and NULL"""
    _run_case(c, cuda_device)


@pytest.mark.parametrize("c", R.SMALL_BOTH, ids=R.case_id)
def test_strided_rows_and_second_destination_in_one_op_exact(c, cuda_device):
    _run_case(c, cuda_device)


# mtiles = 86 (M = 21797 or 21798 rows of 256-row tiles, the last ragged); ntiles and the totals:
#   N = 384 on 256 x 128 tiles: ntiles = 3, total = 258 > 256, 256 % 3 = 1 -> a workgroup's tiles t, t + 256 differ in destination
#   N = 768 on 256 x 256 tiles: ntiles = 3, total = 258 > 256, 256 % 3 = 1
#   N = 512 on 256 x 128 tiles: ntiles = 4, total = 344 > 256, 256 % 4 = 0 -> the destination never changes
# and mtiles = 171 (M = 43557) in the last two: ntiles = 3, total = 513 > 2 * 256, 256 % 3 = 1 -> EVERY workgroup walks two tiles
# (the comments in R.MULTI_TILE_CASES say which case is which; test_ring_ext_cases_reach_what_they_claim asserts the counts)
@pytest.mark.parametrize("c", R.MULTI_TILE_CASES, ids=R.case_id)
def test_several_tiles_per_workgroup_exact_and_repeatable(c, cuda_device):
    mt, nt = R.tiles(c)
    assert mt * nt > 256
    _run_case(c, cuda_device, repeats=REPEATS)
