"""The row-aligned MX grouped 3x3 (k_gconv_mfma<f16, 2, 2, false, true>) without a GPU: the launcher's selection rule and the kernel's LDS
layout restated (csrc/seg_gconv_mfma.hip: ROWS_PITCH, ROWS_IN_TH, ROWS_TILE_BYTES, the tap offsets), and the cases of
test_gpu_gconv_mx_rows.py built on the host."""
import ctypes as C

import pytest

import _gconv_mixed_operands as M
import test_gpu_gconv_mx_rows as R

PITCH, IN_TH, TW = 40, 6, 32
F16_TILE, QT, ST = IN_TH * PITCH * 128, 4096, 1024            # f16 tile; one FP4 tile (256 pixels x 16 B); one plane's scale dwords
QBASE, SBASE = F16_TILE, F16_TILE + 4 * QT
TILE_BYTES = SBASE + 2 * ST

# conv2 of layer3.0 .. layer3.5 and layer4.0 .. layer4.2 of the 1080 x 1920 plan (resnext50_32x4d, output stride 8: 135 x 240 pixels, stride 1,
# dilations 1, 2 x 5 | 2, 4 x 2, widths 512 | 1024), as the mixed plan emits them: AVL_MX_IN_LO, out_mx + AVL_MX_OUT_LO
PLAN_1080P = [M.Case(2, False, True, "mx_f32lo", 1, 135, 240, 512, 1, d, 2, 0) for d in (1, 2, 2, 2, 2, 2)] + \
             [M.Case(2, False, True, "mx_f32lo", 1, 135, 240, 1024, 1, d, 2, 0) for d in (2, 4, 4)]


def test_the_rule_selects_the_nine_conv2_shapes_of_the_1080p_plan():
    assert len(PLAN_1080P) == 9
    for c in PLAN_1080P:
        assert M.pick_th(c, 256)["th"] == 4 and R.rows_path(c), c


def test_the_rule_selects_no_stride_2_and_no_split_weight_case():
    for c in M.CASES:
        if c.s == 2 or c.ws == 1:
            assert not R.rows_path(c), M.case_id(c)
    # ... and every MX case at stride 1 of the existing exact test goes through the new kernel
    assert sum(R.rows_path(c) for c in M.CASES) == sum(c.ws == 2 and c.s == 1 for c in M.CASES) >= 10


def test_two_buffers_fit_lds():
    assert TILE_BYTES == 48 * 1024 and 2 * TILE_BYTES <= 160 * 1024
    assert PITCH % 8 == 0 and PITCH >= TW + 2
    # the DMA groups cover the f16 tile exactly (30 groups of 1 KB in four rounds of eight waves), the FP4 groups of 64 pixels the 240 pixels
    assert IN_TH * (PITCH // 8) * 1024 == F16_TILE and 3 * 8 < IN_TH * (PITCH // 8) <= 4 * 8
    assert -(-IN_TH * PITCH // 64) * 1024 == QT and -(-IN_TH * PITCH // 64) * 256 == ST
    # pixel -> row by one multiply: exact for every pixel of the four 64-pixel groups
    assert all((pix * 1639) >> 16 == pix // PITCH for pix in range(256))


def test_every_immediate_offset_fits_the_ds_offset_field_and_stays_in_its_tile():
    imm_f16 = [(2 * j + r) * PITCH * 128 for j in range(2) for r in range(3)]
    imm_q = [pl * 2 * QT + 2 * j * PITCH * 16 for pl in range(2) for j in range(2)]
    imm_s = [pl * ST + 2 * j * PITCH * 4 for pl in range(2) for j in range(2)]
    assert max(imm_f16) == 20480 and max(imm_f16 + imm_q + imm_s) < 65536
    # lane bases: wave row (part >> 1) in 0..1, column sx + c in 0..33, FP4 tap row t / 3 and column t % 3 of tap t = min(4 g + kq, 8)
    for row0 in range(2):
        for sx in range(32):
            for c in range(3):
                base = (row0 * PITCH + sx + c) * 128 + 7 * 16
                assert all(base + i + 16 <= F16_TILE for i in imm_f16)
            for t in range(9):
                pix = (row0 + t // 3) * PITCH + sx + t % 3
                for win in range(2):
                    assert all(QBASE <= QBASE + win * QT + pix * 16 + i and QBASE + win * QT + pix * 16 + i + 16 <= SBASE for i in imm_q)
                assert all(SBASE + pix * 4 + 3 + i < TILE_BYTES for i in imm_s)
                assert pix + 2 * PITCH < IN_TH * PITCH            # the second sub-tile's pixel lies inside the 240


@pytest.mark.parametrize("c", R.CASES, ids=M.case_id)
def test_case_builds_and_reaches_the_row_aligned_kernel(c):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import AvlSegOp
    assert M.accepted(c)
    t = M.pick_th(c, 256)
    assert t["th"] == 4 and (t["nj"], t["tpw"]) == (c.nj, c.tpw) and R.rows_path(c), (M.case_id(c), t)
    if c == R.WALK:
        assert t["nsp"] == 20 and t["nslots"] == 16 and M.walk_crosses_columns(t) and R.walk_crosses_classes(t)
    v, bufs = M.want(c)                                          # asserts the operand conditions while it builds
    g = M.geometry(c)
    assert v.shape == (g["m"], c.C) and g["rows"] > g["m"]
    plan = C.c_void_p()
    assert _lib.lib().avl_seg_plan_create((AvlSegOp * 1)(M.shape_op(c)), 1, C.byref(plan)) == 0
    _lib.lib().avl_seg_plan_destroy(plan)
