"""The row-aligned MX grouped 3x3 (k_gconv_mfma<f16, 2, 2, false, true>, csrc/seg_gconv_mfma.hip): the launcher takes it for w_split = 2 at
stride 1 with tap distance 1 inside LDS (dilation 1 or the comb) on the four-row tile.  Its LDS tile is 6 rows of 40 pixels (34 used), it is
staged by rows, the taps are read at lane bases + compile-time offsets, and the tile indices are counters advanced in walk order.

The ws = 2, s = 1 cases of test_gpu_gconv_mixed_exact.py reach this kernel by themselves.  The cases here aim at what is new in it:

    narrow image         5 x 3: the image is narrower than one 8-pixel DMA group (every group clamps on both sides); 2 row tiles, the last
                         with one live row
    ragged tiles         9 x 39: the second tile column is 7 pixels wide, its staging reads past the right edge and the pitch padding
                         (columns 34 .. 39) clamps too; 3 row tiles
    batch of two         the ragged shape twice
    comb, dilation 2     13 x 71: residue grids of 7 x 36, 7 x 35, 6 x 36, 6 x 35 on one tile grid (tiles_y of the largest)
    comb, dilation 4     9 x 70: 16 classes of 3 x 18 and smaller, no lo correction
    walk across classes  37 x 45 at C = 1024, dilation 2: 5 tiles per class, 20 tiles on 16 slots -- a run of two goes from the last tile
                         of one residue class to the first of the next: the counters' carry through ty -> tx -> class

Every byte the op may write is compared for equality with the float64 result rounded once (_gconv_mixed_operands.want): both planes, both
FP4 planes, both scale slabs and the fill around them, exactly as test_gpu_gconv_mixed_exact.py does it (its test body runs the case).  No
tolerance.  tests/test_gconv_mx_rows_cpu.py checks without a GPU that the cases build, reach the four-row tile and the fast path."""
import pytest

import _gconv_mixed_operands as M

pytestmark = pytest.mark.gpu

CASES = [
    M.Case(2, False, True, "mx_f32lo", 1, 5, 3, 256, 1, 1, 2, 1),          # narrow image
    M.Case(2, False, True, "mx_f32lo", 1, 9, 39, 256, 1, 1, 2, 1),         # ragged tiles
    M.Case(2, False, True, "mx_f32lo", 2, 9, 39, 256, 1, 1, 2, 1),         # batch of two
    M.Case(2, False, True, "mx_lo", 1, 13, 71, 256, 1, 2, 2, 1),           # comb, dilation 2
    M.Case(2, False, False, "mx_f32lo", 1, 9, 70, 256, 1, 4, 2, 1),        # comb, dilation 4
    M.Case(2, False, True, "mx_f32lo", 1, 37, 45, 1024, 1, 2, 2, 2),       # walk across classes
]
WALK = CASES[5]


def rows_path(c, cus=256):
    """the launcher's rule for the row-aligned kernel (launch_gconv_typed): MX, stride 1, tap distance 1 inside LDS (these cases pad by their
    dilation, so dilation > 1 at stride 1 is the comb), the four-row tile, no lo input plane"""
    t = M.pick_th(c, cus)
    return c.ws == 2 and not c.xs and c.s == 1 and (c.d == 1 or t["comb"]) and t["th"] == 4


def walk_crosses_classes(t):
    """a workgroup's run of tiles goes from the last tile of one residue class to the first tile of the next"""
    per, cls = t["tpw"], t["tiles_x"] * t["tiles_y"]
    return any((slot * per) // cls != (min(t["nsp"], (slot + 1) * per) - 1) // cls for slot in range(t["nslots"]) if slot * per < t["nsp"])


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_mx_rows_exact(c, cuda_device):
    import torch
    import test_gpu_gconv_mixed_exact as E
    cus = torch.cuda.get_device_properties(cuda_device).multi_processor_count
    t = M.pick_th(c, cus)
    assert t["th"] == 4 and rows_path(c, cus), "%s does not reach the row-aligned kernel on this device: %s" % (M.case_id(c), t)
    if c == WALK:
        assert t["tpw"] == 2 and M.walk_crosses_columns(t) and walk_crosses_classes(t), t
    E.test_grouped_conv_mixed_exact(c, cuda_device)          # runs the op alone, compares every buffer bit for bit
