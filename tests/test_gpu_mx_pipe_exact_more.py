"""k_gemm_mx_pipe on exactly computable operands, bit for bit: the address paths of its DMA producer that the cases of
tests/test_gpu_gemm_exact.py do not reach.

The producer keeps six running source pointers that move on by a constant per sub-step / per K macro-block and are set anew at
every tile switch and where the K loop passes from the first input to the second; strides and the planes of an operand's MX
bundle are derived from the operand's K and the bundle's base.  A case is (M, K1, K2, N, form, relu, kernel) and runs through
`_run_mx` of tests/test_gpu_gemm_exact.py (its docstring has the operand design and what is compared: every plane and scale slab the
op writes, and the sentinels around them; `kernel` is asserted against the library's route for the op that runs, and
tests/test_gemm_route_cpu.py walks this table without a GPU).

No tolerance anywhere: bit equality."""
import pytest

from test_gpu_gemm_exact import _run_mx

pytestmark = pytest.mark.gpu

CASES = [
    # a second input along K AND several tiles per workgroup (t256 = 384: tiles of 256 rows on 256 workgroups): the switch first ->
    # second input and the switch to the next tile (back to the first input) both run
    (12100, 512, 512, 2048, "trunk", True, "k_gemm_mx_pipe<1, 8, 0>"),
    # walking several tiles without a quantised output
    (12100, 1024, 0, 2048, "plain", False, "k_gemm_mx_pipe<0, 8, 0>"),
    # K = 2048, eight macro-blocks: layer4's K (the scale pointers advance eight times per tile); t256 = 192
    (5900, 2048, 0, 2048, "split", True, "k_gemm_mx_pipe<1, 8, 0>"),
    # 65 * 8 = 520 tiles of 128 rows on 256 workgroups (t256 = 264)
    (8300, 1024, 0, 2048, "trunk", True, "k_gemm_mx_pipe<1, 4, 1>"),
    # M a whole number of 256-row tiles: no ragged last tile (t256 = 23 * 8 = 184: 128-row tiles)
    (5888, 1024, 0, 2048, "hiq", False, "k_gemm_mx_pipe<1, 4, 1>"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%d+%d-%d-%s-%d" % c[:6])
def test_mx_pipe_exact_more(case, cuda_device):
    _run_mx(case, cuda_device)
