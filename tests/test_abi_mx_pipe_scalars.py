"""k_gemm_mx_pipe keeps its scalars in scalar registers: no SGPR spill traffic inside the software-pipelined stream, and no
more of it in the whole kernel than k_gemm_ring_mx had when the two shared one epilogue (77 lane reads in <1, 8>).

hipcc spills scalar registers into the lanes of a vector register (`v_writelane`) and reads them back one lane at a time
(`v_readlane`, each followed by wait states before a scalar use).  The pipe kernel used to hold every kernel argument across
its stream -- 128 spilled scalars, 308 lane reads between the first and the last MFMA and 804 in the epilogue.  Checked on the
disassembly of the BUILT libavl_hip.so (tools/kernel_notes.py), as tests/test_abi.py does."""
import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SO = os.path.join(ROOT, "vision_semantic_segmentation_amd", "libavl_hip.so")
LLVM_BIN = "/opt/rocm/lib/llvm/bin"

MAX_LANE_READS = 77         # k_gemm_ring_mx<1, 8> before this test was written


def _disassembly():
    if not os.path.exists(SO):
        pytest.fail("libavl_hip.so is not built: run __graft_entry__.build()")
    if not os.path.exists(os.path.join(LLVM_BIN, "llvm-objdump")):
        pytest.skip("ROCm LLVM tools not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_notes
    return kernel_notes.disassembly(SO, "k_gemm_mx_pipe")


def test_mx_pipe_has_no_lane_traffic_in_the_stream_and_little_elsewhere():
    dis = _disassembly()
    assert len(dis) == 4, sorted(dis)
    for sym, ins in dis.items():
        mf = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
        assert len(mf) >= 64, sym
        stream = ins[mf[0]:mf[-1] + 1]
        lane = [l for l in stream if l.startswith(("v_readlane", "v_writelane"))]
        assert not lane, "%s: %d lane reads / writes between the first and the last MFMA, e.g. %s" % (sym, len(lane), lane[:3])
        reads = sum(l.startswith("v_readlane") for l in ins)
        assert reads <= MAX_LANE_READS, "%s: %d v_readlane in the kernel (at most %d)" % (sym, reads, MAX_LANE_READS)


def test_mx_pipe_m0_belongs_to_the_lds_dma_alone():
    """glds16_saddr_m0 (csrc/seg_types.h) writes M0 without saving and restoring it.  That is sound only while hipcc keeps no M0
    value of its own in these kernels (it answers the clobber with "reserved registers ... may not be preserved", and the
    Makefile silences that warning for seg_gemm.hip).  So: every instruction of k_gemm_mx_pipe that names M0 is one of the
    statement's own two -- `s_mov_b32 m0, <sgpr>` and the `global_load_lds_*` it feeds -- each write is followed by its DMA
    with only the wait state between them, and each DMA is preceded by its write."""
    dis = _disassembly()
    for sym, ins in dis.items():
        others = [l for l in ins if "m0" in l.replace(",", " ").split() and not l.startswith("s_mov_b32 m0,")]
        assert not others, "%s: M0 used outside the LDS-DMA statement: %s" % (sym, others[:3])
        dma = [i for i, l in enumerate(ins) if l.startswith("global_load_lds")]
        wr = [i for i, l in enumerate(ins) if l.startswith("s_mov_b32 m0,")]
        assert dma and len(dma) == len(wr), (sym, len(dma), len(wr))
        for w, d in zip(wr, dma):
            assert d == w + 2 and ins[w + 1].startswith("s_nop"), "%s: %s" % (sym, ins[w:w + 3])
