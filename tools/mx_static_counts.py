"""Static instruction counts of the MX GEMM kernels of a built libavl_hip.so: lane reads / writes (SGPR spills),
and the mix of scalar, vector and matrix instructions in the stream (first to last MFMA) and behind it (the epilogue).

    python3 tools/mx_static_counts.py [path/to/libavl_hip.so]
"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_notes as kn  # noqa: E402


def mix(ins):
    c = dict(total=len(ins), scalar=0, vector=0, mfma=0, readlane=0, writelane=0, s_nop=0, lds_dma=0, branch=0, addr64=0, s_load=0)
    for l in ins:
        op = l.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["vector"] += 1
        elif op.startswith("s_"):
            c["scalar"] += 1
        c["readlane"] += op.startswith("v_readlane")
        c["writelane"] += op.startswith("v_writelane")
        c["s_nop"] += op == "s_nop"
        c["lds_dma"] += op.startswith("global_load_lds")
        c["branch"] += op.startswith(("s_cbranch", "s_branch"))
        c["addr64"] += op.startswith(("v_lshlrev_b64", "v_lshl_add_u64", "v_addc_co", "v_mad_u64", "v_mad_i64"))
        c["s_load"] += op.startswith(("s_load", "s_buffer_load"))
    return c


def main(lib):
    for needle in ("k_gemm_mx_pipe", "k_gemm_ring_mx"):
        dis = kn.disassembly(lib, needle)
        dm = kn.demangle(list(dis))
        for sym in sorted(dis, key=lambda s: dm[s]):
            ins = dis[sym]
            mf = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
            name = dm[sym].replace("avl::(anonymous namespace)::", "").split("(")[0].replace("void ", "")
            print(name)
            # one sub-step body = first to last MFMA of one kind (f16: v_mfma_f32_16x16x32, FP4: v_mfma_scale_*); a kernel has one of each
            f16 = [i for i in mf if not ins[i].startswith("v_mfma_scale")]
            fp4 = [i for i in mf if ins[i].startswith("v_mfma_scale")]
            for part, seg in (("kernel", ins), ("stream (first..last MFMA)", ins[mf[0]:mf[-1] + 1]),
                              ("  f16 sub-step body", ins[f16[0]:f16[-1] + 1]), ("  FP4 sub-step body", ins[fp4[0]:fp4[-1] + 1]),
                              ("behind the last MFMA", ins[mf[-1] + 1:])):
                c = mix(seg)
                print("   %-26s %5d instr: %4d scalar (%3d s_nop, %3d branch, %2d s_load) %4d non-MFMA vector (%4d readlane, %3d writelane, %3d 64-bit addr) %3d MFMA %3d LDS-DMA"
                      % (part, c["total"], c["scalar"], c["s_nop"], c["branch"], c["s_load"], c["vector"], c["readlane"], c["writelane"], c["addr64"], c["mfma"], c["lds_dma"]))
            m0 = [l for l in ins if "m0" in l.split("//")[0] and not l.startswith(("s_mov_b32 m0", "global_load_lds"))]
            print("   other instructions that name m0: %d %s" % (len(m0), m0[:3]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                                               "vision_semantic_segmentation_amd", "libavl_hip.so"))
