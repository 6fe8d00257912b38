"""Static instruction counts of the MX grouped 3x3 kernels (k_gconv_mfma<f16, 2, ..>) of a built libavl_hip.so: registers and
SGPR spills from the kernel notes, and the instruction mix -- classified by mnemonic prefix only -- of the whole kernel, of the span from the
first to the last MFMA of the tile loop, and of the span between the MFMA clusters of the two sub-tiles (NJ = 2).

    python3 tools/gconv_static_counts.py [path/to/libavl_hip.so]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_notes as kn  # noqa: E402
import per_launch  # noqa: E402

CLASSES = ("v_mfma", "other v_", "s_", "ds_", "vector memory", "v_readlane/v_writelane")


def mix(ins):
    c = dict.fromkeys(CLASSES, 0)
    for l in ins:
        op = l.split()[0]
        if op.startswith("v_mfma"):
            c["v_mfma"] += 1
        elif op.startswith(("v_readlane", "v_writelane")):
            c["v_readlane/v_writelane"] += 1
        elif op.startswith("v_"):
            c["other v_"] += 1
        elif op.startswith("s_"):
            c["s_"] += 1
        elif op.startswith("ds_"):
            c["ds_"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vector memory"] += 1
    return c


def main(lib):
    notes = kn.kernel_notes(lib)
    dis = kn.disassembly(lib, "k_gconv_mfmaIDF16_Li2E")
    dm = kn.demangle(list(dis))
    for sym in sorted(dis, key=lambda s: dm[s]):
        ins = dis[sym]
        name = dm[sym].replace("avl::(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        n = notes[dm[sym]] if dm[sym] in notes else next(v for k, v in notes.items() if name in k.replace("avl::(anonymous namespace)::", ""))
        if name.startswith("_Z"):          # (c++filt leaves the _Float16 instantiations mangled)
            name = per_launch.label(name, "k_gconv_mfma")
        mf = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
        print("%s   VGPRs %d, SGPRs %d, spilled SGPRs %d, spilled VGPRs %d, scratch %d B" % (
            name, n["vgpr_count"], n["sgpr_count"], n["sgpr_spill_count"], n["vgpr_spill_count"], n["private_segment_fixed_size"]))
        parts = [("kernel", ins), ("first .. last MFMA of the tile loop", ins[mf[0]:mf[-1] + 1])]
        if len(mf) == 60:          # NJ = 2: two clusters of 18 f16 + 12 scaled MFMAs
            parts.append(("between the two sub-tiles' MFMA clusters", ins[mf[29] + 1:mf[30]]))
        print("   %-42s %6s " % ("", "instr") + " ".join("%14s" % k for k in CLASSES))
        for part, seg in parts:
            c = mix(seg)
            print("   %-42s %6d " % (part, len(seg)) + " ".join("%14d" % c[k] for k in CLASSES))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                                               "vision_semantic_segmentation_amd", "libavl_hip.so"))
