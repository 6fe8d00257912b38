"""Table of tools/pmc_mx_pipe.sh: per MX GEMM instantiation, counters summed over its launches of one forward, the
instructions executed per MFMA by kind, and each unit's issue cycles as a share of the wave cycles.

    python3 tools/pmc_mx_pipe_summary.py <dir with p1/ p2/> [family regex, default the MX GEMMs; e.g. k_gconv_mfma]
"""
import collections
import csv
import glob
import re
import sys


def short(name, family):
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import per_launch
    return per_launch.label(name, family) if re.search(family, name) else None


def main(root, family=r"k_gemm_(?:mx_pipe|ring_mx)"):
    agg = collections.defaultdict(lambda: collections.defaultdict(float))
    launches = collections.defaultdict(set)
    for p in ("p1", "p2"):
        for f in glob.glob("%s/%s/**/*counter_collection.csv" % (root, p), recursive=True):
            for r in csv.DictReader(open(f)):
                k = short(r["Kernel_Name"], family)
                if k is None:
                    continue
                agg[k][p + ":" + r["Counter_Name"]] += float(r["Counter_Value"])
                launches[k].add((p, r["Dispatch_Id"]))
    for k in sorted(agg):
        v = agg[k]
        n = len([1 for p, _ in launches[k] if p == "p1"])
        mf = max(1.0, v["p1:SQ_INSTS_MFMA"])
        print("%s  (%d launches)" % (k, n))
        for c in ("SQ_INSTS_MFMA", "SQ_INSTS_SALU", "SQ_INSTS_VALU", "SQ_INSTS_SMEM", "SQ_INSTS_LDS", "SQ_INSTS_VMEM"):
            print("   %-26s %16.0f" % (c, v["p1:" + c]))
        print("   scalar (SALU) per MFMA           %7.3f" % (v["p1:SQ_INSTS_SALU"] / mf))
        print("   non-MFMA vector (VALU-MFMA) per MFMA %7.3f" % ((v["p1:SQ_INSTS_VALU"] - v["p1:SQ_INSTS_MFMA"]) / mf))
        print("   LDS per MFMA                     %7.3f" % (v["p1:SQ_INSTS_LDS"] / mf))
        wc = max(1.0, v["p2:SQ_WAVE_CYCLES"])
        for c in ("SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_SCA", "SQ_ACTIVE_INST_LDS", "SQ_ACTIVE_INST_VMEM",
                  "SQ_ACTIVE_INST_MISC", "SQ_VALU_MFMA_BUSY_CYCLES"):
            print("   %-26s %16.0f  %6.3f of SQ_WAVE_CYCLES" % (c, v["p2:" + c], v["p2:" + c] / wc))


if __name__ == "__main__":
    main(*(sys.argv[1:3] or ["/tmp/pmc_mx_pipe"]))
