"""Per-launch times of a kernel family from a rocprofv3 kernel trace of bench.py: the launches of one instantiation are told
apart by their place in the frame (every forward launches the same sequence), statistics are over the frames.

    python3 tools/per_launch.py <dir with *kernel_trace.csv> <out.csv> [family regex]

The family defaults to the MX GEMMs, k_gemm_(mx_pipe|ring_mx); k_gconv_mfma gives the grouped 3x3 launches (the nine MX ones of layer3 and
layer4 are <f16,2,2,..>).
"""
import csv
import glob
import re
import statistics
import sys


def label(name, family):
    """k_family<template arguments> of a mangled (Li<n>E, Lb<0|1>E, DF16_, DF16b) or demangled kernel name"""
    m = re.search(r"(%s)I((?:DF16_|DF16b|Li\d+E|Lb[01]E)+)" % family, name)
    if m:
        args = [{"DF16_": "f16", "DF16b": "bf16"}.get(a, a[2:-1]) for a in re.findall(r"DF16_|DF16b|Li\d+E|Lb[01]E", m.group(2))]
        return "%s<%s>" % (m.group(1), ",".join(args))
    return re.search(r"(%s)<[^>]*>" % family, name).group(0).replace(" ", "")           # (a demangled trace)


def main(root, out, family=r"k_gemm_(?:mx_pipe|ring_mx)"):
    rows = []
    for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if re.search(family, r["Kernel_Name"]):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    names = [r[2] for r in rows]
    period = next(p for p in range(1, len(names) + 1) if all(names[i] == names[i + p] for i in range(len(names) - p)))
    frames = len(names) // period
    with open(out, "w") as fo:
        fo.write("kernel,launch_in_frame,frames,mean_us,median_us,min_us,max_us\n")
        tot = 0.0
        for pos in range(period):
            us = [(rows[f * period + pos][1] - rows[f * period + pos][0]) / 1e3 for f in range(frames)]
            tot += statistics.median(us)
            k = label(names[pos], family)
            fo.write('"%s",%d,%d,%.2f,%.2f,%.2f,%.2f\n' % (k, pos, frames, statistics.mean(us), statistics.median(us), min(us), max(us)))
    print("%s: %d launches per frame, %d frames, sum of medians %.1f us" % (out, period, frames, tot))


if __name__ == "__main__":
    main(*sys.argv[1:4])
