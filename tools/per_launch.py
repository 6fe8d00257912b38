"""Per-launch times of the MX GEMMs from a rocprofv3 kernel trace of bench.py: the launches of one instantiation are told
apart by their place in the frame (every forward launches the same sequence), statistics are over the frames.

    python3 tools/per_launch.py <dir with *kernel_trace.csv> <out.csv>
"""
import csv
import glob
import re
import statistics
import sys


def main(root, out):
    rows = []
    for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if re.search(r"k_gemm_(mx_pipe|ring_mx)", r["Kernel_Name"]):
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
            m = re.search(r"k_gemm_(mx_pipe|ring_mx)I((?:Li\d+E)+)", names[pos])
            d = re.search(r"k_gemm_(mx_pipe|ring_mx)<[^>]*>", names[pos])           # (a demangled trace)
            k = "k_gemm_%s<%s>" % (m.group(1), ",".join(re.findall(r"Li(\d+)E", m.group(2)))) if m else d.group(0).replace(" ", "")
            fo.write('"%s",%d,%d,%.2f,%.2f,%.2f,%.2f\n' % (k, pos, frames, statistics.mean(us), statistics.median(us), min(us), max(us)))
    print("%s: %d MX GEMM launches per frame, %d frames, sum of medians %.1f us" % (out, period, frames, tot))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
