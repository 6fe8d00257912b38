"""Compare three tools/per_launch.py tables launch by launch: two traces of the parent build and one of this build (medians, us).

    python3 tools/per_launch_compare.py parent_a.csv parent_b.csv new.csv [kernel prefix, e.g. "k_gconv_mfma<f16,2,2"]

A launch counts as lower when it lies below BOTH parent traces by more than the two differ on that launch.  Launches are matched by their
place in the frame; with a prefix only the rows whose kernel starts with it are listed and summed.
"""
import csv
import sys


def rows(path):
    return [(r["kernel"], int(r["launch_in_frame"]), float(r["median_us"])) for r in csv.DictReader(open(path))]


def main(pa, pb, pn, prefix=""):
    a, b, n = rows(pa), rows(pb), rows(pn)
    assert len(a) == len(b) == len(n), "the traces hold different numbers of launches per frame"
    print("%-28s %3s %10s %10s %8s %10s %14s  %s" % ("kernel (this build)", "pos", "parent a", "parent b", "|a - b|", "this build", "new - min(a,b)", "verdict"))
    sa = sb = sn = 0.0
    for (ka, pos, ua), (_, _, ub), (kn, _, un) in zip(a, b, n):
        if not ka.startswith(prefix):
            continue
        d = abs(ua - ub)
        verdict = "lower by more than |a - b|" if un < min(ua, ub) - d else "HIGHER" if un > max(ua, ub) + d else "within the parents' range"
        print("%-28s %3d %10.2f %10.2f %8.2f %10.2f %+14.2f  %s" % (kn, pos, ua, ub, d, un, un - min(ua, ub), verdict))
        sa, sb, sn = sa + ua, sb + ub, sn + un
    print("%-32s %10.1f %10.1f %8s %10.1f %+14.1f" % ("sum (median us per frame)", sa, sb, "", sn, sn - min(sa, sb)))


if __name__ == "__main__":
    main(*sys.argv[1:5])
