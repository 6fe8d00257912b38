"""Which kernel instantiations of the BUILT libavl_hip.so a GPU test run launched, and which it never did.

    rocprofv3 --kernel-trace --mangled-kernels --output-format csv -d <dir> -- python -m pytest tests -q -m gpu
    python tools/kernel_coverage.py <dir or *_kernel_trace.csv ...> [--lib path/to/libavl_hip.so]

The library side: every kernel descriptor symbol (`_Z....kd`) found in the bytes of the shared library (its gfx950 code objects
are bundled uncompressed).  The trace side: the kernel names of every `*kernel_trace.csv` under the given paths.  Names are
compared mangled (rocprofv3 --mangled-kernels); a trace recorded without that option is compared through c++filt, if present.
Prints the instantiations that were never launched, grouped by kernel template, and exits non-zero when fewer than half of the
distinct kernel names launched from the library (names that start with k_ after demangling) match one of its symbols: a
format mismatch must not pass for complete coverage, nor for none.
"""
import argparse
import csv
import os
import re
import shutil
import subprocess
import sys

DEFAULT_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision_semantic_segmentation_amd", "libavl_hip.so")


def library_kernels(lib):
    """mangled kernel symbols (without .kd) of every code object in `lib`"""
    with open(lib, "rb") as f:
        blob = f.read()
    return sorted({m.decode()[:-3] for m in re.findall(rb"_Z[0-9A-Za-z_]+\.kd", blob)})


def trace_files(paths):
    out = []
    for p in paths:
        if os.path.isdir(p):
            for root, _, files in os.walk(p):
                out += [os.path.join(root, f) for f in files if f.endswith("kernel_trace.csv")]
        else:
            out.append(p)
    return sorted(out)


def traced_kernels(files):
    """{kernel name as the trace writes it: dispatch count}"""
    counts = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("KernelName") or row.get("Kernel_name")
                if name is None:
                    raise SystemExit("%s: no Kernel_Name column (columns: %s)" % (path, ", ".join(row)))
                name = name.strip()
                if name.endswith(".kd"):
                    name = name[:-3]
                counts[name] = counts.get(name, 0) + 1
    return counts


# ---- a readable name for the report: the nested name and template arguments of the symbols this library holds
_BUILTIN = {"f": "float", "d": "double", "i": "int", "j": "unsigned", "b": "bool", "h": "uchar", "DF16_": "f16", "DF16b": "bf16"}


def _source_name(s, i):
    m = re.match(r"(\d+)", s[i:])
    n = int(m.group(1))
    i += len(m.group(1))
    return s[i:i + n], i + n


def _template_args(s, i):
    """s[i] == 'I' -> (['arg', ...], index after the closing E)"""
    i += 1
    args = []
    while s[i] != "E":
        if s[i] == "L":                                           # literal: L<type><value>E
            j = s.index("E", i)
            lit = s[i + 1:j]
            m = re.match(r"(DF16[_b]|[a-zA-Z])(n?\d+)$", lit)
            if m is None:
                raise ValueError(lit)
            v = m.group(2).replace("n", "-")
            args.append({"0": "false", "1": "true"}[v] if m.group(1) == "b" else v)
            i = j + 1
        else:
            for code, name in sorted(_BUILTIN.items(), key=lambda kv: -len(kv[0])):
                if s.startswith(code, i):
                    args.append(name)
                    i += len(code)
                    break
            else:
                raise ValueError(s[i:])
    return args, i + 1


def pretty(sym):
    """'_ZN3avl12_GLOBAL__N_16k_gemmIDF16bLi2ELi2EEEvNS0_8GemmArgsE' -> ('k_gemm', 'k_gemm<bf16, 2, 2>'); the symbol on failure"""
    try:
        i = 2
        nested = sym[i] == "N"
        if nested:
            i += 1
        parts, args = [], None
        while True:
            if sym[i].isdigit():
                name, i = _source_name(sym, i)
                parts.append(name)
            elif sym[i] == "I":
                args, i = _template_args(sym, i)
            else:
                break
            if not nested:
                break
        base = parts[-1]
        return base, base + ("<%s>" % ", ".join(args) if args is not None else "")
    except (ValueError, IndexError, AttributeError):
        return sym, sym


def demangle(names):
    tool = shutil.which("c++filt")
    if tool is None or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def _key(name):
    return re.sub(r"\s+", "", name)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("traces", nargs="+", help="rocprofv3 output directories or *kernel_trace.csv files")
    ap.add_argument("--lib", default=DEFAULT_LIB)
    a = ap.parse_args(argv)

    syms = library_kernels(a.lib)
    files = trace_files(a.traces)
    if not files:
        print("no *kernel_trace.csv under %s" % ", ".join(a.traces))
        return 2
    traced = traced_kernels(files)
    mangled_trace = sum(n.startswith("_Z") for n in traced) >= len(traced) / 2
    if mangled_trace:
        lib_key = {s: s for s in syms}
        ours = {n for n in traced if n.startswith("_Z") and re.search(r"\d+k_", n)}
    else:                                                         # a demangled trace: bring the library's names to its form
        dm = demangle(syms)
        lib_key = {s: _key(dm[s]) for s in syms}
        ours = {n for n in traced if re.search(r"(^|::|\s)k_\w+", n)}
    by_key = {}
    for s, k in lib_key.items():
        by_key.setdefault(k, []).append(s)
    launched = set()
    matched = 0
    for n in ours:
        k = n if mangled_trace else _key(n)
        if k in by_key:
            matched += 1
            launched.update(by_key[k])
    dispatches = sum(traced.values())
    print("library: %d kernel instantiations (%s)" % (len(syms), os.path.normpath(a.lib)))
    print("trace:   %d files, %d dispatches, %d distinct kernels, %d of them k_* names; %d of those match a library symbol (%s names)"
          % (len(files), dispatches, len(traced), len(ours), matched, "mangled" if mangled_trace else "demangled"))
    if not ours or matched < 0.5 * len(ours):
        print("FAIL: fewer than half of the launched k_* kernel names match a library symbol: the trace and the library disagree "
              "on the name format (record the trace with rocprofv3 --mangled-kernels) or the trace is of another build")
        return 1
    missing = [s for s in syms if s not in launched]
    groups = {}
    for s in missing:
        base, full = pretty(s)
        groups.setdefault(base, []).append(full)
    print("launched: %d of %d instantiations; never launched: %d" % (len(syms) - len(missing), len(syms), len(missing)))
    for base in sorted(groups):
        print("  %s (%d)" % (base, len(groups[base])))
        for full in sorted(groups[base]):
            print("      %s" % full)
    return 0


if __name__ == "__main__":
    sys.exit(main())
