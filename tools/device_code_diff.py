"""Did the device code of libavl_hip.so move between two builds?

    python tools/device_code_diff.py OLD.so NEW.so

For every kernel of the two libraries (tools/kernel_notes.py unbundles their gfx950 code objects) it compares the resource notes
(registers, spills, LDS and scratch sizes) and the disassembled instruction stream.  Kernels of an anonymous namespace carry a hash
of their compilation unit in the symbol name, which changes with any edit of the source file: it is cut out before names are
compared.  Prints the kernels that differ or exist on one side only, and says whether the kernels lie in the same order in their
code objects (same order and same code: same addresses); the exit status is 1 if anything differs.  A refactor of host code must end
with "0 differ".
"""
import re
import sys

import kernel_notes as kn


def _plain(symbol):
    """a symbol without its compilation-unit hash (_GLOBAL__N__<hash>_<file> in mangled names)"""
    return re.sub(r"_GLOBAL__N__[0-9a-f]+_", "_GLOBAL__N__", symbol)


def device_code(lib):
    """({kernel name: notes}, {symbol: instructions}) of `lib`, names and instruction operands free of the unit hash.  "..." is how
    llvm-objdump prints the zero padding behind the last kernel of a code object (whichever kernel that is): not an instruction"""
    code = {_plain(sym): [_plain(line) for line in ins if line != "..."] for sym, ins in kn.disassembly(lib, "").items()}
    return kn.kernel_notes(lib), code


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (notes_a, code_a), (notes_b, code_b) = device_code(sys.argv[1]), device_code(sys.argv[2])
    bad = []
    for what, a, b in (("notes", notes_a, notes_b), ("code", code_a, code_b)):
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                bad.append("%s only in %s: %s" % (what, "NEW" if name in b else "OLD", name))
            elif a[name] != b[name]:
                if what == "notes":
                    bad.append("notes differ: %s: %s" % (name, {k: (v, b[name][k]) for k, v in a[name].items() if v != b[name][k]}))
                else:
                    first = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
                    bad.append("code differs: %s: %d vs %d instructions, first difference at %d" % (name, len(a[name]), len(b[name]), first))
    print("OLD %s\nNEW %s" % tuple(sys.argv[1:]))
    print("%d kernels with notes, %d symbols and %d instructions compared" % (len(notes_a), len(code_a), sum(len(v) for v in code_a.values())))
    if list(code_a) != list(code_b):
        first = next((i for i, (x, y) in enumerate(zip(code_a, code_b)) if x != y), min(len(code_a), len(code_b)))
        bad.append("the kernels lie in another order in their code objects, from symbol %d on: %s" % (first, (list(code_a) + [None])[first]))
    for line in bad:
        print(line)
    print("%d differ" % len(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
