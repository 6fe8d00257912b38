"""Did the device code of libavl_hip.so move between two builds?

    python tools/device_code_diff.py [--rename OLD=NEW ...] OLD.so NEW.so

For every kernel of the two libraries (tools/kernel_notes.py unbundles their gfx950 code objects) it compares the resource notes
(registers, spills, LDS and scratch sizes) and the disassembled instruction stream.  Kernels of an anonymous namespace carry a hash
of their compilation unit in the symbol name, which changes with any edit of the source file: it is cut out before names are
compared.  Prints the kernels that differ or exist on one side only, and says whether the kernels lie in the same order in their
code objects (same order and same code: same addresses); the exit status is 1 if anything differs.  A refactor of host code must end
with "0 differ".  --rename OLD=NEW replaces OLD by NEW in every symbol first, for a refactor that renames a kernel's parameter type
(mangled names carry the length, 7old_job=7new_job; the notes' names are demangled, old_job=new_job: give both, the longer first).
"""
import re
import sys

import kernel_notes as kn


RENAMES = []          # (old, new) of --rename


def _plain(symbol):
    """a symbol without its compilation-unit hash (_GLOBAL__N__<hash>_<file> in mangled names), the --rename pairs applied"""
    for old, new in RENAMES:
        symbol = symbol.replace(old, new)
    return re.sub(r"_GLOBAL__N__[0-9a-f]+_", "_GLOBAL__N__", symbol)


def device_code(lib):
    """({kernel name: notes}, {symbol: instructions}) of `lib`, names and instruction operands free of the unit hash.  "..." is how
    llvm-objdump prints the zero padding behind the last kernel of a code object (whichever kernel that is): not an instruction"""
    code = {_plain(sym): [_plain(line) for line in ins if line != "..."] for sym, ins in kn.disassembly(lib, "").items()}
    return {_plain(name): notes for name, notes in kn.kernel_notes(lib).items()}, code


def main():
    while len(sys.argv) > 2 and sys.argv[1] == "--rename":
        RENAMES.append(tuple(sys.argv[2].split("=", 1)))
        del sys.argv[1:3]
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
