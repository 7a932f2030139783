#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library, kernel by kernel: the proof a refactor gives that no kernel changed.

    python tools/device_code_diff.py OBJDIR_A OBJDIR_B [--exports LIB_A LIB_B]

Both directories hold the objects of one build (build.py's flags: human-pose-estimation_amd/lib/obj of each tree, or any directory
hipcc -c wrote to).  Every object's code object is disassembled (device_disassembly / parse_kernels of tools/isa_lint.py: llvm-objdump,
no GPU) and each kernel symbol, keyed by object and symbol, is compared as its sequence of (mnemonic, operands) -- addresses and
encodings are left out, branch operands are relative.  Prints the symbol counts, what only one side has, how many kernels were compared
and how many are identical, then per differing kernel its first differing instruction.  With --exports also the sorted hpe_* exports
(nm -D --defined-only) of the two shared libraries.  Exit status 1 on any difference.
"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_lint import device_disassembly, parse_kernels  # noqa: E402


def kernel_code(text):
    """{symbol: [(mnemonic, operands)]} of one disassembly text"""
    return {name: [(mn, ops) for _, _, mn, ops in insns] for name, insns in parse_kernels(text).items()}


def compare(a, b):
    """a, b: {key: [(mnemonic, operands)]}.  Returns (only_a, only_b, common, differing) with differing =
    [(key, index of the first differing instruction, instruction of a or None, instruction of b or None)]"""
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    common = sorted(set(a) & set(b))
    differing = []
    for k in common:
        ia, ib = a[k], b[k]
        if ia == ib:
            continue
        i = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
        differing.append((k, i, ia[i] if i < len(ia) else None, ib[i] if i < len(ib) else None))
    return only_a, only_b, common, differing


def report(a, b, name_a="A", name_b="B"):
    """(text, number of differences) of compare(a, b)"""
    only_a, only_b, common, differing = compare(a, b)
    fmt = lambda ins: "(end of kernel)" if ins is None else ("%s %s" % ins).strip()
    out = ["kernel symbols: %s %d, %s %d" % (name_a, len(a), name_b, len(b)),
           "only in %s (%d):%s" % (name_a, len(only_a), "".join("\n  " + k for k in only_a)),
           "only in %s (%d):%s" % (name_b, len(only_b), "".join("\n  " + k for k in only_b)),
           "%d kernels compared, %d identical" % (len(common), len(common) - len(differing))]
    for k, i, x, y in differing:
        out.append("DIFFERS %s (%d / %d instructions), first at instruction %d:\n  %s: %s\n  %s: %s"
                   % (k, len(a[k]), len(b[k]), i, name_a, fmt(x), name_b, fmt(y)))
    return "\n".join(out), len(only_a) + len(only_b) + len(differing)


def load_dir(objdir):
    """{'object:symbol': code} over every object of a directory"""
    out = {}
    for f in sorted(os.listdir(objdir)):
        if f.endswith(".o"):
            for name, code in kernel_code(device_disassembly(os.path.join(objdir, f))).items():
                out[f + ":" + name] = code
    return out


def exports(lib):
    r = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True)
    return sorted(s for s in (line.split()[-1] for line in r.stdout.splitlines() if line.split()) if s.startswith("hpe_"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("objdir_a")
    ap.add_argument("objdir_b")
    ap.add_argument("--exports", nargs=2, metavar=("LIB_A", "LIB_B"))
    args = ap.parse_args()
    text, bad = report(load_dir(args.objdir_a), load_dir(args.objdir_b))
    print(text)
    if args.exports:
        ea, eb = exports(args.exports[0]), exports(args.exports[1])
        print("\nhpe_* exports (nm -D --defined-only, sorted): A %d, B %d, lists %s" % (len(ea), len(eb), "identical" if ea == eb else "DIFFER"))
        for s in sorted(set(ea) - set(eb)):
            print("< " + s)
        for s in sorted(set(eb) - set(ea)):
            print("> " + s)
        if ea == eb:
            print("  " + " ".join(ea))
        else:
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
