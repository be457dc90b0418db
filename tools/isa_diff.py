#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code of two builds of libwtpse_hip.so.
    python tools/isa_diff.py LIB_A LIB_B [--show REGEX]
Every function symbol of the two libraries is reported as identical, different or only in one; then the VGPR / AGPR / spill / LDS /
scratch figures (tools/kernel_regs.py) of every kernel whose figures or code differ.  The disassembly (tools/kernel_isa.py) is
compared after removing what is position only: the address comments, the symbol-relative offsets in them, and the numbering of the
local labels (renumbered per function in order of appearance).  --show prints the unified diff of the matching different kernels.
Exit status 0: no kernel differs and none is missing on either side."""
import difflib, re, sys
from kernel_isa import kernel_bodies
from kernel_regs import FIELDS, kernel_regs


def normalise(body):
    body = re.sub(r"[ \t]*//.*$", "", body, flags=re.M)            # "// 000000012340: <symbol+0x1A4>"
    names = {}
    return re.sub(r"\bL\d+\b", lambda m: names.setdefault(m.group(0), "L#%d" % len(names)), body)


def main(argv):
    show = re.compile(argv[argv.index("--show") + 1]) if "--show" in argv else None
    lib_a, lib_b = argv[1], argv[2]
    a, b = kernel_bodies(lib_a), kernel_bodies(lib_b)
    ra, rb = kernel_regs(lib_a), kernel_regs(lib_b)
    same, diff, only_a, only_b = [], [], [n for n in a if n not in b], [n for n in b if n not in a]
    for n in a:
        if n in b:
            (same if normalise(a[n]) == normalise(b[n]) else diff).append(n)
    print("%d symbols in A, %d in B: %d identical, %d different, %d only in A, %d only in B"
          % (len(a), len(b), len(same), len(diff), len(only_a), len(only_b)))
    for tag, names in (("different", diff), ("only in A", only_a), ("only in B", only_b)):
        for n in names:
            print("%-10s %s" % (tag, n))
    fmt = lambda r: "  ".join("%s %d" % kv for kv in zip(FIELDS, r)) if r else "-"
    for n in sorted(set(ra) | set(rb)):
        if ra.get(n) != rb.get(n) or n in diff:
            print("%s\n    A: %s\n    B: %s" % (n, fmt(ra.get(n)), fmt(rb.get(n))))
    if show:
        for n in diff:
            if show.search(n):
                sys.stdout.writelines(difflib.unified_diff(normalise(a[n]).splitlines(True), normalise(b[n]).splitlines(True), "A " + n, "B " + n))
    return 1 if diff or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
