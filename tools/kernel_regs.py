#!/usr/bin/env python3
"""VGPR / AGPR / spill / LDS / scratch of the kernels in libwtpse_hip.so whose (demangled-ish) name matches a regex (llvm-readelf notes).
    python tools/kernel_regs.py 'conv_x3_kILi3ELi1E'
kernel_regs(lib) is the reading on its own (tools/isa_diff.py compares two libraries with it)."""
import os, re, shutil, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_isa import BIN, LIB, code_objects

FIELDS = ("vgpr", "agpr", "spill", "lds", "scratch")


def kernel_regs(lib=LIB):
    """-> {kernel name: (vgpr, agpr, spill, lds, scratch)} from the metadata notes of the library's code objects."""
    tmp = tempfile.mkdtemp(prefix="regs_")
    regs = {}
    try:
        for f in code_objects(lib, tmp):
            txt = subprocess.run([os.path.join(BIN, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for e in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
                g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1)) if re.search(r"\.%s:\s+(\d+)" % k, e) else 0
                name = re.search(r"\.name:\s+(\S+)", e).group(1)
                regs[name] = (g("vgpr_count"), int(re.match(r"\s*(\d+)", e).group(1)), g("vgpr_spill_count"), g("group_segment_fixed_size"),
                              g("private_segment_fixed_size"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return regs


if __name__ == "__main__":
    pat = re.compile(sys.argv[1] if len(sys.argv) > 1 else ".")
    for name, r in sorted(kernel_regs().items()):
        if pat.search(name):
            print("%-90s vgpr %3d agpr %3d spill %3d lds %6d scratch %4d" % ((name,) + r))
