#!/usr/bin/env python3
"""Driver of tools/probe/spectrum_host.hip: builds the host rendering of csrc/spectrum.hip's three launches (with the host
sanitizers unless --no-sanitize), writes its in.bin from seeded noisy pictures, runs it and compares out.bin with the float64
specification `input_pipeline.amplitude_mix_host`.  Needs hipcc, no GPU.

    python tools/probe/spectrum_host.py [32 64 128 256 512]        # sides to run; default 32 64 128

Per side: N = 5 with partners [3, -1, 0, 4, 1] (N = 2, [1, 0] at 512), b in {0, 1, S/10, S/2 - 1, S/2}, then every row mixed with
itself (which must return the input bit for bit).  Prints the largest deviation of the unrounded output in grey levels and the
count of uint8 pixels that differ from the specification's (ties only); exits non-zero if a sanitizer fires, the deviation exceeds
1e-3 or an identity is not exact.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tests")]
from test_amplitude_mix_cpu import noisy_images  # noqa: E402
from wtpse_hip.input_pipeline import amplitude_mix_host, twiddle_table  # noqa: E402


def build(out, sanitize):
    cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "wt-pse-code_amd", "wtpse_hip", "csrc"),
           "-I", os.path.join(ROOT, "include")] + (["-Xarch_host", "-fsanitize=address,undefined"] if sanitize else []) \
        + [os.path.join(ROOT, "tools", "probe", "spectrum_host.hip"), "-o", out]
    subprocess.run(cmd, check=True)


def run(exe, tmp, img, partner, lam, b):
    N, S = img.shape[:2]
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        np.array([N, S, b], np.int32).tofile(f)
        img.tofile(f)
        np.asarray(partner, np.int32).tofile(f)
        np.asarray(lam, np.float32).tofile(f)
        twiddle_table(S).tofile(f)
    subprocess.run([exe, src, dst], check=True)
    raw = open(dst, "rb").read()
    return np.frombuffer(raw[:img.size], np.uint8).reshape(img.shape), np.frombuffer(raw[img.size:], np.float32).reshape(img.shape)


def main():
    args = [a for a in sys.argv[1:] if a != "--no-sanitize"]
    sides = [int(a) for a in args] or [32, 64, 128]
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "spectrum_host")
        build(exe, "--no-sanitize" not in sys.argv)
        for S in sides:
            N = 5 if S < 512 else 2
            partner = [3, -1, 0, 4, 1] if N == 5 else [1, 0]
            lam = [0.3, 0.5, 0.8, 1.0, 0.0][:N]
            img = noisy_images(100 + S, N, S)
            for b in sorted({0, 1, S // 10, S // 2 - 1, S // 2}):
                u8, f32 = run(exe, tmp, img, partner, lam, b)
                spec = amplitude_mix_host(img, partner, lam, b, as_float=True)
                dev = float(np.abs(f32 - spec).max())
                differ = int((u8 != np.rint(np.clip(spec, 0, 255)).astype(np.uint8)).sum())
                untouched = all(np.array_equal(u8[n], img[n]) for n in range(N) if partner[n] < 0 or lam[n] == 0.0)
                print("S %3d b %3d: deviation %.3e grey levels, %d uint8 pixels differ, untouched rows exact: %s" % (S, b, dev, differ, untouched))
                ok = ok and dev < 1e-3 and untouched
            u8, f32 = run(exe, tmp, img, list(range(N)), [0.7] * N, S // 2)
            exact = bool(np.array_equal(u8, img) and np.array_equal(f32, img.astype(np.float32)))
            print("S %3d every row its own partner: exact %s" % (S, exact))
            ok = ok and exact
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
