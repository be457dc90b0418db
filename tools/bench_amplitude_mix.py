#!/usr/bin/env python3
"""What the amplitude-mixing stage (csrc/spectrum.hip) costs and how far it lies from its specification -> profiles/amplitude_mix.md.

    python tools/bench_amplitude_mix.py [--out profiles/amplitude_mix.md] [--kernel-stats <rocprofv3 kernel_stats.csv>]
                                        [--parent-tree <built checkout of the parent commit>]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o amix -- python tools/bench_amplitude_mix.py --kernels-only

Times: one `FundusBatches` call at B = 30, S = 256 on the synthetic PNG tree with the stage off, with style = AmplitudeMix() and
with every sample mixed (p = 1) — wall clock around a device synchronisation, alternating, median of --reps calls; and the stage
alone on a batch already in HBM.  The yardstick is the same call at the parent commit: with --parent-tree this program runs itself
as a child process against that checkout's package and library (`--tree DIR --feed-off-only`), once before and once after its own
measurement.  The three kernels' times come from a rocprofv3 run of --kernels-only (a run of its own: tracing slows the host),
handed in with --kernel-stats.
Deviations: per case of tests/test_amplitude_mix_gpu.py the device's largest deviation from `amplitude_mix_host` and that of the
float32 torch.fft restatement on the CPU, in grey levels.
"""
import argparse
import csv
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree DIR: measure that checkout's package instead of this one's (how the parent commit's feed call is timed)
ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(HERE, "tests")]

B, S = 30, 256


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def stage_inputs():
    from test_amplitude_mix_cpu import noisy_images
    from wtpse_hip.input_pipeline import AmplitudeMix, draw_mix
    img = torch.from_numpy(noisy_images(7, B, S)).cuda()
    partner, lam = draw_mix(np.random.RandomState(1), 3, B // 3, AmplitudeMix(p=1.0))
    return img, partner, lam


def kernels_only(reps):
    from wtpse_hip import ops
    img, partner, lam = stage_inputs()
    for b in (25, 128):
        for _ in range(reps + 3):
            ops.amplitude_mix(img, partner, lam, b)
    torch.cuda.synchronize()


def feed_times(reps, off_only=False):
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.trainer import FundusBatches
    with tempfile.TemporaryDirectory() as root:
        make_tree(root, seed=5)
        sets = [FundusTree(root, "train", (i,), size=S) for i in (1, 2, 3)]
    feeds = {"off": FundusBatches(sets, B, "cuda", size=S)}
    if not off_only:
        from wtpse_hip.input_pipeline import AmplitudeMix
        feeds.update(on=FundusBatches(sets, B, "cuda", size=S, style=AmplitudeMix()),
                     all=FundusBatches(sets, B, "cuda", size=S, style=AmplitudeMix(p=1.0)))
    rngs = {k: (random.Random(3), np.random.RandomState(3)) for k in feeds}
    times = {k: [] for k in feeds}
    for k, f in feeds.items():                       # warm-up: code objects, tables, workspace
        for _ in range(3):
            f(*rngs[k])
    for _ in range(reps):                            # alternating: other people's work shares the host
        for k, f in feeds.items():
            times[k] += timed(lambda: f(*rngs[k]), 1)
    return times


def parent_feed_times(tree, reps):
    """The `style=None` feed call of the checkout at `tree`, in a child process of its own -> ms per call."""
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--feed-off-only", "--reps", str(reps)],
                         capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit("the parent's feed call failed:\n" + res.stdout + res.stderr)
    return json.loads(res.stdout.strip().splitlines()[-1])


def stage_times(reps):
    from wtpse_hip import ops
    img, partner, lam = stage_inputs()
    out = {}
    for b in (25, 128):
        for _ in range(3):
            ops.amplitude_mix(img, partner, lam, b)
        out[b] = timed(lambda: ops.amplitude_mix(img, partner, lam, b), reps)
    return out


def deviations():
    from test_amplitude_mix_cpu import mix_float32, noisy_images
    from wtpse_hip import ops
    from wtpse_hip.input_pipeline import amplitude_mix_host
    rows = []
    cases = [(s, 5, [3, -1, 0, 4, 1], [lam] * 5, b) for s in (32, 64, 256) for b in (0, 1, s // 10, s // 2 - 1, s // 2) for lam in (0.0, 0.3, 0.8, 1.0)]
    cases += [(128, 2, [1, 0], [0.8, 0.3], 12), (128, 2, [1, 0], [0.8, 0.3], 64), (512, 2, [1, 0], [0.8, 0.3], 256)]
    for s, n, partner, lam, b in cases:
        img = noisy_images(100 + s, n, s)
        u8, f32 = ops.amplitude_mix(torch.from_numpy(img).cuda(), np.asarray(partner), np.asarray(lam), b, want_float=True)
        spec = amplitude_mix_host(img, partner, lam, b, as_float=True)
        dev = float(np.abs(f32.cpu().numpy().astype(np.float64) - spec).max())
        ref = float(np.abs(mix_float32(img, partner, lam, b).astype(np.float64) - spec).max())
        clipped = np.clip(spec, 0, 255)
        near = np.abs(clipped - np.floor(clipped) - 0.5) <= 4 * ref
        differ = int((u8.cpu().numpy() != np.rint(clipped).astype(np.uint8)).sum())
        rows.append((s, n, b, "%g" % lam[0] if len(set(lam)) == 1 else "/".join("%g" % v for v in lam), dev, ref, 100.0 * near.mean(), differ))
    return rows


def kernel_stats(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "amix_" in r["Name"]:
                rows.append((r["Name"], int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amplitude_mix.md"))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--tree", default=None, help="measure this checkout's package instead (with --feed-off-only)")
    ap.add_argument("--feed-off-only", action="store_true", help="time the style=None feed call alone and print the times as JSON")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X (no fallback)")
    if a.kernels_only:
        return kernels_only(a.reps)
    if a.feed_off_only:
        print(json.dumps(feed_times(a.reps, off_only=True)["off"]))
        return
    med = statistics.median
    parent = [parent_feed_times(a.parent_tree, a.reps)] if a.parent_tree else []
    ft = feed_times(a.reps)
    if a.parent_tree:
        parent.append(parent_feed_times(a.parent_tree, a.reps))
    st, dv = stage_times(a.reps), deviations()
    L = ["# Amplitude mixing between source domains: numbers", "",
         "Stage: `csrc/spectrum.hip` behind `FundusBatches(..., style=AmplitudeMix(...))`.  Tool: `tools/bench_amplitude_mix.py` on one",
         "MI355X; wall clock around a device synchronisation, median (minimum .. maximum) of %d calls, the feeds alternating." % a.reps, "",
         "## One feed call, B = %d, S = %d (synthetic PNG tree, three source domains)" % (B, S), "",
         "| feed | ms per call |", "| --- | --- |"]
    for k, t in enumerate(parent):
        L.append("| the parent commit's call, a process of its own %s this one's measurement: the yardstick | %.2f (%.2f .. %.2f) |"
                 % ("before" if k == 0 else "after", med(t), min(t), max(t)))
    names = {"off": "`style=None`, this commit", "on": "`style=AmplitudeMix()` (p = 0.5, b = 25)",
             "all": "`style=AmplitudeMix(p=1)` (every sample mixed, b = 25)"}
    for k in ("off", "on", "all"):
        L.append("| %s | %.2f (%.2f .. %.2f) |" % (names[k], med(ft[k]), min(ft[k]), max(ft[k])))
    L += ["", "The stage alone on a batch of %d already in HBM, every sample mixed (uploads of `partner` and `lam` and the three launches):" % B, "",
          "| b | ms per call |", "| --- | --- |"]
    for b in sorted(st):
        L.append("| %d%s | %.3f (%.3f .. %.3f) |" % (b, " (the whole spectrum)" if b == S // 2 else "", med(st[b]), min(st[b]), max(st[b])))
    if a.kernel_stats:
        L += ["", "## Per kernel (`rocprofv3 --kernel-trace --stats -- python tools/bench_amplitude_mix.py --kernels-only`)", "",
              "B = %d, S = %d, every sample mixed; the run launches b = 25 and b = 128 equally often, so an average is over both." % (B, S), "",
              "| kernel | launches | average us | minimum us (b = 25) | maximum us |", "| --- | --- | --- | --- | --- |"]
        for name, calls, avg, lo, hi in kernel_stats(a.kernel_stats):
            L.append("| `%s` | %d | %.1f | %.1f | %.1f |" % (name, calls, avg, lo, hi))
    L += ["", "## Deviation from the float64 specification (grey levels)", "",
          "Per case of `tests/test_amplitude_mix_gpu.py`: the device's largest deviation from `amplitude_mix_host`, that of the float32",
          "`torch.fft` restatement on the CPU for the same inputs (the bar is 4 times it), the share of pixels whose specified value lies within",
          "the bar of a half-integer, and the uint8 pixels that differ from the specification's (all of them among those).", "",
          "| S | N | b | lam | device | restatement | device / restatement | near a tie % | uint8 differ |", "| --- | --- | --- | --- | --- | --- | --- | --- | --- |"]
    ratios = {}
    for s, n, b, lam, dev, ref, near, differ in dv:
        if ref > 1e-9:                               # (b = 0 with lam = 1 is exact on both sides: no ratio)
            ratios.setdefault(s, []).append(dev / ref)
    for s, n, b, lam, dev, ref, near, differ in dv:
        L.append("| %d | %d | %d | %s | %.3e | %.3e | %s | %.3f | %d |" % (s, n, b, lam, dev, ref, "%.2f" % (dev / ref) if ref > 0 else "-", near, differ))
    L += ["", "Device / restatement by size: " + "; ".join("S = %d: %.2f .. %.2f" % (s, min(r), max(r)) for s, r in sorted(ratios.items())) + "."]
    text = "\n".join(L) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
