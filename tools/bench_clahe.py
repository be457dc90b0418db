#!/usr/bin/env python3
"""What the CLAHE preprocessing (csrc/clahe.hip) costs -> profiles/clahe.md.

    python tools/bench_clahe.py [--out profiles/clahe.md] [--reps 30] [--inner 20]

Three shapes with the pictures already in HBM — a training batch (N = 30, 256 x 256, tiles (8, 8), luma) and one large picture
(N = 1, 2048 x 2048, tiles (8, 8)) in both modes — and for each, in the same run and alternating:
  * `ops.clahe` as the fronts call it (three allocations, a memset, three launches);
  * each launch alone on buffers that exist already (`wtpse_clahe_hist` with its memset, `wtpse_clahe_lut`, `wtpse_clahe_apply`);
  * a plain device copy of the same bytes (`Tensor.copy_`).
A figure is the time between two device events around --inner back-to-back calls, divided by --inner; median (minimum .. maximum) of
--reps such windows.  Then the training feed (`FundusBatches` on a seeded synthetic tree, 30 samples of 256 x 256) with the stage on
and off: host clock around a call that ends in a device synchronise, alternating, median of --reps calls.  There is no bar: the
stage is new.  The file says how far each launch lies from the copy and why.
"""
import argparse
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "wt-pse-code_amd"), os.path.join(HERE, "tests"), os.path.join(HERE, "tools")]

from stage_bench import alternate, write_profile  # noqa: E402

SHAPES = [("N = 30, 256 x 256, tiles (8, 8), luma", 30, 256, 256, (8, 8), "luma"),
          ("N = 1, 2048 x 2048, tiles (8, 8), luma", 1, 2048, 2048, (8, 8), "luma"),
          ("N = 1, 2048 x 2048, tiles (8, 8), rgb", 1, 2048, 2048, (8, 8), "rgb")]
COPY = "device copy of the same bytes (`Tensor.copy_`)"


def variants(N, H, W, tiles, mode):
    from test_clahe_cpu import smooth_pictures
    from wtpse_hip import ops
    from wtpse_hip.input_pipeline import Clahe
    from wtpse_hip.lib import lib
    clahe = Clahe(2.0, tiles, 0, mode)
    one = smooth_pictures(7, 2, H, W)                  # a smooth picture and a random one, repeated
    img = torch.from_numpy(np.ascontiguousarray(one[np.arange(N) % 2])).cuda()
    out = torch.empty_like(img)
    (ty, tx), P = tiles, clahe.planes
    rows, cols, bands = ops.clahe_tables(H, W, clahe, img.device)
    hist = torch.empty((N, P, ty, tx, 256), dtype=torch.int32, device="cuda")
    luts = torch.empty((N, P, ty, tx, 256), dtype=torch.uint8, device="cuda")
    call, p = lib().call, ops.ptr
    fns = {"`ops.clahe`, the whole call": lambda: ops.clahe(img, clahe),
           "histogram launch alone (memset + kernel)": lambda: call("wtpse_clahe_hist", p(img), p(hist), N, H, W, ty, tx, 0, P, ops.stream_ptr()),
           "LUT launch alone": lambda: call("wtpse_clahe_lut", p(hist), p(luts), N * P * ty * tx, clahe.clip_q8, ops.stream_ptr()),
           "apply launch alone": lambda: call("wtpse_clahe_apply", p(img), p(luts), p(rows), p(cols), p(bands), p(out), N, H, W, ty, tx, 0, P,
                                              ops.stream_ptr()),
           COPY: lambda: out.copy_(img)}
    return fns, (img, out, hist, luts, rows, cols, bands)


def feed_times(reps):
    """Seconds per batch of the training feed with the stage off and on -> {label: [seconds]}."""
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.input_pipeline import Clahe
    from wtpse_hip.trainer import FundusBatches
    times = {"training feed, stage off": [], "training feed, CLAHE on (clip 2, tiles (8, 8), luma)": []}
    with tempfile.TemporaryDirectory() as root:
        make_tree(root, seed=5)
        sets = [FundusTree(root, "train", (i,), size=256) for i in (1, 2, 3)]
        feeds = [FundusBatches(sets, 30, "cuda", size=256), FundusBatches(sets, 30, "cuda", size=256, clahe=Clahe())]
        rngs = [(random.Random(3), np.random.RandomState(3)) for _ in feeds]
        for _ in range(3):
            for f, r in zip(feeds, rngs):
                f(*r)
        torch.cuda.synchronize()
        for _ in range(reps):
            for (label, t), f, r in zip(times.items(), feeds, rngs):
                t0 = time.perf_counter()
                f(*r)
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clahe.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X (no fallback)")
    med = statistics.median
    L = ["# CLAHE preprocessing: numbers", "",
         "Stage: `csrc/clahe.hip` behind `ops.clahe`.  Tool: `tools/bench_clahe.py` on one MI355X.  The pictures are in HBM already.  A",
         "figure is the time between two device events around %d back-to-back calls divided by %d; median (minimum .. maximum) of %d"
         % (a.inner, a.inner, a.reps), "such windows, the variants of a shape alternating.", ""]
    for title, N, H, W, tiles, mode in SHAPES:
        fns, keep = variants(N, H, W, tiles, mode)
        times = alternate(fns, a.reps, a.inner)
        copy = med(times[COPY])
        nbytes = N * H * W * 3
        L += ["## %s (%.1f MB read, as much written)" % (title, nbytes / 1e6), "", "| what | us per call | times the copy |", "| --- | --- | --- |"]
        for k, t in times.items():
            L.append("| %s | %.1f (%.1f .. %.1f) | %.1f |" % (k, 1e3 * med(t), 1e3 * min(t), 1e3 * max(t), med(t) / copy))
        L.append("")
        del keep
    feed = feed_times(a.reps)
    L += ["## The training feed (30 samples of 256 x 256 from a synthetic tree; host clock to a device synchronise)", "",
          "| what | ms per batch |", "| --- | --- |"]
    for k, t in feed.items():
        L.append("| %s | %.2f (%.2f .. %.2f) |" % (k, 1e3 * med(t), 1e3 * min(t), 1e3 * max(t)))
    L.append("")
    write_profile(a.out, L)


if __name__ == "__main__":
    main()
