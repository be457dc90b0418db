#!/usr/bin/env python3
"""Cost of the calibration pass (ops.calibration_hist, csrc/calibration.hip) on three kinds of input — uniform-random maps, a constant
map (every lane of every wave on one key: the worst case for the LDS atomics) and a realistic map (a disc of ones on zeros with a
3-pixel ramp) — against two yardsticks: the bytes it must read (13 per pixel: prob, spread, label fp32 and the region byte) at the
box's plain copy rate (5.84 TB/s), and ops.seg_metrics on the same masks in the same process.  The device result is
compared with calibration.hist_host before anything is timed.  Every repetition reads the same buffers: a working set below the
256 MB of Infinity Cache (both default shapes) may be served from it, so "of the floor" compares against an HBM rate the launch need
not have been bound by; --rotate N times the launch over N copies of the inputs in turn instead.  With --run, also the whole
calibration run's seconds per image at --samples 16 for one and for four scales (untrained networks: the time does not depend on the
weights).

    python tools/bench_calibration.py [--shapes 18x800x800 2x2048x2048] [--reps 30] [--rotate N] [--run [--run-reps 40]]

Reports the median over `reps` repetitions after a warm-up call.  Nothing here is a pass mark: profiles/calibration.md records a run.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]
from wtpse_hip import calibration as C  # noqa: E402
from wtpse_hip import ops  # noqa: E402

COPY_RATE = 5.84e12          # bytes / s: the plain streaming copy on the same box
BYTES_PER_PIXEL = 13


def disc_maps(B, h, w, seed):
    """-> (prob, spread, label) [B,1,h,w] fp32: a disc of ones on zeros whose edge is a 3-pixel linear ramp; the spread is nonzero on
    the ramp only; the label is the disc shifted by two pixels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    prob, spread, label = (np.zeros((B, 1, h, w), np.float32) for _ in range(3))
    s = min(h, w)
    for i in range(B):
        cy, cx, r = h * rng.uniform(0.45, 0.55), w * rng.uniform(0.45, 0.55), s * rng.uniform(0.25, 0.33)
        d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
        prob[i, 0] = np.clip((r + 1.5 - d) / 3.0, 0.0, 1.0)
        spread[i, 0] = 0.4 * prob[i, 0] * (1.0 - prob[i, 0])
        label[i, 0] = np.sqrt((yy - cy - 2) ** 2 + (xx - cx + 2) ** 2) <= r
    return prob, spread, label


def inputs(kind, B, h, w):
    rng = np.random.default_rng(B * h + w)
    if kind == "random":
        prob, spread = rng.random((B, 1, h, w), np.float32), 0.5 * rng.random((B, 1, h, w), np.float32)
        label = (rng.random((B, 1, h, w)) < 0.3).astype(np.float32)
    elif kind == "constant":
        prob, spread, label = np.full((B, 1, h, w), 0.25, np.float32), np.zeros((B, 1, h, w), np.float32), np.zeros((B, 1, h, w), np.float32)
    else:
        prob, spread, label = disc_maps(B, h, w, 3)
    return prob, spread, label, np.ones((B, 1, h, w), np.uint8)


def event_ms(fn, reps):
    """Median HIP-event time of fn() in ms over `reps` calls after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def whole_run(samples, reps):
    """Seconds per image of CalibrationRun on one batch of 9 images with 800 x 800 labels, for one and for four scales."""
    import tempfile
    from wtpse_hip import test_run as T
    from wtpse_hip.calibration_run import CalibrationRun
    nets = T.build_networks("cuda")
    B = 9
    image = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (B, 3, 256, 256)).astype(np.float32)).cuda()
    _, _, label = disc_maps(B, 800, 800, 5)
    od = torch.from_numpy(label).cuda()
    oc = torch.from_numpy(disc_maps(B, 400, 400, 5)[2]).cuda()
    oc = torch.nn.functional.pad(oc, (200, 200, 200, 200)).contiguous()
    feed = [(image, od, oc, ["%d.png" % i for i in range(B)])]
    print("whole run, %d images with 800x800 labels, --samples %d (host clock around run() and a synchronise; median of %d):" % (B, samples, reps))
    for scales in ((1.0,), (0.0, 0.5, 1.0, 2.0)):
        with tempfile.TemporaryDirectory() as out:
            run = CalibrationRun(*nets, out_dir=out, samples=samples, scales=scales)
            run.run(feed)                                            # warm-up
            times = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run.run(feed)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
        print("  scales %-18s : %7.4f s per run (min %.4f, max %.4f) = %.5f s per image" % (
            ",".join("%g" % s for s in scales), statistics.median(times), min(times), max(times), statistics.median(times) / B))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["18x800x800", "2x2048x2048"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rotate", type=int, default=1, help="copies of the inputs the timed launches rotate through (4: 600 MB at 18x800x800)")
    ap.add_argument("--run", action="store_true", help="also time the whole calibration run")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--run-reps", type=int, default=40, help="timed runs per set of scales (a run is tens of milliseconds)")
    a = ap.parse_args()
    for shape in a.shapes:
        B, h, w = (int(v) for v in shape.split("x"))
        floor_us = BYTES_PER_PIXEL * B * h * w / COPY_RATE * 1e6
        print("calibration pass on %d x %d x %d (median of %d, HIP events); bytes-read floor %.1f us (%d B per pixel at %.2f TB/s):"
              % (B, h, w, a.reps, floor_us, BYTES_PER_PIXEL, COPY_RATE / 1e12))
        for kind in ("random", "constant", "disc"):
            host = inputs(kind, B, h, w)
            prob, spread, label, region = (torch.from_numpy(t).cuda() for t in host)
            rec = ops.calibration_hist(prob, spread, label, region)
            want = C.hist_host(host[0][:1], host[1][:1], host[2][:1], host[3][:1])          # one image: the host pass is slow at this size
            assert np.array_equal(rec[:1].cpu().numpy().view(np.uint32), want), kind
            mask = (prob > 0.75).to(torch.uint8).contiguous()
            sets = [(prob, spread, label, region)] + [tuple(t.clone() for t in (prob, spread, label, region)) for _ in range(a.rotate - 1)]
            turn = [0]

            def rotating():
                turn[0] = (turn[0] + 1) % len(sets)
                ops.calibration_hist(*sets[turn[0]])
            t_rot = event_ms(rotating, a.reps * len(sets)) if a.rotate > 1 else None
            t_cal = event_ms(lambda: ops.calibration_hist(prob, spread, label, region), a.reps)
            t_seg = event_ms(lambda: ops.seg_metrics(mask, label), a.reps)
            t_cal2 = event_ms(lambda: ops.calibration_hist(prob, spread, label, region), a.reps)
            nz = int((rec != 0).sum())
            print("  %-8s : %8.1f us (again after the yardstick: %8.1f us) = %.2f of the floor; ops.seg_metrics %8.1f us, ratio %.2f; "
                  "%d nonzero slots" % (kind, 1e3 * t_cal, 1e3 * t_cal2, floor_us / (1e3 * t_cal), 1e3 * t_seg, t_cal / t_seg, nz))
            if t_rot is not None:
                print("             rotating over %d copies of the inputs: %8.1f us = %.2f of the floor" % (len(sets), 1e3 * t_rot, floor_us / (1e3 * t_rot)))
    if a.run:
        whole_run(a.samples, a.run_reps)


if __name__ == "__main__":
    main()
