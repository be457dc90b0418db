#!/usr/bin/env python3
"""What dense weight averaging costs (wtpse_hip/averaging.py; numbers in profiles/averaging.md).

    python tools/bench_averaging.py          ms/step of TrainStep(graph="plan") with and without average=, alternating in one
                                             session; then the averaging call alone over the four networks' parameter counts
                                             against a plain 16-bytes-per-lane copy of as many bytes on the same device

Time is taken with device events around the replayed steps / the launches; nothing synchronises inside a timed block.
The averaging call reads the iterate and the mean and writes the mean: 12 bytes per parameter (8 for the first fold of a segment).
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--steps", type=int, default=100, help="replayed steps per timed block")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3, help="timed blocks per variant, alternating")
ap.add_argument("--calls", type=int, default=200, help="averaging / copy launches per timed block")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

import torch  # noqa: E402

import bench  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip.averaging import WeightAverage  # noqa: E402
from wtpse_hip.step import TrainStep  # noqa: E402
from wtpse_hip.synth import default_hparams, make_batch  # noqa: E402

DEV = torch.device("cuda:0")
HP = default_hparams(True)


def timed(fn, steps):
    """ms per call of fn over `steps` calls, between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def spread(v):
    return {"runs": [round(x, 4) for x in v], "median": round(sorted(v)[len(v) // 2], 4), "spread": round(max(v) - min(v), 4)}


def step_with_and_without():
    B = args.batch
    batch = make_batch(B, args.size, args.size, DEV, seed=1)
    variants, sizes = {}, None
    for name in ("plain", "averaged"):
        nets = bench.build_nets(HP, B // 3, DEV)
        wa = WeightAverage(nets) if name == "averaged" else None
        ts = TrainStep(*nets, HP, graph="plan", average=wa)
        for _ in range(args.warmup):
            ts.step(*batch)
        torch.cuda.synchronize()
        variants[name] = (ts, wa)
        sizes = [int(n.flat_params().numel()) for n in nets]
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, (ts, wa) in variants.items():
            ms[name].append(timed(lambda: ts.step(*batch), args.steps))
            if wa is not None:
                wa.take()              # a segment stays far below 2^24 iterates
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps({"what": "TrainStep(graph='plan') ms/step, B=%d %dx%d, %d steps per block" % (B, args.size, args.size, args.steps),
                      "plain": spread(ms["plain"]), "averaged": spread(ms["averaged"]),
                      "difference_ms": round(med["averaged"] - med["plain"], 4),
                      "difference_percent": round(100.0 * (med["averaged"] - med["plain"]) / med["plain"], 3),
                      "parameters": sizes}))
    return sizes


def call_alone(sizes):
    p = [torch.randn(n, device=DEV) for n in sizes]
    a = [torch.zeros(n, device=DEV) for n in sizes]
    count = torch.ones(1, dtype=torch.int32, device=DEV)
    total = sum(sizes)
    n4 = total // 4 * 4
    src, dst = torch.randn(n4, device=DEV), torch.empty(n4, device=DEV)

    def fold():
        ops.avg_step(a, p, count)

    def copy():
        ops.lib().call("wtpse_copy_probe", src.data_ptr(), dst.data_ptr(), n4, 16, ops.stream_ptr())

    for fn in (fold, copy):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    count.fill_(1)                     # k >= 2 in every timed fold: the 12-byte form
    us = {"avg_step": [], "copy": []}
    for _ in range(args.rounds):
        us["avg_step"].append(1e3 * timed(fold, args.calls))
        count.fill_(1)
        us["copy"].append(1e3 * timed(copy, args.calls))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    print(json.dumps({"what": "wtpse_avg_step over %d parameters in four segments (one call: the fold and the single-wave count bump) "
                              "beside wtpse_copy_probe (16 bytes per lane) over as many floats, us per call" % total,
                      "avg_step_us": spread(us["avg_step"]), "copy_us": spread(us["copy"]),
                      "avg_step_GBps": round(12.0 * total / med["avg_step"] / 1e3, 1),
                      "copy_GBps": round(8.0 * n4 / med["copy"] / 1e3, 1)}))


if __name__ == "__main__":
    call_alone(step_with_and_without())
