#!/usr/bin/env python3
"""What the Lovász hinge loss costs (wtpse_hip/lovasz.py, csrc/lovasz.hip; numbers in profiles/lovasz.md).

    python tools/bench_lovasz.py            wtpse_lovasz_loss alone at B = 32, 256 x 256, with dx — disc and cup form, on random logits
                                            and on logits that agree with the labels except near the contour (few positive errors, as
                                            late in a run) — beside wtpse_overlap_loss on the same tensors (us per call); then ms/step of
                                            TrainStep(graph="plan") with and without lovasz=, alternating in one session
    python tools/bench_lovasz.py --no-step  the entry points only (the form to run under a kernel trace: the lv_*_k kernels then appear
                                            with their own times)

Time is taken with device events around the launches / the replayed steps; nothing synchronises inside a timed block.  The labels
are synth.make_batch's discs, as in bench.py.
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--steps", type=int, default=30, help="replayed steps per timed block")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3, help="timed blocks per variant, alternating")
ap.add_argument("--calls", type=int, default=100, help="entry-point calls per timed block")
ap.add_argument("--no-step", action="store_true")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

import torch  # noqa: E402

import bench  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip.lovasz import LovaszLoss  # noqa: E402
from wtpse_hip.overlap import OverlapLoss  # noqa: E402
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


def loss_alone():
    B, size = args.batch, args.size
    _, od, _ = make_batch(B, size, size, DEV, seed=1)
    n = od.numel()
    x = torch.randn(od.shape, device=DEV) * 3.0
    late = (2.0 * od - 1.0) * 4.0 + torch.randn(od.shape, device=DEV)          # right by a margin of 4 +- 1: e > 0 on ~0.1 % of the pixels
    mask = (torch.rand(od.shape, device=DEV) < 0.6).float()
    w = torch.full((1,), 0.01, device=DEV)
    dx = torch.zeros_like(x)
    cfg = OverlapLoss(1.0)
    fns = {"lv_disc": lambda: ops.lovasz_loss(x, od, w, dx=dx), "lv_cup": lambda: ops.lovasz_loss(x, od, w, mask=mask, dx=dx),
           "lv_disc_late": lambda: ops.lovasz_loss(late, od, w, dx=dx), "lv_cup_late": lambda: ops.lovasz_loss(late, od, w, mask=mask, dx=dx),
           "lv_disc_loss_only": lambda: ops.lovasz_loss(x, od, None),
           "ov_disc": lambda: ops.overlap_loss(x, od, w, cfg, dx=dx), "ov_cup": lambda: ops.overlap_loss(x, od, w, cfg, mask=mask, dx=dx)}
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            us[k].append(1e3 * timed(fn, args.calls))
    _, ranks = ops.lovasz_loss(x, od, None, want_ranks=True)
    _, ranks_late = ops.lovasz_loss(late, od, None, want_ranks=True)
    print(json.dumps({"what": "wtpse_lovasz_loss alone (keys, four radix passes, prefix and apply, the mean) beside wtpse_overlap_loss, "
                              "%d planes of %d elements, us per call" % (B, n // B),
                      "positive_errors": {"random": round(float((ranks >= 0).float().mean()), 4),
                                          "late": round(float((ranks_late >= 0).float().mean()), 4)},
                      "ws_bytes": ops.lib().query("wtpse_lovasz_loss_ws", B, n // B),
                      **{k + "_us": spread(v) for k, v in us.items()}}))


def step_with_and_without():
    B = args.batch
    batch = make_batch(B, args.size, args.size, DEV, seed=1)
    variants = {}
    for name in ("plain", "lovasz"):
        nets = bench.build_nets(HP, B // 3, DEV)
        ts = TrainStep(*nets, HP, graph="plan", lovasz=LovaszLoss(1.0) if name == "lovasz" else None)
        for _ in range(args.warmup):
            ts.step(*batch)
        torch.cuda.synchronize()
        variants[name] = ts
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, ts in variants.items():
            ms[name].append(timed(lambda: ts.step(*batch), args.steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps({"what": "TrainStep(graph='plan') ms/step, B=%d %dx%d, %d steps per block" % (B, args.size, args.size, args.steps),
                      "plain": spread(ms["plain"]), "lovasz": spread(ms["lovasz"]),
                      "difference_ms": round(med["lovasz"] - med["plain"], 4),
                      "ratio": round(med["lovasz"] / med["plain"], 5)}))


if __name__ == "__main__":
    loss_alone()
    if not args.no_step:
        step_with_and_without()
