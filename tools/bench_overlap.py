#!/usr/bin/env python3
"""What the overlap loss costs (wtpse_hip/overlap.py, csrc/overlap.hip; numbers in profiles/overlap.md).

    python tools/bench_overlap.py            wtpse_overlap_loss alone at B = 32, 256 x 256 — loss only (pass 1, a pass 2 that returns
                                             behind its fold, the mean) and loss + gradient (both passes in full), disc and cup form —
                                             beside wtpse_boundary_loss on the same tensors and wtpse_copy_probe (us, GB/s); then
                                             ms/step of TrainStep(graph="plan") with and without overlap=, alternating in one session
    python tools/bench_overlap.py --no-step  the entry points only (the form to run under a kernel trace: ov_sums_k, ov_apply_k and
                                             bd_loss_k then appear with their own times)

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
from wtpse_hip.overlap import OverlapLoss  # noqa: E402
from wtpse_hip.step import TrainStep  # noqa: E402
from wtpse_hip.synth import default_hparams, make_batch  # noqa: E402

DEV = torch.device("cuda:0")
HP = default_hparams(True)
CFG = OverlapLoss(1.0, fp=0.3, fn=0.7, focal=0.75)


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
    mask = (torch.rand(od.shape, device=DEV) < 0.6).float()
    phi = ops.signed_distance(od)
    w = torch.full((1,), 0.01, device=DEV)
    dx = torch.zeros_like(x)
    src, dst = torch.randn(n, device=DEV), torch.empty(n, device=DEV)
    fns = {"ov_disc_loss_only": lambda: ops.overlap_loss(x, od, None, CFG), "ov_cup_loss_only": lambda: ops.overlap_loss(x, od, None, CFG, mask=mask),
           "ov_disc": lambda: ops.overlap_loss(x, od, w, CFG, dx=dx), "ov_cup": lambda: ops.overlap_loss(x, od, w, CFG, mask=mask, dx=dx),
           "bd_disc": lambda: ops.boundary_loss(x, phi, w, dx=dx), "bd_cup": lambda: ops.boundary_loss(x, phi, w, mask=mask, dx=dx),
           "copy": lambda: ops.lib().call("wtpse_copy_probe", src.data_ptr(), dst.data_ptr(), n, 16, ops.stream_ptr())}
    # bytes per element: pass 1 reads x, t [, mask]; pass 2 reads them again and reads and writes dx.  bd_loss_k: x, phi [, mask], dx twice
    nbytes = {"ov_disc_loss_only": 8, "ov_cup_loss_only": 12, "ov_disc": 8 + 16, "ov_cup": 12 + 20, "bd_disc": 16, "bd_cup": 20, "copy": 8}
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            us[k].append(1e3 * timed(fn, args.calls))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    print(json.dumps({"what": "wtpse_overlap_loss alone (two passes and the mean) beside wtpse_boundary_loss (one pass and its reduction) and "
                              "wtpse_copy_probe (16 bytes per lane), %d elements, us per call" % n,
                      **{k + "_us": spread(v) for k, v in us.items()},
                      **{k + "_GBps": round(nbytes[k] * n / med[k] / 1e3, 1) for k in fns},
                      "ov_disc_pass2_us": round(med["ov_disc"] - med["ov_disc_loss_only"], 2),
                      "ov_cup_pass2_us": round(med["ov_cup"] - med["ov_cup_loss_only"], 2)}))


def step_with_and_without():
    B = args.batch
    batch = make_batch(B, args.size, args.size, DEV, seed=1)
    variants = {}
    for name in ("plain", "overlap"):
        nets = bench.build_nets(HP, B // 3, DEV)
        ts = TrainStep(*nets, HP, graph="plan", overlap=CFG if name == "overlap" else None)
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
                      "plain": spread(ms["plain"]), "overlap": spread(ms["overlap"]),
                      "difference_ms": round(med["overlap"] - med["plain"], 4),
                      "ratio": round(med["overlap"] / med["plain"], 5)}))


if __name__ == "__main__":
    loss_alone()
    if not args.no_step:
        step_with_and_without()
