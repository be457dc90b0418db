#!/usr/bin/env python3
"""What the boundary loss costs (wtpse_hip/boundary.py, csrc/boundary.hip; numbers in profiles/boundary.md).

    python tools/bench_boundary.py           wtpse_signed_distance alone at B = 32, 256 x 256 and 512 x 512 (us, planes/s, the row
                                             pass's scanned words per second); wtpse_boundary_loss alone beside wtpse_copy_probe
                                             (GB/s); then ms/step of TrainStep(graph="plan") with and without boundary=,
                                             alternating in one session
    python tools/bench_boundary.py --no-step the two kernels only

Time is taken with device events around the launches / the replayed steps; nothing synchronises inside a timed block.  The labels
are synth.make_batch's discs (a disc and a cup per image), as in bench.py.
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
ap.add_argument("--calls", type=int, default=100, help="kernel launches per timed block")
ap.add_argument("--no-step", action="store_true")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

import torch  # noqa: E402

import bench  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip.boundary import BoundaryLoss  # noqa: E402
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


def distance_alone(size):
    B = args.batch
    _, od, oc = make_batch(B, size, size, DEV, seed=1)
    out = {}
    for name, t in (("disc", od), ("cup", oc)):
        phi, d2_out, d2_in = ops.signed_distance(t, want_d2=True)
        # what the row pass does: a pixel at squared distance d2 from the other set scans ~2 sqrt(d2) words of the staged row
        scanned = float((2.0 * torch.sqrt(torch.maximum(d2_out, d2_in).double())).sum().item())
        for _ in range(10):
            ops.signed_distance(t)
        torch.cuda.synchronize()
        us = [1e3 * timed(lambda: ops.signed_distance(t), args.calls) for _ in range(args.rounds)]
        med = sorted(us)[len(us) // 2]
        out[name] = {"us": spread(us), "planes_per_s": round(B / med * 1e6), "scanned_words_per_call": round(scanned),
                     "scanned_Gwords_per_s": round(scanned / med / 1e3, 1), "mean_abs_phi": round(float(phi.abs().mean().item()), 2),
                     "label_and_phi_GBps": round(8.0 * t.numel() / med / 1e3, 1)}
    print(json.dumps({"what": "wtpse_signed_distance alone (column pass + row pass), B=%d %dx%d, us per call" % (B, size, size), **out}))


def loss_alone():
    B, size = args.batch, args.size
    _, od, _ = make_batch(B, size, size, DEV, seed=1)
    n = od.numel()
    x = torch.randn(od.shape, device=DEV) * 3.0
    mask = (torch.rand(od.shape, device=DEV) < 0.6).float()
    phi = ops.signed_distance(od)
    alpha = torch.full((1,), 0.01, device=DEV)
    dx = torch.zeros_like(x)
    src, dst = torch.randn(n, device=DEV), torch.empty(n, device=DEV)
    fns = {"disc_loss_only": lambda: ops.boundary_loss(x, phi, None), "disc": lambda: ops.boundary_loss(x, phi, alpha, dx=dx),
           "cup": lambda: ops.boundary_loss(x, phi, alpha, mask=mask, dx=dx),
           "copy": lambda: ops.lib().call("wtpse_copy_probe", src.data_ptr(), dst.data_ptr(), n, 16, ops.stream_ptr())}
    nbytes = {"disc_loss_only": 8, "disc": 16, "cup": 20, "copy": 8}          # per element: x, phi [, mask] read, dx read and written
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            us[k].append(1e3 * timed(fn, args.calls))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    print(json.dumps({"what": "wtpse_boundary_loss alone (the pass and its one-block reduction) beside wtpse_copy_probe (16 bytes per lane), "
                              "%d elements, us per call" % n,
                      **{k + "_us": spread(v) for k, v in us.items()},
                      **{k + "_GBps": round(nbytes[k] * n / med[k] / 1e3, 1) for k in fns}}))


def step_with_and_without():
    B = args.batch
    batch = make_batch(B, args.size, args.size, DEV, seed=1)
    variants = {}
    for name in ("plain", "boundary"):
        nets = bench.build_nets(HP, B // 3, DEV)
        ts = TrainStep(*nets, HP, graph="plan", boundary=BoundaryLoss(0.01, 0.0, 1.0) if name == "boundary" else None)
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
                      "plain": spread(ms["plain"]), "boundary": spread(ms["boundary"]),
                      "difference_ms": round(med["boundary"] - med["plain"], 4),
                      "ratio": round(med["boundary"] / med["plain"], 5)}))


if __name__ == "__main__":
    distance_alone(256)
    distance_alone(512)
    loss_alone()
    if not args.no_step:
        step_with_and_without()
