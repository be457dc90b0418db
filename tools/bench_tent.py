#!/usr/bin/env python3
"""Cost of test-time entropy minimisation (wtpse_hip/tent.py): images/s of TentStep.step at B = 9 and 32, 3 x 256 x 256, with
affine_only on and off and in both statistics modes, beside validate.predict_pair alone on the same inputs (train-mode and eval-mode
BatchNorm, what stats="batch" / "frozen" predict with), and the entropy call alone against a device copy of the same bytes.

    python tools/bench_tent.py [--batches 9 32] [--reps 10] [--out profiles/tent.md]

Median over `reps` repetitions after a warm-up call, HIP events; the variants of one batch size alternate in one process, twice (the
first round warms every variant up).  The parent commit has no counterpart of the step: the comparison is predict_pair and
affine_only=False in the same run.  Nothing here is a pass mark; the table is written to --out.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tools")]
from bench_segment import event_ms  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import tent  # noqa: E402
from wtpse_hip import test_run as T  # noqa: E402
from wtpse_hip import validate as V  # noqa: E402

S = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[9, 32])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tent.md"))
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(7)
    nets = T.build_networks("cuda")
    for net in nets:
        net.eval()
        net.ensure_ready(repack=True)
    lines = ["| B | stats | predict_pair, images/s | step affine_only, images/s | of predict_pair | step with weight gradients, images/s | affine_only gain |",
             "|---|---|---|---|---|---|---|"]
    for B in a.batches:
        x = torch.randn((B, 3, S, S), device="cuda", generator=g).clamp_(-1, 1)
        for stats in tent.STATS:
            steps = {on: tent.TentStep(*nets, stats=stats, affine_only=on) for on in (True, False)}

            def predict():
                for n, seg in zip(nets, (True, False, True, False)):
                    n.train(seg and stats == "batch")
                V.predict_pair(*nets, x)
            t = {}
            for _ in range(2):
                t["predict"] = event_ms(predict, a.reps)
                t["on"] = event_ms(lambda: steps[True].step(x), a.reps)
                t["off"] = event_ms(lambda: steps[False].step(x), a.reps)
            ips = {k: 1e3 * B / v for k, v in t.items()}
            lines.append("| %d | %s | %.1f | %.1f | %.2f | %.1f | %.2f |" % (B, stats, ips["predict"], ips["on"], ips["on"] / ips["predict"],
                                                                        ips["off"], ips["on"] / ips["off"]))
    # ---- the entropy call alone: two reads of x and one write of dx (12 bytes per pixel) beside a device copy that moves the same bytes
    lines += ["", "| logits | entropy_loss (value + gradient), us | GB/s | copy of the same bytes, us | ratio | value only, us |", "|---|---|---|---|---|---|"]
    for B in a.batches:
        n = B * S * S
        x = torch.randn((B, 1, S, S), device="cuda", generator=g) * 3.0
        src, dst = torch.empty(3 * n // 2 // 4 * 4, device="cuda"), torch.empty(3 * n // 2 // 4 * 4, device="cuda")
        reps = 10 * a.reps
        t_e = event_ms(lambda: ops.entropy_loss(x), reps)
        t_v = event_ms(lambda: ops.entropy_loss(x, want_grad=False), reps)
        t_c = event_ms(lambda: ops.lib().call("wtpse_copy_probe", src.data_ptr(), dst.data_ptr(), src.numel(), 16, ops.stream_ptr()), reps)
        lines.append("| %d x 1 x %d x %d | %.1f | %.0f | %.1f | %.2f | %.1f |" % (B, S, S, 1e3 * t_e, 12 * n / (t_e * 1e6), 1e3 * t_c, t_e / t_c, 1e3 * t_v))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Test-time entropy minimisation: cost on one MI355X (tools/bench_tent.py)\n\n"
                "Median of %d repetitions, HIP events, 3 x %d x %d inputs, default arithmetic; the variants of a row alternate in one process.\n"
                "A step is, per stage, one taped forward, the entropy call, the backward and one Adam launch over the BatchNorm affines.\n\n" % (a.reps, S, S)
                + text)


if __name__ == "__main__":
    main()
