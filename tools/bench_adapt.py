#!/usr/bin/env python3
"""Cost of BatchNorm adaptation to a target site (wtpse_hip/adapt.py): validate.predict_pair at B = 9 and 32, 256 x 256, in plain
eval mode and blended (batch and stream), the finalize launch alone (wtpse_bn_finalize_blend beside wtpse_bn_eval_coeffs and
wtpse_bn_finalize on the same partials), and SiteStatistics.fit per image on device batches.

    python tools/bench_adapt.py [--batches 9 32] [--reps 20] [--fit-images 36]

Median over `reps` repetitions after a warm-up call, HIP events; the variants of one batch size alternate in one process.  A blended
call pays the statistics epilogues of the convolutions and of the upsampling plus one small launch per BatchNorm layer, and saves the
eval path's wtpse_act_bound launches.  Nothing here is a pass mark: profiles/adapt.md records a run.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tools")]
from bench_segment import event_ms  # noqa: E402
from wtpse_hip import adapt as A  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import test_run as T  # noqa: E402
from wtpse_hip import validate as V  # noqa: E402

S = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[9, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-images", type=int, default=36)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(7)
    nets = T.build_networks("cuda")
    for net in nets:
        net.eval()
        net.ensure_ready(repack=True)
    print("| B | plain eval, ms | blended batch, ms | ratio | blended stream, ms | ratio |")
    print("|---|---|---|---|---|---|")
    for B in a.batches:
        x = torch.randn((B, 3, S, S), device="cuda", generator=g).clamp_(-1, 1)
        batch, stream = A.BlendState(16, "batch"), A.BlendState(16, "stream")

        def blended(state):
            with A.blended(nets, state):
                V.predict_pair(*nets, x)
        t = {}
        for _ in range(2):                                                    # the first round warms every variant up
            t["plain"] = event_ms(lambda: V.predict_pair(*nets, x), a.reps)
            t["batch"] = event_ms(lambda: blended(batch), a.reps)
            t["stream"] = event_ms(lambda: blended(stream), a.reps)
        print("| %d | %.3f | %.3f | %.3f | %.3f | %.3f |" % (B, t["plain"], t["batch"], t["batch"] / t["plain"], t["stream"], t["stream"] / t["plain"]))

    # ---- the finalize alone: the partials of a 32-channel layer at B = 32, 256 x 256 (8192 rows) and of a 256-channel one at 16 x 16
    print()
    print("| partials [nblk, C] | bn_finalize_blend, us | with acc + moments + div + amax, us | bn_finalize, us | bn_eval_coeffs, us |")
    print("|---|---|---|---|---|")
    for nblk, C in ((8192, 32), (64, 256), (288, 64)):
        part = torch.randn((nblk, C, 2), device="cuda", generator=g).abs_()
        gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        rmean, rvar = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
        acc = torch.zeros((C, 2), dtype=torch.float64, device="cuda")
        mom, div = torch.empty((C, 4), dtype=torch.float64, device="cuda"), torch.empty(C, dtype=torch.float64, device="cuda")
        tab = torch.zeros(ops.AMAX_WORDS, dtype=torch.int32, device="cuda")
        count = nblk * 256
        reps = 10 * a.reps
        t_b = event_ms(lambda: ops.bn_finalize_blend(part, count, gamma, beta, rmean, rvar, 0.36), reps)
        t_f = event_ms(lambda: ops.bn_finalize_blend(part, count, gamma, beta, rmean, rvar, 0.36, acc=acc, acc_count=count, moments=mom,
                                                     div=div, act_amax=tab), reps)
        t_s = event_ms(lambda: ops.bn_finalize(part, count, gamma, beta, rmean, rvar, nbt), reps)
        t_e = event_ms(lambda: ops.bn_eval_coeffs(gamma, beta, rmean, rvar), reps)
        print("| %d x %d | %.2f | %.2f | %.2f | %.2f |" % (nblk, C, 1e3 * t_b, 1e3 * t_f, 1e3 * t_s, 1e3 * t_e))

    # ---- site fitting: one stream pass over device batches of 9, per image
    n = max(9, a.fit_images // 9 * 9)
    batches = [torch.randn((9, 3, S, S), device="cuda", generator=g).clamp_(-1, 1) for _ in range(n // 9)]
    fit = A.SiteStatistics(*nets, prior=16, batch_size=9)
    ms = event_ms(lambda: fit.fit(batches), 3)
    plain = event_ms(lambda: [V.predict_pair(*nets, b) for b in batches], 3)
    print()
    print("SiteStatistics.fit over %d images in batches of 9 (checkpoint dict included): %.2f ms per image; predict_pair alone in "
          "plain eval mode: %.2f ms per image" % (n, ms / n, plain / n))


if __name__ == "__main__":
    main()
