#!/usr/bin/env python3
"""Cost of sampled shape latents (wtpse_hip/uncertainty.py): the fused launch (ops.shape_samples) against the same K samples composed
from the entry points that existed before it — per sample ops.randn, ops.reparam_fwd, ops.attn_fuse_fwd, the outc convolution and a
torch accumulation of sum, sum of squares and votes — on the same tensors; the achieved bytes/s of the fused launch against the box's
copy rate (wtpse_copy_probe over as many bytes); the stages of Segmenter.run on one batch with and without samples; the per-sample
post-processing alone; and Segmenter.run as a whole on a written folder.  The two paths are compared on what they computed before
anything is timed.

    python tools/bench_uncertainty.py [--batches 9 32] [--samples 8 32] [--run-samples 16] [--size 800] [--reps 20]

Median over `reps` repetitions after a warm-up call, HIP events.  Nothing here is a pass mark: profiles/uncertainty.md records a run.
"""
import argparse
import os
import sys
import tempfile
import time

import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tools")]
from bench_segment import crops, event_ms  # noqa: E402
from wtpse_hip import nn as E  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import segment as SG  # noqa: E402
from wtpse_hip import test_run as T  # noqa: E402
from wtpse_hip import validate as V  # noqa: E402

S = 256


def launch_pair(net, B, K, seed):
    """-> (fused, composed): two closures over the same random emb / mu / logvar, each -> (mean, std, votes)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    emb = torch.randn((B, 8, S, S), device="cuda", generator=g)
    mu = torch.randn((B, 1, S, S), device="cuda", generator=g)
    logvar = torch.rand((B, 1, S, S), device="cuda", generator=g) * 5.0 - 4.0
    coef = float(net.hparams["shape_attention_coeffient"])
    wb, outc = net.attention_layer.layer1.weight.data_ptr(), net.outc[0]

    def fused(noise=None):
        return ops.shape_samples(emb, mu, logvar, wb, coef, outc.weight.data_ptr(), outc.bias.data_ptr(), 0, K, 11, 0, 1.0, noise)[:3]

    def composed(noise=None):
        """noise None: one ops.randn launch per sample (other numbers than the fused launch draws — the cost is what is timed)."""
        s1, s2 = torch.zeros_like(mu), torch.zeros_like(mu)
        votes = torch.zeros(mu.shape, dtype=torch.uint8, device="cuda")
        with ops.fwd_scope(emb.device):
            for k in range(K):
                eps = ops.randn((B, 1, S, S), "cuda", 11, k * B * S * S) if noise is None else noise[:, k:k + 1].contiguous()
                z = ops.reparam_fwd(mu, logvar, eps)
                fuse = ops.attn_fuse_fwd(z, wb, emb, coef, False, False, False)[3]
                p = torch.sigmoid(E._conv(outc, fuse)[0])
                s1 += p
                s2 += p * p
                votes += p > 0.75
        mean = s1 / K
        return mean, (s2 / K - mean * mean).clamp_min(0).sqrt(), votes

    return fused, composed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[9, 32])
    ap.add_argument("--samples", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--run-samples", type=int, default=16)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    nets = T.build_networks("cuda")
    for n in nets:
        n.eval()
        n.ensure_ready(repack=True)

    print("fused launch against the composed path at %dx%d (median of %d, HIP events):" % (S, S, a.reps))
    for B in a.batches:
        n = B * S * S * 12                                       # floats: the copy probe moves about as many bytes as the fused launch
        src, dst = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        t_copy = event_ms(lambda: ops.lib().call("wtpse_copy_probe", src.data_ptr(), dst.data_ptr(), n, 16, ops.stream_ptr()), a.reps)
        copy_rate = 2 * 4 * n / (t_copy * 1e-3)
        print("  B = %2d: copy probe, %.1f MB each way: %.3f ms = %.2f TB/s" % (B, 4 * n / 1e6, t_copy, copy_rate / 1e12))
        for K in a.samples:
            fused, composed = launch_pair(nets[0], B, K, 100 * B + K)
            noise = ops.randn((B, K, S, S), "cuda", 11, 0)
            f, c = fused(noise), composed(noise)
            assert all(torch.equal(x, y) for x, y in zip(f, fused()))
            torch.cuda.synchronize()
            assert float((f[0] - c[0]).abs().max()) < 1e-4 and float((f[1] - c[1]).abs().max()) < 2e-3, "the two paths disagree"
            assert float((f[2] != c[2]).float().mean()) < 1e-3
            t_f, t_c = event_ms(fused, a.reps), event_ms(composed, max(3, a.reps // 4))
            nbytes = B * S * S * (4 * 10 + 9)                    # emb, mu, logvar in; mean, std, votes out
            print("  B = %2d, K = %2d: fused %8.3f ms (%.2f TB/s of its %d bytes per pixel = %.0f %% of the copy rate), composed %9.3f ms "
                  "(%d launches + torch accumulation), ratio %.1f" % (B, K, t_f, nbytes / (t_f * 1e-3) / 1e12, 49,
                                                                     100.0 * nbytes / (t_f * 1e-3) / copy_rate, t_c, 4 * K, t_c / t_f))

    # ---- the stages of one Segmenter batch
    K, B = a.run_samples, a.batches[0]
    images = crops(B, a.size, a.size)
    sizes = [(a.size, a.size)] * B
    plain = SG.Segmenter(*nets, out_dir=None, batch_size=B)
    samp = SG.Segmenter(*nets, out_dir=None, batch_size=B, samples=K)
    image = plain.front(images)
    reps = max(3, a.reps // 4)
    pred, pred_oc, disc, cup = V.predict_pair_samples(*nets, image, K, 0, 0, 1.0, want_logits=True)
    t_pair = event_ms(lambda: V.predict_pair(*nets, image), reps)
    t_pair_s = event_ms(lambda: V.predict_pair_samples(*nets, image, K, 0, 0, 1.0, want_logits=True), reps)
    t_back = event_ms(lambda: plain.back(image, pred, pred_oc, sizes), reps)
    t_back_s = event_ms(lambda: samp.back(image, pred, pred_oc, sizes, (disc.std, cup.std)), reps)
    t_post = event_ms(lambda: samp.back_samples(disc, cup), reps)
    both = torch.cat((disc.logits.reshape(B * K, 1, S, S), cup.logits.reshape(B * K, 1, S, S)), 0)
    t_post_k = event_ms(lambda: ops.mask_geometry(ops.postprocess_masks(both)), reps)
    print("one batch of %d crops at %dx%d, %d samples (median of %d):" % (B, a.size, a.size, K, reps))
    print("  predict_pair                                                   : %8.3f ms" % t_pair)
    print("  predict_pair_samples (logits kept)                             : %8.3f ms" % t_pair_s)
    print("  Segmenter.back                                                 : %8.3f ms" % t_back)
    print("  Segmenter.back with the two spread maps                        : %8.3f ms" % t_back_s)
    print("  per-sample post-processing: back_samples (kernels, copy, host) : %8.3f ms" % t_post)
    print("  per-sample post-processing: its two kernels on %4d maps alone : %8.3f ms" % (2 * B * K, t_post_k))

    # ---- the whole run on a written folder
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        for i, im in enumerate(images):
            Image.fromarray(im).save(os.path.join(src, "%02d.png" % i))
        times = {}
        for label, k in (("plain", 0), ("samples", K), ("plain", 0), ("samples", K)):       # alternating; the first pair warms up
            t0 = time.perf_counter()
            SG.Segmenter(*nets, out_dir=os.path.join(tmp, label), batch_size=B, samples=k).run(src)
            torch.cuda.synchronize()
            times[label] = 1e3 * (time.perf_counter() - t0)
        print("Segmenter.run on %d files, decoding and PNG writing included (host clock, second of two runs): %.1f ms without, %.1f ms with "
              "%d samples" % (B, times["plain"], times["samples"], K))


if __name__ == "__main__":
    main()
