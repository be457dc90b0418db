#!/usr/bin/env python3
"""Per-batch cost of the validation back half (post-processing + Dice + ASD / HD95 of both classes): the host path of
validate.validate_epoch (scipy, one image at a time) against metrics="device" (csrc/postprocess.hip), with the front half
(validate.predict_pair) for scale.

    python tools/bench_validate.py [--batch 32] [--sizes 256 512] [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]
from wtpse_hip import ops, validate as V  # noqa: E402


def inputs(B, S, seed):
    """Disc-shaped logits with noise (a few stray blobs and holes after thresholding) and disc labels, both classes."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    out = []
    for r in (S / 3, S / 6):                                    # disc, cup
        cy = S / 2 + torch.randn(B, 1, 1, 1, generator=g) * 4
        cx = S / 2 + torch.randn(B, 1, 1, 1, generator=g) * 4
        inside = ((yy - cy) ** 2 + (xx - cx) ** 2) < r * r
        logits = 6.0 * inside.float() - 3.0 + 2.5 * torch.randn(B, 1, S, S, generator=g)
        label = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (r * 1.05) ** 2).float().expand(B, 1, S, S).contiguous()
        out += [logits.cuda(), label.cuda()]
    return out


def host_back_half(pred, pred_oc, label_od, label_oc):
    """validate_epoch's per-image loop on the host (labels copied once per batch, as there)."""
    lod, loc = label_od.cpu().numpy(), label_oc.cpu().numpy()
    acc = 0.0
    for i in range(pred.shape[0]):
        post, post_oc = V.postprocess(pred[i])[0], V.postprocess(pred_oc[i])[0]
        acc += V.dice(post, lod[i, 0]) + V.dice(post_oc, loc[i, 0])
        acc += sum(V.surface_metrics(post_oc, loc[i, 0])) + sum(V.surface_metrics(post, lod[i, 0]))
    return acc


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def front_half_time(B, S, reps):
    import algorithms
    import shape_networks
    from wtpse_hip.synth import default_hparams
    hp = default_hparams(True)
    mk = lambda ts: algorithms.WT_PSE(3, 1, hp, "cuda", ts, per_domain_batch=1, source_domain_num=3).to("cuda")
    mks = lambda: shape_networks.ShapeVariationalDist_x(hp, "cuda", 1, 3, 1).to("cuda")
    nets = [mk(False), mks(), mk(True), mks()]
    for n in nets:
        n.eval()
    img = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    return timed(lambda: V.predict_pair(*nets, img, (S, S)), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--no-front", action="store_true")
    a = ap.parse_args()
    B = a.batch
    for S in a.sizes:
        pred, lod, pred_oc, loc = inputs(B, S, S)
        t_kern = timed(lambda: ops.seg_metrics(ops.postprocess_masks(torch.cat((pred, pred_oc), 0)), torch.cat((lod, loc), 0)), a.reps)
        t_dev = timed(lambda: V.device_metrics(pred, pred_oc, lod, loc), a.reps)
        t_host = timed(lambda: host_back_half(pred, pred_oc, lod, loc), a.host_reps)
        # the two paths agree on this batch (Dice / HD95 bitwise, ASD to 1e-12)
        d = V.device_metrics(pred, pred_oc, lod, loc)
        p0 = V.postprocess(pred[0])[0]
        assert d["disc_dice"][0] == V.dice(p0, lod[0, 0].cpu().numpy())
        hd, asd = V.surface_metrics(p0, lod[0, 0].cpu().numpy())
        assert d["disc_hd"][0] == hd and abs(d["disc_asd"][0] - asd) <= 1e-12 * asd
        print("batch %d, %dx%d, both classes (%d images):" % (B, S, S, 2 * B))
        print("  device back half, kernels (postprocess + metrics) : %8.3f ms" % (1e3 * t_kern))
        print("  device back half, device_metrics incl. copy+finish: %8.3f ms" % (1e3 * t_dev))
        print("  host back half (scipy, one image at a time)       : %8.1f ms  (%.1fx the device)" % (1e3 * t_host, t_host / t_dev))
        if not a.no_front:
            print("  front half (predict_pair), for scale              : %8.3f ms" % (1e3 * front_half_time(B, S, max(3, a.reps // 4))))


if __name__ == "__main__":
    main()
