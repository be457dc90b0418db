#!/usr/bin/env python3
"""Cost of the morphometry pass (ops.onh_profile, csrc/morphometry.hip) on a batch of post-processed-like masks, against its
yardstick in the same process: the two ops.mask_geometry launches over the same two mask stacks, which read exactly the same bytes.
Also the all-ones disc against the ellipse (LDS contention against streaming), the sector count, and Segmenter.back per batch with the
switch off and on (injected logits: no network runs).  The device result is compared with morphometry.profile_host before anything is
timed.

    python tools/bench_morphometry.py [--batch 9] [--sizes 800 2048] [--sectors 24] [--reps 30]

Reports the median over `reps` repetitions after a warm-up call.  Nothing here is a pass mark: profiles/morphometry.md records a run.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]
from wtpse_hip import morphometry as M  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import segment as SG  # noqa: E402


def masks(B, S, seed):
    """B filled discs (radius 0.25 .. 0.33 S, centre jittered) with a cup of half the radius shifted inside: uint8 [B,1,S,S] each."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    disc, cup = np.zeros((B, 1, S, S), np.uint8), np.zeros((B, 1, S, S), np.uint8)
    for i in range(B):
        cy, cx, r = S * rng.uniform(0.45, 0.55), S * rng.uniform(0.45, 0.55), S * rng.uniform(0.25, 0.33)
        disc[i, 0] = ((yy - cy) ** 2 / (0.9 * r) ** 2 + (xx - cx) ** 2 / r ** 2 <= 1.0) * 255
        cup[i, 0] = ((yy - cy - 0.1 * r) ** 2 + (xx - cx + 0.08 * r) ** 2 <= (0.5 * r) ** 2) * 255
    return disc, cup


def pseudo_logits(B, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:256, 0:256]
    lod, loc = np.full((B, 1, 256, 256), -30.0, np.float32), np.full((B, 1, 256, 256), -30.0, np.float32)
    for i in range(B):
        cy, cx, r = 256 * rng.uniform(0.45, 0.55), 256 * rng.uniform(0.45, 0.55), 256 * rng.uniform(0.25, 0.33)
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        lod[i, 0][d2 <= r * r] = 30.0
        loc[i, 0][d2 <= (0.5 * r) ** 2] = 30.0
    return torch.from_numpy(lod).cuda(), torch.from_numpy(loc).cuda()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 2048])
    ap.add_argument("--sectors", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    B, N = a.batch, a.sectors
    for S in a.sizes:
        hd, hc = masks(B, S, S)
        disc, cup = torch.from_numpy(hd).cuda(), torch.from_numpy(hc).cuda()
        geom = ops.mask_geometry(disc)
        prof, mom = ops.onh_profile(disc, cup, geom, N)
        wp, wm = M.profile_host(hd[:1, 0], hc[:1, 0], N)                   # one image: the host pass is slow at this size
        assert np.array_equal(prof[:1].cpu().numpy().view(np.uint32), wp) and np.array_equal(mom[:1].cpu().numpy(), wm)
        ones, none = torch.ones_like(disc), torch.zeros_like(disc)
        g_ones, g_none = ops.mask_geometry(ones), ops.mask_geometry(none)
        both = torch.cat((disc, cup), 0)
        t_pair = event_ms(lambda: (ops.mask_geometry(disc), ops.mask_geometry(cup)), a.reps)
        t_one = event_ms(lambda: ops.mask_geometry(both), a.reps)
        t_onh = event_ms(lambda: ops.onh_profile(disc, cup, geom, N), a.reps)
        t_ones = event_ms(lambda: ops.onh_profile(ones, cup, g_ones, N), a.reps)
        t_none = event_ms(lambda: ops.onh_profile(none, none, g_none, N), a.reps)
        t_pair_ones = event_ms(lambda: (ops.mask_geometry(ones), ops.mask_geometry(cup)), a.reps)
        t_n = {n: event_ms(lambda: ops.onh_profile(disc, cup, geom, n), a.reps) for n in (8, 64, 360) if n != N}
        read = 2 * B * S * S
        wrote = B * N * 16 + B * 64
        print("morphometry pass on %d mask pairs at %dx%d, %d sectors (median of %d, HIP events):" % (B, S, S, N, a.reps))
        print("  object pixels: disc %.1f %%, cup %.1f %%" % (100.0 * (hd != 0).mean(), 100.0 * (hc != 0).mean()))
        print("  bytes per launch: %d read (both masks) + %d records in, %d written (profile %d + moments %d)"
              % (read, B * 64 + (N + 1) * 8, wrote, B * N * 16, B * 64))
        print("  yardstick: ops.mask_geometry(disc) + ops.mask_geometry(cup)   : %8.3f ms" % t_pair)
        print("             the same as one call over both stacks              : %8.3f ms" % t_one)
        print("  ops.onh_profile, ellipse disc with a cup                      : %8.3f ms  = %.2f x the pair, %.0f GB/s" %
              (t_onh, t_onh / t_pair, read / t_onh / 1e6))
        print("  ops.onh_profile, all-ones disc (LDS contention)               : %8.3f ms  = %.2f x the pair on the same masks (%.3f ms)" %
              (t_ones, t_ones / t_pair_ones, t_pair_ones))
        print("  ops.onh_profile, empty masks (streaming alone)                : %8.3f ms" % t_none)
        for n, t in sorted(t_n.items()):
            print("  ops.onh_profile, %3d sectors                                  : %8.3f ms" % (n, t))
    # ---- Segmenter.back, switch off and on
    S = a.sizes[0]
    lod, loc = pseudo_logits(B, 7)
    image = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (B, 3, 256, 256)).astype(np.float32)).cuda()
    sizes = [(S, S)] * B
    off = SG.Segmenter(None, None, None, None, out_dir=None, batch_size=B)
    on = SG.Segmenter(None, None, None, None, out_dir=None, batch_size=B, morphometry=True, sectors=N)
    reps = max(5, a.reps // 3)
    t_off = event_ms(lambda: off.back(image, lod, loc, sizes), reps)
    t_on = event_ms(lambda: on.back(image, lod, loc, sizes), reps)
    t_off2 = event_ms(lambda: off.back(image, lod, loc, sizes), reps)
    print("Segmenter.back on %d crops at %dx%d (median of %d; device work, the one copy and the host's finishing):" % (B, S, S, reps))
    print("  morphometry off : %8.3f ms (repeated after the other: %8.3f ms)" % (t_off, t_off2))
    print("  morphometry on  : %8.3f ms  (+%.3f ms)" % (t_on, t_on - 0.5 * (t_off + t_off2)))


if __name__ == "__main__":
    main()
