#!/usr/bin/env python3
"""Per-batch cost of the test run's picture stage (wtpse_hip/test_run.py): overlay="device" (ops.overlay, csrc/overlay.hip, plus the
copy of both pictures to the host) against overlay="host" (the image copied to the host, overlay_host in numpy / scipy), the whole
TestRun.batch with either side for scale, and the box's device-to-device copy rate to hold the paint kernel's bytes against.

    python tools/bench_test_run.py [--batch 9] [--size 800] [--reps 20] [--host-reps 2] [--stage-only]

The paint kernel's own time comes from a profiler run of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_test_run.py
--stage-only): `overlay_k` moves 22 bytes per pixel (12 of image, 4 of masks in, 6 of pictures out).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import test_run as T  # noqa: E402


def inputs(B, S, seed):
    """A noisy image, a speckled disc / cup prediction and shifted disc / cup labels per image, uint8 masks [B,1,S,S]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    img = rng.uniform(-1.0, 1.0, (B, 3, S, S)).astype(np.float32)
    ms = [np.zeros((B, 1, S, S), np.uint8) for _ in range(4)]
    for i in range(B):
        cy, cx, r = S * rng.uniform(0.45, 0.55), S * rng.uniform(0.45, 0.55), S * rng.uniform(0.25, 0.33)
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        ms[0][i, 0] = (d2 <= r * r) & (rng.random((S, S)) < 0.98)
        ms[1][i, 0] = d2 <= (0.5 * r) ** 2
        g2 = (yy - cy - 5) ** 2 + (xx - cx + 4) ** 2
        ms[2][i, 0] = g2 <= (0.95 * r) ** 2
        ms[3][i, 0] = g2 <= (0.45 * r) ** 2
    return img, ms


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def copy_rate(nbytes=1 << 28, reps=20):
    """Bytes read + written per second by a device-to-device copy of `nbytes`."""
    a = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    b = torch.empty_like(a)
    return 2 * nbytes / timed(lambda: b.copy_(a), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=9)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--stage-only", action="store_true", help="the device picture stage alone (for a profiler run)")
    a = ap.parse_args()
    B, S = a.batch, a.size
    img, ms = inputs(B, S, S)
    dimg, dms = torch.from_numpy(img).cuda(), [torch.from_numpy(m).cuda() for m in ms]

    def stage_device():
        o, v = ops.overlay(dimg, *dms)
        return torch.cat((o.reshape(-1), v.reshape(-1))).cpu()

    t_kernels = timed(lambda: ops.overlay(dimg, *dms), a.reps)
    if a.stage_only:
        print("ops.overlay, batch %d at %dx%d: %.3f ms per call" % (B, S, S, 1e3 * t_kernels))
        return
    t_dev = timed(stage_device, a.reps)
    t_host = timed(lambda: T.overlay_host_batch(dimg.cpu().numpy(), *ms), a.host_reps)
    o, v = ops.overlay(dimg, *dms)
    ho, hv = T.overlay_host_batch(img, *ms)
    assert np.array_equal(o.cpu().numpy(), ho) and np.array_equal(v.cpu().numpy(), hv)      # the two sides agree on what is timed
    print("picture stage, batch %d at %dx%d:" % (B, S, S))
    print("  device: ops.overlay (gt fill + paint kernel)        : %8.3f ms" % (1e3 * t_kernels))
    print("  device: ops.overlay + both pictures copied to host  : %8.3f ms" % (1e3 * t_dev))
    print("  host  : image copied to host + overlay_host per image: %8.1f ms  (%.1fx the device)" % (1e3 * t_host, t_host / t_dev))
    rate = copy_rate()
    print("  device-to-device copy rate of this box (256 MiB)    : %8.2f TB/s read + written" % (rate / 1e12))
    print("  overlay_k moves %.1f MB per call (22 B per pixel): %.3f ms at the copy rate" % (22e-6 * B * S * S, 22e3 * B * S * S / rate))

    # the whole per-batch body of TestRun with either picture side (metrics on the device in both), default-initialised networks
    nets = T.build_networks("cuda")
    for n in nets:
        n.eval()
    image = torch.from_numpy(inputs(B, 256, 1)[0]).cuda()
    lod, loc = (dms[2] == 1).float(), (dms[3] == 1).float()
    for side, reps in (("device", max(3, a.reps // 4)), ("host", a.host_reps)):
        run = T.TestRun(*nets, out_dir=None, overlay=side, metrics="device")
        print("  TestRun.batch, overlay=%-6s (predict, resize, post-processing, metrics, pictures, copy): %8.1f ms"
              % (side, 1e3 * timed(lambda: run.batch(image, lod, loc), reps)))


if __name__ == "__main__":
    main()
