#!/usr/bin/env python3
"""Throughput of the device-side input pipeline against the reference's host path (Pillow, one thread per sample).

    gpurun -- python tools/bench_input_pipeline.py [--batch 32] [--in-size 800]

The augmented leg runs the same samples with all six augmentations on (the natural half of the coins firing) through the device
stage, and through `augment_host` — the numpy restatement of the reference's classes — on one host thread, and compares the two
batches bit for bit.
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]
from wtpse_hip.input_pipeline import Augment, DeviceInputPipeline, augment_host, device_uniform, draw, draw_augment  # noqa: E402


def pillow_crop(img, od, d, S):
    """Resize + RandomScaleCrop as the reference does them per sample (custom_transforms.py), with Pillow itself -> uint8."""
    from PIL import Image
    nw, nh, x1, y1 = d
    im, m = Image.fromarray(img).resize((S, S)), Image.fromarray(od).resize((S, S))
    if (nw, nh) != (S, S):
        im, m = im.resize((nw, nh), Image.BILINEAR), m.resize((nw, nh), Image.NEAREST)
    im, m = im.crop((x1, y1, x1 + S, y1 + S)), m.crop((x1, y1, x1 + S, y1 + S))
    return np.array(im), np.array(m)


def finish(im, mm):
    a = im.astype(np.float32)
    a /= 127.5
    a -= 1.0
    return a.transpose(2, 0, 1), (mm <= 200).astype(np.float32)[None], (mm <= 50).astype(np.float32)[None]


def pillow_path(img, od, d, S):
    """What the reference does per sample without augmentations."""
    return finish(*pillow_crop(img, od, d, S))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--in-size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    S, B, H = 256, a.batch, a.in_size
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, (H, H, 3)).astype(np.uint8) for _ in range(B)]
    ods = [rs.choice(np.array([0, 128, 255], np.uint8), (H, H)) for _ in range(B)]
    rng = random.Random(1)
    draws = [draw(rng, S) for _ in range(B)]
    pipe = DeviceInputPipeline(S, "cuda")
    out = pipe(imgs, ods, draws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        out = pipe(imgs, ods, draws)
    torch.cuda.synchronize()
    t_all = (time.perf_counter() - t0) / a.reps
    dimgs = [torch.from_numpy(x).cuda() for x in imgs]
    dods = [torch.from_numpy(x).cuda() for x in ods]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        out = pipe(dimgs, dods, draws)
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / a.reps
    t0 = time.perf_counter()
    ref = [pillow_path(imgs[i], ods[i], draws[i], S) for i in range(B)]
    t_cpu = time.perf_counter() - t0
    same = all(np.array_equal(out[0][i].cpu().numpy(), ref[i][0]) and np.array_equal(out[1][i].cpu().numpy(), ref[i][1])
               for i in range(B))
    print("batch %d of %dx%d uint8 samples -> [%d,3,256,256] fp32" % (B, H, H, B))
    print("  device pipeline, samples already in HBM : %7.2f ms  (%8.0f images/s)" % (1e3 * t_dev, B / t_dev))
    print("  device pipeline incl. host->device copy : %7.2f ms  (%8.0f images/s)" % (1e3 * t_all, B / t_all))
    print("  reference path (Pillow, one host thread): %7.2f ms  (%8.0f images/s)" % (1e3 * t_cpu, B / t_cpu))
    print("  bit-identical to the Pillow path: %s" % same)
    assert same

    # ---- the augmented leg: all six on, coins as they fall
    aug, np_rng = Augment(), np.random.RandomState(2)
    aug_draws = [draw_augment(rng, np_rng, S, aug) for _ in range(B)]
    active = [i for i, d in enumerate(aug_draws) if d["elastic"]]
    pipe.noise_seed, pipe.noise_pos = 5, 0
    out = pipe(dimgs, dods, draws, aug_draws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        pipe.noise_pos = 0
        out = pipe(dimgs, dods, draws, aug_draws)
    torch.cuda.synchronize()
    t_aug = (time.perf_counter() - t0) / a.reps
    t0 = time.perf_counter()
    for _ in range(a.reps):
        out_plain = pipe(dimgs, dods, draws)
    torch.cuda.synchronize()
    t_plain = (time.perf_counter() - t0) / a.reps
    noise = device_uniform(len(active) * 2 * S * S, 5, 0).cpu().numpy().reshape(len(active), 2, S, S)
    crops = [pillow_crop(imgs[i], ods[i], draws[i], S) for i in range(B)]
    t0 = time.perf_counter()
    ref = [finish(*augment_host(crops[i][0], crops[i][1], aug_draws[i], noise[active.index(i)] if i in active else None))
           for i in range(B)]
    t_host = time.perf_counter() - t0
    same = all(np.array_equal(out[k][i].cpu().numpy(), ref[i][k]) for i in range(B) for k in range(3))
    fired = {k: sum(1 for d in aug_draws if f(d)) for k, f in (
        ("rotate", lambda d: d["k"] > 0), ("flip", lambda d: d["flip_lr"] or d["flip_tb"]), ("elastic", lambda d: d["elastic"]),
        ("salt_pepper", lambda d: d["sp"] is not None), ("light", lambda d: d["lut"] is not None), ("erase", lambda d: d["rect"] is not None))}
    print("augmented batch, all six transforms on, fired: %s" % fired)
    print("  device pipeline with augmentations      : %7.2f ms  (%8.0f images/s)" % (1e3 * t_aug, B / t_aug))
    print("  device pipeline without (same run)      : %7.2f ms  -> the stage costs %.2f ms" % (1e3 * t_plain, 1e3 * (t_aug - t_plain)))
    print("  augmentations alone, numpy restatement of the reference's classes, one host thread: %7.2f ms  (%8.0f images/s)"
          % (1e3 * t_host, B / t_host))
    print("  bit-identical to the host restatement: %s" % same)
    assert same


if __name__ == "__main__":
    main()
