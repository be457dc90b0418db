#!/usr/bin/env python3
"""Per-batch cost of segmenting unlabelled images (wtpse_hip/segment.py), stage by stage, on one batch of synthetic crops: HIP-event
times of the LANCZOS front (upload excluded and included), the predict pair, the resize + post-processing, the label map + geometry and
the ground-truth-free overlay; and the host equivalents of the NEW stages only — Pillow's LANCZOS resize per image, label_map_host and
mask_geometry_host — on the same data.  The two sides are compared on what they computed before anything is timed.

    python tools/bench_segment.py [--batch 9] [--size 800] [--reps 20] [--host-reps 3]

Reports the median over `reps` repetitions after a warm-up call.  Nothing here is a pass mark: profiles/segment.md records a run.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import segment as SG  # noqa: E402
from wtpse_hip import test_run as T  # noqa: E402
from wtpse_hip import validate as V  # noqa: E402


def crops(B, S, seed):
    """Fundus-like uint8 crops [S,S,3]: noise under a bright blob."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = []
    for _ in range(B):
        cy, cx, r = S * rng.uniform(0.45, 0.55), S * rng.uniform(0.45, 0.55), S * rng.uniform(0.25, 0.33)
        blob = 140.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (1.5 * r) ** 2))
        img = rng.integers(0, 64, (S, S, 3)).astype(np.float32) + blob[:, :, None] * np.array([1.0, 0.6, 0.3], np.float32)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def pseudo_logits(B, seed):
    """+-30 disc and cup logits at 256 x 256: the back stages see non-empty masks whatever the networks predict."""
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


def host_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=9)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    B, S = a.batch, a.size
    images = crops(B, S, S)
    nets = T.build_networks("cuda")
    for n in nets:
        n.eval()
    seg = SG.Segmenter(*nets, out_dir=None, batch_size=B)

    # ---- front
    stack = torch.from_numpy(np.stack(images)).cuda()

    def front_kernels():
        t = seg._lanczos_pass(stack, False) if S != 256 else stack
        t = seg._lanczos_pass(t, True) if S != 256 else t
        return ops.image_finish(t)

    image = seg.front(images)
    want = np.stack([np.array(Image.fromarray(im, "RGB").resize((256, 256), Image.LANCZOS)) for im in images]).astype(np.float32)
    want /= 127.5
    want -= 1.0
    assert np.array_equal(image.cpu().numpy(), want.transpose(0, 3, 1, 2)) and torch.equal(front_kernels(), image)
    t_front_k = event_ms(front_kernels, a.reps)
    t_front = event_ms(lambda: seg.front(images), a.reps)
    t_pillow = host_ms(lambda: [np.array(Image.fromarray(im, "RGB").resize((256, 256), Image.LANCZOS)) for im in images], a.host_reps)

    # ---- predict pair (default-initialised networks: the time does not depend on the weights)
    t_predict = event_ms(lambda: V.predict_pair(*nets, image), max(3, a.reps // 4))

    # ---- back, on injected logits
    lod, loc = pseudo_logits(B, 7)

    def post():
        return ops.postprocess_masks(torch.cat((ops.resize_bilinear(lod, (S, S)), ops.resize_bilinear(loc, (S, S))), 0))

    masks = post()
    disc, cup = masks[:B], masks[B:]
    big = ops.resize_bilinear(image, (S, S))
    hm = masks.cpu().numpy()
    assert hm[:B].any(axis=(1, 2, 3)).all() and hm[B:].any(axis=(1, 2, 3)).all()
    assert np.array_equal(ops.label_map(disc, cup).cpu().numpy(), SG.label_map_host(hm[:B], hm[B:]))
    assert np.array_equal(ops.mask_geometry(masks).cpu().numpy(), SG.mask_geometry_host(hm[:, 0]))
    t_post = event_ms(post, a.reps)
    t_label = event_ms(lambda: ops.label_map(disc, cup), a.reps)
    t_geom = event_ms(lambda: ops.mask_geometry(masks), a.reps)
    t_over = event_ms(lambda: ops.overlay(ops.resize_bilinear(image, (S, S)), disc, cup, None, None), a.reps)
    t_paint = event_ms(lambda: ops.overlay(big, disc, cup, None, None), a.reps)
    zero = torch.zeros_like(disc)
    t_paint_gt = event_ms(lambda: ops.overlay(big, disc, cup, zero, zero), a.reps)
    sizes = [(S, S)] * B
    t_back = event_ms(lambda: seg.back(image, lod, loc, sizes), max(3, a.reps // 4))
    t_label_h = host_ms(lambda: SG.label_map_host(hm[:B], hm[B:]), a.host_reps)
    t_geom_h = host_ms(lambda: SG.mask_geometry_host(hm[:, 0]), a.host_reps)

    print("segmenting a batch of %d crops at %dx%d (median of %d, HIP events; host: median of %d, host clock):" % (B, S, S, a.reps, a.host_reps))
    print("  front, device : two LANCZOS passes + normalisation (kernels only)       : %8.3f ms" % t_front_k)
    print("  front, device : the same with the upload of the decoded images          : %8.3f ms" % t_front)
    print("  front, host   : Pillow Image.resize(LANCZOS) per image                  : %8.1f ms" % t_pillow)
    print("  predict pair  : both stages at 256x256                                   : %8.3f ms" % t_predict)
    print("  back, device  : resize of both logit maps + ops.postprocess_masks       : %8.3f ms" % t_post)
    print("  back, device  : ops.label_map                                           : %8.3f ms" % t_label)
    print("  back, device  : ops.mask_geometry (disc and cup)                        : %8.3f ms" % t_geom)
    print("  back, device  : picture resize + ops.overlay without ground truth       : %8.3f ms" % t_over)
    print("  back, device  : ops.overlay without ground truth alone                  : %8.3f ms" % t_paint)
    print("  back, device  : ops.overlay with an all-zero ground truth, for scale    : %8.3f ms" % t_paint_gt)
    print("  back, device  : Segmenter.back (all of the above + the one copy to host): %8.3f ms" % t_back)
    print("  back, host    : label_map_host                                          : %8.1f ms" % t_label_h)
    print("  back, host    : mask_geometry_host (disc and cup)                       : %8.1f ms" % t_geom_h)


if __name__ == "__main__":
    main()
