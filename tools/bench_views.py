#!/usr/bin/env python3
"""Cost of test-time views (wtpse_hip/views.py): the two launches of csrc/views.hip — the view generator (ops.dihedral_views) and
the fused merge (ops.views_merge) — at 9 x 256^2 with V = 8 views and K = 1 and 8 maps per view, against two yardsticks: the same
results composed from torch ops (flip / transpose / sigmoid / mean / std) in the same process, and the bytes-moved floor at the
copy rate of DESIGN.md section 5 (wtpse_copy_probe over about as many bytes, measured here as well).  Then Segmenter.run per image
for --views none / hflip / d4 on a written folder.  The device results are compared with the host specification
(views.view_host, views.merge_host) and with the torch composition before anything is timed.

    python tools/bench_views.py [--batch 9] [--maps 1 8] [--reps 30] [--rotate 8] [--run [--size 800]]

Median over `reps` repetitions after a warm-up call, HIP events.  One merge at K = 8 reads 151 MB and writes as much: --rotate N
runs the timed launches over N copies of the inputs in turn, so that the working set exceeds the 256 MB Infinity Cache at K = 1 as
well.  Nothing here is a pass mark: profiles/views.md records a run.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tools")]
from bench_segment import crops, event_ms  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import segment as SG  # noqa: E402
from wtpse_hip import test_run as T  # noqa: E402
from wtpse_hip import views as VW  # noqa: E402

S = 256
CODES = tuple(range(8))
COPY_RATE = 5.84e12                                              # the plain streaming copy, bytes/s


def torch_view(x, c):
    if c & 4:
        x = x.transpose(-1, -2)
    if c & 2:
        x = x.flip(-2)
    if c & 1:
        x = x.flip(-1)
    return x


def torch_unview(x, c):
    if c & 1:
        x = x.flip(-1)
    if c & 2:
        x = x.flip(-2)
    if c & 4:
        x = x.transpose(-1, -2)
    return x


def composed_views(x):
    return torch.stack([torch_view(x, c).contiguous() for c in CODES])


def composed_merge(logits):
    """[V,B,K,S,S] -> (mean, std, votes, logits [B,V*K,S,S], mean_logit) from torch ops."""
    out = torch.cat([torch_unview(logits[v], c) for v, c in enumerate(CODES)], 1).contiguous()
    p = torch.sigmoid(out)
    return (p.mean(1, keepdim=True), p.std(1, keepdim=True, unbiased=False), (p > 0.75).sum(1, keepdim=True).to(torch.uint8), out,
            out.mean(1, keepdim=True))


def rotating(fn, sets):
    state = {"i": 0}

    def call():
        fn(sets[state["i"] % len(sets)])
        state["i"] += 1
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=9)
    ap.add_argument("--maps", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rotate", type=int, default=8, help="copies of the inputs the timed launches rotate through")
    ap.add_argument("--run", action="store_true", help="also time Segmenter.run per image for --views none / hflip / d4")
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args()
    B, V = a.batch, len(CODES)
    g = torch.Generator(device="cuda").manual_seed(5)

    n = B * S * S * 64
    src, dst = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    t_copy = event_ms(lambda: ops.lib().call("wtpse_copy_probe", src.data_ptr(), dst.data_ptr(), n, 16, ops.stream_ptr()), a.reps)
    here = 2 * 4 * n / (t_copy * 1e-3)
    print("copy probe, %.0f MB each way: %.3f ms = %.2f TB/s here (DESIGN.md section 5: %.2f TB/s)" % (4 * n / 1e6, t_copy, here / 1e12, COPY_RATE / 1e12))
    del src, dst

    # ---- the generator: 3 channels in, V x 3 out
    x = torch.randn((B, 3, S, S), device="cuda", generator=g)
    got = ops.dihedral_views(x, CODES)
    assert all(np.array_equal(got[v].cpu().numpy(), VW.view_host(x.cpu().numpy(), c)) for v, c in enumerate(CODES)), "generator != view_host"
    assert torch.equal(got, composed_views(x))
    sets = [x] + [x.clone() for _ in range(a.rotate - 1)]
    nbytes = 4 * B * 3 * S * S * (1 + V)
    t_f = event_ms(rotating(lambda t: ops.dihedral_views(t, CODES), sets), a.reps * len(sets))
    t_c = event_ms(rotating(composed_views, sets), a.reps * len(sets))
    print("generator  B = %d, V = %d          : fused %7.3f ms (%.2f TB/s of %.1f MB; floor at the copy rate %.3f ms), torch %7.3f ms, ratio %.1f"
          % (B, V, t_f, nbytes / (t_f * 1e-3) / 1e12, nbytes / 1e6, 1e3 * nbytes / COPY_RATE, t_c, t_c / t_f))

    # ---- the merge
    for K in a.maps:
        logits = 2.0 * torch.randn((V, B, K, S, S), device="cuda", generator=g)
        f, c = ops.views_merge(logits, CODES), composed_merge(logits)
        want = VW.merge_host(logits[:, :1].cpu().numpy(), CODES)                # the first image against the host specification
        assert np.array_equal(f[3][:1].cpu().numpy(), want["logits"]) and f[4][:1, 0].cpu().numpy().tobytes() == want["mean_logit"].tobytes()
        assert float(np.abs(f[0][:1, 0].cpu().numpy() - want["mean"]).max()) < 1e-4 and float(np.abs(f[1][:1, 0].cpu().numpy() - want["std"]).max()) < 1e-4
        assert torch.equal(f[3], c[3]) and float((f[0] - c[0]).abs().max()) < 1e-4 and float((f[1] - c[1]).abs().max()) < 1e-3
        assert float((f[2] != c[2]).float().mean()) < 1e-3 and float((f[4] - c[4]).abs().max()) < 1e-4, "the two paths disagree"
        sets = [logits] + [logits.clone() for _ in range(a.rotate - 1)]
        for label, wl, nb in (("all outputs", True, 4 * B * S * S * (2 * V * K + 3) + B * S * S), ("no logits_out", False, 4 * B * S * S * (V * K + 3) + B * S * S)):
            t_f = event_ms(rotating(lambda t: ops.views_merge(t, CODES, 0.75, wl, True), sets), a.reps * len(sets))
            line = "merge      B = %d, V = %d, K = %d, %-13s: fused %7.3f ms (%.2f TB/s of %.1f MB; floor at the copy rate %.3f ms)" \
                % (B, V, K, label, t_f, nb / (t_f * 1e-3) / 1e12, nb / 1e6, 1e3 * nb / COPY_RATE)
            if wl:
                t_c = event_ms(rotating(composed_merge, sets), max(3, a.reps // 3) * len(sets))
                line += ", torch %7.3f ms, ratio %.1f" % (t_c, t_c / t_f)
            print(line)
        del sets, logits, f, c

    if not a.run:
        return
    nets = T.build_networks("cuda")
    for net in nets:
        net.eval()
        net.ensure_ready(repack=True)
    images = crops(B, a.size, a.size)
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "in")
        os.makedirs(folder)
        for i, im in enumerate(images):
            Image.fromarray(im).save(os.path.join(folder, "%02d.png" % i))
        times = {}
        for views in ("none", "hflip", "d4") * 2:                               # the first round warms up
            t0 = time.perf_counter()
            SG.Segmenter(*nets, out_dir=os.path.join(tmp, views), batch_size=B, views=views).run(folder)
            torch.cuda.synchronize()
            times[views] = 1e3 * (time.perf_counter() - t0) / B
        print("Segmenter.run on %d files of %dx%d, decoding and PNG writing included (host clock, second of two runs), per image: "
              "none %.1f ms, hflip %.1f ms, d4 %.1f ms" % (B, a.size, a.size, times["none"], times["hflip"], times["d4"]))


if __name__ == "__main__":
    main()
