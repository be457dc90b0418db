#!/usr/bin/env python3
"""What the JPEG compression stage (csrc/jpeg.hip) costs -> profiles/jpeg.md.

    python tools/bench_jpeg.py [--out profiles/jpeg.md] [--reps 30] [--inner 20]

One batch of B = 32 samples at S = 256 and at S = 512 already in HBM, in the same run and alternating:
  * the stage (`ops.jpeg_roundtrip`: the parameter checks, three small uploads, the launches) with every sample 4:4:4, every sample
    4:2:0, and a drawn mix (`draw_jpeg` with `JpegCompression()`'s defaults: about half the samples copied);
  * the launches alone with the tables already on the device (`wtpse_jpeg_roundtrip`);
  * the image-quality stage on the same batch, every operation on (blur included);
  * a plain device copy of the batch (`Tensor.copy_`: 3 S^2 B bytes read and as many written).
A figure is the time between two device events around --inner back-to-back calls, divided by --inner; median (minimum .. maximum) of
--reps such windows.  There is no bar: the stage is new.  The table also gives the bytes a variant moves through HBM by design and
the rate that makes, as a fraction of the copy's.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "wt-pse-code_amd"), os.path.join(HERE, "tests"), os.path.join(HERE, "tools")]

from stage_bench import alternate, write_profile  # noqa: E402

B = 32


def variants(S):
    """-> {name: (callable, bytes moved through HBM by design)}, what must stay referenced."""
    from test_quality_cpu import K_STD10, params_row, pictures
    from wtpse_hip import ops
    from wtpse_hip.input_pipeline import JpegCompression, draw_jpeg, jpeg_reciprocals, jpeg_tables
    from wtpse_hip.lib import lib
    img = torch.from_numpy(pictures(7, B, S)).cuda()
    out = torch.empty_like(img)
    chroma = torch.empty((B, 2, S // 2, S // 2), dtype=torch.uint8, device="cuda")
    px = S * S
    drawn = draw_jpeg(np.random.RandomState(5), B, JpegCompression())
    cases = {"all 4:4:4, quality 75": (np.full(B, 1), np.broadcast_to(jpeg_tables(75), (B, 2, 64))),
             "all 4:2:0, quality 75": (np.full(B, 2), np.broadcast_to(jpeg_tables(75), (B, 2, 64))),
             "drawn mix (%d copied, %d 4:4:4, %d 4:2:0)" % tuple(int((drawn[0] == m).sum()) for m in (0, 1, 2)): drawn}
    fns, keep = {}, [img, out, chroma]
    for name, (mode, tables) in cases.items():
        mode, tables = np.ascontiguousarray(mode), np.ascontiguousarray(tables)
        # by design: 3 px in and 3 px out per sample; a 4:2:0 sample is read once more and its chroma (px / 2) written and read
        moved = int(sum({0: 6, 1: 6, 2: 10}[int(m)] for m in mode)) * px
        fns["stage: " + name] = ((lambda m=mode, t=tables: ops.jpeg_roundtrip(img, m, t)), moved)
        d = [torch.from_numpy(a.astype(np.int32)).cuda() for a in (mode, tables, jpeg_reciprocals(tables))]
        keep.append(d)
        c = chroma.data_ptr() if (mode == 2).any() else 0
        fns["launches alone: " + name] = ((lambda d=d, c=c: lib().call(
            "wtpse_jpeg_roundtrip", img.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), c, out.data_ptr(), B, S,
            ops.stream_ptr())), moved)
    q = np.stack([params_row(a=300, c=330, beta=2500, k=K_STD10, sigma=1.2)] * B)
    fns["image-quality stage, every operation on (blur sigma 1.2)"] = ((lambda: ops.image_quality(img, q, 3, 0)), 9 * B * px)
    fns["device copy of the batch (`Tensor.copy_`)"] = ((lambda: out.copy_(img)), 6 * B * px)
    return fns, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "jpeg.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X (no fallback)")
    med = statistics.median
    L = ["# JPEG compression augmentation: numbers", "",
         "Stage: `csrc/jpeg.hip` behind `FundusBatches(..., jpeg=JpegCompression(...))`.  Tool: `tools/bench_jpeg.py` on one MI355X, one run.",
         "One batch of B = %d samples already in HBM.  A figure is the time between two device events around %d back-to-back calls" % (B, a.inner),
         "divided by %d; median (minimum .. maximum) of %d such windows after 5 warm-up calls, the variants alternating.  \"MB moved\" is what" % (a.inner, a.reps),
         "the variant moves through HBM by design (6 S^2 bytes per copied or 4:4:4 sample, 10 S^2 per 4:2:0 sample: it is read twice and",
         "its half-resolution chroma written and read; 9 S^2 for the image-quality stage: byte sums, then apply), \"rate\" is that over the",
         "median, as a fraction of the copy's.", ""]
    for S in (256, 512):
        fns, keep = variants(S)
        times = alternate({k: fn for k, (fn, _) in fns.items()}, a.reps, a.inner)
        copy_key = "device copy of the batch (`Tensor.copy_`)"
        copy_rate = fns[copy_key][1] / med(times[copy_key])
        L += ["## S = %d" % S, "", "| what | us per call | times the copy | MB moved | rate / copy's rate |", "| --- | --- | --- | --- | --- |"]
        for k, t in times.items():
            L.append("| %s | %.1f (%.1f .. %.1f) | %.2f | %.1f | %.2f |" % (k, 1e3 * med(t), 1e3 * min(t), 1e3 * max(t), med(t) / med(times[copy_key]),
                                                                           fns[k][1] / 1e6, fns[k][1] / med(t) / copy_rate))
        L.append("")
        del fns, keep
    L += ["\"stage\" is `ops.jpeg_roundtrip` as the input pipeline calls it: the parameter checks on the host, three small uploads, the",
          "allocations, one or two launches.  \"launches alone\" has the tables on the device already.", ""]
    write_profile(a.out, L)


if __name__ == "__main__":
    main()
