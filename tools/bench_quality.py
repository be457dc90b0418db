#!/usr/bin/env python3
"""What the image-quality stage (csrc/quality.hip) costs -> profiles/quality.md.

    python tools/bench_quality.py [--out profiles/quality.md] [--reps 30] [--inner 20]

One batch of B = 30 samples at S = 256 already in HBM, in the same run and alternating:
  * the stage (`ops.image_quality`: uploads of the two tables, the byte sums, the apply launch) with every operation on in every
    sample, with the blur alone, and with the pointwise operations alone (contrast, brightness, noise; no focus);
  * the two launches alone with the tables already on the device (`wtpse_quality_sums`, `wtpse_quality_apply`);
  * the amplitude-mixing stage (`ops.amplitude_mix`, every sample mixed, b = 25);
  * a plain device copy of the same bytes (`Tensor.copy_`).
A figure is the time between two device events around --inner back-to-back calls, divided by --inner; median (minimum .. maximum) of
--reps such windows.  There is no bar: the stage is new.  The file says how far each variant lies from the copy and why.
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

B, S = 30, 256


def variants():
    from test_quality_cpu import K_STD10, params_row, pictures
    from wtpse_hip import ops
    from wtpse_hip.input_pipeline import AmplitudeMix, draw_mix, quality_positions
    from wtpse_hip.lib import lib
    img = torch.from_numpy(pictures(7, B, S)).cuda()
    out = torch.empty_like(img)
    tables = {"every operation on (blur sigma 1.2, sharpen 1.2, contrast, brightness, noise)": [params_row(a=300, c=330, beta=2500, k=K_STD10, sigma=1.2)] * B,
              "blur alone (sigma 1.5)": [params_row(a=-256, sigma=1.5)] * B,
              "pointwise alone (contrast, brightness, noise)": [params_row(c=330, beta=2500, k=K_STD10)] * B,
              "contrast and brightness alone (no noise)": [params_row(c=330, beta=2500)] * B}
    fns, keep = {}, []
    for name, rows in tables.items():
        p = np.stack(rows)
        fns["stage: " + name] = (lambda p=p: ops.image_quality(img, p, 3, 0))
        dparams = torch.from_numpy(p.astype(np.int32)).cuda()
        dpos = torch.from_numpy(quality_positions(p, S, 0)[0].view(np.int64)).cuda()
        sums = torch.empty(B, dtype=torch.int32, device="cuda")
        keep.append((dparams, dpos, sums))
        fns["apply launch alone: " + name] = (lambda d=dparams, q=dpos, s=sums: lib().call(
            "wtpse_quality_apply", img.data_ptr(), d.data_ptr(), s.data_ptr(), q.data_ptr(), 3, out.data_ptr(), B, S, ops.stream_ptr()))
    sums = keep[0][2]
    fns["sums launch alone (memset + kernel)"] = lambda: lib().call("wtpse_quality_sums", img.data_ptr(), sums.data_ptr(), B, S, ops.stream_ptr())
    partner, lam = draw_mix(np.random.RandomState(1), 3, B // 3, AmplitudeMix(p=1.0))
    fns["amplitude mixing stage, every sample mixed, b = 25"] = lambda: ops.amplitude_mix(img, partner, lam, 25)
    fns["device copy of the same bytes (`Tensor.copy_`)"] = lambda: out.copy_(img)
    return fns, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "quality.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X (no fallback)")
    fns, keep = variants()
    times = alternate(fns, a.reps, a.inner)
    med = statistics.median
    copy = med(times["device copy of the same bytes (`Tensor.copy_`)"])
    nbytes = B * S * S * 3
    L = ["# Image-quality augmentation: numbers", "",
         "Stage: `csrc/quality.hip` behind `FundusBatches(..., quality=ImageQuality(...))`.  Tool: `tools/bench_quality.py` on one MI355X.",
         "One batch of B = %d samples at S = %d already in HBM (%.1f MB read, as much written).  A figure is the time between two device" % (B, S, nbytes / 1e6),
         "events around %d back-to-back calls divided by %d; median (minimum .. maximum) of %d such windows, the variants alternating." % (a.inner, a.inner, a.reps), "",
         "| what | us per call | times the copy |", "| --- | --- | --- |"]
    for k, t in times.items():
        L.append("| %s | %.1f (%.1f .. %.1f) | %.1f |" % (k, 1e3 * med(t), 1e3 * min(t), 1e3 * max(t), med(t) / copy))
    L += ["", "\"stage\" is `ops.image_quality` as the input pipeline calls it: the parameter checks on the host, two small uploads, the",
          "memset and the sums launch, the apply launch.  \"launch alone\" has the tables on the device already.", ""]
    write_profile(a.out, L)


if __name__ == "__main__":
    main()
