#!/usr/bin/env python3
"""What the random appearance networks (csrc/appearance.hip) cost -> profiles/appearance.md.

    python tools/bench_appearance.py [--out profiles/appearance.md] [--reps 30] [--inner 20]

One batch of B = 30 samples at S = 256 already in HBM, every sample selected, in the same run and alternating:
  * the stage (`ops.appearance_nets`: the range checks, two uploads, pass 1, pass 2) with two blended nets of 3x3 layers, of 1x1
    layers, of layers as `draw_appearance` draws them, and with a single net of 3x3 layers (blend off);
  * pass 1 alone with the tables already on the device (`wtpse_appearance_nets`: a memset, the byte sums, the nets launch) and pass 2
    alone (`wtpse_appearance_finish`) for the same tables;
  * the image-quality stage with every operation on (`ops.image_quality`);
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

B, S, SPACING = 30, 256, 32


def variants():
    from test_appearance_cpu import net_row, param_row, random_field, rows_of
    from test_quality_cpu import K_STD10, params_row, pictures
    from wtpse_hip import ops
    from wtpse_hip.input_pipeline import AppearanceNets, appearance_grid, draw_appearance
    from wtpse_hip.lib import lib
    img = torch.from_numpy(pictures(7, B, S)).cuda()
    out = torch.empty_like(img)
    field = random_field(1, B, S, SPACING)
    k3, k1 = (3, 3, 3, 3), (1, 1, 1, 1)
    tables = {"two nets blended, every layer 3x3": rows_of(*[param_row(net_row(i, k3), net_row(100 + i, k3)) for i in range(B)]),
              "two nets blended, every layer 1x1": rows_of(*[param_row(net_row(i, k1), net_row(100 + i, k1)) for i in range(B)]),
              "two nets blended, layers as drawn (p_k3 = 0.5)": draw_appearance(np.random.RandomState(3), B, S, AppearanceNets(p=1.0))[0],
              "one net (blend off), every layer 3x3": rows_of(*[param_row(net_row(i, k3)) for i in range(B)])}
    G = appearance_grid(S, SPACING)
    axis = ops.appearance_axis(S, SPACING, img.device)
    work = ops.workspace("appearance", lib().query("wtpse_appearance_workspace", B, S), img.device)
    dfield = torch.from_numpy(field).cuda()
    fns, keep = {}, [dfield]
    for name, p in tables.items():
        fns["stage: " + name] = (lambda p=p: ops.appearance_nets(img, p, field, SPACING))
        d = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).cuda()
        keep.append(d)
        fns["pass 1 alone: " + name] = (lambda d=d: lib().call("wtpse_appearance_nets", img.data_ptr(), d.data_ptr(), work.data_ptr(), B, S,
                                                                 ops.stream_ptr()))
        # pass 2 reads what the pass 1 of the warm-up and of the window before it left in the workspace: z of the same shape
        fns["pass 2 alone: " + name] = (lambda d=d: lib().call("wtpse_appearance_finish", img.data_ptr(), d.data_ptr(), dfield.data_ptr(),
                                                                 axis.data_ptr(), work.data_ptr(), out.data_ptr(), B, S, G, ops.stream_ptr()))
    q = np.stack([params_row(a=300, c=330, beta=2500, k=K_STD10, sigma=1.2)] * B)
    fns["image-quality stage, every operation on"] = lambda: ops.image_quality(img, q, 3, 0)
    fns["device copy of the same bytes (`Tensor.copy_`)"] = lambda: out.copy_(img)
    return fns, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "appearance.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X (no fallback)")
    fns, keep = variants()
    times = alternate(fns, a.reps, a.inner)
    med = statistics.median
    copy = med(times["device copy of the same bytes (`Tensor.copy_`)"])
    nbytes = B * S * S * 3
    L = ["# Random appearance networks: numbers", "",
         "Stage: `csrc/appearance.hip` behind `FundusBatches(..., appearance=AppearanceNets(...))`.  Tool: `tools/bench_appearance.py` on one MI355X.",
         "One batch of B = %d samples at S = %d already in HBM (%.1f MB read, as much written; the workspace holds %.1f MB of z), every" % (B, S, nbytes / 1e6, 8 * nbytes / 1e6),
         "sample selected.  A figure is the time between two device events around %d back-to-back calls divided by %d; median" % (a.inner, a.inner),
         "(minimum .. maximum) of %d such windows, the variants alternating." % a.reps, "",
         "| what | us per call | times the copy |", "| --- | --- | --- |"]
    for k, t in times.items():
        L.append("| %s | %.1f (%.1f .. %.1f) | %.1f |" % (k, 1e3 * med(t), 1e3 * min(t), 1e3 * max(t), med(t) / copy))
    L += ["", "\"stage\" is `ops.appearance_nets` as the input pipeline calls it: the range checks on the host, two uploads, pass 1 (a memset,",
          "the byte sums, the nets launch) and pass 2.  \"pass 1 alone\" and \"pass 2 alone\" have the tables on the device already.", ""]
    write_profile(a.out, L)


if __name__ == "__main__":
    main()
