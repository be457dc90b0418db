#!/usr/bin/env python3
"""Cost of the gradability pass (ops.gradability_record, csrc/gradability.hip) beside ops.locate_cells, which reads the same bytes, on
synthetic photographs (the generator of tests/test_locate_cpu.py) at 2144 x 1424 and 4288 x 2848, in one process:

  * both passes and a device-to-device copy of the picture (HIP events, medians after a warm-up, the three alternating so that they
    share whatever else the box is doing);
  * the record pass again with the field threshold at 255 — almost no pixel in the field, so no histogram atomic, no stencil and
    next to no global add: what is left is the loads and the LDS staging — on one flat colour (the stencil in full, one histogram
    bin, a dozen global adds a workgroup) and on uniform noise (every pixel its own LDS atomic, all 276 global adds), to say where
    the time goes;
  * the crop-level record (t = 0) and cell table at the run's crop side, and the host's `measures` per record.

    python tools/bench_gradability.py [--reps 200] [--sizes 1424x2144,2848x4288]

The device record is compared with gradability.record_host before anything is timed.  Nothing here is a pass mark:
profiles/gradability.md records a run.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tests")]
from test_locate_cpu import synth_photo  # noqa: E402
from wtpse_hip import gradability as GR  # noqa: E402
from wtpse_hip import locate as L  # noqa: E402
from wtpse_hip import ops  # noqa: E402


def alternating_ms(fns, reps):
    """Median HIP-event times in ms of every fn of `fns` over `reps` rounds in which they run one after the other, after a warm-up
    round; -> ([median], [(min, max)])."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sizes", default="1424x2144,2848x4288")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gradability needs the GPU: a time taken anywhere else says nothing")
    for (H, W) in [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]:
        img, _ = synth_photo(H, W, 2, (0.45, 0.2))
        stack = torch.from_numpy(img[None]).cuda()
        area = int((img.max(-1) >= 24).sum())
        c = L.auto_cell(0.13 * L.fov_diameter(area))
        want = GR.record_host(img, 24, 250)
        assert np.array_equal(ops.gradability_record(stack, 24, 250).cpu().numpy(), want), "the device record differs from record_host"
        assert np.array_equal(ops.gradability_record(stack, 255, 250).cpu().numpy(), GR.record_host(img, 255, 250))
        dst = torch.empty_like(stack)
        (t_rec, t_cells, t_copy, t_bare), spread = alternating_ms(
            [lambda: ops.gradability_record(stack, 24, 250), lambda: ops.locate_cells(stack, c, 24), lambda: dst.copy_(stack),
             lambda: ops.gradability_record(stack, 255, 250)], a.reps)
        flat = torch.empty_like(stack)
        flat[...] = torch.tensor([120, 90, 60], dtype=torch.uint8, device="cuda")
        noise = torch.randint(0, 256, stack.shape, dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        (t_flat, t_noise), spread2 = alternating_ms([lambda: ops.gradability_record(flat, 24, 250), lambda: ops.gradability_record(noise, 24, 250)],
                                                    a.reps)
        nbytes = stack.numel()
        rate = 2 * nbytes / t_copy / 1e9
        side = L.roi_side(L.fov_diameter(area))
        crop = stack[:, :side, :side].contiguous()
        cc = GR.crop_cell(side, side)
        (t_crop, t_ccells), _ = alternating_ms([lambda: ops.gradability_record(crop, 0, 250), lambda: ops.locate_cells(crop, cc, 0)], a.reps)
        cells = L.cells_host(img, c, 24)
        t0 = time.perf_counter()
        for _ in range(20):
            m = GR.measures(want[0], cells, c)
        t_host = (time.perf_counter() - t0) / 20
        tiles = -(-W // 256) * -(-H // 32)
        print("%d x %d (%.1f MB), field %d px, cell %d, %d tiles = %d workgroups; medians of %d, (min .. max):"
              % (W, H, nbytes / 1e6, area, c, tiles, min(tiles, 2048), a.reps))
        print("  ops.gradability_record, t = 24                          : %8.3f ms  (%.3f .. %.3f)  %.2f TB/s of picture bytes, %.2f of the copy rate"
              % (t_rec, *spread[0], nbytes / t_rec / 1e9, nbytes / t_rec / 1e9 / rate))
        print("  ops.locate_cells at the auto cell                       : %8.3f ms  (%.3f .. %.3f)  %.2f TB/s, %.2f of the copy rate; record / cells = %.2f"
              % (t_cells, *spread[1], nbytes / t_cells / 1e9, nbytes / t_cells / 1e9 / rate, t_rec / t_cells))
        print("  device copy of the picture                              : %8.3f ms  (%.3f .. %.3f)  %.2f TB/s read + written"
              % (t_copy, *spread[2], rate))
        print("  ops.gradability_record, t = 255 (loads and staging only) : %8.3f ms  (%.3f .. %.3f)" % (t_bare, *spread[3]))
        print("  the same on one flat colour (one luma bin, a dozen global adds) : %8.3f ms  (%.3f .. %.3f)" % (t_flat, *spread2[0]))
        print("  the same on uniform noise (256 bins, no runs, all 276 adds)      : %8.3f ms  (%.3f .. %.3f)" % (t_noise, *spread2[1]))
        print("  crop %d x %d: record at t = 0 %.3f ms, cell table at c = %d %.3f ms" % (side, side, t_crop, cc, t_ccells))
        print("  measures() on the host, per record with its cell table  : %8.3f ms; focus_1 %.1f, focus_ratio %.4f, focus_scale %d, evenness_cv %.3f"
              % (1e3 * t_host, m["focus_1"], m["focus_ratio"], m["focus_scale"], m["evenness_cv"]))


if __name__ == "__main__":
    main()
