#!/usr/bin/env python3
"""Cost of locating the optic disc on whole fundus photographs (wtpse_hip/locate.py) on synthetic photographs (the generator of
tests/test_locate_cpu.py) at 2144 x 1424 and 4288 x 2848:

  * the cell pass ops.locate_cells (HIP events) against two references taken in the same run: the same sums composed from torch ops, and
    the copy-rate floor — the bytes the pass reads over the rate of a device-to-device copy of the same tensor (bytes read + written over
    its time), i.e. half that copy's time;
  * ops.crop_u8 and ops.paste_u8 at the run's crop side;
  * the whole run per image, split into decode, locate (cell passes + candidates), verify, refine, segment and the full-size products
    (host clock around synchronised phases).  The networks are default-initialised, so a disc blob is written into the stage-1 logits
    AFTER the network has run: verification passes and the recentring round runs, at the true cost of every launch.

    python tools/bench_locate.py [--reps 20] [--images 4] [--sizes 1424x2144,2848x4288]

The device results are compared with the host specification before anything is timed.  Nothing here is a pass mark:
profiles/locate.md records a run.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tests")]
from test_locate_cpu import synth_photo  # noqa: E402
from wtpse_hip import locate as L  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip import test_run as T  # noqa: E402


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


def torch_cells(stack, c, t):
    """ops.locate_cells composed from torch ops (int64 throughout)."""
    N, H, W, _ = stack.shape
    f = stack.amax(3) >= t
    y = (stack.to(torch.int64) * torch.tensor([77, 150, 29], device=stack.device)).sum(3) * f
    CH, CW = -(-H // c), -(-W // c)
    pool = lambda v: torch.nn.functional.pad(v, (0, CW * c - W, 0, CH * c - H)).reshape(N, CH, c, CW, c).sum((2, 4))
    return torch.stack((pool(f.to(torch.int64)), pool(y)), -1)


class BlobLocator(L.Locator):
    """Stage 1 at its true cost, then a centred disc in every map: verification passes whatever the weights."""

    def stage1(self, image):
        out = L.Locator.stage1(self, image)
        yy, xx = torch.meshgrid(torch.arange(256, device=out.device), torch.arange(256, device=out.device), indexing="ij")
        blob = ((yy - 118) ** 2 + (xx - 139) ** 2 <= 40 ** 2)
        return torch.where(blob[None, None], torch.full_like(out, 30.0), torch.full_like(out, -30.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--sizes", default="1424x2144,2848x4288")
    a = ap.parse_args()
    nets = T.build_networks("cuda")
    for (H, W) in [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]:
        img, truth = synth_photo(H, W, 2, (0.45, 0.2))
        stack = torch.from_numpy(img[None]).cuda()
        area = int((img.max(-1) >= 24).sum())
        c = L.auto_cell(0.13 * L.fov_diameter(area))
        want = L.cells_host(img, c, 24)
        assert np.array_equal(ops.locate_cells(stack, c, 24).cpu().numpy()[0], want) and np.array_equal(torch_cells(stack, c, 24).cpu().numpy()[0], want)
        p = L.plan(want, c)
        side, box = p["side"], p["boxes"][0]
        t_cells = event_ms(lambda: ops.locate_cells(stack, c, 24), a.reps)
        t_coarse = event_ms(lambda: ops.locate_cells(stack, 256, 24), a.reps)
        t_torch = event_ms(lambda: torch_cells(stack, c, 24), max(3, a.reps // 4))
        dst = torch.empty_like(stack)
        t_copy = event_ms(lambda: dst.copy_(stack), a.reps)
        boxes = torch.tensor([box], dtype=torch.int32, device="cuda")
        crop = ops.crop_u8(stack[0], boxes, side)
        assert np.array_equal(crop.cpu().numpy(), L.crop_host(img, [box], side))
        t_crop = event_ms(lambda: ops.crop_u8(stack[0], boxes, side), a.reps)
        t_paste = event_ms(lambda: ops.paste_u8(dst[0], crop[0], box[0], box[1]), a.reps)
        nbytes = stack.numel()
        print("%d x %d (%.1f MB), field diameter %.0f, cell %d, window %d, crop side %d; candidate 1 %.0f px from the disc centre (radius %.0f):"
              % (W, H, nbytes / 1e6, p["fov_diameter"], c, p["window"], side,
                 np.hypot(*(np.array(L.centre(*p["candidates"][0][:2], p["window"], c)) - truth[:2])), truth[2]))
        print("  ops.locate_cells at the auto cell                       : %8.3f ms  (%.2f TB/s of picture bytes)" % (t_cells, nbytes / t_cells / 1e9))
        print("  ops.locate_cells at c = 256 (the area pass)             : %8.3f ms" % t_coarse)
        print("  the same sums from torch ops                            : %8.3f ms  (x %.1f)" % (t_torch, t_torch / t_cells))
        print("  copy-rate floor (half a device copy of the picture)     : %8.3f ms  (copy %.3f ms = %.2f TB/s read + written)"
              % (t_copy / 2, t_copy, 2 * nbytes / t_copy / 1e9))
        print("  ops.crop_u8, one %d x %d box                          : %8.3f ms" % (side, side, t_crop))
        print("  ops.paste_u8 of that crop                               : %8.3f ms" % t_paste)
        with tempfile.TemporaryDirectory() as tmp:
            src, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
            os.makedirs(src)
            for i in range(a.images):
                Image.fromarray(np.roll(img, 16 * i, 1)).save(os.path.join(src, "p%02d.png" % i), compress_level=1)
            run = L.WholeImageSegmenter(*nets, out_dir=out, batch_size=9)
            run.locator = BlobLocator(nets[0], nets[1], batch_size=9)
            run.locator.seconds = {}
            clock = {}

            def timed(key, fn):
                def wrapped(*args, **kw):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = fn(*args, **kw)
                    torch.cuda.synchronize()
                    clock[key] = clock.get(key, 0.0) + time.perf_counter() - t0
                    return r
                return wrapped
            run._locate_all = timed("locate_all", run._locate_all)
            run.segmenter.run = timed("segment", run.segmenter.run)
            run._write_full = timed("full", run._write_full)
            t0 = time.perf_counter()
            summary = run.run(src)
            total = time.perf_counter() - t0
            sec, n = run.locator.seconds, a.images
            per = lambda s: 1e3 * s / n
            print("  the whole run, %d pictures, per picture (host clock): total %.1f ms; n_verified %d, refine rounds %s"
                  % (n, per(total), summary["n_verified"], [r["refine_rounds"] for r in run.roi_rows]))
            print("    decode + upload + crop PNGs (locate phase minus the three below) : %8.1f ms"
                  % per(clock["locate_all"] - sec["cells"] - sec["verify"] - sec["refine"]))
            print("    locate  : cell passes, table copies, candidates                  : %8.2f ms" % per(sec["cells"]))
            print("    verify  : crops, front, stage 1, post-processing, geometry       : %8.2f ms" % per(sec["verify"]))
            print("    refine  : one recentring round                                   : %8.2f ms" % per(sec["refine"]))
            print("    segment : Segmenter.run on the crops (with its PNGs)             : %8.1f ms" % per(clock["segment"]))
            print("    full    : second decode, pastes, one copy, two full-size PNGs    : %8.1f ms" % per(clock.get("full", 0.0)))


if __name__ == "__main__":
    main()
