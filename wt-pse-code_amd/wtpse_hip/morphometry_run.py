"""The test run with optic-disc morphometry: test_run.TestRun(..., morphometry=True) — per image the moment-based cup-to-disc ratios and
the rim minimum (morphometry.py) of the prediction and of the label, side by side: the place to see how good those numbers are against
ground truth.

    python -m wtpse_hip.morphometry_run --data-dir D --datasetTest 3 --checkpoint C --out O [--batch-size 9] [--sectors 24] [--eye right|left]

writes everything `python -m wtpse_hip.test_run` writes, byte for byte, and

    O/morphometry_errors.csv      index, name, {vcdr_ellipse,hcdr_ellipse,rim_min_rel}_{pred,label,abs_diff}, closed by a row of means

This module is the command line only; the switch, the pass and the table are TestRun's.
"""
import json

import torch

from . import morphometry as M
from .programs import open_test_split, test_run_parser
from .test_run import TestRun


def main(argv=None):
    ap = test_run_parser("morphometry_run", __doc__)
    ap.add_argument("--sectors", type=int, default=24, help="angular sectors of the rim profile: a multiple of 8 in 8..360")
    ap.add_argument("--eye", choices=("right", "left"), default=None)
    args = ap.parse_args(argv)
    M.check_sectors(args.sectors)
    nets, batches = open_test_split("morphometry_run", args)
    run = TestRun(*nets, out_dir=args.out, overlay=args.overlay, metrics=args.metrics, morphometry=True, sectors=args.sectors, eye=args.eye)
    means = run.run(batches)
    torch.cuda.synchronize()
    print(json.dumps(dict(means, **run.morph_means), sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
