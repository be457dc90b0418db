"""Calibration run: a trained checkpoint and a labelled test split -> how far the probabilities and the sampled spread of
`segment --samples K` can be trusted, per `--sample-scale` (calibration.py holds the arithmetic; this is the driver).

    python -m wtpse_hip.calibration_run --data-dir D --datasetTest 3 --checkpoint C --out O
           [--samples 16] [--scales 0,0.5,1,2] [--bins 16] [--seed 0] [--batch-size 9] [--views none|id|hflip|flips|d4|<codes>]

    O/calibration.csv     calibration.CALIBRATION_COLUMNS: one row per scale and structure (disc, cup); the ratio columns
                          (<ratio>_coverage, vcdr_spearman, n_defined) on the cup row, nan (n_defined 0) on the disc row and at scale 0
    O/reliability.csv     scale, structure, bin, lo, hi, n, mean_conf, frac_pos
    O/risk_coverage.csv   scale, structure, level (pixel|image), coverage, risk; no rows at scale 0 (nothing to sort by)
    O/per_image.csv       calibration.PER_IMAGE_COLUMNS: one row per scale and image
    O/summary.json        n, scales, samples, bins, and per structure the scale with the lowest NLL and the one with the lowest ECE;
                          with --views also views, the code list

Scale 0 is the deterministic row: prob = sigmoid of validate.predict_pair's logits at the label size, no spread (every scored pixel sits
in spread bin 0; the spread columns are nan), the U-Nets are not sampled.  A scale s > 0 runs validate.predict_pair_samples with
Segmenter's offset rule — the image at index i of the run draws from position 2 K S^2 i of the stream `seed` — so an image's draws
depend on (seed, i) alone; prob is the mean and spread the standard deviation of the K sampled probabilities, both resized bilinearly
to the label size.  The U-Nets run once per sampled scale and batch, and once for the deterministic prediction every scale shares
(Dice, the cup's region, the ratios of the post-processed masks, and scale 0's probabilities).

The cup is scored only where the bilinearly resized od_pred equals exactly 1.0: outside the predicted disc the cup reads probability
0.5 by construction (the ROI is deterministic), and scoring it there would measure the ROI, not the head.  The pixels left out are
counted by label: n_excluded_neg, and n_excluded_pos — cup label pixels outside the predicted disc, guaranteed misses.

Per batch and scale both structures go through ONE ops.calibration_hist launch (disc images first, then cup, as
validate._device_records stacks them) and the records come back in one device -> host copy (the first scale's also carries the
ops.mask_geometry records of the label masks and of the deterministic post-processed masks, from which `segment.measure` takes the
label's and the prediction's ratios).  The Dice columns are validate.batch_metrics(..., "device") — what test_run writes; the
per-sample ratios are Segmenter.back_samples', which keeps its own copy.

With --views (CalibrationRun(views=...); views.parse names the sets; none, the default, changes nothing) both predictions go through
validate.predict_pair_views: the Dice columns, the cup's region and the ratios come from the merged logits, and EVERY scale is a
sampled row — at scale 0 each of the V views contributes its deterministic prediction (V samples), at a scale s > 0 its K samples
(V K samples; the image at index i draws from position 2 V K S^2 i); prob is the mean and spread the standard deviation over the
merged samples, so scale 0 has spread columns and risk-coverage rows as well.

Image-level numbers on the cup row: <ratio>_coverage = the fraction of images whose label ratio lies inside [p05, p95] of the samples
(a 5-to-95 interval claims 0.9), n_defined the images where vcdr's three values exist, vcdr_spearman the rank correlation of vcdr_std
with |vcdr_pred - vcdr_label|.  The image risk-coverage curve keeps the images with the smallest vcdr_std; risk = 1 - mean Dice (of
the row's structure) of the images kept.
"""
import json
import os

import numpy as np
import torch

from . import calibration as C
from . import ops
from . import validate as V
from . import views as VW
from .segment import Segmenter, measure
from .packed import fetch
from .programs import add_split_arguments, open_test_split

THRESHOLD = 0.75                                # the threshold of od_pred, of the post-processing and of the samples' votes


class CalibrationRun:
    """run(batches) scores every batch of a FundusTestBatches (or any iterable of (image, original_od, original_oc[, names]) device
    tensors) at every scale and writes the files of the module docstring; -> the summary.  `self.records[scale]` keeps the per-image
    records (uint32 [n, 2, REC]: disc, cup), `self.rows` the per-image table, `self.table` calibration.csv's rows.  Eval mode for the
    duration, the previous modes restored."""

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, samples=16, scales=(0.0, 0.5, 1.0, 2.0), bins=16, seed=0,
                 views=None):
        self.nets = [model, model_shape, model_oc, model_shape_oc]
        self.out_dir, self.samples, self.seed = out_dir, int(samples), int(seed)
        self.scales, self.bins = C.parse_scales(scales), C.check_bins(bins)
        if not 1 <= self.samples <= 64:
            raise ValueError("samples must lie in 1..64 (got %r)" % (samples,))
        self.views = VW.parse(views)
        if self.views is not None and len(self.views) * self.samples > VW.MAX_MAPS:
            raise ValueError("views * samples must not exceed %d (got %d x %d)" % (VW.MAX_MAPS, len(self.views), self.samples))
        self.records, self.rows, self.table, self._seg, self._det = {}, [], [], None, None

    def _records(self, prob, spread, label, region, extra=()):
        """One launch for both structures, one copy -> (uint32 [2 B, REC], the extra int64 tensors' host copies)."""
        rec, *out = fetch([ops.calibration_hist(prob, spread, label, region, THRESHOLD), *extra])       # the one copy
        return rec.view(np.uint32), out

    def predict_pair(self, image):
        """The deterministic prediction at the network size -> (pred, pred_oc): validate.predict_pair, or with views the merged pair
        of validate.predict_pair_views (whose V per-view predictions are kept for scale 0)."""
        if self.views is None:
            return V.predict_pair(*self.nets, image)
        pred, pred_oc, disc, cup = V.predict_pair_views(*self.nets, image, self.views)
        self._det = (image, disc, cup)
        return pred, pred_oc

    def predict_samples(self, image, scale, first):
        """The sampled prediction of a batch whose first image has index `first` of the run -> (disc, cup), the two stages'
        uncertainty.ShapeSamples with their logits: validate.predict_pair_samples under the segmenter's offset rule.  With views:
        validate.predict_pair_views — the V views' deterministic predictions at scale 0, their V K samples otherwise."""
        S = image.shape[2]
        if self.views is not None:
            if scale == 0.0:
                if self._det is not None and self._det[0] is image:
                    return self._det[1:]
                return V.predict_pair_views(*self.nets, image, self.views)[2:]
            offset = first * V.noise_share(self.samples, S, len(self.views))
            return V.predict_pair_views(*self.nets, image, self.views, self.samples, self.seed, offset, scale)[2:]
        offset = first * V.noise_share(self.samples, S)
        return V.predict_pair_samples(*self.nets, image, self.samples, self.seed, offset, scale, want_logits=True)[2:]

    def _segmenter(self, B, S):
        if self._seg is None or self._seg.batch_size != B or self._seg.size != S:
            self._seg = Segmenter(*self.nets, out_dir=self.out_dir, batch_size=B, size=S, samples=self.samples, seed=self.seed,
                                  views=self.views)
        return self._seg

    def batch(self, image, label_od, label_oc, first):
        """One batch whose first image has index `first` of the run -> {scale: [per-image dict]} with the keys of per_image.csv (no
        scale, index, name) and "rec" (uint32 [2, REC])."""
        size, B, S = tuple(label_od.shape[2:]), image.shape[0], image.shape[2]
        resize = lambda t: ops.resize_bilinear(t.contiguous(), size) if size != tuple(t.shape[2:]) else t.contiguous()
        seg = self._segmenter(B, S)
        # the deterministic part, the same at every scale: the logits at the label size, Dice, the cup's region, the geometry records
        pred, pred_oc = self.predict_pair(image)
        pair = resize(torch.cat((pred, pred_oc), 0))
        dice = V.batch_metrics(pair[:B], pair[B:], label_od, label_oc, "device")
        od_pred = ops.roi(image.contiguous(), pred)[1]
        region = torch.cat((torch.ones_like(label_od, dtype=torch.uint8), (resize(od_pred) == 1.0).to(torch.uint8)), 0).contiguous()
        label = torch.cat((label_od, label_oc), 0).to(torch.float32).contiguous()
        extra = (ops.mask_geometry((label != 0).to(torch.uint8).contiguous()), ops.mask_geometry(ops.postprocess_masks(pair, THRESHOLD)))
        out, det = {}, None
        for scale in self.scales:
            if scale == 0.0 and self.views is None:
                prob, spread, stats = torch.sigmoid(pair), None, None
            else:
                disc, cup = self.predict_samples(image, scale, first)
                stats = seg.back_samples(disc, cup)
                maps = resize(torch.cat((disc.mean, cup.mean, disc.std, cup.std), 0))
                prob, spread = maps[:2 * B].contiguous(), maps[2 * B:].contiguous()
            rec, geom = self._records(prob, spread, label, region, extra if det is None else ())       # (the geometry rides in the first copy)
            if det is None:
                det = []
                for i in range(B):
                    ml, mp = measure(geom[0][i], geom[0][B + i], *size), measure(geom[1][i], geom[1][B + i], *size)
                    row = {"disc_dice": dice["disc_dice"][i], "cup_dice": dice["cup_dice"][i]}
                    for r in C.RATIOS:
                        row[r + "_label"], row[r + "_pred"] = ml[r], mp[r]
                    det.append(row)
            rows = []
            for i in range(B):
                row = dict(det[i], rec=np.stack((rec[i], rec[B + i])))
                for r in C.RATIOS:
                    for k in ("mean", "std", "p05", "p95"):
                        row["%s_%s" % (r, k)] = stats[i]["%s_%s" % (r, k)] if stats is not None else C.NAN
                v, lo, hi = row["vcdr_label"], row["vcdr_p05"], row["vcdr_p95"]
                row["vcdr_inside"] = C.NAN if (v != v or lo != lo or hi != hi) else float(lo <= v <= hi)
                for j, name in enumerate(C.STRUCTURES):
                    row[name + "_ece"] = C.scores(C.split_record(row["rec"][j])[0], self.bins)["ece"]
                rows.append(row)
            out[scale] = rows
        return out

    def finish(self):
        """The tables from `self.rows` / `self.records`, written; -> the summary."""
        table, rel, risk = [], [], []
        for scale in self.scales:
            rows = [r for r in self.rows if r["scale"] == scale]
            total = self.records[scale].astype(np.int64).sum(0) if len(rows) else np.zeros((2, C.REC), np.int64)
            for j, name in enumerate(C.STRUCTURES):
                hp, hs, tail = C.split_record(total[j])
                sc, sp = C.scores(hp, self.bins), C.spread_scores(hs)
                row = {"scale": scale, "structure": name, "n_scored": int(tail[3]), "n_excluded_neg": int(tail[0]),
                       "n_excluded_pos": int(tail[1]), "n_invalid": int(tail[2]), "error_rate": sp["error_rate"]}
                row.update({k: sc[k] for k in ("ece", "mce", "brier", "nll", "auroc")})
                sampled = scale != 0.0 or self.views is not None
                row.update({k: sp[k] if sampled else C.NAN for k in ("spread_wrong_mean", "spread_right_mean", "spread_auroc")})
                row.update({r + "_coverage": C.NAN for r in C.RATIOS}, vcdr_spearman=C.NAN, n_defined=0)
                if sampled and name == "cup":
                    col = lambda k: [r[k] for r in rows]
                    for r in C.RATIOS:
                        cov, n_def = C.interval_coverage(col(r + "_label"), col(r + "_p05"), col(r + "_p95"))
                        row[r + "_coverage"] = cov
                        if r == "vcdr":
                            row["n_defined"] = n_def
                    row["vcdr_spearman"] = C.spearman(col("vcdr_std"), np.abs(np.array(col("vcdr_pred"), np.float64) - np.array(col("vcdr_label"), np.float64)))
                table.append(row)
                rel.extend(dict(r, scale=scale, structure=name) for r in C.reliability(hp, self.bins))
                if sampled:
                    risk.extend({"scale": scale, "structure": name, "level": "pixel", "coverage": c, "risk": v} for c, v in sp["risk_coverage"])
                    risk.extend({"scale": scale, "structure": name, "level": "image", "coverage": c, "risk": v}
                                for c, v in C.image_risk_coverage([r["vcdr_std"] for r in rows], [r[name + "_dice"] for r in rows]))
        self.table = table
        summary = {"n": len(self.rows) // max(len(self.scales), 1), "scales": list(self.scales), "samples": self.samples, "bins": self.bins}
        if self.views is not None:
            summary["views"] = list(self.views)
        summary.update(C.best_scales(table))
        C.write_csv(self.out_dir, "calibration", table)
        C.write_csv(self.out_dir, "reliability", rel)
        C.write_csv(self.out_dir, "risk_coverage", risk)
        C.write_csv(self.out_dir, "per_image", self.rows)
        C.write_summary(self.out_dir, summary)
        return summary

    def run(self, batches):
        os.makedirs(self.out_dir, exist_ok=True)
        per_scale, recs, count = {s: [] for s in self.scales}, {s: [] for s in self.scales}, 0
        with V.eval_mode(self.nets):
            for item in batches:
                image, label_od, label_oc = item[:3]
                names = item[3] if len(item) > 3 else [""] * image.shape[0]
                res = self.batch(image, label_od, label_oc, count)
                for s in self.scales:
                    for i, row in enumerate(res[s]):
                        recs[s].append(row.pop("rec"))
                        per_scale[s].append(dict(row, scale=s, index=count + i + 1, name=names[i]))
                count += image.shape[0]
        self._det = None
        self.rows = [r for s in self.scales for r in per_scale[s]]
        self.records = {s: np.stack(recs[s]) if recs[s] else np.zeros((0, 2, C.REC), np.uint32) for s in self.scales}
        return self.finish()


# ---- command line -------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    """The command line -> its namespace, with --scales parsed (calibration.parse_scales) and --bins checked (calibration.check_bins):
    a bad value ends the program before anything runs."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip.calibration_run", description=__doc__.split("\n\n")[0])
    add_split_arguments(ap)
    ap.add_argument("--samples", type=int, default=16, help="K sampled shape latents per image and scale")
    ap.add_argument("--scales", default="0,0.5,1,2", help="the --sample-scale values to score, separated by commas; 0 = the deterministic prediction")
    ap.add_argument("--bins", type=int, default=16, help="reliability bins: a divisor of 1024")
    ap.add_argument("--seed", type=int, default=0, help="the noise stream of the samples")
    ap.add_argument("--batch-size", type=int, default=9)
    ap.add_argument("--views", default="none", help="test-time views to merge: none, id, hflip, flips, d4 or a comma list of codes 0..7 (0 first)")
    args = ap.parse_args(argv)
    try:
        args.scales, args.bins = C.parse_scales(args.scales), C.check_bins(args.bins)
        if not 1 <= args.samples <= 64:
            raise ValueError("--samples must lie in 1..64 (got %d)" % args.samples)
        args.views = VW.parse(args.views)
        if args.views is not None and len(args.views) * args.samples > VW.MAX_MAPS:
            raise ValueError("--views times --samples must not exceed %d (got %d x %d)" % (VW.MAX_MAPS, len(args.views), args.samples))
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    nets, batches = open_test_split("calibration_run", args)
    run = CalibrationRun(*nets, out_dir=args.out, samples=args.samples, scales=args.scales, bins=args.bins, seed=args.seed, views=args.views)
    summary = run.run(batches)
    torch.cuda.synchronize()
    print(json.dumps(summary, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
