"""Calibration against labels: are the probabilities calibrated, does a large spread mark wrong pixels, does the label's cup-to-disc
ratio fall inside the sampled interval as often as the interval claims — the labelled counterpart of uncertainty.py.

The device leaves, per image, one integer record (ops.calibration_hist, csrc/calibration.hip): hist_p[q][y], the pixels per quantised
probability q = rint(1024 clip(prob, 0, 1)) and label y; hist_s[u][e], the pixels per quantised spread u = rint(2048 clip(spread, 0,
0.5)) and error e = ((prob > threshold) != y); tail = (excluded background, excluded object, invalid, scored).  Records add: the
record of a test set is the sum of its images' records.  Every number below is a function of such a record, formed here in float64.

This module holds the host side: `hist_host`, the numpy specification of the launch, bit for bit (it sits beside the device path as
profile_host, mask_geometry_host and shape_samples_host do); the pixel scores (`reliability`, `scores`, `spread_scores`); the
image-level table (`interval_coverage`, `spearman`, `image_risk_coverage`); and the tables of calibration_run.py.

The quantisation: a probability is known to 1/1024 and a spread to 1/2048 (half a step: 2^-11 and 2^-12).  ECE / MCE bins are unions
of whole q values (bins divides 1024), so only the bin's mean confidence moves, by at most 2^-11; the Brier score and the NLL are
those of the quantised probability, the NLL with p clipped to [2^-11, 1 - 2^-11], half a step from the ends; the AUROCs count two pixels
that share a q (or a u) as a tie, worth 0.5.
"""
import os

import numpy as np

from . import tables as T

BINS = 1024
REC = 2 * (BINS + 1) * 2 + 4
NAN = float("nan")
COVERAGES = tuple(k / 20.0 for k in range(1, 21))            # 0.05, 0.10 .. 1.0 (level k of 20)
RATIOS = ("vcdr", "hcdr", "acdr")
RATIO_STATS = ("label", "pred", "mean", "std", "p05", "p95")
STRUCTURES = ("disc", "cup")

CALIBRATION_COLUMNS = ("scale", "structure", "n_scored", "n_excluded_neg", "n_excluded_pos", "n_invalid", "ece", "mce", "brier", "nll",
                       "auroc", "error_rate", "spread_wrong_mean", "spread_right_mean", "spread_auroc", "vcdr_coverage", "hcdr_coverage",
                       "acdr_coverage", "vcdr_spearman", "n_defined")
RELIABILITY_COLUMNS = ("scale", "structure", "bin", "lo", "hi", "n", "mean_conf", "frac_pos")
RISK_COLUMNS = ("scale", "structure", "level", "coverage", "risk")
PER_IMAGE_COLUMNS = ("scale", "index", "name", "disc_dice", "cup_dice") + tuple("%s_%s" % (r, s) for r in RATIOS for s in RATIO_STATS) + \
    ("vcdr_inside", "disc_ece", "cup_ece")


# ---- the specification of the device pass -----------------------------------------------------------------------------------------
def hist_host(prob, spread, label, region=None, threshold=0.75):
    """The specification of wtpse_calibration_hist, bit for bit.  prob, label [B, ...] (any trailing shape, one size), spread the
    same or None (every spread 0), region the same (nonzero = score the pixel) or None (every pixel) -> uint32 [B, REC].  Per pixel, in
    this order: region == 0 -> tail[y] += 1; prob or spread NaN -> tail[2] += 1; otherwise tail[3] += 1, hist_p[q][y] += 1 and
    hist_s[u][e] += 1 with q = rint(clip(prob, 0, 1) * 1024), u = rint(clip(spread, 0, 0.5) * 2048) in float32 (the products are
    exact; rint rounds half to even) and e = ((prob > threshold) != y), y = (label != 0)."""
    prob = np.asarray(prob, np.float32)
    B = prob.shape[0]
    prob = prob.reshape(B, -1)
    label = np.asarray(label, np.float32).reshape(B, -1)
    spread = np.zeros_like(prob) if spread is None else np.asarray(spread, np.float32).reshape(B, -1)
    keep = np.ones(prob.shape, bool) if region is None else np.asarray(region).reshape(B, -1) != 0
    if not (prob.shape == label.shape == spread.shape == keep.shape):
        raise ValueError("hist_host: prob %s, spread %s, label %s, region %s" % (prob.shape, spread.shape, label.shape, keep.shape))
    thr = np.float32(threshold)
    rec = np.zeros((B, REC), np.uint32)
    for b in range(B):
        y = label[b] != 0
        bad = keep[b] & (np.isnan(prob[b]) | np.isnan(spread[b]))
        ok = keep[b] & ~bad
        p, s, yo = prob[b][ok], spread[b][ok], y[ok].astype(np.int64)
        q = np.rint(np.minimum(np.maximum(p, np.float32(0)), np.float32(1)) * np.float32(1024))
        u = np.rint(np.minimum(np.maximum(s, np.float32(0)), np.float32(0.5)) * np.float32(2048))
        assert q.dtype == u.dtype == np.float32
        e = ((p > thr) != (yo != 0)).astype(np.int64)
        n = 2 * (BINS + 1)
        rec[b, :n] = np.bincount(2 * q.astype(np.int64) + yo, minlength=n)
        rec[b, n:2 * n] = np.bincount(2 * u.astype(np.int64) + e, minlength=n)
        rec[b, 2 * n:] = (int((~keep[b] & ~y).sum()), int((~keep[b] & y).sum()), int(bad.sum()), int(ok.sum()))
    return rec


def split_record(rec):
    """[..., REC] -> (hist_p [..., BINS + 1, 2], hist_s [..., BINS + 1, 2], tail [..., 4]) as int64."""
    rec = np.asarray(rec)
    if rec.shape[-1] != REC:
        raise ValueError("a calibration record has %d entries (got %s)" % (REC, rec.shape))
    rec = rec.astype(np.int64)
    n = 2 * (BINS + 1)
    lead = rec.shape[:-1]
    return rec[..., :n].reshape(lead + (BINS + 1, 2)), rec[..., n:2 * n].reshape(lead + (BINS + 1, 2)), rec[..., 2 * n:]


# ---- pixel scores -------------------------------------------------------------------------------------------------------------------
def check_bins(bins):
    if isinstance(bins, bool) or int(bins) != bins or int(bins) < 1 or BINS % int(bins):
        raise ValueError("bins must be a positive divisor of %d: a bin is a union of whole quantisation steps (got %r)" % (BINS, bins))
    return int(bins)


def _hist(h):
    h = np.asarray(h)
    if h.shape != (BINS + 1, 2):
        raise ValueError("a histogram is [%d, 2] (got %s)" % (BINS + 1, h.shape))
    return h.astype(np.int64)


def _div(a, b):
    return float(np.float64(a) / np.float64(b)) if b else NAN


def reliability(hist_p, bins=16):
    """hist_p [BINS + 1, 2] -> per equal-width bin k of `bins` over q / 1024 (q = 1024 goes into the last bin) the dict {bin, lo, hi, n,
    mean_conf, frac_pos}; mean_conf and frac_pos are nan for an empty bin.  Both are quotients of integer sums (sum n_q q / 1024 is
    exact), so a histogram with exactly n_q q / 1024 positives per q gives frac_pos == mean_conf to the bit."""
    h, bins = _hist(hist_p), check_bins(bins)
    q = np.arange(BINS + 1, dtype=np.int64)
    which = np.minimum(q * bins // BINS, bins - 1)
    n_q = h.sum(1)
    rows = []
    for k in range(bins):
        m = which == k
        n, pos, qn = int(n_q[m].sum()), int(h[m, 1].sum()), int((n_q[m] * q[m]).sum())
        rows.append({"bin": k, "lo": k / bins, "hi": (k + 1) / bins, "n": n, "mean_conf": _div(qn / 1024.0, n), "frac_pos": _div(pos, n)})
    return rows


def _auroc(h):
    """Mann-Whitney from a [., 2] histogram over an ordered key: column 1 the positives, column 0 the negatives; P(key of a positive >
    key of a negative) + 0.5 P(equal).  nan without a positive or without a negative."""
    neg, pos = h[:, 0].astype(np.float64), h[:, 1].astype(np.float64)
    P, N = pos.sum(), neg.sum()
    if P == 0 or N == 0:
        return NAN
    below = np.cumsum(neg) - neg
    return float((pos * (below + 0.5 * neg)).sum() / (P * N))


def scores(hist_p, bins=16):
    """hist_p [BINS + 1, 2] -> {n, ece, mce, brier, nll, auroc}: expected and maximum calibration error over `reliability`'s bins, the
    Brier score and the negative log-likelihood (natural log, p clipped to [2^-11, 1 - 2^-11]) of p = q / 1024, and the pixel AUROC
    (ties 0.5).  nan where undefined: no scored pixel; no positive or no negative for the AUROC."""
    h = _hist(hist_p)
    n = int(h.sum())
    out = {"n": n, "ece": NAN, "mce": NAN, "brier": NAN, "nll": NAN, "auroc": NAN}
    if n == 0:
        check_bins(bins)
        return out
    gaps = [(r["n"], abs(r["frac_pos"] - r["mean_conf"])) for r in reliability(h, bins) if r["n"]]
    out["ece"] = float(sum(np.float64(k) / n * g for k, g in gaps))
    out["mce"] = float(max(g for _, g in gaps))
    p = np.arange(BINS + 1, dtype=np.float64) / BINS
    neg, pos = h[:, 0].astype(np.float64), h[:, 1].astype(np.float64)
    out["brier"] = float((pos * (1.0 - p) ** 2 + neg * p ** 2).sum() / n)
    pc = np.clip(p, 2.0 ** -11, 1.0 - 2.0 ** -11)
    out["nll"] = float(-(pos * np.log(pc) + neg * np.log1p(-pc)).sum() / n)
    out["auroc"] = _auroc(h)
    return out


def spread_scores(hist_s):
    """hist_s [BINS + 1, 2] (column 1: wrong pixels) -> {n, error_rate, spread_wrong_mean, spread_right_mean, spread_auroc,
    risk_coverage}.  The means are of u / 2048; spread_auroc is the AUROC of "a larger spread marks a wrong pixel" (nan without a wrong
    or without a right pixel); risk_coverage = [(c, risk)] for c in COVERAGES: the error rate among the c n least uncertain pixels, a
    u bin that straddles c n contributing its errors in proportion to the part of it that is kept."""
    h = _hist(hist_s)
    right, wrong = h[:, 0].astype(np.float64), h[:, 1].astype(np.float64)
    n_u = right + wrong
    n = int(h.sum())
    s = np.arange(BINS + 1, dtype=np.float64) / (2 * BINS)
    out = {"n": n, "error_rate": _div(wrong.sum(), n), "spread_wrong_mean": _div((s * wrong).sum(), wrong.sum()),
           "spread_right_mean": _div((s * right).sum(), right.sum()), "spread_auroc": _auroc(h) if n else NAN}
    cum_n, cum_w = np.cumsum(n_u), np.cumsum(wrong)
    curve = []
    for k, c in enumerate(COVERAGES, 1):
        if n == 0:
            curve.append((c, NAN))
            continue
        t = k * n / 20.0                                         # pixels kept
        i = min(int(np.searchsorted(cum_n, t, side="left")), BINS)         # the first bin at which cum_n reaches t: n_u[i] > 0
        before_n, before_w = (cum_n[i - 1], cum_w[i - 1]) if i else (0.0, 0.0)
        curve.append((c, float((before_w + (t - before_n) / n_u[i] * wrong[i]) / t)))
    out["risk_coverage"] = curve
    return out


# ---- the image-level table ----------------------------------------------------------------------------------------------------------
def interval_coverage(label_value, p05, p95):
    """-> (the fraction of images whose label value lies in [p05, p95], the number of images where all three are defined); the fraction
    is nan when there is none.  A 5-to-95 interval claims 0.9."""
    v, lo, hi = (np.asarray(a, np.float64).reshape(-1) for a in (label_value, p05, p95))
    ok = ~(np.isnan(v) | np.isnan(lo) | np.isnan(hi))
    n = int(ok.sum())
    return _div(int(((v >= lo) & (v <= hi) & ok).sum()), n), n


def average_ranks(v):
    """1-based ranks of a 1-D array, ties sharing the average of their positions."""
    v = np.asarray(v, np.float64)
    order = np.argsort(v, kind="stable")
    ranks = np.empty(len(v), np.float64)
    sv = v[order]
    i = 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and sv[j + 1] == sv[i]:
            j += 1
        ranks[order[i:j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return ranks


def spearman(a, b):
    """Spearman's rank correlation over the pairs where both values are defined: Pearson's correlation of the average ranks.  nan
    below 3 defined pairs or when one side is constant."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError("spearman: %d and %d values" % (len(a), len(b)))
    ok = ~(np.isnan(a) | np.isnan(b))
    if int(ok.sum()) < 3:
        return NAN
    ra, rb = average_ranks(a[ok]), average_ranks(b[ok])
    da, db = ra - ra.mean(), rb - rb.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return float((da * db).sum() / den) if den > 0 else NAN


def image_risk_coverage(uncertainty, dice):
    """The image-level curve: the images sorted by `uncertainty` (vcdr_std; ascending, ties and undefined values in index order, the
    undefined ones last), -> [(c, 1 - mean Dice of the ceil(c n) images kept)] for c in COVERAGES; risk nan without an image."""
    u, d = np.asarray(uncertainty, np.float64).reshape(-1), np.asarray(dice, np.float64).reshape(-1)
    if u.shape != d.shape:
        raise ValueError("image_risk_coverage: %d uncertainties, %d Dice values" % (len(u), len(d)))
    n = len(u)
    order = np.argsort(np.where(np.isnan(u), np.inf, u), kind="stable")
    return [(c, float(1.0 - d[order[:(k * n + 19) // 20]].mean()) if n else NAN) for k, c in enumerate(COVERAGES, 1)]


# ---- the run's arguments ------------------------------------------------------------------------------------------------------------
def parse_scales(text):
    """"0,0.5,1,2" -> [0.0, 0.5, 1.0, 2.0]; a list of numbers passes through.  At least one; finite, not negative, no duplicates."""
    parts = [p.strip() for p in text.split(",")] if isinstance(text, str) else list(text)
    try:
        vals = [float(p) for p in parts]
    except (TypeError, ValueError):
        raise ValueError("scales must be numbers separated by commas (got %r)" % (text,))
    if not vals or any(not (0.0 <= v < float("inf")) for v in vals):
        raise ValueError("scales must be finite and not negative, at least one (got %r)" % (text,))
    if len(set(vals)) != len(vals):
        raise ValueError("scales holds a duplicate (got %r)" % (text,))
    return vals


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
TABLES = {"calibration": (CALIBRATION_COLUMNS, ("n_scored", "n_excluded_neg", "n_excluded_pos", "n_invalid", "n_defined"), ("structure",)),
          "reliability": (RELIABILITY_COLUMNS, ("bin", "n"), ("structure",)),
          "risk_coverage": (RISK_COLUMNS, (), ("structure", "level")),
          "per_image": (PER_IMAGE_COLUMNS, ("index",), ("name",))}


def write_csv(out_dir, table, rows):
    """table: a key of TABLES -> out_dir/<table>.csv with that table's columns."""
    columns, ints, texts = TABLES[table]
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, table + ".csv"), columns, rows, ints, texts)


def read_csv(out_dir, table):
    _, ints, texts = TABLES[table]
    return T.read_csv(os.path.join(out_dir, table + ".csv"), ints, texts)


def write_summary(out_dir, summary):
    T.write_json(os.path.join(out_dir, "summary.json"), summary, allow_nan=False)


def best_scales(rows):
    """calibration.csv rows -> {structure: {"lowest_nll": scale, "lowest_ece": scale}}: the first scale that attains the minimum, None
    when the score is defined at no scale."""
    out = {}
    for s in STRUCTURES:
        out[s] = {}
        for key in ("nll", "ece"):
            cand = [(r[key], r["scale"]) for r in rows if r["structure"] == s and r[key] == r[key]]
            out[s]["lowest_" + key] = min(cand, key=lambda t: t[0])[1] if cand else None
    return out
