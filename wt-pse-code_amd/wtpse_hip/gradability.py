"""Gradability check: was the photograph fit to be read?  Focus, exposure and field measures of a fundus picture, in front of the
measurements `locate` and `segment` take from it.

The device leaves, per picture, one integer record (ops.gradability_record, csrc/gradability.hip; `record_host` is its specification,
bit for bit): the luma histogram, channel sums, saturation counts, area and bounding box of the field of view, and the Laplacian and
gradient energies of the green channel at the dilations 1, 2 and 4.  `measures` finishes the record in float64, `Gradability` holds
the optional thresholds and judges, `ranks` orders the pictures of a run without any threshold, and `write_csv` / `read_csv` keep
gradability.csv (tables.py's form).

    field    f(p) = max(R, G, B) >= t; a position outside the picture is not in the field (locate's definition; t = 0: every pixel,
             which is how crops are scored)
    luma     Y = (77 R + 150 G + 29 B + 128) >> 8

    rec[0:256]            the histogram of Y over the field
    rec[256:259]          the sums of R, G, B over the field
    rec[259:262]          the field pixels with R, G, B >= sat, per channel
    rec[262]              the field's area n
    rec[263:267]          top, bottom, left, right of the field's bounding box; (H, -1, W, -1) for an empty field
    rec[267 + 3k : 270 + 3k]   (n_d, E_d, Q_d) for the k-th dilation d of DILATIONS = (1, 2, 4)

For a dilation d a pixel p is interior when p and its four neighbours at distance d along the rows and the columns all lie in the
picture and in the field.  Over the interior pixels, on the green channel: L = 4 G(p) - G(up) - G(down) - G(left) - G(right),
E_d = sum L^2, Q_d = sum (G(right) - G(left))^2 + (G(down) - G(up))^2, n_d their number.

The measures are this project's own integer definitions in the lineage of the Laplacian-energy focus measure and of the field /
clarity / illumination criteria of retinal image-quality work; their agreement with a human grader is not measured
here, and no threshold is recommended: `Gradability` has none by default."""
import math
import os

import numpy as np

from . import tables as T

GRAD_REC = 276
DILATIONS = (1, 2, 4)
_SUMS, _SAT, _AREA, _BOX, _FOCUS = 256, 259, 262, 263, 267

PERCENTILES = (1, 5, 50, 95, 99)
INT_MEASURES = ("fov_area", "focus_scale")
FLOAT_MEASURES = (("fov_fill", "luma_mean", "luma_std") + tuple("luma_p%02d" % q for q in PERCENTILES)
                  + ("contrast", "entropy", "mean_r", "mean_g", "mean_b", "sat_r", "sat_g", "sat_b", "dark_frac", "bright_frac")
                  + tuple("focus_%d" % d for d in DILATIONS) + tuple("edge_%d" % d for d in DILATIONS)
                  + ("focus_ratio", "focus", "evenness_cv", "centre_edge"))
MEASURES = INT_MEASURES + FLOAT_MEASURES
FLAGS = ("ok_focus", "ok_focus_ratio", "ok_dark", "ok_bright", "ok_cv", "ok_fov_fill", "gradable")
MIN_CELLS = 4                          # an illumination figure over fewer cells than this is nan


# ---- the host specification ---------------------------------------------------------------------------------------------------
def record_host(img, t=24, sat=250):
    """[H,W,3] (or [N,H,W,3]) uint8 -> int64 [N, GRAD_REC] (N = 1 for one picture): the module docstring's record, integers only.
    ops.gradability_record's specification."""
    img = np.asarray(img)
    if img.ndim == 3:
        img = img[None]
    if img.dtype != np.uint8 or img.ndim != 4 or img.shape[3] != 3:
        raise ValueError("img must be [H,W,3] or [N,H,W,3] uint8 (got %s %s)" % (img.shape, img.dtype))
    t, sat = int(t), int(sat)
    if not 0 <= t <= 255 or not 1 <= sat <= 255:
        raise ValueError("the threshold must lie in 0..255 and sat in 1..255 (got %r, %r)" % (t, sat))
    N, H, W = img.shape[:3]
    out = np.zeros((N, GRAD_REC), np.int64)
    for i in range(N):
        a = img[i].astype(np.int64)
        f = img[i].max(-1) >= t
        y = (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8
        rec = out[i]
        rec[:256] = np.bincount(y[f], minlength=256)
        rec[_SUMS:_SUMS + 3] = a[f].sum(0)
        rec[_SAT:_SAT + 3] = (a[f] >= sat).sum(0)
        rec[_AREA] = int(f.sum())
        rows, cols = np.nonzero(f.any(1))[0], np.nonzero(f.any(0))[0]
        rec[_BOX:_BOX + 4] = (rows[0], rows[-1], cols[0], cols[-1]) if len(rows) else (H, -1, W, -1)
        g = a[..., 1]
        for k, d in enumerate(DILATIONS):
            if H <= 2 * d or W <= 2 * d:
                continue                                       # no pixel has all four neighbours inside the picture
            part = lambda v: (v[d:H - d, d:W - d], v[:H - 2 * d, d:W - d], v[2 * d:, d:W - d], v[d:H - d, :W - 2 * d], v[d:H - d, 2 * d:])
            fc, fu, fd, fl, fr = part(f)
            gc, gu, gd, gl, gr = part(g)
            inside = fc & fu & fd & fl & fr
            lap = (4 * gc - gu - gd - gl - gr)[inside]
            rec[_FOCUS + 3 * k:_FOCUS + 3 * k + 3] = (int(inside.sum()), int((lap * lap).sum()),
                                                      int((((gr - gl) ** 2 + (gd - gu) ** 2)[inside]).sum()))
    return out


def split_record(rec):
    """[..., GRAD_REC] -> {hist [..., 256], sums [..., 3], sat [..., 3], area [...], box [..., 4], focus [..., 3, 3] = (n_d, E_d, Q_d)
    per dilation} as int64."""
    rec = np.asarray(rec)
    if rec.shape[-1] != GRAD_REC:
        raise ValueError("a gradability record has %d entries (got %s)" % (GRAD_REC, rec.shape))
    rec = rec.astype(np.int64)
    return {"hist": rec[..., :256], "sums": rec[..., _SUMS:_SUMS + 3], "sat": rec[..., _SAT:_SAT + 3], "area": rec[..., _AREA],
            "box": rec[..., _BOX:_BOX + 4], "focus": rec[..., _FOCUS:].reshape(rec.shape[:-1] + (3, 3))}


# ---- the measures -------------------------------------------------------------------------------------------------------------
def _ratio(num, den):
    return float("nan") if den == 0 else float(np.float64(num) / np.float64(den))


def percentile(hist, q):
    """The smallest luma whose cumulative count reaches the rank max(1, ceil(q n / 100)) of the n counted pixels (integers; nan
    for an empty histogram)."""
    hist = np.asarray(hist, np.int64)
    n = int(hist.sum())
    if n == 0:
        return float("nan")
    rank = max(1, -(-int(q) * n // 100))
    return float(int(np.searchsorted(np.cumsum(hist), rank, side="left")))


def focus_scale(area, ref_diameter=1024.0):
    """The dilation the focus is read at: 1 when the field's diameter 2 sqrt(area / pi) is below ref_diameter sqrt(2), 2 below twice
    that, else 4 (a picture of twice the resolution spreads the same optical blur over twice the pixels)."""
    D = 2.0 * math.sqrt(float(area) / math.pi)
    edge = float(ref_diameter) * math.sqrt(2.0)
    return 1 if D < edge else 2 if D < 2.0 * edge else 4


def illumination(cells, c, area, box):
    """locate's cell table [CH,CW,2] = (n, s) at side c, the field's area and bounding box -> (evenness_cv, centre_edge) over the
    cells that lie wholly in the field (n == c c), m = s / n / 256 their mean luma: the (population) standard deviation of m over
    its mean, nan with fewer than MIN_CELLS such cells; and the mean of m over the cells whose centre lies within D / 4 of the
    bounding box's centre over the mean beyond 3 D / 8, D = 2 sqrt(area / pi), nan with fewer than MIN_CELLS cells in either group."""
    nan = float("nan")
    cells = np.asarray(cells, np.int64)
    c = int(c)
    n, s = cells[..., 0], cells[..., 1]
    full = n == c * c
    if int(full.sum()) < MIN_CELLS:
        return nan, nan
    m = s[full].astype(np.float64) / np.float64(c * c) / 256.0
    mean = float(m.mean())
    cv = _ratio(float(m.std()), mean)
    top, bottom, left, right = (int(v) for v in box)
    cy, cx = (top + bottom + 1) / 2.0, (left + right + 1) / 2.0
    D = 2.0 * math.sqrt(float(area) / math.pi)
    ii, jj = np.nonzero(full)
    r = np.hypot((ii + 0.5) * c - cy, (jj + 0.5) * c - cx)
    inner, outer = m[r <= D / 4.0], m[r > 3.0 * D / 8.0]
    if len(inner) < MIN_CELLS or len(outer) < MIN_CELLS:
        return cv, nan
    return cv, _ratio(float(inner.mean()), float(outer.mean()))


def measures(rec, cells=None, c=None, ref_diameter=1024.0, dark=32, bright=240):
    """One record [GRAD_REC] -> {MEASURES}: fov_area and focus_scale as int, the rest float64 formed from the integers, nan wherever a
    denominator is 0.
        fov_fill       n / (pi / 4 box_w box_h): 1 for an ellipse that fills its bounding box, up to 4 / pi for a circle cut straight at
                       the top and bottom (wide-format cameras) or a full rectangle (a crop), below 1 for a ragged or shaded field
        luma_mean, luma_std, luma_pXX (`percentile`), contrast = p95 - p05, entropy (bits) of the luma histogram
        mean_r/g/b, sat_r/g/b (fractions of the field at or above the record's `sat`)
        dark_frac      the fraction with Y < dark; bright_frac with Y >= bright
        focus_d = E_d / n_d, edge_d = Q_d / n_d, focus_ratio = focus_1 / focus_4 (blur removes the finest scale first: the ratio
                       falls with defocus whatever the picture's contrast)
        focus_scale    `focus_scale(n, ref_diameter)`; focus = the focus_d at that dilation
        evenness_cv, centre_edge   `illumination` of locate's cell table `cells` at side `c` (nan without one)
    ref_diameter = 1024 is a convention of this module — the field diameter at which a dilation of 1 is taken as the finest scale —
    not a measured value."""
    r = split_record(rec)
    if r["hist"].ndim != 1:
        raise ValueError("measures takes one record (got %s)" % (np.asarray(rec).shape,))
    hist, n = r["hist"], int(r["area"])
    top, bottom, left, right = (int(v) for v in r["box"])
    levels = np.arange(256, dtype=np.int64)
    s1, s2 = int((hist * levels).sum()), int((hist * levels * levels).sum())
    out = {"fov_area": n, "focus_scale": focus_scale(n, ref_diameter)}
    out["fov_fill"] = _ratio(n, math.pi / 4.0 * (right - left + 1) * (bottom - top + 1)) if n else float("nan")
    out["luma_mean"] = _ratio(s1, n)
    out["luma_std"] = float(math.sqrt(max(_ratio(n * s2 - s1 * s1, n * n), 0.0))) if n else float("nan")
    for q in PERCENTILES:
        out["luma_p%02d" % q] = percentile(hist, q)
    out["contrast"] = out["luma_p95"] - out["luma_p05"]
    p = hist[hist > 0].astype(np.float64) / np.float64(max(n, 1))
    out["entropy"] = float(-(p * np.log2(p)).sum()) if n else float("nan")
    for k, ch in enumerate("rgb"):
        out["mean_" + ch], out["sat_" + ch] = _ratio(int(r["sums"][k]), n), _ratio(int(r["sat"][k]), n)
    out["dark_frac"], out["bright_frac"] = _ratio(int(hist[:int(dark)].sum()), n), _ratio(int(hist[int(bright):].sum()), n)
    for k, d in enumerate(DILATIONS):
        nd, ed, qd = (int(v) for v in r["focus"][k])
        out["focus_%d" % d], out["edge_%d" % d] = _ratio(ed, nd), _ratio(qd, nd)
    f1, f4 = out["focus_1"], out["focus_4"]
    out["focus_ratio"] = float("nan") if not (f1 == f1 and f4 == f4) or f4 == 0.0 else f1 / f4
    out["focus"] = out["focus_%d" % out["focus_scale"]]
    out["evenness_cv"], out["centre_edge"] = illumination(cells, c, n, r["box"]) if cells is not None and n else (float("nan"),) * 2
    return out


# ---- judging ----------------------------------------------------------------------------------------------------------------
class Gradability:
    """The thresholds of a run and the parameters of its records.  judge(measures) -> {FLAGS}: per threshold 1 (pass), 0 (fail) or
    -1 (threshold not given, or the measure is nan), and gradable = 1 if no judged flag fails, 0 if one does, -1 if nothing was
    judged.
        min_focus        focus >= it            min_focus_ratio   focus_ratio >= it
        max_dark         dark_frac <= it        max_bright        bright_frac <= it
        max_cv           evenness_cv <= it      min_fov_fill      fov_fill >= it
    There are NO default thresholds, on purpose: nobody has measured them on real photographs against a grader, and a made-up
    number here would read as a recommendation.  Without any the measures and `ranks` are still written.  dark / bright: the luma
    levels of dark_frac and bright_frac; sat: the channel level counted as saturated; t: the field threshold of a photograph-level
    record where the caller has no other (locate uses its --fov-threshold, crops are scored with 0)."""

    RULES = (("ok_focus", "min_focus", "focus", 1), ("ok_focus_ratio", "min_focus_ratio", "focus_ratio", 1), ("ok_dark", "max_dark", "dark_frac", -1),
             ("ok_bright", "max_bright", "bright_frac", -1), ("ok_cv", "max_cv", "evenness_cv", -1), ("ok_fov_fill", "min_fov_fill", "fov_fill", 1))

    def __init__(self, min_focus=None, min_focus_ratio=None, max_dark=None, max_bright=None, max_cv=None, min_fov_fill=None, dark=32,
                 bright=240, sat=250, t=24):
        for name, v, hi in (("min_focus", min_focus, math.inf), ("min_focus_ratio", min_focus_ratio, math.inf), ("max_dark", max_dark, 1.0),
                            ("max_bright", max_bright, 1.0), ("max_cv", max_cv, math.inf), ("min_fov_fill", min_fov_fill, math.inf)):
            if v is not None and not 0.0 <= float(v) <= hi:
                raise ValueError("%s must lie in 0..%s (got %r)" % (name, "1" if hi == 1.0 else "inf", v))
            setattr(self, name, None if v is None else float(v))
        for name, v, lo in (("dark", dark, 0), ("bright", bright, 0), ("sat", sat, 1), ("t", t, 0)):
            if int(v) != v or not lo <= int(v) <= 255:
                raise ValueError("%s must be an integer in %d..255 (got %r)" % (name, lo, v))
            setattr(self, name, int(v))
        if self.dark > self.bright:
            raise ValueError("dark must not exceed bright (got %d, %d)" % (self.dark, self.bright))

    def config(self):
        """What summary.json records."""
        return {k: getattr(self, k) for _, k, _, _ in self.RULES} | {"dark": self.dark, "bright": self.bright, "sat": self.sat}

    def measures(self, rec, cells=None, c=None):
        return measures(rec, cells, c, dark=self.dark, bright=self.bright)

    def judge(self, m):
        out, judged, failed = {}, 0, 0
        for flag, key, name, sign in self.RULES:
            limit, v = getattr(self, key), float(m[name])
            if limit is None or v != v:
                out[flag] = -1
                continue
            out[flag] = int(v >= limit if sign > 0 else v <= limit)
            judged, failed = judged + 1, failed + (1 - out[flag])
        out["gradable"] = -1 if not judged else int(not failed)
        return out


def ranks(values):
    """Percentile ranks within a run: 100 (the values below + half the values equal, itself included) / the values that are not nan;
    ties share their average, nan stays nan.  A folder's pictures can be ordered by focus_ratio without any threshold."""
    v = np.asarray(values, np.float64)
    ok = v == v
    m = int(ok.sum())
    out = np.full(v.shape, np.nan)
    for i in np.nonzero(ok)[0]:
        out[i] = 100.0 * (float((v[ok] < v[i]).sum()) + 0.5 * float((v[ok] == v[i]).sum())) / m
    return [float(x) for x in out]


# ---- gradability.csv ----------------------------------------------------------------------------------------------------------
def columns(prefixes=("",)):
    """index, name, the measures (once per prefix: locate writes photo_ and roi_), the flags, focus_rank."""
    return ("index", "name") + tuple(p + k for p in prefixes for k in MEASURES) + FLAGS + ("focus_rank",)


def _ints(prefixes):
    return ("index",) + tuple(p + k for p in prefixes for k in INT_MEASURES) + FLAGS


def finish_rows(rows, judge, prefixes=("",)):
    """rows: [{index, name, <prefix><measure> ...}] -> the same rows with `judge`'s flags on the first prefix's measures and focus_rank
    = `ranks` of its focus_ratio over the run."""
    p = prefixes[0]
    rk = ranks([r[p + "focus_ratio"] for r in rows])
    return [dict(r, focus_rank=rk[i], **judge.judge({k: r[p + k] for k in MEASURES})) for i, r in enumerate(rows)]


def summarise(rows, judge):
    return dict(judge.config(), n_judged=sum(1 for r in rows if r["gradable"] != -1), n_gradable=sum(1 for r in rows if r["gradable"] == 1))


def write_csv(out_dir, rows, prefixes=("",)):
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, "gradability.csv"), columns(prefixes), rows, _ints(prefixes))


def read_csv(out_dir):
    path = os.path.join(out_dir, "gradability.csv")
    with open(path) as f:
        header = f.readline().strip().split(",")
    prefixes = tuple(k[:-len("fov_area")] for k in header if k.endswith("fov_area"))
    return T.read_csv(path, _ints(prefixes))


def crop_cell(h, w):
    """The cell side of the table a crop's illumination is read from."""
    return max(2, min(256, min(int(h), int(w)) // 8))


# ---- command line (segment.add_arguments) ---------------------------------------------------------------------------------------
def add_arguments(ap):
    ap.add_argument("--gradability", action="store_true", help="focus, exposure and field measures per image: gradability.csv")
    ap.add_argument("--min-focus", type=float, default=None, help="flag images whose focus (Laplacian energy at the field's scale) is below")
    ap.add_argument("--min-focus-ratio", type=float, default=None, help="flag images whose focus_1 / focus_4 is below")
    ap.add_argument("--max-dark", type=float, default=None, help="flag images with a larger fraction of the field below --grad-dark")
    ap.add_argument("--max-bright", type=float, default=None, help="flag images with a larger fraction of the field at or above --grad-bright")
    ap.add_argument("--max-cv", type=float, default=None, help="flag images whose illumination varies more over the field (evenness_cv)")
    ap.add_argument("--min-fov-fill", type=float, default=None, help="flag images whose field fills less of its bounding ellipse")
    ap.add_argument("--grad-dark", type=int, default=32, help="the luma level below which a pixel counts as dark")
    ap.add_argument("--grad-bright", type=int, default=240, help="the luma level from which a pixel counts as bright")


def from_arguments(args):
    """-> the Gradability of the parsed switches, None with --gradability off (ValueError: a range)."""
    if not args.gradability:
        return None
    return Gradability(args.min_focus, args.min_focus_ratio, args.max_dark, args.max_bright, args.max_cv, args.min_fov_fill,
                       dark=args.grad_dark, bright=args.grad_bright)
