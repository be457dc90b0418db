"""Optic-disc morphometry: what a cup-to-disc tool is expected to say beyond three ratios of bounding boxes — an ellipse fitted to the
disc and to the cup, the width of the neuroretinal rim around the disc, its thinnest place and the ISNT check.

The device does one exact integer pass over a (disc, cup) pair of post-processed masks (ops.onh_profile, csrc/morphometry.hip) behind
ops.mask_geometry's record of the disc: per angular sector around the disc's centroid the largest squared distance and the pixel count
of either mask, and the second-order sums of both.  This module holds the host side: `sector_table`, the one place the sector
directions are made; `profile_host`, the numpy restatement of the pass (it sits beside the device path as segment.mask_geometry_host
does, and equals it bit for bit); `ellipse` / `finish`, the float64 arithmetic behind the records; the tables.

Conventions.  Angles are in degrees, counter-clockwise on the screen from image-right (3 o'clock), so 90 is up (superior).  Sector s
of N covers [360 s / N, 360 (s + 1) / N); its centre is 360 (s + 0.5) / N.  Lengths are in pixels of the masks' own size.  The centre
is the disc's centroid rounded to half a pixel.  A sector's radius is the largest centre-to-pixel-centre distance of the mask's pixels
in it, `rim[s]` the disc's radius minus the cup's: a sector without a cup pixel has cup radius 0 (with many sectors — narrower than
about a pixel at the cup's edge — that reads as "no cup here"), a sector without a disc pixel is nan, and a cup that sticks out of the
disc gives a negative width, reported as it is (the cup is NOT clipped to the disc, segment.py's convention).  Quadrants: superior
[45, 135), left [135, 225), inferior [225, 315), right [315, 45).  eye = "right": the macula lies to the left of the disc in the
photograph, so temporal = left and nasal = right; eye = "left" mirrors that; eye = None leaves nasal / temporal / isnt undefined (nan).
"""
import math
import os

import numpy as np

from . import tables as T

MIN_SECTORS, MAX_SECTORS = 8, 360
EYES = (None, "right", "left")
SCALE = 1 << 20

INT_COLUMNS = ("height", "width", "sectors", "disc_area", "cup_area")
ELLIPSE_FIELDS = ("major", "minor", "angle", "v_extent", "h_extent")
FLOAT_COLUMNS = ("centre_y", "centre_x") + tuple("%s_%s" % (m, f) for m in ("disc", "cup") for f in ELLIPSE_FIELDS) + \
    ("vcdr_ellipse", "hcdr_ellipse", "rim_min", "rim_min_rel", "rim_min_angle", "rim_superior", "rim_inferior", "rim_left", "rim_right",
     "rim_nasal", "rim_temporal", "isnt")
MORPH_COLUMNS = ("index", "name", "eye") + INT_COLUMNS + FLOAT_COLUMNS
STAT_KEYS = ("vcdr_ellipse", "hcdr_ellipse", "rim_min_rel")
STATS = ("mean", "std", "p05", "p95")
STAT_COLUMNS = ("n_samples", "n_defined") + tuple("%s_%s" % (r, s) for r in STAT_KEYS for s in STATS)
ERROR_COLUMNS = tuple("%s_%s" % (k, s) for k in STAT_KEYS for s in ("pred", "label", "abs_diff"))
NAN = float("nan")


def check_sectors(N):
    if isinstance(N, bool) or int(N) != N or not (MIN_SECTORS <= int(N) <= MAX_SECTORS and int(N) % 8 == 0):
        raise ValueError("sectors must be a multiple of 8 in %d..%d (got %r)" % (MIN_SECTORS, MAX_SECTORS, N))
    return int(N)


def check_eye(eye):
    if eye not in EYES:
        raise ValueError("eye must be None, 'right' or 'left' (got %r)" % (eye,))
    return eye


# ---- the host specification -----------------------------------------------------------------------------------------------
def sector_table(N):
    """-> int32 [N + 1, 2]: T[k] = (rint(2^20 cos(2 pi k / N)), rint(2^20 sin(2 pi k / N))) in float64, k = 0..N.  The device and
    profile_host read these integers and nothing else (no atan2 on either side).  N % 8 == 0 makes the axis entries exact."""
    N = check_sectors(N)
    a = 2.0 * np.pi * np.arange(N + 1, dtype=np.float64) / N
    return np.stack((np.rint(SCALE * np.cos(a)), np.rint(SCALE * np.sin(a))), -1).astype(np.int32)


def centre2(rec_disc):
    """A disc's geometry record -> (c2y, c2x): twice its centroid rounded half up, exact in Python ints; (0, 0) when it is empty."""
    area, sum_r, sum_c = int(rec_disc[0]), int(rec_disc[5]), int(rec_disc[6])
    if area == 0:
        return 0, 0
    return (4 * sum_r + area) // (2 * area), (4 * sum_c + area) // (2 * area)


def sectors_of(px, py, T):
    """int64 pixel vectors -> the sector of each: the s with cross(T[s], p) >= 0 > cross(T[s + 1], p); p = 0 -> 0.  Raises if a
    vector has not exactly one such s (it always has: the table's directions turn strictly counter-clockwise)."""
    px, py = np.asarray(px, np.int64).reshape(-1), np.asarray(py, np.int64).reshape(-1)
    T = np.asarray(T, np.int64)
    if len(px) > 1 << 16:                                                     # [N + 1, n] int64 at a time: keep it small
        return np.concatenate([sectors_of(px[i:i + (1 << 16)], py[i:i + (1 << 16)], T) for i in range(0, len(px), 1 << 16)])
    ge = (T[:, 0, None] * py[None] - T[:, 1, None] * px[None]) >= 0          # [N + 1, n]
    hit = ge[:-1] & ~ge[1:]
    zero = (px == 0) & (py == 0)
    if not np.all((hit.sum(0) == 1) | zero):
        raise AssertionError("a pixel vector with %s sectors" % sorted(set(hit.sum(0)[~zero].tolist())))
    return np.where(zero, 0, hit.argmax(0)).astype(np.int64)


def profile_host(disc, cup, N):
    """wtpse_onh_profile in numpy: disc, cup [..., h, w] (nonzero = object; leading dimensions are flattened to B) ->
    (profile uint32 [B, N, 4] = (disc_r2, cup_r2, disc_n, cup_n) per sector, moments int64 [B, 2, 4] = per mask (sum y^2, sum x^2,
    sum x y, .) with c2y in the disc's fourth slot and c2x in the cup's).  Built on segment.mask_geometry_host."""
    from .segment import mask_geometry_host
    T = sector_table(N)
    disc, cup = np.asarray(disc) != 0, np.asarray(cup) != 0
    if disc.shape != cup.shape or disc.ndim < 2:
        raise ValueError("disc %s and cup %s must be masks of one shape" % (disc.shape, cup.shape))
    h, w = disc.shape[-2:]
    disc, cup = disc.reshape(-1, h, w), cup.reshape(-1, h, w)
    B = disc.shape[0]
    profile, moments = np.zeros((B, N, 4), np.uint32), np.zeros((B, 2, 4), np.int64)
    geom = mask_geometry_host(disc)
    for b in range(B):
        c2y, c2x = centre2(geom[b])
        for j, m in enumerate((disc[b], cup[b])):
            y, x = [v.astype(np.int64) for v in np.nonzero(m)]
            moments[b, j, :3] = ((y * y).sum(), (x * x).sum(), (x * y).sum())
            if geom[b, 0] == 0 or len(y) == 0:
                continue
            px, py = 2 * x - c2x, c2y - 2 * y
            s, r2 = sectors_of(px, py, T), px * px + py * py
            np.maximum.at(profile[b, :, j], s, r2.astype(np.uint32))
            profile[b, :, 2 + j] = np.bincount(s, minlength=N).astype(np.uint32)
        moments[b, 0, 3], moments[b, 1, 3] = c2y, c2x
    return profile, moments


# ---- the finishing arithmetic ---------------------------------------------------------------------------------------------
def central_moments(area, sum_r, sum_c, syy, sxx, sxy):
    """-> (mu_yy, mu_xx, mu_xy) of a mask's pixels as unit squares: (A S2 - S1^2) / A^2 (+ 1/12 on the diagonal), the integer numerators
    exact in Python ints, divided in float64.  nan for an empty mask."""
    A, sy, sx, syy, sxx, sxy = int(area), int(sum_r), int(sum_c), int(syy), int(sxx), int(sxy)
    if A == 0:
        return NAN, NAN, NAN
    a2 = float(A * A)
    return (float(A * syy - sy * sy) / a2 + 1.0 / 12.0, float(A * sxx - sx * sx) / a2 + 1.0 / 12.0, float(A * sxy - sy * sx) / a2)


def ellipse(area, sum_r, sum_c, syy, sxx, sxy):
    """The ellipse with a mask's second moments -> {major, minor (full lengths 4 sqrt(lambda), pixels), angle (degrees in [0, 180) of
    the major axis, counter-clockwise on the screen from image-right), v_extent = 4 sqrt(mu_yy), h_extent = 4 sqrt(mu_xx)}; all nan
    for an empty mask."""
    myy, mxx, mxy = central_moments(area, sum_r, sum_c, syy, sxx, sxy)
    if myy != myy:
        return dict.fromkeys(ELLIPSE_FIELDS, NAN)
    mid, half = 0.5 * (mxx + myy), 0.5 * (mxx - myy)
    rad = math.sqrt(half * half + mxy * mxy)
    l1, l2 = mid + rad, max(mid - rad, 0.0)
    # image rows grow downwards: the axis' angle on the screen is minus its angle in (x, y) image coordinates
    ang = math.degrees(-0.5 * math.atan2(2.0 * mxy, mxx - myy)) % 180.0
    return {"major": 4.0 * math.sqrt(l1), "minor": 4.0 * math.sqrt(l2), "angle": 0.0 if ang >= 180.0 else ang,
            "v_extent": 4.0 * math.sqrt(myy), "h_extent": 4.0 * math.sqrt(mxx)}


def _nanmean(v):
    v = [x for x in v if x == x]
    return float(np.mean(np.array(v, np.float64))) if v else NAN


def quadrant_means(rim):
    """A rim profile of N sectors -> (superior, left, inferior, right): the means over the non-nan sectors whose centre lies in
    [45, 135), [135, 225), [225, 315), [315, 45)."""
    N = len(rim)
    e = N // 8
    rim = [float(v) for v in rim]
    return (_nanmean(rim[e:3 * e]), _nanmean(rim[3 * e:5 * e]), _nanmean(rim[5 * e:7 * e]), _nanmean(rim[7 * e:] + rim[:e]))


def isnt_rule(inferior, superior, nasal, temporal):
    """1.0 when inferior >= superior >= nasal >= temporal, 0.0 when not, nan when one of them is undefined."""
    v = (inferior, superior, nasal, temporal)
    if any(x != x for x in v):
        return NAN
    return 1.0 if v[0] >= v[1] >= v[2] >= v[3] else 0.0


def finish(rec_disc, rec_cup, moments, profile, h, w, eye=None):
    """One image's two geometry records, its moments [2, 4] and profile [N, 4] -> its row without index and name: MORPH_COLUMNS plus
    "rim" and "rim_rel", lists of N floats.  float64 throughout."""
    check_eye(eye)
    d, c = [int(v) for v in rec_disc], [int(v) for v in rec_cup]
    moments, profile = np.asarray(moments), np.asarray(profile)
    N = check_sectors(profile.shape[0])
    row = {"height": int(h), "width": int(w), "sectors": N, "eye": eye or "", "disc_area": d[0], "cup_area": c[0]}
    row["centre_y"], row["centre_x"] = (int(moments[0, 3]) / 2.0, int(moments[1, 3]) / 2.0) if d[0] else (NAN, NAN)
    mu = {}
    for j, (name, r) in enumerate((("disc", d), ("cup", c))):
        args = (r[0], r[5], r[6], int(moments[j, 0]), int(moments[j, 1]), int(moments[j, 2]))
        mu[name] = central_moments(*args)
        row.update({"%s_%s" % (name, k): v for k, v in ellipse(*args).items()})
    for key, i in (("vcdr_ellipse", 0), ("hcdr_ellipse", 1)):
        row[key] = NAN if d[0] == 0 else 0.0 if c[0] == 0 else math.sqrt(mu["cup"][i] / mu["disc"][i])
    rim = []
    for s in range(N):
        dr2, cr2, dn, cn = [int(v) for v in profile[s]]
        rim.append(math.sqrt(dr2) / 2.0 - (math.sqrt(cr2) / 2.0 if cn else 0.0) if d[0] and dn else NAN)
    unit = math.sqrt(d[0] / math.pi) if d[0] else NAN
    row["rim"], row["rim_rel"] = rim, [v / unit for v in rim]
    defined = [s for s in range(N) if rim[s] == rim[s]]
    if defined:
        s0 = min(defined, key=lambda s: (rim[s], s))                 # the first minimum wins
        row["rim_min"], row["rim_min_rel"], row["rim_min_angle"] = rim[s0], rim[s0] / unit, 360.0 * (s0 + 0.5) / N
    else:
        row["rim_min"] = row["rim_min_rel"] = row["rim_min_angle"] = NAN
    row["rim_superior"], row["rim_left"], row["rim_inferior"], row["rim_right"] = quadrant_means(rim)
    if eye is None:
        row["rim_nasal"] = row["rim_temporal"] = row["isnt"] = NAN
    else:
        row["rim_temporal"], row["rim_nasal"] = (row["rim_left"], row["rim_right"]) if eye == "right" else (row["rim_right"], row["rim_left"])
        row["isnt"] = isnt_rule(row["rim_inferior"], row["rim_superior"], row["rim_nasal"], row["rim_temporal"])
    return row


def finish_batch(rec, moments, profile, h, w, eye=None):
    """rec [2 n, 8] (the n discs' records, then the n cups'), moments [n, 2, 4], profile [n, N, 4] -> n rows."""
    n = len(moments)
    return [finish(rec[j], rec[n + j], moments[j], profile[j], h, w, eye) for j in range(n)]


def summarise(rows, eye=None):
    """-> {sectors, mean_vcdr_ellipse, mean_rim_min_rel} (means over the rows where defined, None when there is none) and, with an
    eye, n_isnt_violations: the rows whose isnt is 0."""
    out = {"sectors": rows[0]["sectors"] if rows else None}
    for k in ("vcdr_ellipse", "rim_min_rel"):
        m = _nanmean([r[k] for r in rows])
        out["mean_" + k] = m if m == m else None
    if eye is not None:
        out["n_isnt_violations"] = sum(1 for r in rows if r["isnt"] == 0.0)
    return out


def sample_statistics(samples):
    """samples: the `finish` rows of one image's K samples -> {STAT_COLUMNS, "rim_rel_std": [N]}.  A sample with an empty disc is left
    out and n_defined counts the others; with none left every statistic is nan.  std is the population standard deviation, the
    percentiles numpy.percentile's (linear interpolation) — uncertainty.ratio_statistics' rule; a nan among the kept values (a
    disc without a rim sector cannot happen, but the rule is stated) is left out of that key's statistics.  rim_rel_std[s] is the
    population standard deviation of rim_rel[s] over the kept samples in which the sector is defined."""
    keep = [s for s in samples if s["disc_area"] > 0]
    out = {"n_samples": len(samples), "n_defined": len(keep)}
    for r in STAT_KEYS:
        v = np.array([s[r] for s in keep if s[r] == s[r]], np.float64)
        vals = (float(v.mean()), float(v.std()), float(np.percentile(v, 5)), float(np.percentile(v, 95))) if len(v) else (NAN,) * 4
        out.update({"%s_%s" % (r, s): x for s, x in zip(STATS, vals)})
    N = samples[0]["sectors"] if samples else 0
    std = []
    for s in range(N):
        v = np.array([k["rim_rel"][s] for k in keep if k["rim_rel"][s] == k["rim_rel"][s]], np.float64)
        std.append(float(v.std()) if len(v) else NAN)
    out["rim_rel_std"] = std
    return out


def error_row(pred, label):
    """Two `finish` rows of one image -> {ERROR_COLUMNS}: the predicted and the label's value of each STAT_KEYS and |difference|."""
    out = {}
    for k in STAT_KEYS:
        out[k + "_pred"], out[k + "_label"], out[k + "_abs_diff"] = pred[k], label[k], abs(pred[k] - label[k])
    return out


def error_means(rows):
    """-> {"mean_<ERROR_COLUMNS>": the mean over the rows where defined, None when there is none}."""
    out = {}
    for k in ERROR_COLUMNS:
        m = _nanmean([r[k] for r in rows])
        out["mean_" + k] = m if m == m else None
    return out


# ---- the tables -----------------------------------------------------------------------------------------------------------
def rim_columns(N):
    return tuple("rim_%03d" % s for s in range(N))


def write_csv(out_dir, rows):
    """rows: [{MORPH_COLUMNS, rim}] -> out_dir/morphometry.csv and out_dir/rim_profile.csv (index, name, rim_000 .. rim_{N-1}, pixels
    at the image's own size).  Floats as repr: they read back to the same float64; nan as "nan"."""
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, "morphometry.csv"), MORPH_COLUMNS, rows, ("index",) + INT_COLUMNS, ("name", "eye"))
    cols = rim_columns(rows[0]["sectors"]) if rows else ()
    T.write_csv(os.path.join(out_dir, "rim_profile.csv"), ("index", "name") + cols,
                [dict(zip(cols, r["rim"]), index=r["index"], name=r["name"]) for r in rows], ("index",))


def read_csv(out_dir):
    """-> the rows as write_csv wrote them, "rim" (from rim_profile.csv) included."""
    rows = T.read_csv(os.path.join(out_dir, "morphometry.csv"), ("index",) + INT_COLUMNS, ("name", "eye"))
    rims = T.read_csv(os.path.join(out_dir, "rim_profile.csv"), ("index",))
    for r, p in zip(rows, rims):
        assert (r["index"], r["name"]) == (p["index"], p["name"])
        r["rim"] = [p[k] for k in rim_columns(r["sectors"])]
    return rows


def write_uncertainty_csv(out_dir, rows):
    """rows: [{index, name, sample_statistics(...)}] -> out_dir/morphometry_uncertainty.csv: STAT_COLUMNS and rim_rel_std_000 ..."""
    os.makedirs(out_dir, exist_ok=True)
    cols = tuple("rim_rel_std_%03d" % s for s in range(len(rows[0]["rim_rel_std"]))) if rows else ()
    T.write_csv(os.path.join(out_dir, "morphometry_uncertainty.csv"), ("index", "name") + STAT_COLUMNS + cols,
                [dict(r, **dict(zip(cols, r["rim_rel_std"]))) for r in rows], ("index", "n_samples", "n_defined"))


def read_uncertainty_csv(out_dir):
    rows = T.read_csv(os.path.join(out_dir, "morphometry_uncertainty.csv"), ("index", "n_samples", "n_defined"))
    return [dict({k: v for k, v in r.items() if not k.startswith("rim_rel_std_")},
                 rim_rel_std=[v for k, v in r.items() if k.startswith("rim_rel_std_")]) for r in rows]


def write_errors_csv(out_dir, rows):
    """rows: [{index, name, ERROR_COLUMNS}] -> out_dir/morphometry_errors.csv, closed by a row named "mean" (index 0): the means over
    the images where the value is defined.  -> error_means(rows)."""
    os.makedirs(out_dir, exist_ok=True)
    means = error_means(rows)
    last = dict({k: NAN if means["mean_" + k] is None else means["mean_" + k] for k in ERROR_COLUMNS}, index=0, name="mean")
    T.write_csv(os.path.join(out_dir, "morphometry_errors.csv"), ("index", "name") + ERROR_COLUMNS, list(rows) + [last], ("index",))
    return means


def read_errors_csv(out_dir):
    """-> (rows, the closing row of means)."""
    rows = T.read_csv(os.path.join(out_dir, "morphometry_errors.csv"), ("index",))
    return rows[:-1], rows[-1]
