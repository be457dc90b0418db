"""wtpse_hip/calibration.py on the host: hist_host (the specification of wtpse_calibration_hist) on a hand-made case with every count
written out, the scores against direct computation from the pixels (no histogram), histograms whose scores are known in closed form,
the risk-coverage curve against a sort of the expanded pixels, and the small functions of the image-level table and of the run's
command line."""
import math

import numpy as np
import pytest

NAN = float("nan")


# ---- hist_host ------------------------------------------------------------------------------------------------------------------
def special_case():
    """15 pixels (prob, spread, label, region) at threshold 0.75 and what they must count, as {(histogram, bin, column): count} and
    the tail.  tests/test_calibration_gpu.py plants the same pixels."""
    f = np.float32
    px = [(0.0, 0.0, 0, 1),                     # 0  prob exactly 0:            p[0][0]     s[0][0]
          (1.0, 0.0, 1, 1),                     # 1  prob exactly 1:            p[1024][1]  s[0][0]
          (-0.25, 0.25, 1, 1),                  # 2  clamped to 0, a miss:      p[0][1]     s[512][1]
          (1.5, 0.7, 0, 1),                     # 3  clamped to 1, spread to .5 p[1024][0]  s[1024][1]
          (NAN, 0.0, 1, 1),                     # 4  NaN prob:                  tail[2]
          (0.5, NAN, 0, 1),                     # 5  NaN spread:                tail[2]
          (0.5 / 1024, 0.0, 0, 1),              # 6  tie 0.5 -> 0:              p[0][0]     s[0][0]
          (1.5 / 1024, 0.0, 1, 1),              # 7  tie 1.5 -> 2, a miss:      p[2][1]     s[0][1]
          (0.75, 0.125, 1, 1),                  # 8  prob == threshold: not predicted, a miss   p[768][1]  s[256][1]
          (0.9, 0.0, 0, 0),                     # 9  region 0, background:      tail[0]
          (0.1, 0.0, 1, 0),                     # 10 region 0, object:          tail[1]
          (NAN, 0.0, 1, 0),                     # 11 region 0 comes first:      tail[1]
          (0.8, 0.25, 2.0, 1),                  # 12 a label of 2 is an object; float32(0.8) * 1024 = 819.2..: p[819][1]  s[512][0]
          (2.5 / 1024, 0.5 / 2048, 0, 1),       # 13 ties 2.5 -> 2, 0.5 -> 0:   p[2][0]     s[0][0]
          (float(np.nextafter(f(0.75), f(1))), 1.5 / 2048, 0, 1)]       # 14 just above the threshold, a false alarm; tie 1.5 -> 2: p[768][0]  s[2][1]
    want = {("p", 0, 0): 2, ("p", 0, 1): 1, ("p", 2, 0): 1, ("p", 2, 1): 1, ("p", 768, 0): 1, ("p", 768, 1): 1, ("p", 819, 1): 1,
            ("p", 1024, 0): 1, ("p", 1024, 1): 1,
            ("s", 0, 0): 4, ("s", 0, 1): 1, ("s", 2, 1): 1, ("s", 256, 1): 1, ("s", 512, 0): 1, ("s", 512, 1): 1, ("s", 1024, 1): 1}
    tail = (1, 2, 2, 10)
    a = np.array(px, np.float64)
    return a[:, 0].astype(f), a[:, 1].astype(f), a[:, 2].astype(f), a[:, 3].astype(np.uint8), want, tail


def expected_record(want, tail):
    from wtpse_hip import calibration as C
    rec = np.zeros(C.REC, np.uint32)
    for (which, b, col), n in want.items():
        rec[(0 if which == "p" else 2 * (C.BINS + 1)) + 2 * b + col] = n
    rec[-4:] = tail
    return rec


def test_hist_host_on_the_hand_made_case():
    from wtpse_hip import calibration as C
    prob, spread, label, region, want, tail = special_case()
    shape = (1, 3, 5)
    rec = C.hist_host(prob.reshape(shape), spread.reshape(shape), label.reshape(shape), region.reshape(shape), 0.75)
    assert rec.dtype == np.uint32 and rec.shape == (1, C.REC) and C.REC == 4104
    hp, hs, tl = C.split_record(rec[0])
    got = {("p", b, c): int(hp[b, c]) for b, c in np.argwhere(hp)}
    got.update({("s", b, c): int(hs[b, c]) for b, c in np.argwhere(hs)})
    assert got == want
    assert tuple(int(v) for v in tl) == tail
    assert np.array_equal(rec[0], expected_record(want, tail))
    assert hp.sum() == hs.sum() == tl[3] and tl.sum() == 15
    # no region, no spread: the excluded pixels are scored (pixel 11 is invalid now), every spread is bin 0
    rec = C.hist_host(prob.reshape(shape), None, label.reshape(shape), None, 0.75)
    hp, hs, tl = C.split_record(rec[0])
    assert tuple(int(v) for v in tl) == (0, 0, 2, 13)             # pixel 5's spread is no longer NaN, pixel 11's prob is
    assert int(hs[0].sum()) == 13 and int(hs[1:].sum()) == 0
    assert int(hp[922, 0]) == 1 and int(hp[102, 1]) == 1 and int(hp[512, 0]) == 1        # pixels 9, 10, 5
    with pytest.raises(ValueError):
        C.hist_host(prob.reshape(shape), spread.reshape(1, 15, 1)[:, :14], label.reshape(shape))
    with pytest.raises(ValueError):
        C.split_record(np.zeros(10))


# ---- scores against the pixels ----------------------------------------------------------------------------------------------------
def _pairs(seed, n):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1025, n)
    q[:4] = (0, 1024, 64, 960)                                       # the ends and two bin edges
    y = (rng.random(n) < 0.15 + 0.7 * q / 1024.0).astype(np.int64)
    return q, y


def _hist_of(q, y):
    h = np.zeros((1025, 2), np.int64)
    np.add.at(h, (q, y), 1)
    return h


def _auroc_pairs(score, positive):
    """O(n^2): P(score of a positive > score of a negative) + 0.5 P(equal)."""
    pos, neg = score[positive], score[~positive]
    gt = (pos[:, None] > neg[None, :]).sum()
    eq = (pos[:, None] == neg[None, :]).sum()
    return (gt + 0.5 * eq) / (len(pos) * len(neg))


@pytest.mark.parametrize("bins", [16, 8, 1024])
def test_scores_and_reliability_match_direct_computation(bins):
    from wtpse_hip import calibration as C
    q, y = _pairs(11, 4000)
    p = q / 1024.0
    h = _hist_of(q, y)
    which = np.minimum(np.floor(p * bins).astype(int), bins - 1)
    ece, mce = 0.0, 0.0
    rel = C.reliability(h, bins)
    assert len(rel) == bins
    for k in range(bins):
        m = which == k
        assert rel[k]["bin"] == k and rel[k]["lo"] == k / bins and rel[k]["hi"] == (k + 1) / bins and rel[k]["n"] == int(m.sum())
        if not m.any():
            assert rel[k]["mean_conf"] != rel[k]["mean_conf"] and rel[k]["frac_pos"] != rel[k]["frac_pos"]
            continue
        assert abs(rel[k]["mean_conf"] - p[m].mean()) < 1e-12 and abs(rel[k]["frac_pos"] - y[m].mean()) < 1e-12
        gap = abs(y[m].mean() - p[m].mean())
        ece += m.sum() / len(q) * gap
        mce = max(mce, gap)
    pc = np.clip(p, 2.0 ** -11, 1 - 2.0 ** -11)
    s = C.scores(h, bins)
    assert s["n"] == 4000
    assert abs(s["ece"] - ece) < 1e-12 and abs(s["mce"] - mce) < 1e-12
    assert abs(s["brier"] - ((p - y) ** 2).mean()) < 1e-12
    assert abs(s["nll"] - (-(y * np.log(pc) + (1 - y) * np.log(1 - pc)).mean())) < 1e-12
    assert rel[-1]["n"] >= 1 and int(h[1024].sum()) >= 1             # q = 1024 sits in the last bin


def test_auroc_matches_a_pair_count_with_ties():
    from wtpse_hip import calibration as C
    rng = np.random.default_rng(5)
    q = rng.integers(500, 520, 300)                                  # 20 values for 300 pixels: many ties
    y = (rng.random(300) < (q - 495) / 30.0).astype(np.int64)
    assert 0 < y.sum() < 300
    assert abs(C.scores(_hist_of(q, y))["auroc"] - _auroc_pairs(q, y == 1)) < 1e-12
    assert C.scores(_hist_of(q, np.zeros(300, np.int64)))["auroc"] != C.scores(_hist_of(q, np.zeros(300, np.int64)))["auroc"]      # no positive
    assert math.isnan(C.scores(_hist_of(q, np.ones(300, np.int64)))["auroc"])                                                      # no negative
    assert C.scores(_hist_of(np.array([3, 9]), np.array([0, 1])))["auroc"] == 1.0
    assert C.scores(_hist_of(np.array([9, 3]), np.array([0, 1])))["auroc"] == 0.0
    assert C.scores(_hist_of(np.array([7, 7]), np.array([0, 1])))["auroc"] == 0.5


def test_undefined_scores_are_nan():
    from wtpse_hip import calibration as C
    s = C.scores(np.zeros((1025, 2), np.int64))
    assert s["n"] == 0 and all(math.isnan(s[k]) for k in ("ece", "mce", "brier", "nll", "auroc"))
    sp = C.spread_scores(np.zeros((1025, 2), np.int64))
    assert sp["n"] == 0 and all(math.isnan(sp[k]) for k in ("error_rate", "spread_wrong_mean", "spread_right_mean", "spread_auroc"))
    assert len(sp["risk_coverage"]) == 20 and all(math.isnan(r) for _, r in sp["risk_coverage"])
    h = np.zeros((1025, 2), np.int64)
    h[0, 0] = 5                                                      # right pixels only
    sp = C.spread_scores(h)
    assert sp["error_rate"] == 0.0 and math.isnan(sp["spread_wrong_mean"]) and sp["spread_right_mean"] == 0.0 and math.isnan(sp["spread_auroc"])
    with pytest.raises(ValueError):
        C.scores(np.zeros((1024, 2), np.int64))


def test_exactly_calibrated_histogram_and_its_flip():
    from wtpse_hip import calibration as C
    rng = np.random.default_rng(2)
    h = np.zeros((1025, 2), np.int64)
    n_q = 1024 * rng.integers(0, 6, 1025)                            # a multiple of 1024 per q ...
    q = np.arange(1025)
    h[:, 1] = n_q * q // 1024                                        # ... of which exactly n_q q / 1024 are objects
    h[:, 0] = n_q - h[:, 1]
    for bins in (16, 4, 1, 1024):
        s = C.scores(h, bins)
        assert s["ece"] == 0.0 and s["mce"] == 0.0
        assert all(r["frac_pos"] == r["mean_conf"] for r in C.reliability(h, bins) if r["n"])
    # the labels flipped: frac_pos = 1 - mean_conf per bin, ECE = sum_b n_b / n |1 - 2 mean_conf_b|
    flip = h[:, ::-1]
    rel = C.reliability(h, 16)
    want = sum(r["n"] / n_q.sum() * abs(1 - 2 * r["mean_conf"]) for r in rel if r["n"])
    assert abs(C.scores(flip, 16)["ece"] - want) < 1e-12
    # and one small enough to state: 1024 pixels at p = 0.25 with 256 objects, 1024 at p = 0.75 with 768
    h = np.zeros((1025, 2), np.int64)
    h[256], h[768] = (768, 256), (256, 768)
    s = C.scores(h, 16)
    assert s["ece"] == 0.0 and s["brier"] == 0.1875 and s["auroc"] == (768 * 768 + 0.5 * (256 * 768 + 768 * 256)) / (1024 * 1024)
    f = C.scores(h[:, ::-1], 16)
    assert f["ece"] == 0.5 and f["mce"] == 0.5 and f["brier"] == 0.25 * 0.0625 + 0.75 * 0.5625
    assert [r["n"] for r in C.reliability(h, 16)] == [0, 0, 0, 0, 2048 // 2, 0, 0, 0, 0, 0, 0, 0, 2048 // 2, 0, 0, 0]
    assert abs(f["nll"] - (-(0.75 * math.log(0.25) + 0.25 * math.log(0.75)))) < 1e-14


# ---- the spread -------------------------------------------------------------------------------------------------------------------
def _risk_by_sorting(u, e, k):
    """The error rate among the k n / 20 least uncertain of the expanded pixels; the group of equal u that the cut falls into gives
    its errors in proportion."""
    order = np.argsort(u, kind="stable")
    us, es = u[order], e[order]
    t = k * len(u) / 20.0
    last = us[int(math.ceil(t)) - 1]
    full, group = us < last, us == last
    return (es[full].sum() + (t - full.sum()) / group.sum() * es[group].sum()) / t


@pytest.mark.parametrize("sizes", [(95, 40, 30, 20, 15), (101, 7, 53, 29, 13)], ids=["n200", "n203"])
def test_risk_coverage_matches_a_sort_of_the_pixels(sizes):
    """Five spread bins whose error rate rises with u.  n = 200: every level is a whole number of pixels and all but the last fall
    inside a bin; n = 203: the cuts are fractional pixels."""
    from wtpse_hip import calibration as C
    bins = (0, 3, 40, 500, 1024)
    rates = (0.02, 0.1, 0.3, 0.5, 0.8)
    h = np.zeros((1025, 2), np.int64)
    u, e = [], []
    for b, n, r in zip(bins, sizes, rates):
        wrong = int(round(n * r))
        h[b] = (n - wrong, wrong)
        u += [b] * n
        e += [0] * (n - wrong) + [1] * wrong
    u, e = np.array(u), np.array(e)
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(u))
    u, e = u[perm], e[perm]
    sp = C.spread_scores(h)
    curve = sp["risk_coverage"]
    assert [c for c, _ in curve] == [k / 20.0 for k in range(1, 21)]
    for k, (c, risk) in enumerate(curve, 1):
        assert abs(risk - _risk_by_sorting(u, e, k)) < 1e-12, (k, risk)
    risks = [r for _, r in curve]
    assert all(b >= a - 1e-15 for a, b in zip(risks, risks[1:])) and risks[0] < risks[-1]      # (equal inside the first bin, to rounding)
    assert abs(risks[-1] - e.mean()) < 1e-12 and abs(sp["error_rate"] - e.mean()) < 1e-12
    assert abs(sp["spread_wrong_mean"] - (u[e == 1] / 2048.0).mean()) < 1e-12
    assert abs(sp["spread_right_mean"] - (u[e == 0] / 2048.0).mean()) < 1e-12
    assert abs(sp["spread_auroc"] - _auroc_pairs(u, e == 1)) < 1e-12 and sp["spread_auroc"] > 0.5


# ---- the image-level table ----------------------------------------------------------------------------------------------------------
def test_interval_coverage():
    from wtpse_hip import calibration as C
    cov, n = C.interval_coverage([0.5, 0.2, 0.9, NAN, 0.4, 0.3], [0.4, 0.3, 0.9, 0.1, NAN, 0.3], [0.6, 0.4, 0.9, 0.9, 0.5, 0.3])
    assert n == 4 and cov == 0.75                                    # inside, below, on both ends, undefined, undefined, on both ends
    cov, n = C.interval_coverage([NAN], [0.1], [0.2])
    assert n == 0 and math.isnan(cov)
    cov, n = C.interval_coverage([], [], [])
    assert n == 0 and math.isnan(cov)


def test_spearman():
    from wtpse_hip import calibration as C
    assert C.spearman([1, 2, 3, 4], [10, 20, 25, 100]) == 1.0
    assert C.spearman([1, 2, 3, 4], [4, 3, 2, 1]) == -1.0
    assert np.array_equal(C.average_ranks([30, 10, 30, 20, 30]), [4, 1, 4, 2, 4])
    # ties: ranks a = (1, 2.5, 2.5, 4), b = (1, 3.5, 3.5, 2) -> Pearson of the ranks, written out
    ra, rb = np.array([1, 2.5, 2.5, 4]), np.array([1, 3.5, 3.5, 2])
    want = ((ra - 2.5) * (rb - 2.5)).sum() / math.sqrt(((ra - 2.5) ** 2).sum() * ((rb - 2.5) ** 2).sum())
    assert abs(C.spearman([1, 2, 2, 4], [10, 20, 20, 15]) - want) < 1e-15 and abs(want - 1.5 / 4.5) < 1e-15
    assert math.isnan(C.spearman([1, 2], [2, 1]))                    # fewer than 3 pairs
    assert math.isnan(C.spearman([1, 2, NAN, 4], [1, NAN, 3, 4]))    # 2 defined pairs
    assert C.spearman([1, 2, NAN, 4, 5], [1, 2, 3, NAN, 9]) == 1.0   # 3 defined pairs
    assert math.isnan(C.spearman([1, 1, 1], [1, 2, 3]))              # one side constant
    with pytest.raises(ValueError):
        C.spearman([1, 2, 3], [1, 2])


def test_image_risk_coverage():
    from wtpse_hip import calibration as C
    #            most certain ......................... least, then the undefined one
    std = [0.05, 0.01, NAN, 0.02, 0.05]
    dice = [0.6, 0.9, 0.1, 0.8, 0.5]
    curve = C.image_risk_coverage(std, dice)
    assert [c for c, _ in curve] == list(C.COVERAGES) and len(curve) == 20
    order = [0.9, 0.8, 0.6, 0.5, 0.1]                                # ties in index order, nan last
    for k, (c, risk) in enumerate(curve, 1):
        kept = -(-k * 5 // 20)
        assert abs(risk - (1 - sum(order[:kept]) / kept)) < 1e-15
    assert all(math.isnan(r) for _, r in C.image_risk_coverage([], []))


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def test_csv_round_trip(tmp_path):
    from wtpse_hip import calibration as C
    rows = []
    for i, s in enumerate((0.0, 0.5)):
        r = {k: (i + 1) * 0.1 + j / 3.0 for j, k in enumerate(C.CALIBRATION_COLUMNS)}
        r.update(scale=s, structure=C.STRUCTURES[i], n_scored=10 ** 9 + i, n_excluded_neg=3, n_excluded_pos=0, n_invalid=1, n_defined=i,
                 spread_auroc=NAN, nll=1e-300)
        rows.append(r)
    C.write_csv(str(tmp_path), "calibration", rows)
    back = C.read_csv(str(tmp_path), "calibration")
    assert len(back) == 2 and all(_same(b[k], r[k]) for b, r in zip(back, rows) for k in C.CALIBRATION_COLUMNS)
    with open(tmp_path / "calibration.csv") as f:
        assert f.readline().strip().split(",") == list(C.CALIBRATION_COLUMNS)
    per = [dict({k: 0.1 * j for j, k in enumerate(C.PER_IMAGE_COLUMNS)}, scale=2.0, index=7, name='a "quoted", name.png', vcdr_inside=NAN)]
    C.write_csv(str(tmp_path), "per_image", per)
    back = C.read_csv(str(tmp_path), "per_image")
    assert all(_same(back[0][k], per[0][k]) for k in C.PER_IMAGE_COLUMNS)
    risk = [{"scale": 1.0, "structure": "cup", "level": "image", "coverage": 0.05, "risk": 1 / 3}]
    C.write_csv(str(tmp_path), "risk_coverage", risk)
    assert C.read_csv(str(tmp_path), "risk_coverage") == risk
    rel = [dict(r, scale=0.0, structure="disc") for r in C.reliability(np.ones((1025, 2), np.int64), 4)]
    C.write_csv(str(tmp_path), "reliability", rel)
    assert C.read_csv(str(tmp_path), "reliability") == rel
    assert C.PER_IMAGE_COLUMNS[:5] == ("scale", "index", "name", "disc_dice", "cup_dice") and C.PER_IMAGE_COLUMNS[-3:] == ("vcdr_inside", "disc_ece", "cup_ece")
    assert C.PER_IMAGE_COLUMNS[5:11] == ("vcdr_label", "vcdr_pred", "vcdr_mean", "vcdr_std", "vcdr_p05", "vcdr_p95") and len(C.PER_IMAGE_COLUMNS) == 26


def test_best_scales():
    from wtpse_hip import calibration as C
    rows = [{"scale": s, "structure": n, "nll": nll, "ece": ece} for s, n, nll, ece in
            ((0.0, "disc", 0.3, 0.02), (1.0, "disc", 0.2, 0.05), (2.0, "disc", 0.2, 0.01), (0.0, "cup", NAN, NAN), (1.0, "cup", NAN, 0.5))]
    assert C.best_scales(rows) == {"disc": {"lowest_nll": 1.0, "lowest_ece": 2.0}, "cup": {"lowest_nll": None, "lowest_ece": 1.0}}


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_bins_and_scales_are_checked():
    from wtpse_hip import calibration as C
    from wtpse_hip.calibration_run import CalibrationRun, parse_args
    assert [C.check_bins(b) for b in (1, 2, 16, 1024)] == [1, 2, 16, 1024]
    for bad in (7, 15, 0, -4, 2048, 2.5, True):
        with pytest.raises(ValueError):
            C.check_bins(bad)
        if bad is not True:
            with pytest.raises(ValueError):
                C.reliability(np.zeros((1025, 2), np.int64), bad)
    assert C.parse_scales("0,0.5,1,2") == [0.0, 0.5, 1.0, 2.0] and C.parse_scales(" 1 ") == [1.0] and C.parse_scales((0, 2)) == [0.0, 2.0]
    for bad in ("-1,0", "0,1,1", "0,1.0,1", "", "0,,1", "a", "inf", "nan", ()):
        with pytest.raises(ValueError):
            C.parse_scales(bad)
    base = ["--data-dir", "D", "--datasetTest", "3", "--checkpoint", "C", "--out", "O"]
    args = parse_args(base)
    assert (args.samples, args.scales, args.bins, args.seed, args.batch_size) == (16, [0.0, 0.5, 1.0, 2.0], 16, 0, 9)
    assert parse_args(base + ["--bins", "32", "--scales", "0,1"]).scales == [0.0, 1.0]
    for bad in (["--bins", "7"], ["--scales", "-1,0"], ["--scales", "0,1,1"], ["--samples", "0"], ["--samples", "65"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    with pytest.raises(ValueError):
        CalibrationRun(None, None, None, None, "O", bins=7)
    with pytest.raises(ValueError):
        CalibrationRun(None, None, None, None, "O", scales=(0, 0))
