"""wtpse_hip/gradability.py on the host: record_host (the specification of wtpse_gradability_record) on a hand-made picture with
every entry worked out, pictures without interior pixels, `measures` on hand-made records and a hand-made cell table, the focus
measures under quality_host's blur and unsharp masking, brightness and contrast, `Gradability.judge`, `ranks`, the table, the parser
and the header's declaration.

Measured here on synth_photo(300, 300, 3, (0.55, 0.8)) at t = 24 (the test asserts the ordering, not the numbers):

    sigma              focus_1    focus_ratio
    0                  355.1      0.1435
    0.5                160.7      0.0747
    1                  30.6       0.0228
    2                  5.26       0.0112
    unsharp (1, 1)     920.0      0.4859
"""
import argparse
import math
import os

import numpy as np
import pytest

from test_locate_cpu import photo

from wtpse_hip import gradability as GR

SIGMAS = (0.0, 0.5, 1.0, 2.0)


# ---- the record -------------------------------------------------------------------------------------------------------------------
def hand_made():
    """9 x 9, every pixel (40, 50, 30) except (0, 1) = (10, 20, 5), outside the field at t = 24, and the centre (4, 4) = (255, 60, 30),
    saturated in R at sat = 250."""
    img = np.empty((9, 9, 3), np.uint8)
    img[:] = (40, 50, 30)
    img[0, 1] = (10, 20, 5)
    img[4, 4] = (255, 60, 30)
    return img


def test_record_host_on_a_hand_made_picture():
    rec = GR.record_host(hand_made(), 24, 250)
    assert rec.shape == (1, GR.GRAD_REC) and rec.dtype == np.int64
    r = GR.split_record(rec[0])
    # luma: (77 * 40 + 150 * 50 + 29 * 30 + 128) >> 8 = 11578 >> 8 = 45; the centre (19635 + 9000 + 870 + 128) >> 8 = 29633 >> 8 = 115
    want = np.zeros(256, np.int64)
    want[45], want[115] = 79, 1
    assert np.array_equal(r["hist"], want)
    assert r["sums"].tolist() == [79 * 40 + 255, 79 * 50 + 60, 80 * 30]
    assert r["sat"].tolist() == [1, 0, 0]
    assert int(r["area"]) == 80 and r["box"].tolist() == [0, 8, 0, 8]
    # d = 1: rows and columns 1..7 are 49 pixels, (1, 1) has (0, 1) above it: 48.  L = 4 * 60 - 4 * 50 = 40 at the centre, 4 * 50 - 60 - 150
    # = -10 at its four neighbours, 0 elsewhere: E = 1600 + 4 * 100.  The gradient sees the centre from those four only: Q = 4 * 10^2.
    # d = 2: rows and columns 2..6, none next to (0, 1): 25 pixels, the same five nonzero terms at distance 2.
    # d = 4: the centre alone has all four neighbours inside the picture: L = 40, no gradient.
    assert r["focus"].tolist() == [[48, 2000, 400], [25, 2000, 400], [1, 1600, 0]]
    # t = 0: (0, 1) joins the field, and with it (1, 1) the interior at d = 1: L = 4 * 50 - 20 - 150 = 30, (dy)^2 = (50 - 20)^2
    r0 = GR.split_record(GR.record_host(hand_made(), 0, 61)[0])
    assert int(r0["area"]) == 81 and r0["focus"][0].tolist() == [49, 2000 + 900, 400 + 900] and r0["sat"].tolist() == [1, 0, 0]
    assert int(r0["hist"][(770 + 3000 + 145 + 128) >> 8]) == 1
    assert GR.split_record(GR.record_host(hand_made(), 24, 60)[0])["sat"].tolist() == [1, 1, 0]
    # a stack is its pictures' records
    both = GR.record_host(np.stack([hand_made(), hand_made()[::-1].copy()]), 24, 250)
    assert np.array_equal(both[0], rec[0]) and both[1, 263:267].tolist() == [0, 8, 0, 8] and both[1, 267:].tolist() == rec[0, 267:].tolist()


def test_pictures_without_interior_pixels():
    rng = np.random.default_rng(0)
    r8 = GR.split_record(GR.record_host(rng.integers(30, 256, (8, 8, 3), dtype=np.uint8), 24, 250)[0])
    assert r8["focus"][2].tolist() == [0, 0, 0] and r8["focus"][1, 0] == 16 and r8["focus"][0, 0] == 36
    r1 = GR.split_record(GR.record_host(np.full((1, 1, 3), 200, np.uint8), 24, 250)[0])
    assert r1["focus"].tolist() == [[0, 0, 0]] * 3 and int(r1["area"]) == 1 and r1["box"].tolist() == [0, 0, 0, 0]
    dark = GR.record_host(np.zeros((5, 7, 3), np.uint8), 24, 250)[0]
    assert dark[263:267].tolist() == [5, -1, 7, -1] and not dark[:263].any() and not dark[267:].any()
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            GR.record_host(bad)
    for t, sat in ((-1, 250), (256, 250), (24, 0), (24, 256)):
        with pytest.raises(ValueError):
            GR.record_host(np.zeros((4, 4, 3), np.uint8), t, sat)


# ---- the measures -----------------------------------------------------------------------------------------------------------------
def _record(hist=(), sums=(0, 0, 0), sat=(0, 0, 0), box=(0, 9, 0, 9), focus=((0, 0, 0),) * 3):
    rec = np.zeros(GR.GRAD_REC, np.int64)
    for level, count in hist:
        rec[level] = count
    rec[256:259], rec[259:262], rec[262], rec[263:267] = sums, sat, rec[:256].sum(), box
    rec[267:] = np.asarray(focus).reshape(-1)
    return rec


def test_measures_on_hand_made_records():
    # 100 pixels: the ranks 1, 5, 50, 95, 99 are reached exactly at the levels 10, 20, 30, 40, 50
    rec = _record(hist=((10, 1), (20, 4), (30, 45), (40, 45), (50, 4), (60, 1)), sums=(1000, 2000, 3050), sat=(5, 0, 100),
                  focus=((64, 6400, 640), (36, 360, 72), (4, 8, 0)))
    m = GR.measures(rec, dark=30, bright=50)
    assert [m["luma_p%02d" % q] for q in GR.PERCENTILES] == [10.0, 20.0, 30.0, 40.0, 50.0] and m["contrast"] == 20.0
    assert m["fov_area"] == 100 and abs(m["fov_fill"] - 4 / math.pi) < 1e-15           # the default box is 10 x 10
    assert m["luma_mean"] == 35.0                                              # (10 + 80 + 1350 + 1800 + 200 + 60) / 100
    assert abs(m["luma_std"] - math.sqrt((625 + 4 * 225 + 45 * 25 + 45 * 25 + 4 * 225 + 625) / 100)) < 1e-12
    p = np.array([1, 4, 45, 45, 4, 1]) / 100.0
    assert abs(m["entropy"] - float(-(p * np.log2(p)).sum())) < 1e-12
    assert (m["mean_r"], m["mean_g"], m["mean_b"], m["sat_r"], m["sat_g"], m["sat_b"]) == (10.0, 20.0, 30.5, 0.05, 0.0, 1.0)
    assert (m["dark_frac"], m["bright_frac"]) == (0.05, 0.05)                  # Y < 30: 1 + 4; Y >= 50: 4 + 1
    assert (m["focus_1"], m["focus_2"], m["focus_4"], m["edge_1"], m["edge_2"], m["edge_4"]) == (100.0, 10.0, 2.0, 10.0, 2.0, 0.0)
    assert m["focus_ratio"] == 50.0 and m["focus_scale"] == 1 and m["focus"] == 100.0
    assert m["evenness_cv"] != m["evenness_cv"] and m["centre_edge"] != m["centre_edge"]
    assert set(m) == set(GR.MEASURES) and all(isinstance(m[k], int) for k in GR.INT_MEASURES)
    # one pixel: every rank is 1
    one = GR.measures(_record(hist=((7, 1),)))
    assert [one["luma_p%02d" % q] for q in GR.PERCENTILES] == [7.0] * 5 and one["entropy"] == 0.0 and one["luma_std"] == 0.0
    # empty denominators: no field at all; a field without interior pixels; a focus_4 of exactly 0
    empty = GR.measures(np.zeros(GR.GRAD_REC, np.int64))
    assert empty["fov_area"] == 0 and empty["focus_scale"] == 1
    assert all(empty[k] != empty[k] for k in GR.FLOAT_MEASURES)
    flat = GR.measures(_record(hist=((9, 4),), focus=((4, 0, 0), (0, 0, 0), (0, 0, 0))))
    assert flat["focus_1"] == 0.0 and flat["focus_2"] != flat["focus_2"] and flat["focus_ratio"] != flat["focus_ratio"]
    zero4 = GR.measures(_record(hist=((9, 4),), focus=((4, 8, 0), (4, 0, 0), (4, 0, 0))))
    assert zero4["focus_4"] == 0.0 and zero4["focus_ratio"] != zero4["focus_ratio"]
    with pytest.raises(ValueError):
        GR.measures(np.zeros((2, GR.GRAD_REC), np.int64))
    with pytest.raises(ValueError):
        GR.split_record(np.zeros(GR.GRAD_REC - 1, np.int64))


def test_focus_scale_at_the_two_switch_over_diameters():
    # 2 sqrt(n / pi) < 1024 sqrt(2)  <=>  n < pi 2^19 = 1647099.3;  < 2048 sqrt(2)  <=>  n < pi 2^21 = 6588397.3
    assert math.floor(math.pi * 2 ** 19) == 1647099 and math.floor(math.pi * 2 ** 21) == 6588397
    focus = ((10, 10, 0), (10, 20, 0), (10, 40, 0))
    for n, scale in ((1647099, 1), (1647100, 2), (6588397, 2), (6588398, 4)):
        m = GR.measures(_record(hist=((100, n),), focus=focus))
        assert (m["focus_scale"], m["focus"]) == (scale, float(scale)), n
    m = GR.measures(_record(hist=((100, 1647099),), focus=focus), ref_diameter=512.0)       # the convention is a parameter
    assert m["focus_scale"] == 2 and GR.focus_scale(100) == 1


def test_illumination_on_a_hand_made_cell_table():
    # a 32 x 32 field of 8 x 8 cells of side 4: D = 2 sqrt(1024 / pi) = 36.1, the box's centre (16, 16), a cell's centre (4 i + 2, 4 j + 2).
    # Within D / 4 = 9.03: the 4 x 4 block i, j in 2..5 (its corners at sqrt(72) = 8.49; (1, 3) is at sqrt(104) = 10.2).  Beyond
    # 3 D / 8 = 13.54: the 28 border cells ((0, 3) is at sqrt(200) = 14.1) and the four (1, 1)-like corners at sqrt(200); (1, 2) at
    # sqrt(136) = 11.7 is in neither.
    cells = np.zeros((8, 8, 2), np.int64)
    cells[..., 0] = 16
    luma = np.full((8, 8), 50)
    luma[2:6, 2:6] = 100
    luma[1, 2] = 75
    cells[..., 1] = luma * 256 * 16
    cv, ce = GR.illumination(cells, 4, 1024, (0, 31, 0, 31))
    assert ce == 2.0
    mean = (16 * 100 + 47 * 50 + 75) / 64.0
    var = (16 * (100 - mean) ** 2 + 47 * (50 - mean) ** 2 + (75 - mean) ** 2) / 64.0
    assert abs(cv - math.sqrt(var) / mean) < 1e-12
    # a cell that is not wholly in the field is left out: the same figures without (1, 2)
    part = cells.copy()
    part[1, 2] = (15, 75 * 256 * 15)
    cv2, ce2 = GR.illumination(part, 4, 1023, (0, 31, 0, 31))
    mean = (16 * 100 + 47 * 50) / 63.0
    assert abs(cv2 - math.sqrt((16 * (100 - mean) ** 2 + 47 * (50 - mean) ** 2) / 63.0) / mean) < 1e-12 and ce2 == 2.0
    # fewer than four cells in a group: centre_edge is nan, the evenness stays; fewer than four full cells: both are
    few = cells.copy()
    few[..., 0] = 15
    few[3:5, 3:5, 0] = 16
    cv3, ce3 = GR.illumination(few, 4, 1000, (0, 31, 0, 31))
    assert cv3 == 0.0 and ce3 != ce3
    few[3, 3, 0] = 15
    assert all(v != v for v in GR.illumination(few, 4, 1000, (0, 31, 0, 31)))
    # measures passes the table through
    rec = _record(hist=((50, 1024),), box=(0, 31, 0, 31))
    m = GR.measures(rec, cells, 4)
    assert (m["evenness_cv"], m["centre_edge"]) == (cv, ce)


# ---- what the measures respond to -------------------------------------------------------------------------------------------------
def _quality(img, a=0, c=256, beta=0, sigma=0.0):
    from wtpse_hip.input_pipeline.quality import quality_host, quality_neutral, quality_taps
    p = quality_neutral(1)
    p[0, :3] = (a, c, beta)
    p[0, 4:] = quality_taps(sigma)
    return quality_host(img[None], p)[0]


@pytest.fixture(scope="module")
def blurred():
    img = photo(300, 300)[0]
    out = {s: GR.measures(GR.record_host(_quality(img, a=-256, sigma=s) if s else img)[0]) for s in SIGMAS}
    out["unsharp"] = GR.measures(GR.record_host(_quality(img, a=256, sigma=1.0))[0])
    return out


def test_focus_measures_fall_with_blur_and_rise_with_unsharp_masking(blurred):
    for s in SIGMAS + ("unsharp",):
        print("sigma %-8s focus_1 %10.3f focus_4 %10.3f focus_ratio %.4f edge_1 %.3f" % (s, blurred[s]["focus_1"], blurred[s]["focus_4"],
                                                                                          blurred[s]["focus_ratio"], blurred[s]["edge_1"]))
    for key in ("focus_1", "focus_ratio"):
        vals = [blurred[s][key] for s in SIGMAS]
        assert all(a > b for a, b in zip(vals, vals[1:])), (key, vals)
        assert blurred["unsharp"][key] > blurred[0.0][key], key
    assert all(blurred[s]["focus_scale"] == 1 and blurred[s]["focus"] == blurred[s]["focus_1"] for s in SIGMAS)


def test_brightness_moves_the_mean_and_contrast_the_spread():
    img = np.minimum(photo(300, 300)[0], 200)                      # nothing clips under a shift of 10 levels
    img[img.max(-1) < 24] = 0                                      # and nothing enters the field
    base = GR.measures(GR.record_host(img)[0])
    up = _quality(img, beta=2560)
    assert np.array_equal(up, img + 10)
    shifted = GR.measures(GR.record_host(up)[0])
    assert abs(shifted["luma_mean"] - base["luma_mean"] - 10.0) < 1e-9 and shifted["fov_area"] == base["fov_area"]
    for k in ("focus_1", "focus_2", "focus_4", "edge_1", "focus_ratio", "contrast", "luma_std"):
        assert shifted[k] == base[k] or abs(shifted[k] - base[k]) < 1e-9 * base[k], k
    assert shifted["focus_1"] == base["focus_1"]
    # the contrast stage moves every byte, the black surround too, towards the mean: scored as a crop is (t = 0)
    whole = GR.measures(GR.record_host(img, 0)[0])
    low = GR.measures(GR.record_host(_quality(img, c=128), 0)[0])
    assert low["contrast"] < whole["contrast"] and low["luma_std"] < whole["luma_std"] and low["fov_area"] == whole["fov_area"] == 90000


# ---- judging ----------------------------------------------------------------------------------------------------------------------
def test_judge_each_flag_alone_and_gradable_in_its_three_states():
    m = dict.fromkeys(GR.MEASURES, 0.0)
    m.update(focus=50.0, focus_ratio=0.1, dark_frac=0.2, bright_frac=0.05, evenness_cv=0.3, fov_fill=0.9)
    none = GR.Gradability().judge(m)
    assert set(none) == set(GR.FLAGS) and all(v == -1 for v in none.values())
    for flag, key, (passes, fails) in (("ok_focus", "min_focus", (50.0, 50.5)), ("ok_focus_ratio", "min_focus_ratio", (0.1, 0.11)),
                                       ("ok_dark", "max_dark", (0.2, 0.19)), ("ok_bright", "max_bright", (0.05, 0.04)),
                                       ("ok_cv", "max_cv", (0.3, 0.29)), ("ok_fov_fill", "min_fov_fill", (0.9, 0.95))):
        for limit, want in ((passes, 1), (fails, 0)):
            got = GR.Gradability(**{key: limit}).judge(m)
            assert got[flag] == want and got["gradable"] == want, (flag, limit)
            assert all(got[f] == -1 for f in GR.FLAGS[:-1] if f != flag)
    both = GR.Gradability(min_focus=10.0, max_dark=0.1).judge(m)
    assert (both["ok_focus"], both["ok_dark"], both["gradable"]) == (1, 0, 0)
    # a nan measure is not judged: alone it leaves gradable at -1, beside a judged flag it does not count
    nan = dict(m, focus_ratio=float("nan"))
    assert GR.Gradability(min_focus_ratio=0.05).judge(nan) == dict(none)
    got = GR.Gradability(min_focus_ratio=0.05, min_focus=10.0).judge(nan)
    assert (got["ok_focus_ratio"], got["ok_focus"], got["gradable"]) == (-1, 1, 1)


def test_gradability_validates_its_ranges():
    g = GR.Gradability(min_focus=1, max_dark=1.0, dark=0, bright=255, sat=1, t=0)
    assert g.config() == dict(min_focus=1.0, min_focus_ratio=None, max_dark=1.0, max_bright=None, max_cv=None, min_fov_fill=None, dark=0,
                              bright=255, sat=1)
    for kw in (dict(min_focus=-1), dict(min_focus_ratio=-0.1), dict(max_dark=1.5), dict(max_bright=-0.1), dict(max_cv=-1), dict(min_fov_fill=-1),
               dict(dark=-1), dict(bright=256), dict(sat=0), dict(t=256), dict(dark=1.5), dict(dark=100, bright=50), dict(min_focus=float("nan"))):
        with pytest.raises(ValueError):
            GR.Gradability(**kw)


def test_ranks():
    nan = float("nan")
    assert GR.ranks([0.3, 0.1]) == [75.0, 25.0]
    got = GR.ranks([2.0, nan, 1.0, 2.0, 5.0])
    assert got[1] != got[1] and [got[i] for i in (0, 2, 3, 4)] == [50.0, 12.5, 50.0, 87.5]
    assert GR.ranks([]) == [] and GR.ranks([7.0]) == [50.0] and all(v != v for v in GR.ranks([nan, nan]))


# ---- the table, the parser, the header ------------------------------------------------------------------------------------------------
def test_gradability_csv_round_trips(tmp_path):
    img = photo(300, 300)[0]
    judge = GR.Gradability(min_focus_ratio=0.05, max_dark=0.5)
    rows = []
    for i, (im, name) in enumerate(((img, "a.png"), (np.zeros_like(img), 'b "x", y.png'), (_quality(img, a=-256, sigma=2.0), "c.png"))):
        rows.append(dict(judge.measures(GR.record_host(im)[0]), index=i + 1, name=name))
    rows = GR.finish_rows(rows, judge)
    assert [r["gradable"] for r in rows] == [1, -1, 0] and rows[1]["focus_rank"] != rows[1]["focus_rank"]
    assert (rows[0]["focus_rank"], rows[2]["focus_rank"]) == (75.0, 25.0)
    GR.write_csv(str(tmp_path), rows)
    with open(tmp_path / "gradability.csv") as f:
        assert tuple(f.readline().strip().split(",")) == GR.columns() == ("index", "name") + GR.MEASURES + GR.FLAGS + ("focus_rank",)
    back = GR.read_csv(str(tmp_path))
    assert len(back) == 3
    for a, b in zip(rows, back):
        assert set(b) == set(GR.columns())
        for k in GR.columns():
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k
            assert type(b[k]) is (str if k == "name" else int if k in ("index",) + GR.INT_MEASURES + GR.FLAGS else float), k
    assert GR.summarise(rows, judge) == dict(judge.config(), n_judged=2, n_gradable=1)
    # locate's form: both prefixes, the flags on the first
    two = [dict({"photo_" + k: r[k] for k in GR.MEASURES}, **{"roi_" + k: rows[0][k] for k in GR.MEASURES}, index=r["index"], name=r["name"])
           for r in rows]
    two = GR.finish_rows(two, judge, ("photo_", "roi_"))
    assert [r["gradable"] for r in two] == [1, -1, 0]
    out = tmp_path / "two"
    GR.write_csv(str(out), two, ("photo_", "roi_"))
    back = GR.read_csv(str(out))
    assert tuple(back[0]) == GR.columns(("photo_", "roi_")) and back[2]["roi_focus_1"] == rows[0]["focus_1"] and back[2]["photo_fov_area"] == rows[2]["fov_area"]


def _parse(extra):
    from wtpse_hip import segment
    ap = argparse.ArgumentParser()
    segment.add_arguments(ap)
    return ap, segment.segmenter_arguments(ap, ap.parse_args(["--images", "d", "--checkpoint", "c", "--out", "o"] + extra))


def test_the_switch_adds_one_keyword_and_off_changes_nothing():
    from wtpse_hip import locate
    _, off = _parse(["--min-focus", "3", "--grad-dark", "40"])     # thresholds without the switch: still off
    assert off == dict(batch_size=9, overlay=True, samples=0, seed=0, scale=1.0, morphometry=False, sectors=24, eye=None, views=None)
    _, on = _parse(["--gradability", "--min-focus-ratio", "0.05", "--max-dark", "0.4", "--grad-dark", "40", "--grad-bright", "230"])
    grad = on.pop("gradability")
    assert on == off and isinstance(grad, GR.Gradability)
    assert grad.config() == dict(min_focus=None, min_focus_ratio=0.05, max_dark=0.4, max_bright=None, max_cv=None, min_fov_fill=None, dark=40,
                                 bright=230, sat=250)
    with pytest.raises(SystemExit):
        _parse(["--gradability", "--max-dark", "2"])
    have = {s for a in locate.parser()._actions for s in a.option_strings}
    assert {"--gradability", "--min-focus", "--min-focus-ratio", "--max-dark", "--max-bright", "--max-cv", "--min-fov-fill", "--grad-dark",
            "--grad-bright"} <= have


def test_segmenter_takes_a_gradability_or_none():
    from wtpse_hip.segment import Segmenter
    assert Segmenter(None, None, None, None, out_dir=None).gradability is None
    g = GR.Gradability()
    assert Segmenter(None, None, None, None, out_dir=None, gradability=g).gradability is g
    with pytest.raises(ValueError):
        Segmenter(None, None, None, None, out_dir=None, gradability=True)


def test_header_declares_the_entry():
    from wtpse_hip import build, ops
    text = open(build.HEADER).read()
    assert text.count("int wtpse_gradability_record(const unsigned char* img, long long* rec, int N, int H, int W, int t, int sat, void* stream);") == 1
    assert "#define WTPSE_GRAD_REC 276" in text and GR.GRAD_REC == ops.GRAD_REC == 276
    assert build.parse_prototypes()["wtpse_gradability_record"] == ["const unsigned char*", "long long*", "int", "int", "int", "int", "int", "void*"]
    assert os.path.isfile(os.path.join(build.CSRC, "gradability.hip"))
