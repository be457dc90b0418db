"""wtpse_hip/locate.py without a GPU: the host specifications (cells_host, crop_host, paste_host) on hand-made inputs, the candidate
rule on hand-made cell tables, the rule on synthetic photographs (whose generator lives here), choose, the recentring arithmetic,
roi.csv and the command line's parser."""
import math

import numpy as np
import pytest

from wtpse_hip import locate as L


# ---- the synthetic photograph -------------------------------------------------------------------------------------------------
def synth_photo(H, W, seed, disc=(0.5, 0.72), exudates=True, glare=True):
    """A fundus photograph as a camera writes it -> ([H,W,3] uint8, (disc_cy, disc_cx, disc_radius)): a circular field with vignetting
    (cut straight at the top and bottom as wide-format cameras do) on black with a few grey levels of noise outside it; a disc of radius
    0.065 D at the relative position `disc` of the field; a cluster of 25 small bright exudates; a glare crescent at the left rim; six
    dark vessels leaving the disc; sensor noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = H / 2.0, W / 2.0
    R = min(0.47 * min(H, W) * (1.15 if W > H else 1.0), 0.49 * W)
    r = np.hypot(yy - cy, xx - cx)
    fov = (r < R) & (yy > 0.04 * H) & (yy < 0.96 * H)
    vig = 1.0 - 0.45 * (r / R) ** 2
    img = np.stack([170.0 * vig, 80.0 * vig, 35.0 * vig], -1)
    dy, dx, rd = cy + (disc[0] - 0.5) * 2 * R, cx + (disc[1] - 0.5) * 2 * R, 0.065 * 2 * R
    m = np.clip((rd - np.hypot((yy - dy) / 1.08, xx - dx)) / (0.15 * rd), 0, 1)
    img += m[..., None] * np.array([70.0, 110.0, 70.0])
    if exudates:
        sg = 0.012 * R
        for _ in range(25):
            ey, ex = cy + rng.normal(0.25 * R, 0.05 * R), cx + rng.normal(-0.3 * R, 0.05 * R)
            ya, yb, xa, xb = (int(max(0, v)) for v in (ey - 5 * sg, ey + 5 * sg + 2, ex - 5 * sg, ex + 5 * sg + 2))
            e = np.exp(-((yy[ya:yb, xa:xb] - ey) ** 2 + (xx[ya:yb, xa:xb] - ex) ** 2) / (2 * sg ** 2))
            img[ya:yb, xa:xb] += e[..., None] * np.array([60.0, 120.0, 40.0])
    if glare:
        g = np.clip((r - 0.9 * R) / (0.1 * R), 0, 1) * (xx < cx - 0.5 * R)
        img += g[..., None] * np.array([60.0, 90.0, 60.0])
    for a in np.linspace(0, 2 * math.pi, 7)[:-1]:
        t = np.linspace(0, 1, 400)
        for y_, x_ in zip(dy + t * R * 1.2 * np.sin(a + t), dx + t * R * 1.2 * np.cos(a + t)):
            y0, x0 = int(y_), int(x_)
            if 1 <= y0 < H - 1 and 1 <= x0 < W - 1:
                img[y0 - 1:y0 + 2, x0 - 1:x0 + 2] *= 0.8
    img += rng.normal(0, 3, img.shape)
    img = np.where(fov[..., None], img, rng.integers(0, 6, (H, W, 1)).astype(np.float64))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), (dy, dx, rd)


_PHOTOS = {}


def photo(H, W):
    """The one photograph per size the tests share (left unchanged)."""
    if (H, W) not in _PHOTOS:
        seed, disc = {(600, 800): (1, (0.5, 0.72)), (1424, 2144): (2, (0.45, 0.2)), (300, 300): (3, (0.55, 0.8))}.get((H, W), (H + W, (0.5, 0.7)))
        _PHOTOS[(H, W)] = synth_photo(H, W, seed, disc)
    return _PHOTOS[(H, W)]


def host_plan(img, count=3, t=24):
    """The host composition: the field's area -> the auto cell -> cells_host -> plan."""
    area = int((img.max(-1) >= t).sum())
    c = L.auto_cell(0.13 * L.fov_diameter(area))
    return L.plan(L.cells_host(img, c, t), c, count)


# ---- cells_host -----------------------------------------------------------------------------------------------------------------
def hand_image():
    """5 x 7: pixel (y, x) = (30 + y, 40 + x, 25), luma 9035 + 77 y + 150 x, except (2, 3) = (23, 23, 23), below the threshold 24."""
    img = np.zeros((5, 7, 3), np.uint8)
    for y in range(5):
        for x in range(7):
            img[y, x] = (30 + y, 40 + x, 25)
    img[2, 3] = 23
    return img


HAND_N = [[4, 4, 4, 2], [4, 3, 4, 2], [2, 2, 2, 1]]
HAND_S = [[36594, 37794, 38994, 19947], [37210, 28771, 39610, 20255], [18836, 19436, 20036, 10243]]


def test_cells_host_on_a_hand_made_image():
    got = L.cells_host(hand_image(), 2, 24)
    assert got.dtype == np.int64 and got.shape == (3, 4, 2)
    assert got[..., 0].tolist() == HAND_N and got[..., 1].tolist() == HAND_S
    # a full cell in closed form: 4 * 9035 + 77 * 2 (4 i + 1) + 150 * 2 (4 j + 1)
    assert HAND_S[0][2] == 4 * 9035 + 154 * 1 + 300 * 9 and HAND_S[1][0] == 4 * 9035 + 154 * 5 + 300 * 1
    # the cell with the dark pixel: its three others; the corner cell: the one pixel (4, 6)
    assert HAND_S[1][1] == (9035 + 154 + 300) + (9035 + 231 + 300) + (9035 + 231 + 450) and HAND_S[2][3] == 9035 + 308 + 900
    # threshold 0 counts every pixel; a batch is the stack of its pictures
    assert L.cells_host(hand_image(), 2, 0)[..., 0].tolist() == [[4, 4, 4, 2], [4, 4, 4, 2], [2, 2, 2, 1]]
    assert np.array_equal(L.cells_host(np.stack([hand_image()] * 2), 2, 24)[1], got)
    white = L.cells_host(np.full((256, 256, 3), 255, np.uint8), 256, 24)
    assert white.tolist() == [[[65536, 2 ** 32 - 2 ** 24]]] and white[0, 0, 1] > 2 ** 31


# ---- candidates -----------------------------------------------------------------------------------------------------------------
def table(n, s):
    return np.stack([np.asarray(n, np.int64), np.asarray(s, np.int64)], -1)


def test_candidates_break_ties_by_row_then_column():
    n, s = np.full((7, 9), 4), np.full((7, 9), 100)
    for i, j in ((4, 3), (1, 5), (1, 1)):                    # rings disjoint, all inside the table: three equal scores
        s[i, j] = 400
    got = L.candidates(table(n, s), 2, 1, 3)
    assert [(i, j) for i, j, _ in got] == [(1, 1), (1, 5), (4, 3)]
    assert got[0][2] == got[1][2] == got[2][2] == (400 / 4 - 800 / 32) / 256.0
    assert [(i, j) for i, j, _ in L.candidates(table(n, s), 2, 1, 2)] == [(1, 1), (1, 5)]


def test_candidates_suppress_below_k_in_both_axes_only():
    n, s = np.full((12, 12), 4), np.full((12, 12), 40)
    s[3:5, 3:5], s[3:5, 5:7] = 1000, 900
    score, valid = L.window_scores(table(n, s), 2, 2)
    assert valid.all() and score[3, 3] > score[3, 4] > score[3, 5] > 0
    got = L.candidates(table(n, s), 2, 2, 2)
    assert [(i, j) for i, j, _ in got] == [(3, 3), (3, 5)]     # (3, 4) is one cell away in both axes; (3, 5) exactly k columns away
    assert got[1][2] == score[3, 5]
    assert L.centre(3, 3, 2, 2) == (8.0, 8.0) and L.centre(3, 5, 3, 2) == (9.0, 13.0)


def test_candidates_never_pick_an_invalid_window():
    # field fraction: the brightest cell holds one pixel of four (4 * 1 < 3 * 4)
    n, s = np.full((5, 5), 4), np.full((5, 5), 100)
    n[2, 2], s[2, 2] = 1, 250
    score, valid = L.window_scores(table(n, s), 2, 1)
    assert not valid[2, 2] and valid.sum() == 24
    assert all((i, j) != (2, 2) for i, j, _ in L.candidates(table(n, s), 2, 1, 25))
    n[2, 2], s[2, 2] = 3, 750                                  # 4 * 3 >= 12: now it is valid, and the best
    assert L.candidates(table(n, s), 2, 1, 1)[0][:2] == (2, 2)
    # ring: a bright cell whose surround holds fewer field pixels than itself
    n, s = np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64)
    n[1, 1], s[1, 1], n[0, 0], s[0, 0] = 4, 1000, 3, 30
    assert L.candidates(table(n, s), 2, 1, 3) == []
    n[0, 1], s[0, 1] = 1, 10                                   # n_ring = n_in
    assert [(i, j) for i, j, _ in L.candidates(table(n, s), 2, 1, 3)] == [(1, 1)]
    assert L.candidates(table([[4]], [[1000]]), 2, 1, 3) == [] and L.candidates(table([[4]], [[1000]]), 2, 2, 3) == []


def test_candidates_stop_at_a_non_positive_score():
    n, s = np.full((6, 6), 4), np.full((6, 6), 100)
    assert L.candidates(table(n, s), 2, 1, 3) == []           # every score is 0
    s[2, 2] = 500
    got = L.candidates(table(n, s), 2, 1, 3)                   # the neighbours' rings hold the bright cell: negative; the rest 0
    assert [(i, j) for i, j, _ in got] == [(2, 2)]
    assert L.candidates(table(np.zeros((6, 6)), np.zeros((6, 6))), 2, 1, 3) == []
    assert L.plan(table(np.zeros((6, 6)), np.zeros((6, 6))), 2)["candidates"] == []


def test_auto_cell_and_window():
    for D, c, k in ((96, 2, 6), (626, 8, 10), (1487, 16, 12)):
        assert L.auto_cell(0.13 * D) == c and L.window_cells(0.13 * D, c) == k
    assert L.auto_cell(0.0) == 2 and L.auto_cell(1e9) == 256 and L.window_cells(0.4, 2) == 1
    assert L.roi_side(2000.0) == 800 and L.roi_side(2001.3) == 800 and L.roi_side(2003.0) == 802 and L.roi_side(1.0) == 2
    assert L.box_at(8.0, 13.5, 6) == (5, 10) and L.box_at(2.0, 2.0, 8) == (-2, -2)


# ---- the rule on synthetic photographs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(600, 800), (1424, 2144)], ids=lambda s: "%dx%d" % s)
def test_disc_is_the_first_candidate(size):
    img, (dy, dx, rd) = photo(*size)
    p = host_plan(img)
    assert p["candidates"]
    cy, cx = L.centre(*p["candidates"][0][:2], p["window"], p["cell"])
    assert math.hypot(cy - dy, cx - dx) <= rd, (p, (dy, dx, rd))
    assert abs(p["side"] - 0.4 * p["fov_diameter"]) <= 1.0 and p["side"] % 2 == 0


def test_disc_is_among_the_first_three_at_300():
    img, (dy, dx, rd) = photo(300, 300)
    p = host_plan(img)
    dist = [math.hypot(cy - dy, cx - dx) for cy, cx in (L.centre(i, j, p["window"], p["cell"]) for i, j, _ in p["candidates"])]
    assert len(dist) >= 1 and min(dist) <= rd, (p, dist, rd)


# ---- choose -------------------------------------------------------------------------------------------------------------------------
def rec(area, top=50, bottom=150, left=60, right=160):
    return [area, top, bottom, left, right, 100 * area, 110 * area, 0]


def test_choose():
    S, cands = 256, [(0, 0, 3.0), (5, 5, 2.0), (9, 9, 1.0)]
    lo, hi = int(0.01 * S * S) + 1, int(0.5 * S * S)             # 656 (655.36 rounded up) and 32768: both bounds inclusive
    assert L.choose(cands, [rec(5000), rec(5000), rec(5000)], S) == (0, 1)                      # rank order
    assert L.choose(cands, [rec(lo - 1), rec(5000), rec(5000)], S) == (1, 1)
    assert L.choose(cands, [rec(lo - 1), rec(hi + 1), rec(lo)], S) == (2, 1)
    assert L.choose(cands, [rec(hi), rec(5000), rec(5000)], S) == (0, 1)
    assert L.choose(cands[:1], [rec(655)], S, min_area=655 / 65536.0) == (0, 1)                  # exactly the lower bound
    for touch in (dict(top=0), dict(bottom=255), dict(left=0), dict(right=255)):
        assert L.choose(cands, [rec(5000, **touch), rec(5000), rec(5000)], S) == (1, 1), touch
        assert L.choose(cands[:1], [rec(5000, **touch)], S) == (0, 0), touch
    assert L.choose(cands, [rec(5000, top=1, bottom=254, left=1, right=254)] * 3, S) == (0, 1)
    empty = [0, 256, -1, 256, -1, 0, 0, 0]
    assert L.choose(cands, [empty, rec(10), rec(hi + 1)], S) == (0, 0)                             # fallback: candidate 1, flagged
    assert L.choose(cands[:1], [empty], S, min_area=0.0) == (0, 0)


# ---- recentring --------------------------------------------------------------------------------------------------------------------
def test_recentre_arithmetic():
    assert L.recentre(100, 200, 800, [2, 0, 0, 0, 0, 255, 255, 0], 256) == (100, 200)            # centroid (127.5, 127.5): stays
    # cy = 100, cx = 150.25: y = 100 + 100.5 * 3.125 - 0.5 = 413.5625, x = 200 + 150.75 * 3.125 - 0.5 = 670.59375
    assert L.recentre(100, 200, 800, [4, 0, 0, 0, 0, 400, 601, 0], 256) == (14, 271)
    # a box already partly outside, pushed further: y = 10 + 20.5 * 2 - 0.5 = 50.5, x = -50 + 30.5 * 2 - 0.5 = 10.5
    assert L.recentre(10, -50, 512, [1, 0, 0, 0, 0, 20, 30, 0], 256) == (-205, -245)


# ---- crop and paste ----------------------------------------------------------------------------------------------------------------
PLACEMENTS = [(10, 20), (-3, 20), (95, 20), (10, -5), (10, 128), (-4, -6), (94, 127), (-300, 5), (5, 131), (97, 0), (0, 0)]


def test_crop_host_against_slicing():
    rng = np.random.default_rng(0)
    for C in (1, 3):
        img = rng.integers(1, 256, (97, 131, C)).astype(np.uint8)
        assert np.array_equal(L.crop_host(img, [(10, 20)], 7)[0], img[10:17, 20:27])
        got = L.crop_host(img, [(-3, 128)], 7)[0]
        assert np.array_equal(got[3:, :3], img[0:4, 128:131]) and not got[:3].any() and not got[:, 3:].any()
        got = L.crop_host(img, PLACEMENTS, 7)
        assert got.shape == (len(PLACEMENTS), 7, 7, C) and not got[7].any() and not got[8].any() and not got[9].any()
        big = L.crop_host(img, [(-80, -63)], 257)[0]
        assert np.array_equal(big[80:177, 63:194], img) and int((big != 0).sum()) == img.size


def test_paste_host_against_slicing():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (97, 131, 3)).astype(np.uint8)
    patch = rng.integers(0, 256, (7, 9, 3)).astype(np.uint8)
    want = img.copy()
    want[10:17, 20:29] = patch
    assert np.array_equal(L.paste_host(img.copy(), patch, 10, 20), want)
    want = img.copy()
    want[0:3, 126:131] = patch[4:, :5]
    assert np.array_equal(L.paste_host(img.copy(), patch, -4, 126), want)
    for top, left in ((-7, 0), (97, 0), (0, -9), (0, 131)):
        assert np.array_equal(L.paste_host(img.copy(), patch, top, left), img)
    for top, left in PLACEMENTS:                                 # a crop pasted back at its own box restores the picture
        assert np.array_equal(L.paste_host(img.copy(), L.crop_host(img, [(top, left)], 64)[0], top, left), img)


# ---- roi.csv and the command line ---------------------------------------------------------------------------------------------------
def test_roi_csv_round_trip(tmp_path):
    rows = [dict(L._blank_row(1424, 2144), index=1, name="a, \"b\".png"),
            dict(L._blank_row(600, 800), index=2, name="c.png", fov_area=307200, fov_diameter=L.fov_diameter(307200), cell=8, window=10,
                 located=1, verified=1, candidate=2, score=0.1 + 0.2, roi_top=-12, roi_left=431, roi_side=250, refine_rounds=1,
                 disc_cy=113.25, disc_cx=556.125, cup_cy=1 / 3.0, cup_cx=float("nan"))]
    L.write_roi_csv(str(tmp_path), rows)
    assert open(tmp_path / "roi.csv").readline().strip().split(",") == list(L.ROI_COLUMNS)
    got = L.read_roi_csv(str(tmp_path))
    assert len(got) == 2 and set(got[0]) == set(L.ROI_COLUMNS)
    for g, r in zip(got, rows):
        for k in L.ROI_COLUMNS:
            assert g[k] == r[k] or (isinstance(r[k], float) and math.isnan(r[k]) and math.isnan(g[k])), (k, g[k], r[k])
    assert got[0]["located"] == 0 and got[0]["verified"] == -1 and got[1]["score"] == 0.1 + 0.2


def test_parser_accepts_every_segment_switch():
    import argparse
    from wtpse_hip import segment, views
    ref = argparse.ArgumentParser()
    segment.add_arguments(ref)
    ap = L.parser()
    have = {s for a in ap._actions for s in a.option_strings}
    want = {s for a in ref._actions for s in a.option_strings}
    assert want <= have and {"--candidates", "--refine", "--disc-scale", "--roi-scale", "--roi-side", "--cell", "--fov-threshold",
                             "--min-area", "--max-area", "--no-full"} <= have
    args = ap.parse_args(["--images", "d", "--checkpoint", "c", "--out", "o", "--batch-size", "4", "--no-overlay", "--samples", "3", "--seed", "7",
                          "--sample-scale", "0.5", "--morphometry", "--sectors", "32", "--eye", "left", "--views", "flips", "--candidates", "2",
                          "--refine", "0", "--roi-side", "640", "--cell", "16", "--no-full"])
    kw = segment.segmenter_arguments(ap, args)
    assert list(kw.pop("views")) == list(views.parse("flips"))
    assert kw == dict(batch_size=4, overlay=False, samples=3, seed=7, scale=0.5, morphometry=True, sectors=32, eye="left")
    assert (args.candidates, args.refine, args.roi_side, args.cell, args.no_full, args.roi_scale) == (2, 0, 640, "16", True, 0.4)
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "d", "--checkpoint", "c", "--out", "o", "--roi-side", "640", "--roi-scale", "0.3"])
    # segment's own program takes what it took before
    seg = argparse.ArgumentParser()
    segment.add_arguments(seg)
    assert seg.parse_args(["--images", "d", "--checkpoint", "c", "--out", "o"]).batch_size == 9
