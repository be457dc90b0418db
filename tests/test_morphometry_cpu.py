"""wtpse_hip/morphometry.py without a GPU: the sector table, the host specification of the profile pass, the accuracy of the ellipse
fit and of the rim width on rasterised analytic shapes, the conventions (empty masks, eye, ISNT), the tables, the constructors'
argument checks and the C entry point's validation."""
import math
import os

import numpy as np
import pytest

from wtpse_hip import morphometry as M
from wtpse_hip.segment import mask_geometry_host

NAN = float("nan")


def raster_ellipse(h, w, cy, cx, a, b, theta=0.0):
    """A filled ellipse: the pixel centres within semi-axes (a, b), the major axis `theta` radians counter-clockwise on the screen from
    image-right, centre (cy, cx) in pixel coordinates (rows grow downwards) -> uint8 [h, w]."""
    y, x = np.mgrid[:h, :w].astype(np.float64)
    dx, dy = x - cx, cy - y
    u, v = dx * math.cos(theta) + dy * math.sin(theta), -dx * math.sin(theta) + dy * math.cos(theta)
    return ((u / a) ** 2 + (v / b) ** 2 <= 1.0).astype(np.uint8)


def finish_masks(disc, cup, N=24, eye=None):
    prof, mom = M.profile_host(disc, cup, N)
    return M.finish(mask_geometry_host(disc), mask_geometry_host(cup), mom[0], prof[0], disc.shape[0], disc.shape[1], eye)


def same(a, b):
    return (a != a and b != b) or a == b


# ---- sector_table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 24, 360])
def test_sector_table(N):
    T = M.sector_table(N)
    assert T.dtype == np.int32 and T.shape == (N + 1, 2)
    one = 1 << 20
    assert T[0].tolist() == T[N].tolist() == [one, 0]
    assert T[N // 4].tolist() == [0, one] and T[N // 2].tolist() == [-one, 0] and T[3 * N // 4].tolist() == [0, -one]
    t = T.astype(np.int64)
    cross = t[:-1, 0] * t[1:, 1] - t[:-1, 1] * t[1:, 0]
    assert (cross > 0).all()


@pytest.mark.parametrize("N", [0, 4, 12, 20, 368, 7.5, -8, True])
def test_sector_table_rejects(N):
    with pytest.raises(ValueError):
        M.sector_table(N)


# ---- profile_host ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 24, 360])
def test_profile_host_partitions_a_full_mask(N):
    ones = np.ones((64, 64), np.uint8)
    prof, mom = M.profile_host(ones, ones, N)
    assert prof.dtype == np.uint32 and prof.shape == (1, N, 4) and mom.dtype == np.int64 and mom.shape == (1, 2, 4)
    assert int(prof[0, :, 2].sum()) == 64 * 64 == int(prof[0, :, 3].sum())         # sectors_of raised unless every pixel had one sector
    assert mom[0, 0, 3] == 63 and mom[0, 1, 3] == 63                               # 2 * 31.5
    s2 = sum(i * i for i in range(64)) * 64
    assert mom[0, 0, :3].tolist() == [s2, s2, (63 * 32) ** 2] == mom[0, 1, :3].tolist()
    # every pixel vector has exactly one sector, whatever its direction, and the origin has sector 0
    T = M.sector_table(N)
    py, px = [v.reshape(-1) for v in np.mgrid[-40:41, -40:41]]
    s = M.sectors_of(px, py, T)
    assert s.min() == 0 and s.max() <= N - 1 and s[(px == 0) & (py == 0)].tolist() == [0]
    assert N > 24 or len(set(s.tolist())) == N                                     # (a 1 degree sector next to an axis needs |p| > 57)
    ang = np.degrees(np.arctan2(py, px)) % 360.0
    far = (px != 0) | (py != 0)
    lo, hi = 360.0 * s / N, 360.0 * (s + 1) / N
    assert ((ang >= lo - 1e-3) & (ang < hi + 1e-3))[far].all()                      # the sector that holds the direction
    assert s[(px == 5) & (py == 0)].tolist() == [0] and s[(px == 0) & (py == 5)].tolist() == [N // 4]
    assert s[(px == -5) & (py == 0)].tolist() == [N // 2] and s[(px == 0) & (py == -5)].tolist() == [3 * N // 4]


def test_profile_host_orientation_and_mirror():
    N, h, w = 24, 65, 65
    # a disc with a bump to the upper right and a cup towards image-right; the centroid's x is no half-integer multiple of 1/4, so its
    # rounding to the half-pixel grid commutes with the mirror
    disc = raster_ellipse(h, w, 32, 31, 20, 20) | raster_ellipse(h, w, 32 - 15, 31 + 15, 4, 4)
    cup = raster_ellipse(h, w, 30, 40, 6, 4)
    prof, mom = M.profile_host(disc, cup, N)
    c2y, c2x = int(mom[0, 0, 3]), int(mom[0, 1, 3])
    g = mask_geometry_host(disc)
    assert (c2y, c2x) == M.centre2(g) and abs(c2y / 2 - g[5] / g[0]) <= 0.25 and abs(c2x / 2 - g[6] / g[0]) <= 0.25
    # the cup lies to the right and slightly up: its pixels are in the sectors around 0 degrees, none on the left half
    assert prof[0, N // 4 + 2:3 * N // 4 - 1, 3].sum() == 0 and prof[0, 0, 3] > 0
    # up on the screen is sector N / 4, which starts at 90 degrees: it holds the topmost disc pixel of the centre's column
    top = int(np.nonzero(disc[:, c2x // 2])[0].min())                              # px = 0 or -1: at or just past 90 degrees
    assert prof[0, N // 4, 0] >= (c2y - 2 * top) ** 2 > 0
    # the bump at 45 degrees makes sectors 2 and 3 the farthest
    assert int(prof[0, :, 0].argmax()) in (2, 3)
    mp, mm = M.profile_host(disc[:, ::-1], cup[:, ::-1], N)
    assert int(mm[0, 0, 3]) == c2y and int(mm[0, 1, 3]) == 2 * (w - 1) - c2x          # the mirror keeps the centre on the grid
    assert mm[0, :, 0].tolist() == mom[0, :, 0].tolist()
    # every pixel lands in the sector that holds its mirrored direction (-px, py)
    T = M.sector_table(N)
    want = np.zeros((N, 4), np.uint32)
    for j, m in enumerate((disc, cup)):
        y, x = [v.astype(np.int64) for v in np.nonzero(m)]
        px, py = 2 * x - c2x, c2y - 2 * y
        s = M.sectors_of(-px, py, T)
        np.maximum.at(want[:, j], s, (px * px + py * py).astype(np.uint32))
        want[:, 2 + j] = np.bincount(s, minlength=N)
        # which is sector N/2 - 1 - s of the original for every pixel that is not exactly on a sector border
        t = T.astype(np.int64)
        inner = np.all(t[:N, 0, None] * py[None] - t[:N, 1, None] * px[None] != 0, axis=0)
        assert inner.sum() > 0.9 * len(px) and (s[inner] == (N // 2 - 1 - M.sectors_of(px, py, T)[inner]) % N).all()
    assert np.array_equal(mp[0], want)


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------
# (size, semi-axes a, b, angle in rad); centres 0.3 px below and 0.2 px left of the image centre.  Measured with this code:
#   256 (60, 52) 0.3: semi-axes -0.0237 / -0.0256 px, angle -0.00105 rad, vertical semi-extent -0.0304 px
#   256 (25, 22) 1.0:           +0.0067 / +0.0343 px,       -0.01467 rad,                      -0.0249 px
#    64 (14, 12) 0.5:           +0.0154 / +0.0621 px,       +0.01020 rad,                      +0.0675 px
#   800 (200, 180) 0.2:         -0.0106 / +0.0044 px,       -0.00029 rad,                      +0.0014 px
# (horizontal semi-extent: -0.0193, +0.0663, +0.0087, -0.0080 px: held to the vertical one's bound)
# The bounds are 3 x the worst of the four (0.0621 px, 0.01467 rad, 0.0675 px): the margin covers another rasterisation rule at the
# boundary and nothing else.
ELLIPSES = [(256, 60, 52, 0.3), (256, 25, 22, 1.0), (64, 14, 12, 0.5), (800, 200, 180, 0.2)]
AXIS_BOUND, ANGLE_BOUND, EXTENT_BOUND = 3 * 0.0621, 3 * 0.01467, 3 * 0.0675


@pytest.mark.parametrize("case", ELLIPSES, ids=str)
def test_ellipse_accuracy(case):
    S, a, b, th = case
    disc = raster_ellipse(S, S, (S - 1) / 2 + 0.3, (S - 1) / 2 - 0.2, a, b, th)
    row = finish_masks(disc, np.zeros_like(disc))
    v = math.sqrt(a * a * math.sin(th) ** 2 + b * b * math.cos(th) ** 2)
    hx = math.sqrt(a * a * math.cos(th) ** 2 + b * b * math.sin(th) ** 2)
    err = (row["disc_major"] / 2 - a, row["disc_minor"] / 2 - b, math.radians(row["disc_angle"]) - th, row["disc_v_extent"] / 2 - v,
           row["disc_h_extent"] / 2 - hx)
    print("ellipse %s: semi-axes %+.4f / %+.4f px, angle %+.5f rad, vertical %+.4f px, horizontal %+.4f px" % ((case,) + err))
    assert abs(err[0]) <= AXIS_BOUND and abs(err[1]) <= AXIS_BOUND
    assert abs(err[2]) <= ANGLE_BOUND
    assert abs(err[3]) <= EXTENT_BOUND and abs(err[4]) <= EXTENT_BOUND
    assert abs(row["centre_y"] - ((S - 1) / 2 + 0.3)) <= 0.5 and abs(row["centre_x"] - ((S - 1) / 2 - 0.2)) <= 0.5


def test_ellipse_of_a_rectangle_and_angle_convention():
    # a 1 x 1 pixel: the unit square's moments, 4 sqrt(1 / 12)
    e = M.ellipse(1, 3, 4, 9, 16, 12)
    assert abs(e["major"] - 4 * math.sqrt(1 / 12)) < 1e-12 and abs(e["minor"] - e["major"]) < 1e-12
    # a thin bar from the lower left to the upper right of the screen: 45 degrees; its mirror image: 135
    bar = np.eye(40, dtype=np.uint8)[::-1]
    y, x = [v.astype(np.int64) for v in np.nonzero(bar)]
    args = lambda y, x: (len(y), int(y.sum()), int(x.sum()), int((y * y).sum()), int((x * x).sum()), int((x * y).sum()))
    assert abs(M.ellipse(*args(y, x))["angle"] - 45.0) < 1e-9
    assert abs(M.ellipse(*args(y, 39 - x))["angle"] - 135.0) < 1e-9
    flat = M.ellipse(*args(np.zeros(40, np.int64), np.arange(40)))
    tall = M.ellipse(*args(np.arange(40), np.zeros(40, np.int64)))
    assert flat["angle"] == 0.0 and abs(tall["angle"] - 90.0) < 1e-9 and 0.0 <= flat["angle"] < 180.0
    assert flat["h_extent"] == flat["major"] and tall["v_extent"] == tall["major"]
    assert all(v != v for v in M.ellipse(0, 0, 0, 0, 0, 0).values())


@pytest.mark.parametrize("case", [(256, 60, 25, 24), (256, 25.5, 9, 8), (128, 40, 22.3, 64)], ids=str)
def test_rim_of_concentric_circles(case):
    """Radii are maxima over pixel centres: each within one pixel of the true edge and inside it, so every defined rim[s] lies within
    one pixel of R - r."""
    S, R, r, N = case
    c = (S - 1) / 2
    row = finish_masks(raster_ellipse(S, S, c, c, R, R), raster_ellipse(S, S, c, c, r, r), N)
    rim = np.array(row["rim"])
    assert len(rim) == N and not np.isnan(rim).any()
    print("rim %s: %.3f .. %.3f against %.3f" % (case, rim.min(), rim.max(), R - r))
    assert np.abs(rim - (R - r)).max() <= 1.0
    assert abs(row["rim_min"] - rim.min()) == 0.0 and row["rim_min_angle"] == 360.0 * (int(rim.argmin()) + 0.5) / N
    assert abs(row["vcdr_ellipse"] - r / R) < 0.01 and abs(row["hcdr_ellipse"] - r / R) < 0.01
    unit = math.sqrt(row["disc_area"] / math.pi)
    assert row["rim_rel"] == [v / unit for v in row["rim"]] and row["rim_min_rel"] == row["rim_min"] / unit


# ---- conventions ------------------------------------------------------------------------------------------------------------------
def test_empty_disc_is_all_nan():
    cup = raster_ellipse(64, 64, 30, 30, 8, 8)
    row = finish_masks(np.zeros_like(cup), cup, eye="right")
    assert row["disc_area"] == 0 and row["cup_area"] > 0
    for k in M.FLOAT_COLUMNS:
        if not k.startswith("cup_"):
            assert row[k] != row[k], k
    assert row["cup_major"] > 0 and all(v != v for v in row["rim"]) and all(v != v for v in row["rim_rel"])
    prof, mom = M.profile_host(np.zeros_like(cup), cup, 24)
    assert not prof.any() and mom[0, 0].tolist() == [0, 0, 0, 0] and mom[0, 1, 3] == 0 and mom[0, 1, 0] > 0


def test_empty_cup():
    disc = raster_ellipse(64, 64, 31.5, 31.5, 20, 20)
    row = finish_masks(disc, np.zeros_like(disc))
    assert row["vcdr_ellipse"] == 0.0 and row["hcdr_ellipse"] == 0.0 and row["cup_major"] != row["cup_major"]
    prof, _ = M.profile_host(disc, np.zeros_like(disc), 24)
    assert row["rim"] == [math.sqrt(int(v)) / 2.0 for v in prof[0, :, 0]]          # the disc's radius
    assert all(abs(v - 20) <= 1.0 for v in row["rim"])


def test_cup_outside_the_disc_gives_a_negative_width():
    disc = raster_ellipse(64, 64, 31.5, 31.5, 10, 10)
    cup = raster_ellipse(64, 64, 31.5, 45.5, 8, 3)                                 # sticks out to the right
    row = finish_masks(disc, cup)
    assert row["rim"][0] < -5.0 and row["rim_min"] == min(row["rim"]) and row["rim_min_angle"] in (7.5, 352.5)


def _profile(N, rim_by_sector, cup=0):
    """A hand-made record: disc radius rim + cup, cup radius `cup`, in half-pixel units squared."""
    p = np.zeros((N, 4), np.uint32)
    for s, v in enumerate(rim_by_sector):
        if v is not None:
            p[s] = ((2 * (v + cup)) ** 2, (2 * cup) ** 2, 1, 1 if cup else 0)
    return p


def test_quadrants_eye_and_isnt():
    N = 8                                                                          # sector centres 22.5, 67.5, ...: two per quadrant
    rec_d, rec_c = [100, 0, 9, 0, 9, 450, 450, 0], [10, 0, 1, 0, 1, 5, 5, 0]
    mom = np.array([[3000, 3000, 2025, 9], [5, 5, 2, 9]], np.int64)
    #        right  sup    sup    left   left   inf    inf    right
    rims = [4, 7, 9, 6, 6, 10, 12, 2]
    fin = lambda eye, r=rims: M.finish(rec_d, rec_c, mom, _profile(N, r, cup=3), 10, 10, eye)
    row = fin(None)
    assert (row["rim_superior"], row["rim_left"], row["rim_inferior"], row["rim_right"]) == (8.0, 6.0, 11.0, 3.0)
    assert row["rim_nasal"] != row["rim_nasal"] and row["rim_temporal"] != row["rim_temporal"] and row["isnt"] != row["isnt"]
    assert row["rim_min"] == 2.0 and row["rim_min_angle"] == 337.5 and row["eye"] == ""
    right = fin("right")                                                           # temporal = left
    assert (right["rim_temporal"], right["rim_nasal"], right["isnt"], right["eye"]) == (6.0, 3.0, 0.0, "right")    # N < T
    left = fin("left")                                                             # mirrored
    assert (left["rim_temporal"], left["rim_nasal"], left["isnt"], left["eye"]) == (3.0, 6.0, 1.0, "left")         # 11 >= 8 >= 6 >= 3
    assert fin("left", [4, 12, 12, 6, 6, 10, 10, 2])["isnt"] == 0.0                # superior above inferior
    assert fin("left", [3, 8, 8, 8, 8, 8, 8, 3])["isnt"] == 1.0                    # ties hold
    # the first minimum wins; nan sectors are ignored, in the minimum and in the means
    tie = fin("left", [5, 2, None, 2, 6, None, None, 5])
    assert tie["rim_min"] == 2.0 and tie["rim_min_angle"] == 67.5 and tie["rim_superior"] == 2.0 and tie["rim_left"] == 4.0
    assert tie["rim_inferior"] != tie["rim_inferior"] and tie["isnt"] != tie["isnt"] and tie["rim"][2] != tie["rim"][2]
    with pytest.raises(ValueError):
        fin("both")
    s = M.summarise([right, left, tie], "left")
    assert s["sectors"] == 8 and s["n_isnt_violations"] == 1 and s["mean_rim_min_rel"] == np.mean([r["rim_min_rel"] for r in (right, left, tie)])
    assert "n_isnt_violations" not in M.summarise([row]) and M.summarise([], None)["mean_vcdr_ellipse"] is None


def test_sample_statistics():
    disc = raster_ellipse(64, 64, 31.5, 31.5, 20, 18)
    rows = [finish_masks(disc, raster_ellipse(64, 64, 31.5, 31.5, r, r), 8) for r in (6, 8, 11)]
    rows.append(finish_masks(np.zeros_like(disc), disc, 8))                        # an empty disc: left out
    st = M.sample_statistics(rows)
    assert st["n_samples"] == 4 and st["n_defined"] == 3 and len(st["rim_rel_std"]) == 8
    v = np.array([r["vcdr_ellipse"] for r in rows[:3]], np.float64)
    assert st["vcdr_ellipse_mean"] == float(v.mean()) and st["vcdr_ellipse_std"] == float(v.std())
    assert st["vcdr_ellipse_p05"] == float(np.percentile(v, 5)) and st["vcdr_ellipse_p95"] == float(np.percentile(v, 95))
    assert st["rim_rel_std"][3] == float(np.array([r["rim_rel"][3] for r in rows[:3]]).std()) > 0
    none = M.sample_statistics(rows[3:])
    assert none["n_defined"] == 0 and all(none[k] != none[k] for k in M.STAT_COLUMNS[2:]) and all(x != x for x in none["rim_rel_std"])


# ---- I/O ----------------------------------------------------------------------------------------------------------------------------
def test_csv_round_trip_is_bitwise(tmp_path):
    disc = raster_ellipse(70, 90, 33.3, 41.7, 25, 19, 0.4)
    rows = [dict(finish_masks(disc, raster_ellipse(70, 90, 35, 40, 11, 7, 1.1), 16, "left"), index=1, name='a, "quoted".png'),
            dict(finish_masks(np.zeros_like(disc), disc, 16, "left"), index=2, name="empty disc.png"),
            dict(finish_masks(disc, np.zeros_like(disc), 16, None), index=3, name="c.png")]
    M.write_csv(str(tmp_path), rows)
    with open(tmp_path / "morphometry.csv") as f:
        assert f.readline().strip().split(",") == list(M.MORPH_COLUMNS)
    with open(tmp_path / "rim_profile.csv") as f:
        assert f.readline().strip().split(",") == ["index", "name"] + ["rim_%03d" % s for s in range(16)]
    back = M.read_csv(str(tmp_path))
    assert len(back) == 3
    for a, b in zip(rows, back):
        for k in M.MORPH_COLUMNS:
            assert same(a[k], b[k]) and type(a[k]) is type(b[k]), (k, a[k], b[k])
        assert len(b["rim"]) == 16 and all(same(x, y) for x, y in zip(a["rim"], b["rim"]))
    stats = [dict(M.sample_statistics(rows), index=1, name="a.png"), dict(M.sample_statistics(rows[1:2]), index=2, name="b.png")]
    M.write_uncertainty_csv(str(tmp_path), stats)
    for a, b in zip(stats, M.read_uncertainty_csv(str(tmp_path))):
        assert set(a) == set(b)
        for k in M.STAT_COLUMNS + ("index", "name"):
            assert same(a[k], b[k]), k
        assert all(same(x, y) for x, y in zip(a["rim_rel_std"], b["rim_rel_std"])) and len(b["rim_rel_std"]) == 16
    errs = [dict(M.error_row(rows[0], rows[2]), index=1, name="x.png"), dict(M.error_row(rows[1], rows[0]), index=2, name="y.png")]
    means = M.write_errors_csv(str(tmp_path), errs)
    got, last = M.read_errors_csv(str(tmp_path))
    for a, b in zip(errs, got):
        assert all(same(a[k], b[k]) for k in M.ERROR_COLUMNS + ("index", "name"))
    assert errs[0]["vcdr_ellipse_abs_diff"] == abs(rows[0]["vcdr_ellipse"] - 0.0) and errs[1]["vcdr_ellipse_abs_diff"] != errs[1]["vcdr_ellipse_abs_diff"]
    assert last["name"] == "mean" and last["vcdr_ellipse_abs_diff"] == means["mean_vcdr_ellipse_abs_diff"] == errs[0]["vcdr_ellipse_abs_diff"]


@pytest.mark.parametrize("kw", [{"sectors": 12}, {"sectors": 368}, {"sectors": 0}, {"eye": "both"}, {"eye": "Right"}], ids=str)
def test_constructors_reject_bad_arguments(kw, tmp_path):
    from wtpse_hip.segment import Segmenter
    from wtpse_hip.test_run import TestRun
    for morphometry in (False, True):
        with pytest.raises(ValueError):
            Segmenter(None, None, None, None, out_dir=str(tmp_path / "s"), morphometry=morphometry, **kw)
        with pytest.raises(ValueError):
            TestRun(None, None, None, None, out_dir=str(tmp_path / "t"), morphometry=morphometry, **kw)
    assert not os.path.exists(tmp_path / "s") and not os.path.exists(tmp_path / "t")
    ok = Segmenter(None, None, None, None, out_dir=str(tmp_path / "s"), morphometry=True, sectors=64, eye="left")
    assert (ok.morphometry, ok.sectors, ok.eye) == (True, 64, "left")
    assert Segmenter(None, None, None, None, out_dir=str(tmp_path / "s")).morphometry is False


def test_command_lines_check_the_sectors_first():
    from wtpse_hip import morphometry_run, segment
    tail = ["--checkpoint", "c", "--out", "o", "--morphometry", "--sectors", "12", "--eye", "left"]
    with pytest.raises(ValueError, match="sectors"):                               # before the GPU is asked for
        segment.main(["--images", "x"] + tail)
    with pytest.raises(ValueError, match="sectors"):
        morphometry_run.main(["--data-dir", "x", "--datasetTest", "1"] + [a for a in tail if a != "--morphometry"])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_validates_without_a_gpu():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    protos = build.parse_prototypes()
    assert protos["wtpse_onh_profile"] == ["const unsigned char*", "const unsigned char*", "const long long*", "const int*", "unsigned*",
                                           "long long*", "int", "int", "int", "int", "void*"]
    fn = lib().raw("wtpse_onh_profile")
    p = 4096                                                                       # never dereferenced: validation comes first
    assert fn(None, p, p, p, p, p, 24, 1, 8, 8, None) == -1
    assert fn(p, p, p, p, p, None, 24, 1, 8, 8, None) == -1
    for N in (12, 0, 4, 368):
        assert fn(p, p, p, p, p, p, N, 1, 8, 8, None) == -1
    assert fn(p, p, p, p, p, p, 24, 0, 8, 8, None) == -1 and fn(p, p, p, p, p, p, 24, 8192, 8, 8, None) == -1
    assert fn(p, p, p, p, p, p, 24, 1, 4097, 8, None) == -1 and fn(p, p, p, p, p, p, 24, 1, 8, 0, None) == -1
    assert fn(p, p, p + 4, p, p, p, 24, 1, 8, 8, None) == -1                       # records 8-byte aligned
