"""wtpse_hip/test_run.py without a GPU: the host specification of the overlays (overlay_host) against an INDEPENDENT oracle, the
host part of the test feed against tests/golden/testfeed.npz (the reference's own FundusSegmentation(phase='test',
state='prediction') under Resize(256) / Normalize_tf / ToTensor: tools/make_golden_testfeed.py), the new ABI entries, and the
per-image table writer.

The oracle below is a literal marching-squares enumeration — for every 2 x 2 cell the 16-case table, segment end points placed with
the (level - a) / (b - a) interpolation — painted in the reference's statement order (utils.py:408-448) with numpy fancy indexing.
The product derives the same pictures from "adjacent pixel pairs that differ" instead, so the two check each other.  Segments are not
joined into contours: one map's contours are all painted in one colour, so the picture depends on the vertex set alone.  Where the
reference would raise IndexError (ground truth touching the last row / column) the oracle drops that one write, the stated deviation.
"""
import hashlib
import os

import numpy as np
import pytest

from oracle import postprocess_cpu as P
from oracle.fundus_tree import make_tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testfeed.npz")

# ---- the oracle -----------------------------------------------------------------------------------------------------------
# corners of a cell: ul = (r, c), ur = (r, c+1), ll = (r+1, c), lr = (r+1, c+1); case = ul | ur << 1 | ll << 2 | lr << 3 (above level).
# Segments as pairs of cell edges T(op) B(ottom) L(eft) R(ight); the two saddles (6, 9) cut all four edges whichever way they pair.
MS_TABLE = {0: [], 1: ["TL"], 2: ["RT"], 3: ["RL"], 4: ["LB"], 5: ["TB"], 6: ["LT", "RB"], 7: ["RB"], 8: ["BR"], 9: ["TR", "BL"],
            10: ["BT"], 11: ["BL"], 12: ["LR"], 13: ["TR"], 14: ["LT"], 15: []}


def marching_squares_vertices(a, level=0.5):
    """Every segment end point of every cell, in cell order -> (rows, cols) float64."""
    a = np.asarray(a, dtype=np.float64)
    frac = lambda p, q: (level - p) / (q - p)
    rows, cols = [], []
    for r in range(a.shape[0] - 1):
        for c in range(a.shape[1] - 1):
            ul, ur, ll, lr = a[r, c], a[r, c + 1], a[r + 1, c], a[r + 1, c + 1]
            case = int(ul > level) | int(ur > level) << 1 | int(ll > level) << 2 | int(lr > level) << 3
            for seg in MS_TABLE[case]:
                for edge in seg:
                    if edge == "T":
                        p = (r, c + frac(ul, ur))
                    elif edge == "B":
                        p = (r + 1, c + frac(ll, lr))
                    elif edge == "L":
                        p = (r + frac(ul, ll), c)
                    else:
                        p = (r + frac(ur, lr), c + 1)
                    rows.append(p[0])
                    cols.append(p[1])
    return np.array(rows, dtype=np.float64), np.array(cols, dtype=np.float64)


def _write(canvas, r, c, colour):
    try:
        canvas[r, c, :] = colour
    except IndexError:                      # the reference ends here; the oracle drops the one write that is out of range
        for ri, ci in zip(r, c):
            try:
                canvas[ri, ci, :] = colour
            except IndexError:
                pass


def oracle_paint(canvas, m, colour):
    """utils.py:409-415, statement by statement."""
    r, c = marching_squares_vertices(m)
    _write(canvas, (r).astype(int), (c).astype(int), colour)
    _write(canvas, (r + 1.0).astype(int), (c).astype(int), colour)
    _write(canvas, (r + 1.0).astype(int), (c + 1.0).astype(int), colour)
    _write(canvas, (r).astype(int), (c + 1.0).astype(int), colour)
    _write(canvas, (r - 1.0).astype(int), (c).astype(int), colour)
    _write(canvas, (r - 1.0).astype(int), (c - 1.0).astype(int), colour)
    _write(canvas, (r).astype(int), (c - 1.0).astype(int), colour)


def oracle_overlay(img, pred_od, pred_oc, gt_od, gt_oc):
    h, w = pred_od.shape
    patch = ((img + np.float32(1)) * np.float32(127.5)).transpose(1, 2, 0)
    original = patch.astype(np.uint8)
    mask = np.zeros((h, w, 2))
    mask[pred_od == 1] = [0, 1]
    mask[pred_oc == 1] = [1, 1]
    target = np.zeros((h, w, 2))
    target[gt_od == 1] = [0, 1]
    target[gt_oc == 1] = [1, 1]
    disc_map, cup_map = mask[:, :, 0], mask[:, :, 1]
    for mp in (disc_map, cup_map):
        mp[:, 0] = 0
        mp[:, w - 1] = 0
        mp[0, :] = 0
        mp[h - 1, :] = 0
    canvas = patch.copy()
    oracle_paint(canvas, cup_map, [0, 255, 0])
    oracle_paint(canvas, disc_map, [0, 0, 255])
    gt_disc = P.get_largest_fillhole(target[:, :, 0] * 128).astype(np.uint8)
    gt_cup = P.get_largest_fillhole(target[:, :, 1] * 128).astype(np.uint8)
    oracle_paint(canvas, gt_cup, [255, 0, 0])
    oracle_paint(canvas, gt_disc, [255, 0, 0])
    return original, canvas.astype(np.uint8)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).astype(np.uint8)


def _blobs(rng, h, w, p):
    from scipy.ndimage import gaussian_filter
    f = gaussian_filter(rng.standard_normal((h, w)), 2.0, mode="constant")
    return (f > np.quantile(f, 1.0 - p)).astype(np.uint8)


def _image(rng, h, w):
    img = rng.uniform(-1.0, 1.0, (3, h, w)).astype(np.float32)
    img[:, 0, 0] = (-1.0, 1.0, 0.0)                                # the ends of the range: 0, 255 and 127.5 -> 127
    return img


def overlay_cases():
    """-> [(name, img [3,h,w] fp32, pred_od, pred_oc, gt_od, gt_oc [h,w] uint8)]."""
    rng = np.random.default_rng(77)
    z = lambda h, w: np.zeros((h, w), np.uint8)
    out = []
    for k, (h, w) in enumerate(((40, 48), (37, 53), (64, 64))):
        out.append(("blobs%d" % k, _image(rng, h, w), _blobs(rng, h, w, 0.4), _blobs(rng, h, w, 0.15), _blobs(rng, h, w, 0.4),
                    _blobs(rng, h, w, 0.15)))
    out.append(("noise", _image(rng, 33, 35), *[(rng.random((33, 35)) < p).astype(np.uint8) for p in (0.5, 0.3, 0.55, 0.45)]))
    h, w = 37, 53
    out.append(("nested", _image(rng, h, w), _disc(h, w, 18, 26, 14), _disc(h, w, 19, 25, 6), _disc(h, w, 17, 27, 13), _disc(h, w, 17, 27, 5)))
    out.append(("cup_outside_disc", _image(rng, 30, 30), _disc(30, 30, 10, 10, 6), _disc(30, 30, 21, 22, 4), _disc(30, 30, 20, 9, 5),
                _disc(30, 30, 8, 22, 3)))
    out.append(("empty_prediction", _image(rng, 20, 24), z(20, 24), z(20, 24), _disc(20, 24, 10, 12, 6), _disc(20, 24, 10, 12, 2)))
    out.append(("empty_everything", _image(rng, 9, 11), z(9, 11), z(9, 11), z(9, 11), z(9, 11)))
    sad = z(6, 7)
    sad[2, 2] = sad[3, 3] = 1
    sad2 = z(6, 7)
    sad2[2, 4] = sad2[3, 3] = 1
    out.append(("saddle", _image(rng, 6, 7), sad, sad2, sad2, sad))
    one = z(9, 8)
    one[4, 3] = 1
    one2 = z(9, 8)
    one2[6, 6] = 1
    out.append(("one_pixel", _image(rng, 9, 8), one, one2, one2, one))
    full = np.ones((17, 19), np.uint8)
    out.append(("prediction_touches_border", _image(rng, 17, 19), full, _disc(17, 19, 0, 0, 7), _disc(17, 19, 8, 9, 5), _disc(17, 19, 8, 9, 2)))
    top = z(21, 23)
    top[0:6, 5:14] = 1
    topc = z(21, 23)
    topc[0:3, 7:10] = 1
    left = z(21, 23)
    left[8:15, 0:5] = 1
    out.append(("gt_touches_top_row", _image(rng, 21, 23), _disc(21, 23, 10, 11, 6), _disc(21, 23, 10, 11, 3), top, topc))
    out.append(("gt_touches_first_column_and_corner", _image(rng, 21, 23), _disc(21, 23, 10, 11, 6), z(21, 23), left | _disc(21, 23, 0, 0, 4),
                _disc(21, 23, 0, 0, 2)))
    last = z(21, 23)
    last[15:21, 4:12] = 1
    lastc = z(21, 23)
    lastc[18:21, 6:9] = 1
    right = z(21, 23)
    right[3:12, 17:23] = 1
    out.append(("gt_touches_last_row", _image(rng, 21, 23), _disc(21, 23, 10, 11, 6), _disc(21, 23, 10, 11, 3), last, lastc))
    out.append(("gt_touches_last_column_and_corner", _image(rng, 21, 23), _disc(21, 23, 10, 11, 6), z(21, 23), right | _disc(21, 23, 20, 22, 5),
                _disc(21, 23, 20, 22, 2)))
    out.append(("gt_full_frame", _image(rng, 12, 13), z(12, 13), z(12, 13), np.ones((12, 13), np.uint8), _disc(12, 13, 6, 6, 3)))
    for k in range(16):                                             # every 2 x 2 ground truth; the prediction's border is the whole map
        g = np.array([[k & 1, (k >> 1) & 1], [(k >> 2) & 1, (k >> 3) & 1]], np.uint8)
        out.append(("2x2_%d" % k, _image(rng, 2, 2), np.ones((2, 2), np.uint8), g, g, g[::-1].copy()))
    out.append(("3x2", _image(rng, 3, 2), np.ones((3, 2), np.uint8), z(3, 2), np.array([[0, 1], [1, 1], [0, 0]], np.uint8), z(3, 2)))
    out.append(("2x5", _image(rng, 2, 5), z(2, 5), z(2, 5), np.array([[0, 1, 1, 0, 1], [0, 0, 1, 0, 0]], np.uint8),
                np.array([[0, 0, 1, 0, 0], [0, 0, 0, 0, 0]], np.uint8)))
    return out


CASES = overlay_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_overlay_host_matches_marching_squares_oracle(case):
    from wtpse_hip.test_run import overlay_host
    _, img, pod, poc, god, goc = case
    want_o, want_v = oracle_overlay(img, pod, poc, god, goc)
    got_o, got_v = overlay_host(img, pod, poc, god, goc)
    assert got_o.dtype == got_v.dtype == np.uint8 and got_o.shape == got_v.shape == pod.shape + (3,)
    assert np.array_equal(got_o, want_o)
    assert np.array_equal(got_v, want_v), int((got_v != want_v).any(axis=2).sum())


def test_cases_reach_the_quirks():
    """The cases above really exercise what they are named for: a red pixel in the last row that only the -1 wrap explains, and a
    write the oracle had to drop."""
    from wtpse_hip.test_run import overlay_host, contour_vertices
    by = {c[0]: c for c in CASES}
    _, img, pod, poc, god, goc = by["gt_touches_top_row"]
    _, over = overlay_host(img, pod, poc, god, goc)
    assert (over[-1] == (255, 0, 0)).all(axis=1).any() and not god[-3:].any()
    _, _, _, _, god, _ = by["gt_touches_last_row"]
    r, _ = contour_vertices(god)
    assert (r + 1).astype(int).max() == god.shape[0]               # the index the reference raises IndexError on
    untouched = by["empty_everything"]
    o, v = overlay_host(*untouched[1:])
    assert np.array_equal(o, v) and tuple(o[0, 0]) == (0, 255, 127)


def test_batch_wrapper_and_argument_shapes():
    from wtpse_hip.test_run import overlay_host, overlay_host_batch
    cs = [c for c in CASES if c[2].shape == (21, 23)]
    assert len(cs) >= 4
    img = np.stack([c[1] for c in cs])
    ms = [np.stack([c[k] for c in cs])[:, None] for k in (2, 3, 4, 5)]
    o, v = overlay_host_batch(img, *ms)
    assert o.shape == v.shape == (len(cs), 21, 23, 3)
    for i, c in enumerate(cs):
        wo, wv = overlay_host(*c[1:])
        assert np.array_equal(o[i], wo) and np.array_equal(v[i], wv)


# ---- the feed against the reference's loader ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fundus_test"))
    make_tree(root, seed=5)
    return root


@pytest.mark.parametrize("domain", [1, 2, 3, 4])
def test_feed_matches_reference_loader(tree, domain):
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.test_run import FundusTestBatches, label_thresholds_host
    g = np.load(GOLDEN)
    ref_names = [str(n) for n in g["d%d_names" % domain]]
    feed = FundusTestBatches(FundusTree(tree, phase="test", splitid=(domain,), state="prediction"), 1, device="cpu")
    assert len(feed) == len(ref_names) == 2
    assert sorted(feed.names) == sorted(ref_names)                  # glob order is the file system's: compare per file
    for b in range(len(feed)):
        image, mask, names = feed.host_batch(b)
        j = ref_names.index(names[0])
        assert image.dtype == np.float32 and image.shape == (1, 3, 256, 256) and mask.dtype == np.uint8
        assert hashlib.sha256(image[0].tobytes()).hexdigest() == str(g["d%d_image_sha256" % domain][j]), names[0]
        od, oc = label_thresholds_host(mask[0, 0])
        assert np.array_equal(od, g["d%d_od_%d" % (domain, j)]) and np.array_equal(oc, g["d%d_oc_%d" % (domain, j)]), names[0]
        assert od.any() and oc.any() and not od.all() and (od >= oc).all()


def test_feed_batching_rules(tree):
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.test_run import FundusTestBatches
    t = FundusTree(tree, phase="test", splitid=(3,), state="prediction")
    feed = FundusTestBatches(t, 2, device="cpu")
    assert len(feed) == 1
    with pytest.raises(ValueError) as e:                            # the two files of Domain3/test differ in size
        feed.host_batch(0)
    assert all(n in str(e.value) for n in feed.names)
    assert len(FundusTestBatches(t, 1, device="cpu")) == 2
    with pytest.raises(ValueError, match="prediction"):
        FundusTestBatches(FundusTree(tree, phase="test", splitid=(3,)), 1)
    # a short last batch: three equal-sized samples, two per batch
    feed = FundusTestBatches(t, 2, device="cpu")
    feed.images, feed.masks, feed.names = [feed.images[0]] * 3, [feed.masks[0]] * 3, ["a", "b", "c"]
    assert len(feed) == 2
    assert [feed.host_batch(b)[2] for b in range(2)] == [["a", "b"], ["c"]]
    assert feed.host_batch(0)[0].shape == (2, 3, 256, 256) and feed.host_batch(1)[1].shape[:2] == (1, 1)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_entries():
    import ctypes
    from wtpse_hip import lib
    protos = lib.parse_header()
    p, i = ctypes.c_void_p, ctypes.c_int
    assert protos["wtpse_overlay_ws"] == [i, i, i]
    assert protos["wtpse_overlay"] == [p] * 8 + [i, i, i, p]
    assert protos["wtpse_label_thresholds"] == [p, p, p, ctypes.c_longlong, p]


def test_library_exports_the_new_entries_and_sizes_its_workspace():
    from wtpse_hip.lib import lib
    L = lib()
    assert L.query("wtpse_overlay_ws", 1, 1, 8) == -1 and L.query("wtpse_overlay_ws", 1, 8, 4097) == -1
    assert L.query("wtpse_overlay_ws", 0, 8, 8) == -1
    for B, h, w in ((1, 2, 2), (9, 800, 800), (2, 37, 53)):
        pp, n2 = L.query("wtpse_postprocess_ws", 2 * B, h, w), 2 * B * h * w
        assert L.query("wtpse_overlay_ws", B, h, w) == (pp + 3) // 4 * 4 + n2 + (n2 + 3) // 4
    assert L.query("wtpse_overlay_ws", 1, 4096, 4096) > 0


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_table_writer_round_trip(tmp_path):
    from wtpse_hip import validate as V
    from wtpse_hip.test_run import CSV_COLUMNS, read_table, write_table
    assert CSV_COLUMNS == ("index", "name", "disc_dice", "cup_dice", "disc_hd", "disc_asd", "cup_hd", "cup_asd")
    m1 = dict(disc_dice=[0.9, 1 / 3], cup_dice=[0.8, 0.1], disc_hd=[2.5, 100.0], disc_asd=[0.7, 100.0], cup_hd=[3.0, 1e-3], cup_asd=[1.1, 2 / 7])
    m2 = dict(disc_dice=[0.5], cup_dice=[0.25], disc_hd=[7.0], disc_asd=[1 / 9], cup_hd=[8.0], cup_asd=[0.3])
    acc, rows = V.MetricMeans(), []
    for m, names in ((m1, ["G-1.png", 'odd,"name".png']), (m2, ["S-3.png"])):
        acc.add(m)
        for i, n in enumerate(names):
            rows.append(dict({k: m[k][i] for k in V.METRIC_KEYS}, index=len(rows) + 1, name=n))
    means = acc.means()
    assert means["n"] == 3 and means["disc_dice"] == (0.9 + 1 / 3 + 0.5) / 3 and means["cup_asd"] == (1.1 + 2 / 7 + 0.3) / 3
    write_table(str(tmp_path), rows, means)
    with open(os.path.join(str(tmp_path), "per_image.csv")) as f:
        assert f.readline().strip() == ",".join(CSV_COLUMNS)
    got_rows, got_means = read_table(str(tmp_path))
    assert got_means == means
    assert [r["index"] for r in got_rows] == [1, 2, 3] and [r["name"] for r in got_rows] == [r["name"] for r in rows]
    for a, b in zip(got_rows, rows):
        assert all(a[k] == b[k] for k in V.METRIC_KEYS)            # repr round-trips float64 exactly


def test_validate_epoch_sums_through_the_shared_helper():
    """validate_epoch and TestRun tabulate the same per-image lists: MetricMeans is validate_epoch's old accumulation."""
    from wtpse_hip import validate as V
    acc = V.MetricMeans()
    assert acc.means() == dict(cup_dice=0.0, disc_dice=0.0, cup_hd=0.0, disc_hd=0.0, cup_asd=0.0, disc_asd=0.0, n=0)
    assert set(V.METRIC_KEYS) == set(acc.acc)
    with pytest.raises(ValueError):
        from wtpse_hip.test_run import TestRun
        TestRun(None, None, None, None, "x", overlay="gpu")
