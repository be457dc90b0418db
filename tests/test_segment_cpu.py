"""wtpse_hip/segment.py on the host: the LANCZOS coefficient tables against the live Pillow (a numpy emulation of the two 8-bit
fixed-point passes csrc/pipeline.hip runs), the label encoding's round trip through PNG and FundusTree, the geometry records and
the table row on hand-checked masks, the image feed and the table writer."""
import hashlib
import json
import os

import numpy as np
import pytest
from PIL import Image

from wtpse_hip import segment as SG
from wtpse_hip.input_pipeline import PRECISION_BITS, resample_table

SIZES = [(800, 800), (613, 517), (256, 256), (100, 120), (257, 255), (300, 256), (1634, 1634)]      # (h, w)


def content(h, w, kind):
    """[h,w,3] uint8: seeded noise, or a smooth picture (two crossed gradients and a bright blob)."""
    if kind == "random":
        return np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    blob = 120.0 * np.exp(-((yy - 0.45 * h) ** 2 + (xx - 0.55 * w) ** 2) / (2 * (0.2 * min(h, w)) ** 2))
    chans = [255.0 * xx / max(w - 1, 1), 255.0 * yy / max(h - 1, 1), 128 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0)]
    return np.clip(np.stack(chans, 2) * 0.5 + blob[:, :, None], 0, 255).astype(np.uint8)


def resample_pass_host(src, bounds, kk, vertical):
    """resample_u8_k in numpy: src [H,W,C] uint8 -> one axis resampled with 22-bit coefficients, + half, >> 22, clipped to 8 bits."""
    a = src.astype(np.int64)
    if not vertical:
        a = a.transpose(1, 0, 2)
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    for o, (first, n) in enumerate(bounds):
        ss = np.tensordot(kk[o, :n].astype(np.int64), a[first:first + n], 1) + (1 << (PRECISION_BITS - 1))
        out[o] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out if vertical else out.transpose(1, 0, 2)


def lanczos_host(img, S=256):
    """The two passes Segmenter.front launches: horizontal then vertical, a pass whose axis already has S entries skipped."""
    H, W = img.shape[:2]
    if W != S:
        b, k, _ = resample_table(W, S, "lanczos")
        img = resample_pass_host(img, b, k, False)
    if H != S:
        b, k, _ = resample_table(H, S, "lanczos")
        img = resample_pass_host(img, b, k, True)
    return img


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_lanczos_tables_reproduce_pillow(size):
    h, w = size
    for kind in ("random", "smooth"):
        img = content(h, w, kind)
        want = np.array(Image.fromarray(img, "RGB").resize((256, 256), Image.LANCZOS))
        got = lanczos_host(img)
        assert got.shape == want.shape == (256, 256, 3)
        assert np.array_equal(got, want), (size, kind, int((got != want).sum()))


def test_lanczos_table_shape_and_support():
    b, k, ks = resample_table(800, 256, "lanczos")
    assert ks == int(np.ceil(3.0 * 800 / 256)) * 2 + 1 and k.shape == (256, ks) and b.shape == (256, 2)
    assert k.dtype == np.int32 and b.dtype == np.int32
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 800).all() and (b[:, 1] <= ks).all()
    assert (np.abs(k.astype(np.int64).sum(1) - (1 << PRECISION_BITS)) <= ks).all()          # normalised rows, rounded per tap
    b, k, ks = resample_table(100, 256, "lanczos")                                         # enlarging: support 3, seven taps
    assert ks == 7


# sha256 of bounds + kk as resample_table gave them before "lanczos" was added
PINNED = [(("bicubic", 800, 256, 0, None), 15, "d5103262c567273c"), (("bicubic", 613, 256, 0, None), 11, "664432c220db2a6f"),
          (("bicubic", 100, 256, 0, None), 5, "c07293be1b7b266e"), (("bilinear", 256, 300, 17, 256), 3, "e5e9c2385cec308d"),
          (("bilinear", 256, 383, 100, 256), 3, "06f370bb07565c2f"), (("bilinear", 256, 256, 0, 256), 3, "c78c4e6521c1bb0c")]


def test_bilinear_and_bicubic_tables_are_unchanged():
    for (filt, a, b, first, count), ksize, digest in PINNED:
        bd, kk, ks = resample_table(a, b, filt, first, count)
        assert ks == ksize and hashlib.sha256(bd.tobytes() + kk.tobytes()).hexdigest()[:16] == digest, (filt, a, b)


# ---- label encoding -----------------------------------------------------------------------------------------------------------
def _random_masks(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (((yy - h / 2) ** 2 + (xx - w / 2) ** 2) <= (0.35 * min(h, w)) ** 2) & (rng.random((h, w)) < 0.95)
    cup = (((yy - h / 2) ** 2 + (xx - w / 2 - 3) ** 2) <= (0.15 * min(h, w)) ** 2) | (rng.random((h, w)) < 0.01)    # some outside the disc
    disc = disc.astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)            # object values other than 1
    cup = cup.astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    return disc, cup


def test_label_map_host_values_and_inverse():
    from wtpse_hip.test_run import label_thresholds_host
    disc, cup = _random_masks(1, 61, 47)
    assert ((cup != 0) & (disc == 0)).any() and (disc > 1).any()
    lm = SG.label_map_host(disc, cup)
    assert lm.dtype == np.uint8 and set(np.unique(lm)) == {0, 128, 255}
    assert (lm[cup != 0] == 0).all() and (lm[(cup == 0) & (disc != 0)] == 128).all() and (lm[(cup == 0) & (disc == 0)] == 255).all()
    od, oc = label_thresholds_host(lm)
    assert np.array_equal(oc, (cup != 0).astype(np.uint8)) and np.array_equal(od, ((disc != 0) | (cup != 0)).astype(np.uint8))


def test_label_map_round_trip_through_png_and_fundus_tree(tmp_path):
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.test_run import label_thresholds_host
    names = ("G-1-L_test.png", "N-2-R_test.png")
    for sub in ("image", "mask"):
        os.makedirs(tmp_path / "Domain3" / "test" / "ROIs" / sub)
    want = {}
    for k, n in enumerate(names):
        h, w = (61, 47) if k == 0 else (40, 72)
        disc, cup = _random_masks(10 + k, h, w)
        want[n] = (SG.label_map_host(disc, cup), disc, cup)
        Image.fromarray(want[n][0], "L").save(tmp_path / "Domain3" / "test" / "ROIs" / "mask" / n)
        Image.fromarray(content(h, w, "smooth"), "RGB").save(tmp_path / "Domain3" / "test" / "ROIs" / "image" / n)
    tree = FundusTree(str(tmp_path), phase="test", splitid=(3,), state="prediction")
    _, masks, got_names = tree.pools[tree.keys()[0]]
    assert sorted(got_names) == sorted(names)
    for m, n in zip(masks, got_names):
        lm, disc, cup = want[n]
        back = np.array(m).astype(np.uint8)
        assert m.mode == "L" and np.array_equal(back, lm)
        od, oc = label_thresholds_host(back)
        assert np.array_equal(oc, (cup != 0).astype(np.uint8)) and np.array_equal(od, ((disc != 0) | (cup != 0)).astype(np.uint8))


# ---- geometry and the table row -----------------------------------------------------------------------------------------------
def test_mask_geometry_host_on_hand_checked_masks():
    h, w = 5, 7
    empty = np.zeros((h, w), np.uint8)
    assert SG.mask_geometry_host(empty).tolist() == [0, h, -1, w, -1, 0, 0, 0]
    for (r, c) in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = empty.copy()
        m[r, c] = 9
        assert SG.mask_geometry_host(m).tolist() == [1, r, r, c, c, r, c, 0]
    corners = empty.copy()
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 1
    assert SG.mask_geometry_host(corners).tolist() == [4, 0, h - 1, 0, w - 1, 2 * (h - 1), 2 * (w - 1), 0]
    full = np.ones((h, w), np.uint8)
    assert SG.mask_geometry_host(full).tolist() == [35, 0, 4, 0, 6, 7 * (0 + 1 + 2 + 3 + 4), 5 * (0 + 1 + 2 + 3 + 4 + 5 + 6), 0]
    batch = SG.mask_geometry_host(np.stack([empty, full])[:, None])
    assert batch.shape == (2, 1, 8) and batch.dtype == np.int64 and batch[1, 0, 0] == 35 and batch[0, 0, 1] == h


def test_measure_disc_with_cup():
    disc, cup = np.zeros((20, 30), np.uint8), np.zeros((20, 30), np.uint8)
    disc[4:14, 5:25] = 1                 # rows 4..13 (10), columns 5..24 (20)
    cup[6:11, 10:14] = 1                 # rows 6..10 (5), columns 10..13 (4)
    row = SG.measure(SG.mask_geometry_host(disc), SG.mask_geometry_host(cup), 20, 30)
    assert (row["height"], row["width"], row["disc_area"], row["cup_area"]) == (20, 30, 200, 20)
    assert (row["disc_top"], row["disc_bottom"], row["disc_left"], row["disc_right"]) == (4, 13, 5, 24)
    assert (row["cup_top"], row["cup_bottom"], row["cup_left"], row["cup_right"]) == (6, 10, 10, 13)
    assert row["vcdr"] == 0.5 and row["hcdr"] == 0.2 and row["acdr"] == 0.1
    assert (row["disc_cy"], row["disc_cx"], row["cup_cy"], row["cup_cx"]) == (8.5, 14.5, 8.0, 11.5)
    assert set(row) == set(SG.INT_COLUMNS + SG.FLOAT_COLUMNS)


def test_measure_empty_masks():
    empty, cup = np.zeros((8, 9), np.uint8), np.zeros((8, 9), np.uint8)
    cup[2:4, 3:6] = 1
    row = SG.measure(SG.mask_geometry_host(empty), SG.mask_geometry_host(cup), 8, 9)           # empty disc, a cup: undefined
    assert all(np.isnan(row[k]) for k in ("vcdr", "hcdr", "acdr", "disc_cy", "disc_cx")) and row["cup_cy"] == 2.5 and row["cup_cx"] == 4.0
    assert (row["disc_top"], row["disc_bottom"], row["disc_left"], row["disc_right"]) == (8, -1, 9, -1)
    row = SG.measure(SG.mask_geometry_host(cup), SG.mask_geometry_host(empty), 8, 9)           # a disc, no cup: zero
    assert row["vcdr"] == 0.0 and row["hcdr"] == 0.0 and row["acdr"] == 0.0 and np.isnan(row["cup_cy"]) and np.isnan(row["cup_cx"])
    row = SG.measure(SG.mask_geometry_host(empty), SG.mask_geometry_host(empty), 8, 9)
    assert all(np.isnan(row[k]) for k in SG.FLOAT_COLUMNS)
    # the cup is not clipped to the disc: a cup taller than the disc gives a ratio above one
    disc = np.zeros((8, 9), np.uint8)
    disc[3, 3:6] = 1
    assert SG.measure(SG.mask_geometry_host(disc), SG.mask_geometry_host(cup), 8, 9)["vcdr"] == 2.0


# ---- the feed -------------------------------------------------------------------------------------------------------------------
def test_image_folder(tmp_path):
    px = Image.fromarray(content(6, 5, "smooth"), "RGB")
    for n in ("b.PNG", "a.jpg", "c.Tiff", "d.bmp", "notes.txt", "e.png.bak"):
        if n.endswith((".txt", ".bak")):
            (tmp_path / n).write_text("x")
        else:
            px.save(tmp_path / n, format={"png": "PNG", "jpg": "JPEG", "tiff": "TIFF", "bmp": "BMP"}[n.rsplit(".", 1)[1].lower()])
    (tmp_path / "sub.png").mkdir()
    f = SG.ImageFolder(str(tmp_path))
    assert [os.path.basename(p) for p in f.paths] == ["a.jpg", "b.PNG", "c.Tiff", "d.bmp"] and len(f) == 4
    assert f.names == ["a.png", "b.png", "c.png", "d.png"]
    a = f.load(1)
    assert a.dtype == np.uint8 and a.shape == (6, 5, 3) and np.array_equal(a, np.array(px))
    order = [str(tmp_path / "d.bmp"), str(tmp_path / "a.jpg")]
    assert SG.ImageFolder(order).paths == order and SG.ImageFolder(order).names == ["d.png", "a.png"]
    px.save(tmp_path / "a.png")
    with pytest.raises(ValueError, match="a.png"):
        SG.ImageFolder(str(tmp_path))
    with pytest.raises(ValueError):
        SG.ImageFolder([str(tmp_path / "a.jpg"), str(tmp_path / "a.png")])
    assert len(SG.ImageFolder([])) == 0


def test_image_folder_decodes_grey_and_palette_as_rgb(tmp_path):
    g = content(7, 9, "random")[:, :, 0]
    Image.fromarray(g, "L").save(tmp_path / "g.png")
    a = SG.ImageFolder(str(tmp_path)).load(0)
    assert a.shape == (7, 9, 3) and all(np.array_equal(a[:, :, c], g) for c in range(3))


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_table_round_trip(tmp_path):
    disc, cup = np.zeros((20, 30), np.uint8), np.zeros((20, 30), np.uint8)
    disc[3:14, 5:12] = 1
    cup[6:9, 7:10] = 1
    empty = np.zeros_like(disc)
    g = SG.mask_geometry_host
    rows = [dict(SG.measure(g(disc), g(cup), 20, 30), index=1, name="a.png"),
            dict(SG.measure(g(empty), g(cup), 20, 30), index=2, name='odd, "name".png'),
            dict(SG.measure(g(disc), g(empty), 20, 30), index=3, name="c.png")]
    summary = SG.summarise(rows)
    assert summary["n"] == 3 and summary["n_empty_disc"] == 1 and summary["n_empty_cup"] == 1
    assert summary["mean_vcdr"] == (3 / 11 + 0.0) / 2 and summary["mean_acdr"] == float(np.mean(np.array([9 / 77, 0.0])))
    SG.write_measurements(str(tmp_path), rows, summary)
    got, got_summary = SG.read_measurements(str(tmp_path))
    assert got_summary == summary
    assert open(tmp_path / "measurements.csv").readline().strip().split(",") == list(SG.CSV_COLUMNS)
    for a, b in zip(got, rows):
        assert a["index"] == b["index"] and a["name"] == b["name"]
        for k in SG.INT_COLUMNS:
            assert a[k] == b[k] and isinstance(a[k], int)
        for k in SG.FLOAT_COLUMNS:
            assert (np.isnan(a[k]) and np.isnan(b[k])) or a[k] == b[k], k            # 3 / 11 reads back to the same float64
    assert "nan" in open(tmp_path / "measurements.csv").read().splitlines()[2].split(",")
    # no defined ratio at all: the means are null in the JSON
    none = SG.summarise(rows[1:2])
    SG.write_measurements(str(tmp_path), rows[1:2], none)
    text = open(tmp_path / "summary.json").read()
    assert json.loads(text)["mean_vcdr"] is None and '"mean_vcdr": null' in text and "NaN" not in text
    assert SG.summarise([]) == {"n": 0, "n_empty_disc": 0, "n_empty_cup": 0, "mean_vcdr": None, "mean_hcdr": None, "mean_acdr": None}
