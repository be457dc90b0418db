"""The CLAHE preprocessing's specification (`input_pipeline.clahe_host` and its helpers) and the stage's boundaries: nothing here
needs a GPU.  The device is held to this specification byte for byte in tests/test_clahe_gpu.py, which takes its pictures from here."""
import argparse
import io

import numpy as np
import pytest
import torch

from wtpse_hip.input_pipeline import (Clahe, clahe_axis_table, clahe_bounds, clahe_host, clahe_lut, clahe_luts_host,
                                      clahe_redistribute, parse_clahe)


def smooth_pictures(seed, N, H, W):
    """[N,H,W,3] uint8, seeded: even samples a smooth blob per channel plus mild noise (many pixels share a bin, as on a fundus
    picture), odd samples uniform-random bytes."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    yy, xx = yy / float(H), xx / float(W)
    out = []
    for n in range(N):
        if n % 2:
            out.append(rng.randint(0, 256, (H, W, 3)).astype(np.float64))
        else:
            cy, cx = rng.uniform(0.3, 0.7, 2)
            blob = 25 + 190 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 0.25 ** 2))
            out.append(blob[..., None] * rng.uniform(0.5, 1.0, 3) + rng.uniform(-6, 6, (H, W, 3)))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


FIELD = dict(H=96, W=80, tiles=(4, 4), floor=24)


def field_fixture():
    """A bright disc of radius 0.3 min(H, W) on a field of value 3 -> [1,96,80,3] uint8."""
    H, W = FIELD["H"], FIELD["W"]
    yy, xx = np.mgrid[0:H, 0:W]
    inside = np.hypot(yy - H / 2.0, xx - W / 2.0) < 0.3 * min(H, W)
    bright = np.maximum(smooth_pictures(11, 1, H, W)[0], 40)
    return np.where(inside[..., None], bright, 3).astype(np.uint8)[None]


# ---------------------------------------------------------------------------------------------------------------- axis tables
@pytest.mark.parametrize("L,t", [(64, 8), (37, 3), (53, 5), (16, 16), (40, 1), (96, 4), (256, 8), (7, 7), (300, 2)])
def test_axis_table(L, t):
    k0, w = clahe_axis_table(L, t)
    assert k0.shape == (L,) and w.shape == (L,)
    b = clahe_bounds(L, t)
    assert b[0] == 0 and b[-1] == L and (np.diff(b) >= 1).all()
    c2 = b[:-1] + b[1:]
    p = 2 * np.arange(L) + 1
    outer = (p <= c2[0]) | (p >= c2[-1])
    assert (w[outer] == 0).all() and (k0[p <= c2[0]] == 0).all() and (k0[p >= c2[-1]] == t - 1).all()
    assert (w >= 0).all() and (w <= 255).all()                     # (every pair of centres here lies less than 512 apart)
    assert (np.diff(k0) >= 0).all() and k0.min() >= 0 and k0.max() <= t - 1
    if t == 1:
        assert not k0.any() and not w.any()
    # between two centres the weight grows with the pixel
    for k in range(t - 1):
        sel = (k0 == k) & ~outer
        assert (np.diff(w[sel]) >= 0).all()


def test_axis_table_far_centres():
    """Where two centres lie 512 or more doubled units apart the formula's rounding reaches 256 at the last pixel in front of the
    upper centre (all of the upper tile): the table is wider than a byte there, and the blend still fits 32 bits."""
    k0, w = clahe_axis_table(1024, 2)
    assert w.max() == 256 and k0[np.argmax(w)] == 0 and (w >= 0).all()
    assert (256 * 256 * 255 + 32768) < 1 << 32


# ---------------------------------------------------------------------------------------------------------------- redistribution
def _dominant(remainder, clip_q8=512):
    """A histogram with one dominant bin whose excess % 256 is `remainder`: 255 bins of 1 and bin 100 searched upwards."""
    for big in range(1000, 5000):
        h = np.ones(256, np.int64)
        h[100] = big
        n = int(h.sum())
        limit = max(1, (clip_q8 * n) >> 16)
        excess = int(np.maximum(h - limit, 0).sum())
        if excess > 0 and excess % 256 == remainder:
            return h
    raise AssertionError("no histogram with remainder %d" % remainder)


@pytest.mark.parametrize("remainder,step", [(1, 256), (2, 128), (3, 85), (127, 2), (128, 2), (129, 1), (255, 1)])
def test_redistribution(remainder, step):
    assert max(256 // remainder, 1) == step
    h = _dominant(remainder)
    n = int(h.sum())
    out = clahe_redistribute(h, 512)
    assert int(out.sum()) == n and (out >= 0).all()
    limit = max(1, (512 * n) >> 16)
    excess = int(np.maximum(h - limit, 0).sum())
    base = np.minimum(h, limit) + excess // 256
    extra = out - base
    assert set(np.unique(extra)) <= {0, 1} and int(extra.sum()) == remainder
    assert np.array_equal(np.nonzero(extra)[0], np.arange(remainder) * step)
    lut = clahe_lut(h, 512)
    assert (np.diff(lut) >= 0).all() and lut[-1] == 255 and lut.min() >= 0


def test_empty_tile_lut_is_identity():
    assert np.array_equal(clahe_lut(np.zeros(256, np.int64), 512), np.arange(256))


# ---------------------------------------------------------------------------------------------------------------- whole pictures
def test_no_clipping_is_plain_equalisation():
    """tiles (1, 1) with clip 256: limit = n, nothing is clipped, no interpolation: plain histogram equalisation per channel."""
    x = smooth_pictures(3, 2, 40, 36)
    got = clahe_host(x, clip=256, tiles=(1, 1), mode="rgb")
    for n in range(2):
        for c in range(3):
            v = x[n, :, :, c]
            count = v.size
            cdf = np.cumsum(np.bincount(v.ravel(), minlength=256)).astype(np.int64)
            lut = np.minimum((cdf * 255 + count // 2) // count, 255)
            assert np.array_equal(got[n, :, :, c], lut[v])


def _float_reference(img, clip_q8, tiles, floor, mode):
    """An independent evaluation of one picture [H,W,3]: loops over pixels, LUTs from python integers, true bilinear weights between
    the tile centres in float64 (no Q8), one rounding at the end."""
    H, W = img.shape[:2]
    ty, tx = tiles
    by = [(k * H) // ty for k in range(ty + 1)]
    bx = [(k * W) // tx for k in range(tx + 1)]
    P = 1 if mode == "luma" else 3

    def plane_value(px, p):
        r, g, b = (int(v) for v in px)
        return (77 * r + 150 * g + 29 * b + 128) >> 8 if mode == "luma" else int(px[p])

    luts = {}
    for i in range(ty):
        for j in range(tx):
            for p in range(P):
                h = [0] * 256
                for y in range(by[i], by[i + 1]):
                    for x in range(bx[j], bx[j + 1]):
                        if max(int(v) for v in img[y, x]) >= floor:
                            h[plane_value(img[y, x], p)] += 1
                n = sum(h)
                if n == 0:
                    luts[i, j, p] = list(range(256))
                    continue
                limit = max(1, (clip_q8 * n) >> 16)
                excess = sum(max(v - limit, 0) for v in h)
                h = [min(v, limit) + excess // 256 for v in h]
                r = excess % 256
                if r:
                    step = max(256 // r, 1)
                    for m in range(r):
                        h[m * step] += 1
                acc, lut = 0, []
                for v in h:
                    acc += v
                    lut.append(min((acc * 255 + n // 2) // n, 255))
                luts[i, j, p] = lut

    def axis(pos, b, t):
        centres = [(b[k] + b[k + 1]) / 2.0 for k in range(t)]
        c = pos + 0.5
        if c <= centres[0]:
            return 0, 0, 0.0
        if c >= centres[-1]:
            return t - 1, t - 1, 0.0
        k = max(k for k in range(t) if centres[k] <= c)
        return k, k + 1, (c - centres[k]) / (centres[k + 1] - centres[k])

    out = np.zeros((H, W, 3), np.float64)
    for y in range(H):
        i0, i1, fy = axis(y, by, ty)
        for x in range(W):
            j0, j1, fx = axis(x, bx, tx)
            px = img[y, x]
            if max(int(v) for v in px) < floor:
                out[y, x] = px
                continue
            new = []
            for p in range(P):
                v = plane_value(px, p)
                top = (1 - fx) * luts[i0, j0, p][v] + fx * luts[i0, j1, p][v]
                bottom = (1 - fx) * luts[i1, j0, p][v] + fx * luts[i1, j1, p][v]
                new.append((1 - fy) * top + fy * bottom)
            if mode == "luma":
                out[y, x] = np.clip(px.astype(np.float64) + (new[0] - plane_value(px, 0)), 0, 255)
            else:
                out[y, x] = new
    return out


@pytest.mark.parametrize("mode", ["luma", "rgb"])
def test_independent_float_evaluation(mode):
    x = smooth_pictures(5, 1, 24, 20)
    got = clahe_host(x, clip=2.0, tiles=(3, 2), floor=0, mode=mode)[0].astype(np.float64)
    want = _float_reference(x[0], 512, (3, 2), 0, mode)
    assert np.abs(got - want).max() <= 1.0
    assert not np.array_equal(got, x[0])


@pytest.mark.parametrize("mode", ["luma", "rgb"])
def test_transposition(mode):
    x = smooth_pictures(7, 2, 37, 53)
    a = clahe_host(x, tiles=(3, 5), mode=mode, floor=30)
    b = clahe_host(np.ascontiguousarray(x.transpose(0, 2, 1, 3)), tiles=(5, 3), mode=mode, floor=30)
    assert np.array_equal(a.transpose(0, 2, 1, 3), b)
    assert not np.array_equal(a, x)


@pytest.mark.parametrize("mode", ["luma", "rgb"])
def test_field_mask(mode):
    x = field_fixture()
    H, W, (ty, tx), floor = FIELD["H"], FIELD["W"], FIELD["tiles"], FIELD["floor"]
    field = x[0].max(-1) >= floor
    by, bx = clahe_bounds(H, ty), clahe_bounds(W, tx)
    cover = np.array([[field[by[i]:by[i + 1], bx[j]:bx[j + 1]].mean() for j in range(tx)] for i in range(ty)])
    assert (cover == 0).any() and ((cover > 0) & (cover < 1)).any()          # the fixture has an empty and a partly covered tile
    clahe = Clahe(2.0, (ty, tx), floor, mode)
    out = clahe_host(x, clahe)
    assert np.array_equal(out[0][~field], x[0][~field])
    assert not np.array_equal(out[0][field], x[0][field])
    luts = clahe_luts_host(x, clahe)
    assert luts.shape == (1, clahe.planes, ty, tx, 256)
    for i, j in np.argwhere(cover == 0):
        assert (luts[0, :, i, j] == np.arange(256)).all()
    # a partly covered tile counts its field pixels alone: the LUT of their histogram, not of the whole tile's
    i, j = np.argwhere((cover > 0) & (cover < 1))[0]
    tile = x[0, by[i]:by[i + 1], bx[j]:bx[j + 1]].astype(np.int64)
    plane = (77 * tile[..., 0] + 150 * tile[..., 1] + 29 * tile[..., 2] + 128) >> 8 if mode == "luma" else tile[..., 0]
    inside = field[by[i]:by[i + 1], bx[j]:bx[j + 1]]
    assert np.array_equal(luts[0, 0, i, j], clahe_lut(np.bincount(plane[inside], minlength=256), 512))
    assert not np.array_equal(luts[0, 0, i, j], clahe_lut(np.bincount(plane.ravel(), minlength=256), 512))


def test_constants():
    for mode in ("luma", "rgb"):
        c = clahe_host(np.full((2, 40, 44, 3), 77, np.uint8), tiles=(4, 4), mode=mode)
        assert len(np.unique(c)) == 1
        rng = np.random.RandomState(2)
        x = (rng.randint(0, 2, (2, 40, 44, 1)) * 255).astype(np.uint8).repeat(3, -1)
        out = clahe_host(x, tiles=(4, 4), mode=mode)
        assert (out[x == 255] == 255).all()


def test_luts_are_monotone():
    luts = clahe_luts_host(smooth_pictures(9, 2, 48, 40), clip=3.0, tiles=(4, 3), mode="rgb").astype(np.int64)
    assert (np.diff(luts, axis=-1) >= 0).all() and (luts[..., -1] == 255).all()


# ---------------------------------------------------------------------------------------------------------------- boundaries
def test_range_checks():
    Clahe()
    Clahe(1.0, (1, 1), 0, "rgb")
    Clahe(256, (16, 16), 255, "luma")
    for kw in (dict(clip=0.99), dict(clip=256.5), dict(clip="x"), dict(tiles=(0, 8)), dict(tiles=(8, 17)), dict(tiles=8),
               dict(tiles=(8.5, 8)), dict(floor=-1), dict(floor=256), dict(floor=1.5), dict(mode="hsv"), dict(mode=None)):
        with pytest.raises(ValueError):
            Clahe(**kw)
    x = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        clahe_host(x, tiles=(9, 8))
    with pytest.raises(ValueError):
        clahe_host(x, tiles=(8, 9))
    with pytest.raises(ValueError):
        clahe_host(x.astype(np.float32))
    with pytest.raises(ValueError):
        clahe_host(x[0])
    with pytest.raises(ValueError):
        clahe_host(np.zeros((1, 4, 4097, 3), np.uint8), tiles=(1, 1))
    with pytest.raises(ValueError):
        clahe_host(x, Clahe(), clip=3.0)


def test_record_round_trip():
    for c in (Clahe(), Clahe(3.3, (4, 6), 24, "rgb"), Clahe(1.0, (1, 16), 255, "luma"), Clahe(256, (16, 1))):
        d = c.record()
        assert set(d) == {"clip_q8", "ty", "tx", "floor", "mode"}
        assert all(type(v) in (int, str) for v in d.values())
        back = Clahe.from_record(d)
        assert back == c and back.record() == d
        assert back.clip_q8 == int(np.rint(c.clip * 256)) and back.tiles == c.tiles
    assert Clahe() != Clahe(2.5)
    for bad in ({}, {"clip_q8": 512}, dict(Clahe().record(), mode="hsv"), dict(Clahe().record(), ty=0), dict(Clahe().record(), clip_q8=100)):
        with pytest.raises(ValueError):
            Clahe.from_record(bad)


def test_switch_parsing():
    assert parse_clahe("checkpoint") == "checkpoint"
    assert parse_clahe("off") is None
    assert parse_clahe("2.5") == Clahe(2.5)
    assert parse_clahe("3:4,6") == Clahe(3.0, (4, 6))
    assert parse_clahe("3:4,6:24") == Clahe(3.0, (4, 6), 24)
    assert parse_clahe("3:4,6:24:rgb") == Clahe(3.0, (4, 6), 24, "rgb")
    for bad in ("", "on", "2:8", "2:8,8,8", "2:8,8:x", "2:8,8:0:hsv", "2:8,8:0:luma:1", "0.5", "2:0,8", "2:8,8:300"):
        with pytest.raises(ValueError):
            parse_clahe(bad)


def test_switch_against_the_checkpoint(capsys):
    from wtpse_hip.programs import add_clahe_argument, resolve_clahe
    ap = argparse.ArgumentParser()
    add_clahe_argument(ap)
    assert ap.parse_args([]).clahe == "checkpoint"
    help_text = io.StringIO()
    ap.print_help(help_text)
    flat = " ".join(help_text.getvalue().split())
    assert "OpenCV" in flat and "unmeasured" in flat and "off" in flat
    record = Clahe(3.0, (4, 4), 24).record()
    assert resolve_clahe(ap, "checkpoint", None) is None
    assert resolve_clahe(ap, "checkpoint", record) == Clahe(3.0, (4, 4), 24)
    assert resolve_clahe(ap, "off", None) is None
    assert resolve_clahe(ap, "3:4,4:24", record) == Clahe(3.0, (4, 4), 24)
    assert capsys.readouterr().out == ""                                 # nothing was overridden so far
    assert resolve_clahe(ap, "off", record) is None
    assert len(capsys.readouterr().out.strip().splitlines()) == 1
    assert resolve_clahe(ap, "2.0", record) == Clahe(2.0)
    assert len(capsys.readouterr().out.strip().splitlines()) == 1
    assert resolve_clahe(ap, "2.0", None) == Clahe(2.0)
    assert len(capsys.readouterr().out.strip().splitlines()) == 1
    with pytest.raises(SystemExit):
        resolve_clahe(ap, "nonsense", None)
    with pytest.raises(SystemExit):
        resolve_clahe(ap, "checkpoint", {"clip_q8": 5})


@pytest.mark.parametrize("program", ["segment", "locate", "adapt", "test_run", "calibration_run", "morphometry_run"])
def test_every_program_takes_the_switch(program):
    import importlib
    mod = importlib.import_module("wtpse_hip." + program)
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0


def test_program_help_names_the_switch(capsys):
    from wtpse_hip import segment
    with pytest.raises(SystemExit):
        segment.main(["--help"])
    assert "--clahe" in capsys.readouterr().out


def test_checkpoint_entry(tmp_path):
    """The entry is a plain dict that torch.load(weights_only=True) reads; adapt's checkpoint carries its source's over and has none
    without; a checkpoint without the entry keeps exactly its keys."""
    from wtpse_hip.adapt import site_checkpoint
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    sds = [{"bn.running_mean": torch.zeros(2), "bn.running_var": torch.ones(2), "w": torch.arange(3.0)} for _ in CHECKPOINT_KEYS]
    site = dict(prior=16.0, images=1, source="x", layers={})
    plain = site_checkpoint(sds, {}, site)
    assert "clahe" not in plain and set(plain) == set(CHECKPOINT_KEYS) | {"site"}
    record = Clahe(2.5, (4, 8), 24, "rgb").record()
    with_entry = site_checkpoint(sds, {}, site, record)
    assert with_entry["clahe"] == record and with_entry["clahe"] is not record
    assert set(with_entry) == set(plain) | {"clahe"}
    path = str(tmp_path / "c.pth.tar")
    torch.save(with_entry, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert back["clahe"] == record and Clahe.from_record(back["clahe"]) == Clahe(2.5, (4, 8), 24, "rgb")
    assert torch.equal(back["model"]["w"], sds[0]["w"])


def test_train_run_sees_both_records():
    from wtpse_hip.trainer import _clahe_record_of

    class Feed:
        def __init__(self, clahe):
            self.clahe = clahe

        def clahe_record(self):
            return None if self.clahe is None else self.clahe.record()

        def triples(self):
            return iter(())

    from wtpse_hip.test_run import FundusTestBatches

    class Tree:
        phase, state, size, pools = "test", "prediction", 64, {}

        def keys(self):
            return []

    plain = FundusTestBatches(Tree(), 1, device="cpu")
    assert _clahe_record_of(plain) == (True, None) and _clahe_record_of(plain.triples) == (True, None)      # it applies none
    assert _clahe_record_of(None) == (False, None)
    assert _clahe_record_of([1, 2]) == (False, None)
    assert _clahe_record_of(lambda: []) == (False, None)
    assert _clahe_record_of(Feed(None)) == (True, None)
    assert _clahe_record_of(Feed(Clahe()).triples) == (True, Clahe().record())
