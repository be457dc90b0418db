"""JPEG compression augmentation, host side: `jpeg_host` (the integer specification of csrc/jpeg.hip) against Pillow's own round trip
— save as baseline JPEG, open, convert to RGB — with zero differing bytes, `jpeg_tables` against the tables of the file Pillow wrote,
the 32-bit claim and libjpeg's clamp window over the same inputs, `draw_jpeg`'s stream, the refusals, and the device quantiser's
reciprocal against the division, exhaustively.  `jpeg_pictures` is shared with tests/test_jpeg_gpu.py."""
import functools
import io

import numpy as np
import pytest
from PIL import Image

from wtpse_hip.input_pipeline import (JPEG_IDCT_WINDOW, JpegCompression, _check_jpeg_size, check_jpeg_params, draw_jpeg, jpeg_host,
                                      jpeg_is_neutral, jpeg_neutral, jpeg_reciprocals, jpeg_tables)

SIZES = (16, 32, 48, 64)
QUALITIES = (1, 5, 37, 50, 75, 95, 100)
KINDS = ("uniform noise", "smooth sinusoid with mild noise", "0/255 checkerboard", "random 0/255 per channel", "constant")


@functools.lru_cache(maxsize=None)
def jpeg_pictures(S):
    """[5,S,S,3] uint8, seeded, one picture of every kind of KINDS (read-only: shared)."""
    rng = np.random.RandomState(1000 + S)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    phase = np.array([0.0, 1.3, 2.9])
    smooth = 128 + 100 * np.sin(2 * np.pi * (xx[..., None] / 23.0 + yy[..., None] / 31.0) + phase) + rng.normal(0, 2.0, (S, S, 3))
    checker = np.repeat((((yy + xx) % 2) * 255)[..., None], 3, -1)
    out = np.stack([rng.randint(0, 256, (S, S, 3)), np.clip(np.rint(smooth), 0, 255), checker,
                    rng.randint(0, 2, (S, S, 3)) * 255, np.broadcast_to(np.array([200, 30, 90]), (S, S, 3))]).astype(np.uint8)
    out.setflags(write=False)
    return out


def pillow_roundtrip(picture, quality, mode):
    """-> (the bytes Pillow reads back from the baseline JPEG it writes, that file's quantisation tables [2,64] as Pillow reports them)."""
    buf = io.BytesIO()
    Image.fromarray(picture, "RGB").save(buf, "JPEG", quality=quality, subsampling={1: 0, 2: 2}[mode])
    im = Image.open(io.BytesIO(buf.getvalue()))
    q = np.array([im.quantization[0], im.quantization[1]], np.int64)
    return np.asarray(im.convert("RGB")), q


@functools.lru_cache(maxsize=None)
def against_pillow(S, mode):
    """Every quality and picture kind at one size and mode, once -> ({(quality, kind): differing bytes}, {quality: Pillow's tables},
    the ranges of every intermediate)."""
    pics = jpeg_pictures(S)
    N = len(pics)
    diffs, tabs, ranges = {}, {}, {}
    for q in QUALITIES:
        got = jpeg_host(pics, np.full(N, mode), np.broadcast_to(jpeg_tables(q), (N, 2, 64)), ranges=ranges)
        for i, kind in enumerate(KINDS):
            want, tabs[q] = pillow_roundtrip(pics[i], q, mode)
            diffs[(q, kind)] = int((got[i] != want).sum())
    return diffs, tabs, ranges


# ---------------------------------------------------------------------------------------------------------------- the Pillow pin
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("S", SIZES)
def test_equals_pillow_byte_for_byte(S, mode):
    diffs, tabs, _ = against_pillow(S, mode)
    assert len(diffs) == len(QUALITIES) * len(KINDS)
    bad = {k: v for k, v in diffs.items() if v}
    assert not bad, "bytes that differ from Pillow's round trip at S = %d, mode %d: %r" % (S, mode, bad)
    for q in QUALITIES:
        # Pillow (8.3 and later) reports a file's tables de-zigzagged: natural order, like jpeg_tables
        assert np.array_equal(tabs[q], jpeg_tables(q)), q


def test_tables():
    t = jpeg_tables(50)
    assert t.shape == (2, 64) and t.dtype == np.int32
    assert t[0, :8].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and t[1, :4].tolist() == [17, 18, 24, 47]      # scale 100: Annex K
    assert (jpeg_tables(100) == 1).all() and jpeg_tables(1).max() == 255 and jpeg_tables(1).min() >= 1
    for q in (0, 101, 50.5):
        with pytest.raises(ValueError):
            jpeg_tables(q)


# ---------------------------------------------------------------------------------------------------------------- 32 bits, the window
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("S", SIZES)
def test_intermediates_fit_32_bits_and_the_clamp_window(S, mode):
    _, _, ranges = against_pillow(S, mode)
    assert {"colour forward", "fdct rows", "fdct columns", "coefficient", "dequantised", "idct columns", "idct rows", "idct output",
            "colour back"} <= set(ranges)
    for name, (lo, hi) in ranges.items():
        assert -2 ** 31 <= lo and hi < 2 ** 31, (name, lo, hi)
    # the quantiser's reciprocal is exact for |c| <= 32767
    assert max(abs(v) for v in ranges["coefficient"]) <= 32767
    # libjpeg's range table clamps like a clip inside the window and wraps outside it
    lo, hi = ranges["idct output"]
    assert JPEG_IDCT_WINDOW[0] <= lo and hi <= JPEG_IDCT_WINDOW[1], (lo, hi)
    assert lo < 0 and hi > 255                                                # the clamp is exercised


# ---------------------------------------------------------------------------------------------------------------- the draws
class Spy:
    """A RandomState that lists the calls made on it."""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def random_sample(self):
        self.calls.append("random_sample")
        return self.rs.random_sample()

    def randint(self, lo, hi):
        self.calls.append(("randint", lo, hi))
        return self.rs.randint(lo, hi)


def test_draws_consume_the_documented_numbers():
    j = JpegCompression(p=0.6, quality=(20, 90), p_420=0.5)
    spy, ref = Spy(7), np.random.RandomState(7)
    mode, tables = draw_jpeg(spy, 40, j)
    assert mode.dtype == np.int32 and mode.shape == (40,) and tables.dtype == np.int32 and tables.shape == (40, 2, 64)
    calls = []
    for i in range(40):
        calls.append("random_sample")
        if ref.random_sample() < 0.6:
            calls.append(("randint", 20, 91))
            q = ref.randint(20, 91)
            calls.append("random_sample")
            want = 2 if ref.random_sample() < 0.5 else 1
            assert mode[i] == want and np.array_equal(tables[i], jpeg_tables(q))
        else:
            assert mode[i] == 0 and (tables[i] == 1).all()
    assert spy.calls == calls
    assert spy.rs.get_state()[1].tolist() == ref.get_state()[1].tolist() and spy.rs.get_state()[2] == ref.get_state()[2]
    assert set(mode.tolist()) == {0, 1, 2}


def test_draws_edge_probabilities():
    spy = Spy(1)
    mode, tables = draw_jpeg(spy, 9, JpegCompression(p=0))
    assert spy.calls == [] and not mode.any() and jpeg_is_neutral(mode).all()
    mode, tables = draw_jpeg(np.random.RandomState(1), 9, JpegCompression(p=1, quality=(37, 37), p_420=1))
    assert (mode == 2).all() and all(np.array_equal(t, jpeg_tables(37)) for t in tables)
    mode, _ = draw_jpeg(np.random.RandomState(1), 9, JpegCompression(p=1, p_420=0))
    assert (mode == 1).all()


def test_neutral_rows_are_copies():
    pics = jpeg_pictures(32)
    mode, tables = jpeg_neutral(5)
    assert np.array_equal(jpeg_host(pics, mode, tables), pics)
    mode[[1, 3]] = (1, 2)
    tables[[1, 3]] = jpeg_tables(20)
    tables[0] = 0                                                 # a neutral row's tables are not read
    got = jpeg_host(pics, mode, tables)
    for i in range(5):
        assert np.array_equal(got[i], pics[i]) == (i not in (1, 3)), i


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    mode, tables = jpeg_neutral(3)
    check_jpeg_params(mode, tables, 3)
    for bad in (3, -1):
        m = mode.copy()
        m[1] = bad
        with pytest.raises(ValueError):
            check_jpeg_params(m, tables, 3)
    for bad in (0, 256):
        t = tables.copy()
        t[2, 1, 63] = bad
        check_jpeg_params(mode, t, 3)                             # mode 0: not read
        with pytest.raises(ValueError):
            check_jpeg_params(np.array([0, 0, 1]), t, 3)
    with pytest.raises(ValueError):
        check_jpeg_params(mode, tables, 4)
    with pytest.raises(ValueError):
        check_jpeg_params(mode.astype(np.float64), tables, 3)
    with pytest.raises(ValueError):
        check_jpeg_params(mode, tables[:, :1], 3)
    for S in (8, 24, 40, 100, 0, 4112):
        with pytest.raises(ValueError):
            _check_jpeg_size(S)
    for S in (16, 256, 512):
        _check_jpeg_size(S)
    with pytest.raises(ValueError):
        jpeg_host(np.zeros((1, 24, 24, 3), np.uint8), [1], np.ones((1, 2, 64), np.int64))
    with pytest.raises(ValueError):
        jpeg_host(np.zeros((1, 16, 16, 3), np.float32), [1], np.ones((1, 2, 64), np.int64))
    for kw in (dict(quality=(0, 50)), dict(quality=(50, 101)), dict(quality=(60, 50)), dict(quality=(30.5, 90)), dict(quality=50),
               dict(p=1.5), dict(p=-0.1), dict(p_420=2)):
        with pytest.raises(ValueError):
            JpegCompression(**kw)
    j = JpegCompression()
    assert (j.p, j.quality, j.p_420) == (0.5, (30, 95), 0.75)
    assert JpegCompression(quality=(1, 100)).quality == (1, 100)


# ---------------------------------------------------------------------------------------------------------------- the reciprocal
def test_reciprocal_quantiser_equals_the_division_everywhere():
    """csrc/jpeg.hip divides by mulhi(|c| + (8 Q >> 1), ceil(2^32 / (8 Q))) in 32-bit integers: every |c| in 0 .. 32767 against every
    divisor 8 Q, Q in 1 .. 255."""
    Q = np.arange(1, 256, dtype=np.int64)
    M = jpeg_reciprocals(Q)
    assert M.dtype == np.int32 and M.min() > 0                    # positive int32: the signed multiply-high sees what is meant
    M, d = M.astype(np.int64)[None, :], 8 * Q[None, :]
    n = np.arange(32768, dtype=np.int64)[:, None] + (d >> 1)
    assert n.max() < 2 ** 31
    assert np.array_equal((n * M) >> 32, n // d)


def test_feed_refuses_a_side_that_is_no_multiple_of_16():
    from wtpse_hip.trainer import FundusBatches
    with pytest.raises(ValueError):
        FundusBatches([object()], 1, "cuda", size=72, jpeg=JpegCompression(), pipe=object())
    with pytest.raises(ValueError):
        FundusBatches([object()], 1, "cuda", size=64, jpeg="yes", pipe=object())
