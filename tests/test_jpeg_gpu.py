"""The device's JPEG compression stage (csrc/jpeg.hip) against `jpeg_host`, the integer specification that tests/test_jpeg_cpu.py pins
to Pillow: every comparison is torch.equal on bytes.  The kernels' tiles are 64 x 32 pixels (jpeg_apply_k) and 64 x 64 pixels
(jpeg_chroma_k, 4:2:0 only): S = 16 is one MCU (every upsampling edge case at once), S = 32 has first / last columns and rows next to
interior ones, S = 48 one MCU with neighbours on all eight sides, and S = 80 and 144 are multiples of 16 but of neither tile in either
direction (80 = 64 + 16 = 2 * 32 + 16, 144 = 2 * 64 + 16 = 4 * 32 + 16): partial tiles, and chroma neighbours across tile seams."""
import random

import numpy as np
import pytest
import torch

from test_jpeg_cpu import KINDS, jpeg_pictures
from test_quality_gpu import _inputs, normalised, to_u8
from wtpse_hip import ops
from wtpse_hip.input_pipeline import (AmplitudeMix, AppearanceNets, Augment, Clahe, DeviceInputPipeline, ImageQuality, JpegCompression,
                                      draw, draw_jpeg, draw_quality, jpeg_host, jpeg_neutral, jpeg_tables)

pytestmark = pytest.mark.gpu

MODES = np.array([0, 1, 2, 2, 1])
QUALITIES = (None, 1, 37, 75, 100)


def mixed_tables():
    return np.stack([np.ones((2, 64), np.int32) if q is None else jpeg_tables(q) for q in QUALITIES])


def check(img, mode, tables, what=""):
    """Device against specification, byte for byte; the input buffer is left as it was.  -> the device's bytes (a tensor)."""
    img = np.ascontiguousarray(img)
    dimg = torch.from_numpy(img.copy()).cuda()
    got = ops.jpeg_roundtrip(dimg, mode, tables)
    want = torch.from_numpy(jpeg_host(img, mode, tables))
    if not torch.equal(got.cpu(), want):
        g, w = got.cpu().numpy(), want.numpy()
        bad = g != w
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d bytes differ (per sample %s), the first at %s: device %d, specification %d"
                             % (what, int(bad.sum()), bad.reshape(len(bad), -1).sum(1).tolist(), first, g[first], w[first]))
    assert np.array_equal(dimg.cpu().numpy(), img), "%s: the input was written" % what
    return got


@pytest.mark.parametrize("S", [16, 32, 48, 80, 144])
def test_smallest_shapes_that_can_go_wrong(S):
    """N = 5 with modes (0, 1, 2, 2, 1) and qualities (-, 1, 37, 75, 100); the five picture kinds rotate through the five slots, so
    every kind meets every mode and quality."""
    pics = jpeg_pictures(S)
    assert len(pics) == len(KINDS) == 5
    tables = mixed_tables()
    for shift in range(5):
        img = np.roll(pics, shift, 0)
        got = check(img, MODES, tables, what="S=%d shift=%d" % (S, shift)).cpu().numpy()
        assert np.array_equal(got[0], img[0])                                   # mode 0: a byte copy
        if shift == 0:
            assert all(not np.array_equal(got[i], img[i]) for i in (1, 2, 3))   # quality 1, 37, 75 change noise, sinusoid, checkerboard


@pytest.mark.parametrize("entry", [1, 255])
def test_custom_tables(entry):
    """All-ones (nothing is quantised away: what is left is the transforms' and the colour conversions' rounding) and all-255 tables,
    in both modes."""
    pics = jpeg_pictures(48)
    tables = np.full((5, 2, 64), entry, np.int32)
    check(pics, np.array([1, 2, 1, 2, 1]), tables, what="tables of %d" % entry)
    check(pics, np.array([2, 1, 2, 1, 2]), tables, what="tables of %d, modes swapped" % entry)


def test_independent_of_batch_position():
    pics = jpeg_pictures(80)
    tables = mixed_tables()
    got = check(pics, MODES, tables, what="in order")
    perm = np.array([3, 0, 4, 2, 1])
    moved = check(pics[perm], MODES[perm], tables[perm], what="permuted")
    assert torch.equal(moved, got[torch.from_numpy(perm).cuda()])


def test_neutral_batch_and_neutral_rows():
    pics = jpeg_pictures(32)
    dimg = torch.from_numpy(pics.copy()).cuda()
    mode, tables = jpeg_neutral(5)
    assert ops.jpeg_roundtrip(dimg, mode, tables) is dimg                       # nothing is launched
    mode[2] = 2
    tables[2] = jpeg_tables(10)
    got = ops.jpeg_roundtrip(dimg, mode, tables)
    assert got is not dimg and torch.equal(got.cpu(), torch.from_numpy(jpeg_host(pics, mode, tables)))
    for i in range(5):
        assert torch.equal(got[i], dimg[i]) == (i != 2), i


def test_refusals_on_the_device():
    dimg = torch.from_numpy(jpeg_pictures(32).copy()).cuda()
    mode, tables = np.array([1, 2, 1, 2, 1]), np.ones((5, 2, 64), np.int32)
    bad_tables = tables.copy()
    bad_tables[3, 0, 5] = 256
    for args in ((dimg, mode[:4], tables), (dimg, np.array([1, 2, 3, 0, 0]), tables), (dimg, mode, bad_tables),
                 (dimg.to(torch.float32), mode, tables), (dimg[:, :, :, :2], mode, tables), (dimg.cpu(), mode, tables),
                 (torch.zeros((5, 24, 24, 3), dtype=torch.uint8, device="cuda"), mode, tables),
                 (torch.zeros((5, 32, 16, 3), dtype=torch.uint8, device="cuda"), mode, tables)):
        with pytest.raises(ValueError):
            ops.jpeg_roundtrip(*args)
    # the kernels load and store 16 bytes at a time: a contiguous view one byte into a buffer is refused, not misread
    shifted = torch.zeros(dimg.numel() + 1, dtype=torch.uint8, device="cuda")[1:].view(dimg.shape)
    assert shifted.is_contiguous()
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip(shifted, mode, tables)


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def test_pipeline_stage_off():
    S, N = 32, 4
    imgs, masks = _inputs(S, N)
    draws = [draw(random.Random(i), S) for i in range(N)]
    pipe = DeviceInputPipeline(S, "cuda", noise_seed=3)
    plain = pipe(imgs, masks, draws)
    off = pipe(imgs, masks, draws, jpeg_draws=None)
    neutral = pipe(imgs, masks, draws, jpeg_draws=jpeg_neutral(N))
    assert all(torch.equal(a, b) for a, b in zip(plain, off)) and all(torch.equal(a, b) for a, b in zip(plain, neutral))


def test_pipeline_stage_sits_between_image_quality_and_clahe(monkeypatch):
    """The tensor ops.jpeg_roundtrip receives is the image-quality stage's output; the specification applied to it, then CLAHE and the
    normalisation, is the pipeline's own output."""
    S, N = 32, 4
    imgs, masks = _inputs(S, N)
    draws = [draw(random.Random(i), S) for i in range(N)]
    np_rng = np.random.RandomState(4)
    params = draw_quality(np_rng, N, ImageQuality(p_focus=1, p_contrast=1, p_brightness=1, p_noise=1))
    mode, tables = draw_jpeg(np_rng, N, JpegCompression(p=1, quality=(5, 60), p_420=0.5))
    mode[:3] = (2, 0, 1)
    clahe = Clahe(tiles=(2, 2))
    seen = []
    real = ops.jpeg_roundtrip

    def spy(img, m, t):
        seen.append((img.clone(), np.array(m), np.array(t)))
        return real(img, m, t)

    monkeypatch.setattr(ops, "jpeg_roundtrip", spy)
    got = DeviceInputPipeline(S, "cuda", noise_seed=9)(imgs, masks, draws, quality_draws=params, clahe=clahe, jpeg_draws=(mode, tables))
    assert len(seen) == 1 and np.array_equal(seen[0][1], mode) and np.array_equal(seen[0][2], tables)
    before = DeviceInputPipeline(S, "cuda", noise_seed=9)(imgs, masks, draws, quality_draws=params)
    assert len(seen) == 1                                                       # jpeg_draws=None: no call
    assert np.array_equal(seen[0][0].cpu().numpy(), to_u8(before[0]))           # in: what the image-quality stage wrote
    want = torch.from_numpy(jpeg_host(seen[0][0].cpu().numpy(), mode, tables)).cuda()
    assert not torch.equal(want, seen[0][0]) and torch.equal(want[1], seen[0][0][1])
    assert np.array_equal(got[0].cpu().numpy(), normalised(ops.clahe(want, clahe).cpu().numpy()))       # out: into CLAHE
    assert torch.equal(got[1], before[1]) and torch.equal(got[2], before[2])    # the masks are not touched
    with pytest.raises(ValueError):
        DeviceInputPipeline(40, "cuda")(imgs, masks, [draw(random.Random(i), 40) for i in range(N)], jpeg_draws=jpeg_neutral(N))


# ---------------------------------------------------------------------------------------------------------------- the feed
def _sets(tmp_path):
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    return [FundusTree(root, "train", (i,), size=64) for i in (1, 2, 3)]


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


class Recorder:
    """A DeviceInputPipeline that lists the draws it is called with."""

    def __init__(self, pipe):
        self.pipe, self.calls = pipe, []

    def __getattr__(self, name):
        return getattr(self.pipe, name)

    def __call__(self, images, masks, draws, aug_draws=None, **kw):
        self.calls.append(dict(kw, draws=draws, aug_draws=aug_draws))
        return self.pipe(images, masks, draws, aug_draws, **kw)


def test_feed_draw_order_and_resume(tmp_path):
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)
    # ---- p = 0: the batches and the generators are those of a feed without the stage
    runs = []
    for jpeg in (None, JpegCompression(p=0)):
        f, py, rs = FundusBatches(sets, 6, "cuda", size=64, jpeg=jpeg), random.Random(3), np.random.RandomState(3)
        runs.append(([f(py, rs), f(py, rs)], py.getstate(), rs.get_state(), f.state()))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert all(torch.equal(a, b) for a, b in zip(x, y))
    assert runs[0][1] == runs[1][1] and _same(list(runs[0][2]), list(runs[1][2])) and runs[0][3] == runs[1][3]

    # ---- p = 1: a feed restored from state() reproduces the next batch bit for bit
    def feed():
        return FundusBatches(sets, 6, "cuda", size=64, jpeg=JpegCompression(p=1, quality=(5, 40)))

    a, py_a, np_a = feed(), random.Random(3), np.random.RandomState(3)
    first, second = a(py_a, np_a), a(py_a, np_a)
    saved = (a.state(), py_a.getstate(), np_a.get_state())
    assert set(saved[0]) == {"order"}                                           # no feed state of the stage's own
    third = a(py_a, np_a)
    b, py_b, np_b = feed(), random.Random(0), np.random.RandomState(0)
    b.load_state(saved[0])
    py_b.setstate(saved[1])
    np_b.set_state(saved[2])
    assert all(torch.equal(x, y) for x, y in zip(b(py_b, np_b), third))
    # the stage did something, to the pictures alone
    plain = runs[0][0][0]
    assert torch.equal(plain[1], first[1]) and torch.equal(plain[2], first[2]) and not torch.equal(plain[0], first[0])

    # ---- every other stage on: the JPEG stage's draws come behind theirs and leave them as they were
    recs, clahe = [], Clahe(tiles=(4, 4))
    for jpeg in (None, JpegCompression(p=0.7)):
        f = FundusBatches(sets, 6, "cuda", size=64, augment=Augment(), style=AmplitudeMix(p=0.6), quality=ImageQuality(),
                          clahe=clahe, appearance=AppearanceNets(p=0.8), jpeg=jpeg)
        f.pipe = Recorder(f.pipe)
        py, rs = random.Random(11), np.random.RandomState(11)
        f(py, rs)
        recs.append((f.pipe.calls[0], py.getstate()))
    off, on = recs[0][0], recs[1][0]
    assert "jpeg_draws" not in off and set(on) == set(off) | {"jpeg_draws"}
    for key in off:
        assert _same(off[key], on[key]) or off[key] is on[key], key
    assert recs[0][1] == recs[1][1]
    assert on["jpeg_draws"][0].any()
