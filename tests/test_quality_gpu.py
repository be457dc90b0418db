"""The device's image-quality stage (csrc/quality.hip) against `quality_host`, the integer specification: every comparison is
np.array_equal.  The tile of the apply kernel is 32 rows x 64 pixels with an 8-pixel halo: S = 20 lies inside one tile and clamps on
both sides at once, S = 67 has odd 201-byte rows (dword and byte accesses both run) and partial tiles, S = 128 has seams on both
axes."""
import random

import numpy as np
import pytest
import torch

from test_quality_cpu import K_STD10, params_row, pictures
from wtpse_hip import ops
from wtpse_hip.input_pipeline import (AmplitudeMix, Augment, DeviceInputPipeline, ImageQuality, draw, draw_augment, draw_mix,
                                      draw_quality, quality_host, quality_neutral)

pytestmark = pytest.mark.gpu

SEED = (0x1234ABCD << 32) | 0x9E3779B9
_PICTURES = {}


def batch(S, N):
    """The seeded batch of one size, made once and shared (nobody writes to it) -> (host, device)."""
    if (S, N) not in _PICTURES:
        img = pictures(200 + S, N, S)
        img.setflags(write=False)
        _PICTURES[(S, N)] = (img, torch.from_numpy(img.copy()).cuda())
    return _PICTURES[(S, N)]


def check(img, dimg, params, seed=SEED, pos=0, what=""):
    """Device against specification, bit for bit; the input buffer is left as it was.  -> the device's bytes."""
    params = np.stack(params)
    got = ops.image_quality(dimg, params, seed, pos).cpu().numpy()
    want = quality_host(img, params, seed, pos)
    bad = got != want
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        delta = got.astype(np.int16) - want.astype(np.int16)
        raise AssertionError("%s: %d bytes differ (per sample %s), the first at %s: device %d, specification %d; differences from %d to %d"
                             % (what, int(bad.sum()), bad.reshape(len(bad), -1).sum(1).tolist(), first, got[first], want[first],
                                delta.min(), delta.max()))
    assert np.array_equal(dimg.cpu().numpy(), img), "%s: the input was written" % what
    return got


ALL_ON = dict(a=300, c=330, beta=2500, k=K_STD10, sigma=1.2)
SINGLE = (dict(a=-256, sigma=1.5), dict(a=450, sigma=0.8), dict(c=180), dict(c=0), dict(beta=-5000), dict(k=K_STD10))


def test_smaller_than_a_tile():
    """S = 20, N = 2: radius 8 (sigma 2.0) reaches beyond the picture on both sides of most pixels."""
    img, dimg = batch(20, 2)
    got = check(img, dimg, [params_row(a=-256, sigma=2.0), params_row(**ALL_ON)], what="S=20")
    assert not np.array_equal(got, img)
    check(img, dimg, [params_row(a=512, sigma=2.0, k=30000), params_row(a=-256, sigma=0.5)], pos=999, what="S=20 sharpen")


def test_odd_side_mixed_batch():
    """S = 67, N = 3: one sample neutral, one blur only, one with everything on."""
    img, dimg = batch(67, 3)
    got = check(img, dimg, [params_row(), params_row(a=-256, sigma=1.0), params_row(**ALL_ON)], what="S=67 mixed")
    assert np.array_equal(got[0], img[0]) and not np.array_equal(got[1], img[1]) and not np.array_equal(got[2], img[2])
    # all neutral: a copy
    assert np.array_equal(check(img, dimg, list(quality_neutral(3)), what="S=67 neutral"), img)


@pytest.mark.parametrize("which", range(len(SINGLE)))
def test_odd_side_one_operation_alone(which):
    img, dimg = batch(67, 3)
    got = check(img, dimg, [params_row(**SINGLE[which])] * 3, pos=1 << 33, what="S=67 %r" % (SINGLE[which],))
    assert not np.array_equal(got, img)


def test_seams_between_tiles():
    """S = 128, N = 2: 2 x 4 tiles per sample; a wrong halo shows at a tile border."""
    img, dimg = batch(128, 2)
    check(img, dimg, [params_row(a=-256, sigma=2.0), params_row(**ALL_ON)], what="S=128")
    check(img, dimg, [params_row(a=512, sigma=1.7, c=512), params_row(c=400, beta=-3000, k=20000)], what="S=128 second")


@pytest.mark.parametrize("sigma", [2.0, 0.25])
def test_extremes(sigma):
    """All-0, all-255 and random pictures at the parameter bounds (B reaches 255 * 2^24: unsigned)."""
    S = 67
    img = np.concatenate([np.zeros((1, S, S, 3), np.uint8), np.full((1, S, S, 3), 255, np.uint8), batch(67, 3)[0][:1]])
    dimg = torch.from_numpy(img).cuda()
    for beta in (16320, -16320):
        check(img, dimg, [params_row(a=512, c=512, beta=beta, k=181000, sigma=sigma)] * 3, what="extremes beta=%d" % beta)
        check(img, dimg, [params_row(a=-256, c=512, beta=beta, k=181000, sigma=sigma)] * 3, what="extremes blur beta=%d" % beta)


def test_noise_positions():
    S = 67
    img, dimg = batch(S, 3)
    params = [params_row(k=40000), params_row(c=300), params_row(k=K_STD10, beta=100)]
    pos = (1 << 32) - 1000                                     # the counter's low word wraps inside sample 0
    got, nxt = ops.image_quality(dimg, np.stack(params), SEED, pos, want_pos=True)
    got = got.cpu().numpy()
    assert nxt == pos + 2 * S * S
    assert np.array_equal(got, quality_host(img, np.stack(params), SEED, pos))
    # sample 2 uses pos + S^2: the same bytes as that sample alone at that position
    alone = ops.image_quality(dimg[2:3].contiguous(), np.stack(params[2:]), SEED, pos + S * S).cpu().numpy()
    assert np.array_equal(alone[0], got[2])
    # a second call continues where the first stopped: other noise, the specification's at that position
    second = ops.image_quality(dimg, np.stack(params), SEED, nxt).cpu().numpy()
    assert np.array_equal(second, quality_host(img, np.stack(params), SEED, nxt))
    assert not np.array_equal(second[0], got[0]) and np.array_equal(second[1], got[1])
    # the same (seed, pos) twice gives the same bytes
    assert np.array_equal(ops.image_quality(dimg, np.stack(params), SEED, pos).cpu().numpy(), got)


def test_refusals_on_the_device():
    dimg = batch(20, 2)[1]
    with pytest.raises(ValueError):
        ops.image_quality(dimg, quality_neutral(3), 0, 0)
    with pytest.raises(ValueError):
        ops.image_quality(dimg, np.stack([params_row(a=600)] * 2), 0, 0)
    with pytest.raises(ValueError):
        ops.image_quality(dimg.to(torch.float32), quality_neutral(2), 0, 0)
    with pytest.raises(ValueError):
        ops.image_quality(torch.zeros((1, 20, 24, 3), dtype=torch.uint8, device="cuda"), quality_neutral(1), 0, 0)


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def to_u8(image):
    """The inverse of the normalisation used here: the pipeline hands out fp32 u / 127.5 - 1 for a byte u, so rint((v + 1) * 127.5)
    recovers u exactly (the fp32 error is below 1e-4 of a level).  [N,3,S,S] fp32 -> [N,S,S,3] uint8."""
    v = (image.cpu().numpy().astype(np.float64) + 1.0) * 127.5
    u = np.rint(v)
    assert np.abs(v - u).max() < 1e-4
    return np.ascontiguousarray(u.astype(np.uint8).transpose(0, 2, 3, 1))


def normalised(u8):
    out = u8.astype(np.float32)
    out /= 127.5
    out -= 1.0
    return out.transpose(0, 3, 1, 2)


def _inputs(S, N):
    rs = np.random.RandomState(31)
    sizes = [(S + 9, S + 4), (S, S), (2 * S - 3, S + 7), (S + 1, S + 12)][:N]
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    masks = [np.where(np.hypot(*(np.mgrid[0:h, 0:w] - np.array([h / 2, w / 2])[:, None, None])) < min(h, w) * 0.3, 0, 255).astype(np.uint8)
             for h, w in sizes]
    return imgs, masks


def test_pipeline_neutral_and_real_draws():
    S, N = 32, 4
    imgs, masks = _inputs(S, N)
    draws = [draw(random.Random(i), S) for i in range(N)]
    pipe = DeviceInputPipeline(S, "cuda", noise_seed=SEED)
    plain = pipe(imgs, masks, draws)
    neutral = pipe(imgs, masks, draws, quality_draws=quality_neutral(N))
    assert all(torch.equal(a, b) for a, b in zip(plain, neutral)) and pipe.quality_pos == 0
    params = draw_quality(np.random.RandomState(2), N, ImageQuality(p_focus=1, p_contrast=1, p_brightness=1, p_noise=1))
    params[1] = quality_neutral(1)[0]
    pipe.quality_pos = 777
    got = pipe(imgs, masks, draws, quality_draws=params)
    assert pipe.quality_pos == 777 + 3 * S * S
    assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])           # the masks are not touched
    want = quality_host(to_u8(plain[0]), params, SEED, 777)
    assert np.array_equal(got[0].cpu().numpy(), normalised(want))
    assert torch.equal(got[0][1], plain[0][1]) and not torch.equal(got[0][0], plain[0][0])
    # a second call continues the noise stream
    again = pipe(imgs, masks, draws, quality_draws=params)
    assert np.array_equal(again[0].cpu().numpy(), normalised(quality_host(to_u8(plain[0]), params, SEED, 777 + 3 * S * S)))


def test_pipeline_stage_order():
    """augment, mix, quality: the batch with all three equals the batch with the first two pushed through the specification."""
    S, N = 32, 4
    imgs, masks = _inputs(S, N)
    py_rng, np_rng = random.Random(5), np.random.RandomState(5)
    draws = [draw(py_rng, S) for _ in range(N)]
    aug_draws = [draw_augment(py_rng, np_rng, S, Augment()) for _ in range(N)]
    mix = AmplitudeMix(p=1.0)
    partner, lam = draw_mix(np_rng, 2, 2, mix)
    mix_draws = (partner, lam, mix.band(S))
    params = draw_quality(np_rng, N, ImageQuality(p_focus=1, p_contrast=1, p_brightness=1, p_noise=1))
    two = DeviceInputPipeline(S, "cuda", noise_seed=9)(imgs, masks, draws, aug_draws, mix_draws=mix_draws)
    three = DeviceInputPipeline(S, "cuda", noise_seed=9)(imgs, masks, draws, aug_draws, mix_draws=mix_draws, quality_draws=params)
    assert torch.equal(two[1], three[1]) and torch.equal(two[2], three[2])
    want = quality_host(to_u8(two[0]), params, 9, 0)
    assert np.array_equal(three[0].cpu().numpy(), normalised(want))
    assert not torch.equal(two[0], three[0])


# ---------------------------------------------------------------------------------------------------------------- the feed
def _sets(tmp_path):
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    return [FundusTree(root, "train", (i,), size=64) for i in (1, 2, 3)]


def test_feed_resumes_bitwise(tmp_path):
    """FundusBatches(quality=ImageQuality()) on a synthetic PNG tree: two batches, the state saved, one batch more; a fresh feed loaded
    from that state reproduces the third batch bit for bit."""
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)

    def feed():
        f = FundusBatches(sets, 6, "cuda", size=64, quality=ImageQuality())
        f.set_seed(3)
        return f

    a, py_a, np_a = feed(), random.Random(3), np.random.RandomState(3)
    first, second = a(py_a, np_a), a(py_a, np_a)
    saved = (a.state(), py_a.getstate(), np_a.get_state())
    assert saved[0]["quality_pos"] > 0 and saved[0]["quality_pos"] % (64 * 64) == 0
    third = a(py_a, np_a)
    b, py_b, np_b = feed(), random.Random(0), np.random.RandomState(0)
    b.load_state(saved[0])
    py_b.setstate(saved[1])
    np_b.set_state(saved[2])
    again = b(py_b, np_b)
    assert all(torch.equal(x, y) for x, y in zip(again, third))
    assert b.state() == a.state()
    # without the saved position the noise differs (when the third batch has any)
    if a.state()["quality_pos"] > saved[0]["quality_pos"]:
        c, py_c, np_c = feed(), random.Random(0), np.random.RandomState(0)
        c.load_state({"order": saved[0]["order"]})
        py_c.setstate(saved[1])
        np_c.set_state(saved[2])
        assert not torch.equal(c(py_c, np_c)[0], third[0])
    # the stage did something, to the pictures alone
    d = FundusBatches(sets, 6, "cuda", size=64)
    plain = d(random.Random(3), np.random.RandomState(3))
    assert torch.equal(plain[1], first[1]) and torch.equal(plain[2], first[2]) and not torch.equal(plain[0], first[0])
    assert not torch.equal(first[0], second[0])
