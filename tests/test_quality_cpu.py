"""Image-quality augmentation, host side: `quality_taps`, `quality_host` (the integer specification of csrc/quality.hip) against its
exact identities, scipy's Gaussian filter and the 32-bit claim, the noise against an independent restatement of the Philox block,
`draw_quality`'s stream, `ImageQuality`'s bounds and the feed's state.  `pictures` and `params_row` are shared with
tests/test_quality_gpu.py."""
import random

import numpy as np
import pytest

from wtpse_hip.input_pipeline import (QUALITY_COLS, ImageQuality, draw_quality, quality_host, quality_neutral, quality_positions,
                                      quality_taps)

SIGMAS = (0.25, 0.4, 0.5, 0.8, 1.0, 1.5, 2.0)
K_STD10 = int(np.rint(10.0 * 256.0 * 4096.0 / np.sqrt(21845.0)))       # noise of 10 grey levels nominal: 70945


def pictures(seed, N, S):
    """[N,S,S,3] uint8, seeded: even rows uniform-random pixels, odd rows a smooth blob per channel."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S] / float(S)
    out = []
    for n in range(N):
        if n % 2 == 0:
            out.append(rng.randint(0, 256, (S, S, 3)).astype(np.float64))
        else:
            cy, cx = rng.uniform(0.3, 0.7, 2)
            blob = 30 + 200 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 0.2 ** 2))
            out.append(blob[..., None] * rng.uniform(0.5, 1.0, 3))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


def params_row(a=0, c=256, beta=0, k=0, sigma=0.0):
    row = np.zeros(QUALITY_COLS, np.int32)
    row[:4] = (a, c, beta, k)
    row[4:] = quality_taps(sigma)
    return row


# ---------------------------------------------------------------------------------------------------------------- taps
@pytest.mark.parametrize("sigma", SIGMAS)
def test_taps(sigma):
    w = quality_taps(sigma)
    assert w.dtype == np.int32 and w.shape == (9,)
    assert int(w[0]) + 2 * int(w[1:].sum()) == 4096
    assert (w >= 0).all() and (np.diff(w) <= 0).all()
    radius = min(8, int(4 * sigma + 0.5))
    assert radius >= 1 and not w[radius + 1:].any()
    # the rounded taps are the normalised Gaussian's, to half a unit (w[0] collects the rounding of the others)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 * x * x / sigma ** 2)
    phi /= phi.sum()
    assert np.abs(w[1:radius + 1] - 4096 * phi[radius + 1:]).max() <= 0.5
    assert abs(w[0] - 4096 * phi[radius]) <= 0.5 * 2 * radius


def test_taps_identity():
    ident = [4096] + [0] * 8
    for sigma in (0.0, -1.0, 0.1):                      # 0.1: radius int(0.9) = 0
        assert quality_taps(sigma).tolist() == ident
    assert quality_taps(2.0)[7] > 0 and quality_taps(5.0)[8] > 0          # 5.0: the radius stops at 8


# ---------------------------------------------------------------------------------------------------------------- the specification
def test_neutral_and_zero_amount_return_the_input():
    img = pictures(1, 3, 23)
    assert np.array_equal(quality_host(img, quality_neutral(3)), img)
    p = np.stack([params_row(a=0, sigma=s) for s in (0.5, 1.0, 2.0)])
    assert np.array_equal(quality_host(img, p), img)
    # identity taps with any amount: the blur is the picture itself
    p = np.stack([params_row(a=a, sigma=0.0) for a in (-256, 300, 512)])
    assert np.array_equal(quality_host(img, p), img)


def test_constant_picture_stays_constant():
    img = np.empty((3, 19, 19, 3), np.uint8)
    img[0], img[1], img[2] = 0, 255, 77
    for a in (-256, 300, 512):
        for sigma in (0.25, 2.0):
            p = np.stack([params_row(a=a, sigma=sigma)] * 3)
            assert np.array_equal(quality_host(img, p), img), (a, sigma)


def test_zero_contrast_is_the_mean():
    img = pictures(2, 2, 21)
    out = quality_host(img, np.stack([params_row(c=0), params_row(c=0, a=200, sigma=1.0)]))
    for n in range(2):
        cnt = img[n].size
        m8 = (256 * int(img[n].astype(np.int64).sum()) + cnt // 2) // cnt
        assert (out[n] == ((m8 + 128) >> 8)).all()


def test_contrast_and_brightness_by_hand():
    img = pictures(3, 1, 9)
    cnt = img.size
    m8 = (256 * int(img.astype(np.int64).sum()) + cnt // 2) // cnt
    x8 = img[0].astype(np.int64) << 8
    for c, beta in ((300, 0), (100, -4000), (256, 16320), (512, -16320)):
        t = m8 + ((c * (x8 - m8) + 128) >> 8) + beta
        want = np.clip((t + 128) >> 8, 0, 255).astype(np.uint8)
        assert np.array_equal(quality_host(img, params_row(c=c, beta=beta)[None])[0], want)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_blur_against_scipy(sigma):
    """a = -256 is scipy's gaussian_filter(mode="nearest"), truncated at the same radius, within 1 grey level (Q12 taps, one rounding
    to Q8 and one to the byte; the prototype measured 0.58), on a random and a smooth 67 x 67 picture."""
    from scipy.ndimage import gaussian_filter
    img = pictures(4, 2, 67)
    radius = min(8, int(4 * sigma + 0.5))
    out = quality_host(img, np.stack([params_row(a=-256, sigma=sigma)] * 2))
    ref = gaussian_filter(img.astype(np.float64), sigma=(0, sigma, sigma, 0), mode="nearest", truncate=radius / sigma)
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print("sigma %.2f: %.3f grey levels from scipy" % (sigma, err))
    assert err <= 1.0
    assert (sigma < 0.5) or not np.array_equal(out[0], img[0])      # (0.25 moves 2 / 4096 of a neighbour: below half a level)


def test_sharpen_is_unsharp_masking():
    """x + amount (x - blur(x)) with scipy's blur, within 1 + amount grey levels (the blur's level of error, amplified) before the clip."""
    from scipy.ndimage import gaussian_filter
    img = pictures(5, 2, 41)
    out = quality_host(img, np.stack([params_row(a=384, sigma=1.0)] * 2))
    x = img.astype(np.float64)
    ref = np.clip(x + 1.5 * (x - gaussian_filter(x, sigma=(0, 1.0, 1.0, 0), mode="nearest", truncate=4.0)), 0, 255)
    assert np.abs(out - ref).max() <= 2.5


def test_nothing_leaves_32_bits():
    """At the parameter bounds, on all-0, all-255 and random pictures: B fits unsigned 32 bits, everything else signed 32 bits."""
    S = 33
    img = np.concatenate([np.zeros((1, S, S, 3), np.uint8), np.full((1, S, S, 3), 255, np.uint8), pictures(6, 1, S)])
    checker = ((np.indices((S, S)).sum(0) % 2) * 255).astype(np.uint8)                 # the largest x8 - b8
    img = np.concatenate([img, np.repeat(checker[None, :, :, None], 3, 3)])
    ranges = {}
    for a in (-256, 512):
        for c in (0, 512):
            for beta in (-16320, 16320):
                for sigma in (0.25, 2.0):
                    quality_host(img, np.stack([params_row(a, c, beta, 181000, sigma)] * 4), seed=11, pos=5, ranges=ranges)
    assert set(ranges) >= {"H", "B", "s", "t", "u", "a*(x8-b8)+128", "c*(s-m8)+128", "k*g+2048", "u+128"}
    for name, (lo, hi) in ranges.items():
        if name in ("H", "B"):
            assert 0 <= lo and hi < 2 ** 32, (name, lo, hi)
        else:
            assert -2 ** 31 <= lo and hi < 2 ** 31, (name, lo, hi)
    assert ranges["B"][1] == 255 << 24 and ranges["B"][1] >= 2 ** 31                   # B does need the unsigned range


def test_params_are_checked():
    img = pictures(7, 1, 8)
    for bad in (dict(a=-257), dict(a=513), dict(c=-1), dict(c=513), dict(beta=16321), dict(beta=-16321), dict(k=-1), dict(k=181001)):
        with pytest.raises(ValueError):
            quality_host(img, params_row(**bad)[None])
    row = params_row(a=-256, sigma=1.0)
    row[4] += 1                                          # the taps no longer sum to 4096
    with pytest.raises(ValueError):
        quality_host(img, row[None])
    with pytest.raises(ValueError):
        quality_host(img, quality_neutral(2))
    with pytest.raises(ValueError):
        quality_host(img.astype(np.float32), quality_neutral(1))


# ---------------------------------------------------------------------------------------------------------------- noise
def philox_words(seed, ctr):
    """Words 0 .. 2 of the Philox4x32-10 block with key `seed` and counter (ctr lo, ctr hi, 0, 1), restated after philox_uniform
    of tests/test_augment_cpu.py — whose counter ends in (0, 0)."""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c = [ctr & MASK, (ctr >> 32) & MASK, 0, 1]
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c[:3]


def noise_by_hand(S, seed, pos, k):
    """((k g + 2048) >> 12) [S,S,3] from the restated block."""
    out = np.empty((S, S, 3), np.int64)
    for y in range(S):
        for x in range(S):
            for ch, word in enumerate(philox_words(seed, pos + y * S + x)):
                g = sum((word >> s) & 255 for s in (0, 8, 16, 24)) - 510
                out[y, x, ch] = (k * g + 2048) >> 12
    return out


def test_noise_block_and_statistics():
    S, seed, pos = 64, (0xDEADBEEF << 32) | 12345, (1 << 32) - 100               # the counter's low word wraps inside the picture
    assert K_STD10 == 70945
    img = np.full((1, S, S, 3), 128, np.uint8)
    out = quality_host(img, params_row(k=K_STD10)[None], seed=seed, pos=pos)
    u = (128 << 8) + noise_by_hand(S, seed, pos, K_STD10)
    assert np.array_equal(out[0], np.clip((u + 128) >> 8, 0, 255).astype(np.uint8))
    d = out[0].astype(np.float64) - 128.0
    print("noise: mean %.4f, std %.4f" % (d.mean(), d.std()))
    assert abs(d.mean()) <= 0.2
    assert abs(d.std() - 10.0) <= 0.5
    assert not np.array_equal(out[0, :, :, 0], out[0, :, :, 1]) and not np.array_equal(out[0, :, :, 1], out[0, :, :, 2])
    assert not np.array_equal(out[0, :, :, 0], out[0, :, :, 2])
    # another seed and another position are other noise; k = 0 consumes nothing
    assert not np.array_equal(out, quality_host(img, params_row(k=K_STD10)[None], seed=seed + 1, pos=pos))
    assert not np.array_equal(out, quality_host(img, params_row(k=K_STD10)[None], seed=seed, pos=pos + 1))


def test_noise_positions():
    S = 10
    p = np.stack([params_row(k=5000), params_row(), params_row(k=9000), params_row(c=300)])
    table, nxt = quality_positions(p, S, 7)
    assert table.dtype == np.uint64 and table.tolist() == [7, 107, 107, 207] and nxt == 207
    img = pictures(8, 4, S)
    out = quality_host(img, p, seed=3, pos=7)
    assert np.array_equal(out[2], quality_host(img[2:3], p[2:3], seed=3, pos=7 + S * S)[0])
    assert np.array_equal(out[0], quality_host(img[0:1], p[0:1], seed=3, pos=7)[0])
    assert np.array_equal(out[1], img[1])


# ---------------------------------------------------------------------------------------------------------------- draws
class LoggingRng:
    """A RandomState that logs what is drawn from it."""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def random_sample(self):
        self.log.append(("random_sample",))
        return self.rs.random_sample()

    def uniform(self, lo, hi):
        self.log.append(("uniform", lo, hi))
        return self.rs.uniform(lo, hi)


def test_draw_quality_order_and_values():
    q = ImageQuality(p_focus=1.0, p_contrast=1.0, p_brightness=1.0, p_noise=1.0)
    rng, twin = LoggingRng(4), np.random.RandomState(4)
    params = draw_quality(rng, 6, q)
    assert params.dtype == np.int32 and params.shape == (6, 13)
    log, kinds = list(rng.log), set()
    for i in range(6):
        assert twin.random_sample() < 1.0 and log.pop(0) == ("random_sample",)
        blur = twin.random_sample() < 0.5
        assert log.pop(0) == ("random_sample",)
        kinds.add(blur)
        if blur:
            assert log.pop(0) == ("uniform", 0.25, 1.5)
            sigma, a = twin.uniform(0.25, 1.5), -256
        else:
            assert log.pop(0) == ("uniform", 0.5, 1.5) and log.pop(0) == ("uniform", 0.5, 2.0)
            sigma = twin.uniform(0.5, 1.5)
            a = int(np.rint(256 * twin.uniform(0.5, 2.0)))
        assert log.pop(0) == ("random_sample",) and log.pop(0) == ("uniform", 0.75, 1.25)
        twin.random_sample()
        c = int(np.rint(256 * twin.uniform(0.75, 1.25)))
        assert log.pop(0) == ("random_sample",) and log.pop(0) == ("uniform", -0.1, 0.1)
        twin.random_sample()
        beta = int(np.rint(65280 * twin.uniform(-0.1, 0.1)))
        assert log.pop(0) == ("random_sample",) and log.pop(0) == ("uniform", 0.0, 0.05)
        twin.random_sample()
        k = int(np.rint(twin.uniform(0.0, 0.05) * 65280 * 4096 / np.sqrt(21845.0)))
        assert params[i].tolist() == [a, c, beta, k] + quality_taps(sigma).tolist(), i
    assert not log and kinds == {True, False}
    assert rng.rs.random_sample() == twin.random_sample()


def test_disabled_operations_draw_nothing():
    rng = LoggingRng(1)
    params = draw_quality(rng, 5, ImageQuality(p_focus=0, p_contrast=0, p_brightness=0, p_noise=0))
    assert rng.log == [] and np.array_equal(params, quality_neutral(5))
    assert rng.rs.random_sample() == np.random.RandomState(1).random_sample()
    # one operation on: its coin, and its parameter when the coin fires; nothing for the others
    for kw, col in ((dict(p_contrast=1.0), 1), (dict(p_brightness=1.0), 2), (dict(p_noise=1.0), 3)):
        off = dict(p_focus=0, p_contrast=0, p_brightness=0, p_noise=0)
        off.update(kw)
        rng = LoggingRng(2)
        params = draw_quality(rng, 4, ImageQuality(**off))
        assert [e[0] for e in rng.log] == ["random_sample", "uniform"] * 4
        changed = [j for j in range(13) if not np.array_equal(params[:, j], quality_neutral(4)[:, j])]
        assert changed == [col]
    # a coin that does not fire draws nothing else: p tiny
    rng = LoggingRng(3)
    params = draw_quality(rng, 4, ImageQuality(p_focus=1e-12, p_contrast=1e-12, p_brightness=1e-12, p_noise=1e-12))
    assert rng.log == [("random_sample",)] * 16 and np.array_equal(params, quality_neutral(4))


def test_draws_stay_inside_their_bounds():
    q = ImageQuality(p_focus=1, blur_sigma=(0.0, 2.0), sharpen_sigma=(0.0, 2.0), sharpen_amount=(0.0, 2.0), p_contrast=1,
                     contrast=(0.0, 2.0), p_brightness=1, brightness=0.25, p_noise=1, noise=0.1)
    params = draw_quality(np.random.RandomState(5), 400, q).astype(np.int64)
    a, c, beta, k = params[:, 0], params[:, 1], params[:, 2], params[:, 3]
    assert a.min() >= -256 and a.max() <= 512 and (a == -256).any() and (a > 0).any()
    assert c.min() >= 0 and c.max() <= 512 and np.abs(beta).max() <= 16320 and k.min() >= 0 and k.max() <= 181000
    assert k.max() > 150000 and np.abs(beta).max() > 15000                          # the bounds are nearly reached
    assert (params[:, 4:] >= 0).all() and (params[:, 4] + 2 * params[:, 5:].sum(1) == 4096).all()
    # the largest k a draw can give lies inside the bound
    assert np.rint(0.1 * 65280 * 4096 / np.sqrt(21845.0)) <= 181000
    quality_host(np.zeros((400, 4, 4, 3), np.uint8), params)                          # accepted as they are


def test_image_quality_raises_on_every_bound():
    ImageQuality(blur_sigma=(2.0, 2.0), sharpen_amount=(2.0, 2.0), contrast=(0.0, 2.0), brightness=0.25, noise=0.1)
    for bad in (dict(p_focus=1.1), dict(p_contrast=-0.1), dict(p_brightness=2), dict(p_noise=-1), dict(blur_sigma=(0.25, 2.1)),
                dict(blur_sigma=(-0.1, 1.0)), dict(blur_sigma=(1.5, 0.5)), dict(sharpen_sigma=(0.5, 2.5)), dict(sharpen_amount=(0.5, 2.1)),
                dict(sharpen_amount=(-1, 1)), dict(contrast=(0.5, 2.1)), dict(contrast=(-0.1, 1.0)), dict(brightness=0.26),
                dict(brightness=-0.1), dict(noise=0.11), dict(noise=-0.01), dict(contrast=1.0)):
        with pytest.raises(ValueError):
            ImageQuality(**bad)


# ---------------------------------------------------------------------------------------------------------------- the feed
class RecordingPipe:
    """Stands in for DeviceInputPipeline: keeps the arguments of every call."""

    def __init__(self):
        self.noise_seed, self.noise_pos, self.quality_pos, self.calls = 0, 0, 0, []

    def __call__(self, images, masks, draws, *args, **kw):
        self.calls.append((len(images), args, kw))
        return None


def _sets(tmp_path, size=64):
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    return [FundusTree(root, "train", (i,), size=size) for i in (1, 2, 3)]


def test_feed_draws_come_last_and_state(tmp_path):
    from wtpse_hip.input_pipeline import AmplitudeMix, Augment, draw_mix
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)
    q = ImageQuality()
    for augment in (None, Augment()):
        for style in (None, AmplitudeMix()):
            plain_pipe, pipe = RecordingPipe(), RecordingPipe()
            plain = FundusBatches(sets, 6, "cuda", size=64, augment=augment, style=style, pipe=plain_pipe)
            feed = FundusBatches(sets, 6, "cuda", size=64, augment=augment, style=style, quality=q, pipe=pipe)
            py_p, np_p = random.Random(3), np.random.RandomState(3)
            py_q, np_q = random.Random(3), np.random.RandomState(3)
            for _ in range(2):
                plain(py_p, np_p)
                feed(py_q, np_q)
                # the stage's draws come after all the others: the plain feed's generator stands where they start
                want = draw_quality(np_p, 6, q)
                n, args, kw = pipe.calls[-1]
                assert n == 6 and np.array_equal(kw["quality_draws"], want)
                assert py_p.getstate() == py_q.getstate()
                assert all(np.array_equal(x, y) for x, y in zip(np_p.get_state()[1:3], np_q.get_state()[1:3]))
                # without the stage the pipeline is called as it always was
                _, pargs, pkw = plain_pipe.calls[-1]
                assert "quality_draws" not in pkw and len(pargs) == len(args)
                assert set(kw) - {"quality_draws"} == set(pkw)
                if style is not None:
                    assert np.array_equal(kw["mix_draws"][0], pkw["mix_draws"][0])
            assert ("quality_pos" in feed.state()) and ("quality_pos" not in plain.state())
            assert ("noise_pos" in feed.state()) == (augment is not None)


def test_feed_without_the_stage_consumes_what_it_did(tmp_path):
    """quality=None: the generators stand where a hand count of the draws puts them (one index per sample, one crop draw each)."""
    from wtpse_hip.fundus_data import multi_batch
    from wtpse_hip.input_pipeline import draw
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)
    pipe = RecordingPipe()
    feed = FundusBatches(sets, 6, "cuda", size=64, pipe=pipe)
    py_a, np_a = random.Random(9), np.random.RandomState(9)
    feed(py_a, np_a)
    py_b, np_b = random.Random(9), np.random.RandomState(9)
    order = [0, 1, 2]
    py_b.shuffle(order)
    images, _ = multi_batch([sets[i] for i in order], 2, np_b)
    for _ in images:
        draw(py_b, 64)
    assert py_a.getstate() == py_b.getstate() and np_a.random_sample() == np_b.random_sample()
    assert pipe.calls[0][1] == () and pipe.calls[0][2] == {}
    assert feed.state() == {"order": order}


def test_feed_state_round_trip(tmp_path):
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)
    feed = FundusBatches(sets, 6, "cuda", size=64, quality=ImageQuality(), pipe=RecordingPipe())
    feed.pipe.quality_pos = 12345
    state = feed.state()
    assert state["quality_pos"] == 12345 and "noise_pos" not in state
    other = FundusBatches(sets, 6, "cuda", size=64, quality=ImageQuality(), pipe=RecordingPipe())
    other.load_state(state)
    assert other.pipe.quality_pos == 12345
    other.load_state({"order": [2, 0, 1]})               # a state saved before the field existed
    assert other.pipe.quality_pos == 0 and other.order == [2, 0, 1]
    other.set_seed(77)
    assert other.pipe.noise_seed == 77                   # the stage's noise runs on the seed set_seed already sets
    with pytest.raises(ValueError):
        FundusBatches(sets, 6, "cuda", size=1024, quality=ImageQuality(), pipe=RecordingPipe())


def test_entry_points_refuse_bad_shapes_without_a_gpu():
    from wtpse_hip.lib import lib
    assert lib().raw("wtpse_quality_sums")(0, 0, 2, 64, 0) == -1
    assert lib().raw("wtpse_quality_apply")(0, 0, 0, 0, 0, 0, 2, 64, 0) == -1
    assert len(lib().protos["wtpse_quality_apply"]) == 9
