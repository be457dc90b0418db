"""The augmentation stage's host side (no GPU): `draw_augment` + `augment_host` against tests/golden/augment.npz — the reference's
own classes (tools/make_golden_augment.py) — bit for bit, the number of draws, the Philox uniform's definition, and the feed state
that carries the noise position."""
import os
import random

import numpy as np
import pytest

from wtpse_hip.input_pipeline import Augment, augment_host, draw_augment, gaussian_weights

NAMES = ("rotate", "flip", "elastic", "salt_pepper", "light", "erase")


def fixture_cases(golden_dir):
    """-> [(S, tag, Augment, py_seed, np_seed, input image, input mask, noise or None, out image, out mask, next pair)]"""
    g = np.load(os.path.join(golden_dir, "augment.npz"))
    assert tuple(g["names"]) == NAMES
    out = []
    for S in (int(s) for s in g["sizes"]):
        for tag in g["s%d_cases" % S]:
            key = "s%d_%s_" % (S, tag)
            py_seed, np_seed, _, degree = (int(v) for v in g[key + "seeds"])
            aug = Augment(rotate_degree=degree or "random", **dict(zip(NAMES, (bool(b) for b in g[key + "enabled"]))))
            noise = g[key + "noise"] if key + "noise" in g.files else None
            out.append((S, str(tag), aug, py_seed, np_seed, g["s%d_img" % S], g["s%d_mask" % S], noise, g[key + "img"], g[key + "mask"],
                        g[key + "next"]))
    return out


# ---- the Philox4x32-10 uniform of wtpse_uniform_f64, restated: number g of stream `seed` -> a double in [0, 1)
def philox_uniform(seed, pos, n):
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    out = np.empty(n, np.float64)
    for i in range(n):
        g = pos + i
        ctr = g >> 1
        c = [ctr & MASK, (ctr >> 32) & MASK, 0, 0]
        k0, k1 = seed & MASK, (seed >> 32) & MASK
        for _ in range(10):
            p0, p1 = M0 * c[0], M1 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        a, b = (c[2], c[3]) if g & 1 else (c[0], c[1])
        out[i] = ((a >> 5) * 67108864 + (b >> 6)) / 9007199254740992.0
    return out


def test_host_equals_reference_fixture(golden_dir):
    cases = fixture_cases(golden_dir)
    assert len(cases) == 20
    seen = set()
    for S, tag, aug, py_seed, np_seed, img, mask, noise, want_img, want_mask, nxt in cases:
        py_rng, np_rng = random.Random(py_seed), np.random.RandomState(np_seed)
        d = draw_augment(py_rng, np_rng, S, aug)
        assert d["elastic"] == (noise is not None), (S, tag)
        got_img, got_mask = augment_host(img, mask, d, noise)
        assert got_img.dtype == np.uint8 and got_mask.dtype == np.uint8
        assert np.array_equal(got_img, want_img), (S, tag, int((got_img != want_img).sum()))
        assert np.array_equal(got_mask, want_mask), (S, tag, int((got_mask != want_mask).sum()))
        # the generators stand where the reference's stand after the chain: the same number of draws was made
        assert py_rng.random() == nxt[0] and np_rng.random_sample() == nxt[1], (S, tag)
        if tag == "none":
            assert np.array_equal(got_img, img) and np.array_equal(got_mask, mask)
        seen.add(("k", d["k"]) if aug.rotate and not aug.flip else None)
        seen.add(("sp", d["sp"][0]) if d["sp"] is not None else None)
        seen.add(("flip", d["flip_lr"], d["flip_tb"]))
    # every branch is in the fixture: three quarter turns (360 degrees = none), salt and pepper, each flip alone and both
    assert {("k", 1), ("k", 2), ("k", 3), ("k", 0), ("sp", 0), ("sp", 1), ("flip", True, True), ("flip", True, False),
            ("flip", False, True)} <= seen


def test_per_sample_degree_draws_after_the_coin():
    """rotate_degree="random" (not the reference's behaviour: it draws one angle per run): randint(1, 4) right after a coin that
    fired, nothing after one that did not."""
    aug = Augment(flip=False, elastic=False, salt_pepper=False, light=False, erase=False)
    ks = set()
    for seed in range(40):
        rng, twin = random.Random(seed), random.Random(seed)
        d = draw_augment(rng, np.random.RandomState(0), 64, aug)
        if twin.random() > 0.5:
            assert d["k"] == twin.randint(1, 4) % 4
        else:
            assert d["k"] == 0
        assert rng.random() == twin.random()
        ks.add(d["k"])
    assert ks == {0, 1, 2, 3}
    with pytest.raises(ValueError):
        Augment(rotate_degree=45)


def test_disabled_transforms_draw_nothing():
    off = Augment(rotate=False, flip=False, elastic=False, salt_pepper=False, light=False, erase=False)
    py_rng, np_rng = random.Random(3), np.random.RandomState(3)
    d = draw_augment(py_rng, np_rng, 64, off)
    assert d == {"k": 0, "flip_lr": False, "flip_tb": False, "elastic": False, "sp": None, "lut": None, "rect": None}
    assert py_rng.random() == random.Random(3).random() and np_rng.random_sample() == np.random.RandomState(3).random_sample()


def test_gaussian_weights_and_blur_are_scipys():
    """The 1-D kernel and the summation order are scipy's: the numpy restatement equals scipy.ndimage.gaussian_filter bitwise."""
    from scipy.ndimage import gaussian_filter
    from wtpse_hip.input_pipeline import elastic_displacement
    w, radius = gaussian_weights(256 * 0.08)
    assert radius == 82 and len(w) == 83
    assert gaussian_weights(50 * 0.08)[1] == 16
    S = 50
    u = np.random.RandomState(1).rand(2, S, S)
    want = np.stack([gaussian_filter(u[i] * 2 - 1, S * 0.08, mode="constant", cval=0) * (S * 2) for i in range(2)])
    assert np.array_equal(elastic_displacement(u, S), want)


def test_philox_uniform_restatement():
    u = philox_uniform(1234, 0, 600)
    assert u.min() >= 0.0 and u.max() < 1.0 and 0.4 < u.mean() < 0.6 and len(np.unique(u)) == 600
    # position-addressable: a number depends on (seed, position) only, odd positions included
    assert np.array_equal(philox_uniform(1234, 37, 100), u[37:137])
    assert np.array_equal(philox_uniform(1234, (1 << 40) + 3, 4)[1:], philox_uniform(1234, (1 << 40) + 4, 3))
    assert not np.array_equal(philox_uniform(1235, 0, 8), u[:8])


class _Pool:
    """A stand-in dataset: FundusBatches only asks for len() and get()."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def get(self, index, rng):
        raise AssertionError("no batch is drawn here")


class _Pipe:
    """What FundusBatches keeps of its pipeline between calls (the real one refuses to exist without a GPU)."""
    noise_seed = noise_pos = 0


def _feed(augment):
    from wtpse_hip.trainer import FundusBatches
    return FundusBatches([_Pool(3), _Pool(4), _Pool(3)], 6, "cpu", size=64, augment=augment, pipe=_Pipe())


def test_feed_state_carries_the_noise_position():
    plain = _feed(None)
    assert plain.state() == {"order": [0, 1, 2]}                 # without augmentations the feed state is what it was
    a = _feed(Augment())
    a.order, a.pipe.noise_pos = [2, 0, 1], 5 * 2 * 64 * 64
    a.set_seed(77)
    assert a.pipe.noise_seed == 77
    st = a.state()
    assert st == {"order": [2, 0, 1], "noise_pos": 40960}
    b = _feed(Augment())
    b.load_state(st)
    assert b.order == [2, 0, 1] and b.pipe.noise_pos == 40960 and b.state() == st
    # a state written before the position existed loads, with position 0
    b.load_state({"order": [1, 2, 0]})
    assert b.order == [1, 2, 0] and b.pipe.noise_pos == 0
