"""Amplitude mixing between source domains, host side: `amplitude_mix_host` (the float64 specification of csrc/spectrum.hip) against
the textbook form and its exact identities, `draw_mix`'s stream, the refusals, the host-only workspace query.  The helpers at the top
(noisy pictures, the float32 restatement) are shared with tests/test_amplitude_mix_gpu.py."""
import numpy as np
import pytest
import torch

from wtpse_hip.input_pipeline import AmplitudeMix, amplitude_mix_host, draw_mix, twiddle_table


def noisy_images(seed, N, S):
    """[N,S,S,3] uint8, seeded: even rows a smooth blob plus Gaussian noise of sigma 12, odd rows uniform-random pixels.  (The phase of
    a near-zero coefficient is ill-conditioned in any fp32 transform: flat synthetic pictures would test that, not the kernel.)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S] / float(S)
    out = []
    for n in range(N):
        if n % 2:
            out.append(rng.randint(0, 256, (S, S, 3)).astype(np.float64))
        else:
            cy, cx = rng.uniform(0.3, 0.7, 2)
            s = rng.uniform(0.1, 0.3)
            blob = 40 + 160 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            out.append(blob[..., None] * rng.uniform(0.5, 1.0, 3) + rng.normal(0, 12, (S, S, 3)))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


def window_mask(S, b):
    k = np.fft.fftfreq(S, 1.0 / S)
    inside = np.abs(k) <= b
    return inside[:, None] & inside[None, :]


def mix_float32(images_u8, partner, lam, b):
    """The specification restated in float32 with torch.fft on the CPU: what an fp32 transform of another make leaves of it.  Its
    deviation from the float64 specification is the yardstick the device's is measured with."""
    x = torch.from_numpy(np.array(images_u8)).to(torch.float32)
    S = x.shape[1]
    window = torch.from_numpy(window_mask(S, b))[..., None]
    out = x.clone()
    for n, p in enumerate(partner):
        if p < 0:
            continue
        F, G = torch.fft.fft2(x[n], dim=(0, 1)), torch.fft.fft2(x[int(p)], dim=(0, 1))
        aF, aG = F.abs(), G.abs()
        unit = torch.where(aF == 0, torch.ones_like(F), F / torch.where(aF == 0, torch.ones_like(aF), aF))
        D = torch.where(window, torch.tensor(np.float32(lam[n])) * (aG - aF) * unit, torch.zeros_like(F))
        out[n] = x[n] + torch.fft.ifft2(D, dim=(0, 1)).real
    return out.numpy()


def test_lam_zero_and_self_partner_return_the_input():
    img = noisy_images(1, 4, 32)
    for as_float in (False, True):
        want = img.astype(np.float64) if as_float else img
        assert np.array_equal(amplitude_mix_host(img, [1, 2, 3, 0], np.zeros(4), 16, as_float=as_float), want)
        assert np.array_equal(amplitude_mix_host(img, [0, 1, 2, 3], np.full(4, 0.7), 5, as_float=as_float), want)


@pytest.mark.parametrize("b", [0, 1, 3, 15, 16])
def test_spec_equals_textbook_form(b):
    """ifft2(((1 - lam) |F| + lam |G|) exp(i angle F)) on the window and F outside it, within 1e-9 at S = 32; and the spectrum of the
    float result equals F outside the window to 1e-9."""
    S, lam = 32, np.array([0.3, 1.0, 0.8])
    img = noisy_images(2 + b, 3, S)
    partner = [2, 0, 1]
    got = amplitude_mix_host(img, partner, lam, b, as_float=True)
    w = window_mask(S, b)[..., None]
    for n in range(3):
        F = np.fft.fft2(img[n].astype(np.float64), axes=(0, 1))
        G = np.fft.fft2(img[partner[n]].astype(np.float64), axes=(0, 1))
        mixed = ((1 - lam[n]) * np.abs(F) + lam[n] * np.abs(G)) * np.exp(1j * np.angle(F))
        full = np.fft.ifft2(np.where(w, mixed, F), axes=(0, 1))
        assert np.abs(full.imag).max() < 1e-9
        assert np.abs(got[n] - full.real).max() < 1e-9
        outside = np.broadcast_to(~w, F.shape)
        assert np.abs(np.fft.fft2(got[n], axes=(0, 1)) - F)[outside].max(initial=0.0) < 1e-9
    assert np.abs(got - img).max() > 1.0                       # something was mixed


def test_black_own_image_is_finite_and_real():
    img = noisy_images(3, 2, 32)
    img[0] = 0
    got = amplitude_mix_host(img, [1, -1], [0.6, 0.0], 4, as_float=True)
    assert got.dtype == np.float64 and np.all(np.isfinite(got))
    # F = 0, phase taken as 1: the result is lam |G| on zero phase
    G = np.fft.fft2(img[1].astype(np.float64), axes=(0, 1))
    want = np.fft.ifft2(np.where(window_mask(32, 4)[..., None], 0.6 * np.abs(G), 0.0), axes=(0, 1))
    assert np.abs(want.imag).max() < 1e-9 and np.abs(got[0] - want.real).max() < 1e-9
    assert np.array_equal(got[1], img[1].astype(np.float64))


def test_rows_without_partner_are_untouched_and_partners_are_read_from_the_input():
    img = noisy_images(4, 4, 32)
    got = amplitude_mix_host(img, [1, 2, -1, -1], [1.0, 1.0, 0.5, 0.5], 16)
    assert np.array_equal(got[2:], img[2:]) and not np.array_equal(got[0], img[0])
    # row 0 takes row 1's ORIGINAL amplitude, although row 1 is mixed itself
    alone = amplitude_mix_host(img, [1, -1, -1, -1], [1.0, 0.0, 0.0, 0.0], 16)
    assert np.array_equal(got[0], alone[0])


class CountingRng:
    """A RandomState that counts the numbers drawn from it."""

    def __init__(self, seed):
        self.rs, self.count = np.random.RandomState(seed), 0

    def _one(self, name, *a):
        self.count += 1
        return getattr(self.rs, name)(*a)

    def random_sample(self):
        return self._one("random_sample")

    def randint(self, n):
        return self._one("randint", n)

    def uniform(self, lo, hi):
        return self._one("uniform", lo, hi)


def test_draw_mix_stream():
    mix = AmplitudeMix()
    a = draw_mix(np.random.RandomState(9), 3, 4, mix)
    b = draw_mix(np.random.RandomState(9), 3, 4, mix)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].dtype == np.int32 and a[0].shape == (12,) and a[1].shape == (12,)
    fired = 0
    for seed in range(20):                                     # the partner always lies in another domain
        partner, lam = draw_mix(np.random.RandomState(seed), 3, 4, AmplitudeMix(p=0.7, alpha=0.5))
        for i, p in enumerate(partner):
            assert p == -1 or (0 <= p < 12 and p // 4 != i // 4)
            assert (lam[i] == 0.0) if p < 0 else (0.0 <= lam[i] < 0.5)
        fired += int((partner >= 0).sum())
    assert 100 < fired < 220                                   # 240 coins at p = 0.7
    for p, per_row in ((0.0, 1), (1.0, 4)):                    # a coin that does not fire draws nothing else
        rng = CountingRng(1)
        partner, _ = draw_mix(rng, 3, 4, AmplitudeMix(p=p))
        assert rng.count == per_row * 12 and bool((partner >= 0).all()) == (p == 1.0)
    two = set()
    for seed in range(10):                                     # two domains, one sample each: the partner is the other row
        partner, _ = draw_mix(np.random.RandomState(seed), 2, 1, AmplitudeMix(p=1.0))
        two.add(tuple(partner.tolist()))
    assert two == {(1, 0)}


def test_band():
    assert AmplitudeMix().band(256) == 25 and AmplitudeMix(window=0.5).band(64) == 32 and AmplitudeMix(window=0.0).band(64) == 0
    assert AmplitudeMix(window=0.49).band(32) == 15
    for bad in (dict(p=1.5), dict(alpha=-0.1), dict(window=0.6)):
        with pytest.raises(ValueError):
            AmplitudeMix(**bad)


def test_refusals(tmp_path):
    with pytest.raises(ValueError):
        draw_mix(np.random.RandomState(0), 1, 6, AmplitudeMix())
    with pytest.raises(ValueError):                            # S = 48: no power of two
        amplitude_mix_host(np.zeros((2, 48, 48, 3), np.uint8), [1, 0], [0.5, 0.5], 4)
    with pytest.raises(ValueError):
        amplitude_mix_host(np.zeros((2, 32, 32, 3), np.uint8), [1, 0], [0.5, 0.5], 17)
    with pytest.raises(ValueError):
        amplitude_mix_host(np.zeros((2, 32, 32, 3), np.uint8), [2, 0], [0.5, 0.5], 4)
    # one domain raises when the feed is built (before anything touches a device)
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.trainer import FundusBatches
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    one = [FundusTree(root, "train", (1,), size=64)]
    with pytest.raises(ValueError, match="two source domains"):
        FundusBatches(one, 2, "cuda", size=64, style=AmplitudeMix(), pipe=object())
    two = [FundusTree(root, "train", (i,), size=48) for i in (1, 2)]
    with pytest.raises(ValueError, match="power of two"):
        FundusBatches(two, 2, "cuda", size=48, style=AmplitudeMix(), pipe=object())


def test_twiddle_table():
    t = twiddle_table(64)
    assert t.dtype == np.float32 and t.shape == (64, 2)
    assert t[0].tolist() == [1.0, 0.0] and t[16].tolist() == [np.float32(np.cos(np.pi / 2)), -1.0]
    k = np.arange(64)
    assert np.array_equal(t[:, 0], np.cos(2 * np.pi * k / 64).astype(np.float32))


def test_workspace_query_answers_without_a_gpu():
    from wtpse_hip.lib import lib
    q = lambda *a: lib().query("wtpse_amix_workspace", *a)
    assert q(30, 256, 25) == 4 * 30 * 3 * 26 * 256
    assert q(1, 32, 0) == 4 * 3 * 32 and q(2, 512, 256) == 4 * 2 * 3 * 257 * 512
    for bad in ((0, 256, 4), (4, 48, 4), (4, 16, 4), (4, 1024, 4), (4, 64, 33), (4, 64, -1), (65535, 512, 256)):
        assert q(*bad) == -1, bad
    # the entry point refuses the same shapes before any launch (null pointers never reach a kernel either)
    assert lib().raw("wtpse_amplitude_mix")(0, 0, 0, 0, 0, 0, 0, 4, 48, 4, 0) == -1
    assert lib().raw("wtpse_amplitude_mix")(0, 0, 0, 0, 0, 0, 0, 4, 64, 4, 0) == -1
