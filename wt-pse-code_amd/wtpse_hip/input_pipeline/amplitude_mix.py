"""Optional amplitude-mixing stage (`AmplitudeMix`, `draw_mix`, `amplitude_mix_host`; csrc/spectrum.hip): a sample keeps the phase of its
2-D spectrum and moves the amplitude of a low-frequency window towards that of a sample from another source domain of the same
batch (FDA; FedDG's continuous frequency space interpolation; FACT's amplitude mix — PAPERS.md), after the augmentations and before
the normalisation.  This stage has no counterpart in the reference: `amplitude_mix_host` (float64) is its specification, and the
device stage is held to it within the error of an fp32 transform (tests/test_amplitude_mix_gpu.py).
"""
import math

import numpy as np

MIX_SIZES = (32, 64, 128, 256, 512)


def _check_mix_size(S):
    if S not in MIX_SIZES:
        raise ValueError("amplitude mixing takes square samples whose side is a power of two from 32 to 512, got %r" % (S,))


class AmplitudeMix:
    """The amplitude-mixing stage's parameters.  p: the probability that a sample is mixed; alpha: its weight lam is drawn from
    uniform(0, alpha) — lam = 0 leaves the amplitude alone, lam = 1 replaces it with the partner's; window: half width of the mixed
    square of frequencies as a fraction of the side, `band(S)` = min(S // 2, floor(window * S)) (0: the mean colour alone; 0.5: the
    whole spectrum)."""

    def __init__(self, p=0.5, alpha=1.0, window=0.1):
        if not (0.0 <= p <= 1.0 and 0.0 <= alpha <= 1.0 and 0.0 <= window <= 0.5):
            raise ValueError("AmplitudeMix needs 0 <= p <= 1, 0 <= alpha <= 1 and 0 <= window <= 0.5, got %r, %r, %r" % (p, alpha, window))
        self.p, self.alpha, self.window = float(p), float(alpha), float(window)

    def band(self, size):
        return min(int(size) // 2, int(math.floor(self.window * int(size))))


def draw_mix(np_rng, n_domains, per_domain, mix):
    """The stage's draws for one domain-major batch of n_domains * per_domain samples from the run's numpy generator, sample by
    sample in batch order: a coin `random_sample() < p`; if it fires, another domain of the batch (`randint(n_domains - 1)`, skipping
    the sample's own), a sample of that domain (`randint(per_domain)`) and lam = `uniform(0, alpha)`; a coin that does not fire draws
    nothing else.  -> (partner [N] int32, -1: leave the sample alone; lam [N] float64)."""
    n_domains, per_domain = int(n_domains), int(per_domain)
    if n_domains < 2:
        raise ValueError("amplitude mixing needs samples of at least two source domains in a batch, got %d" % n_domains)
    N = n_domains * per_domain
    partner, lam = np.full(N, -1, np.int32), np.zeros(N, np.float64)
    for i in range(N):
        if np_rng.random_sample() < mix.p:
            own = i // per_domain
            other = int(np_rng.randint(n_domains - 1))
            other += other >= own
            partner[i] = other * per_domain + int(np_rng.randint(per_domain))
            lam[i] = np_rng.uniform(0, mix.alpha)
    return partner, lam


def check_mix_params(partner, lam, b, N, S):
    """-> (partner [N] int64, lam [N] float64, b int) after the checks the stage rests on (ValueError otherwise): a side the
    transform takes, partner indices in -1 .. N - 1, finite weights, the band within 0 .. S / 2."""
    _check_mix_size(S)
    partner, lam = np.asarray(partner), np.asarray(lam, np.float64)
    if partner.shape != (N,) or lam.shape != (N,) or partner.dtype.kind not in "iu":
        raise ValueError("partner must be [%d] integers and lam [%d] floats, got %s %s and %s" % (N, N, partner.shape, partner.dtype, lam.shape))
    if N and (partner.min() < -1 or partner.max() >= N):
        raise ValueError("partner indices must lie in -1 .. %d" % (N - 1))
    if not np.all(np.isfinite(lam)):
        raise ValueError("lam must be finite")
    if not 0 <= int(b) <= S // 2:
        raise ValueError("the band b must lie in 0 .. S/2 = %d, got %r" % (S // 2, b))
    return partner.astype(np.int64), lam, int(b)


def _check_mix_args(images_u8, partner, lam, b):
    img = np.asarray(images_u8)
    if img.ndim != 4 or img.shape[1] != img.shape[2] or img.shape[3] != 3 or img.dtype != np.uint8:
        raise ValueError("amplitude mixing takes a [N,S,S,3] uint8 batch, got %s %s" % (img.shape, img.dtype))
    return (img,) + check_mix_params(partner, lam, b, *img.shape[:2])


def amplitude_mix_host(images_u8, partner, lam, b, as_float=False):
    """The specification of the device stage in numpy float64: images [N,S,S,3] uint8, partner [N] int (-1: leave the row alone),
    lam [N] float, b = half width of the window.  Per row with a partner and per channel, x = the row's own channel, g = the
    partner's (always read from the input, never from a mixed row), F = fft2(x), G = fft2(g); with signed frequencies k in
    [-S/2, S/2 - 1], inside the window |k_y| <= b and |k_x| <= b (b = S/2: everything, the Nyquist lines included)
        D = lam (|G| - |F|) F / |F|      (F / |F| := 1 where |F| = 0)
    and D = 0 outside; y = x + real(ifft2(D)): the amplitude (1 - lam) |F| + lam |G| on the phase of F, written as a correction
    to x.  -> rint(clip(y, 0, 255)) as uint8, or y itself (float64) with as_float."""
    img, partner, lam, b = _check_mix_args(images_u8, partner, lam, b)
    N, S = img.shape[:2]
    k = np.fft.fftfreq(S, 1.0 / S)                       # signed: 0 .. S/2 - 1, -S/2 .. -1
    inside = np.abs(k) <= b
    window = inside[:, None] & inside[None, :]
    out = img.astype(np.float64)
    for n in range(N):
        if partner[n] < 0:
            continue
        F = np.fft.fft2(img[n].astype(np.float64), axes=(0, 1))
        G = np.fft.fft2(img[partner[n]].astype(np.float64), axes=(0, 1))
        aF, aG = np.abs(F), np.abs(G)
        unit = np.where(aF == 0.0, 1.0, F / np.where(aF == 0.0, 1.0, aF))
        D = np.where(window[..., None], lam[n] * (aG - aF) * unit, 0.0)
        out[n] = out[n] + np.real(np.fft.ifft2(D, axes=(0, 1)))
    if as_float:
        return out
    return np.rint(np.clip(out, 0.0, 255.0)).astype(np.uint8)


def twiddle_table(S):
    """exp(-2 pi i t / S), t = 0 .. S - 1, computed in float64 and rounded once -> [S,2] float32 = (cos, -sin)."""
    t = np.arange(int(S), dtype=np.float64) * (2.0 * np.pi / int(S))
    return np.stack([np.cos(t), -np.sin(t)], 1).astype(np.float32)
