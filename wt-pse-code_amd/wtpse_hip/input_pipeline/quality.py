"""Optional image-quality stage (`ImageQuality`, `draw_quality`, `quality_host`; csrc/quality.hip): Gaussian blur or unsharp masking,
contrast about the sample's mean, a brightness shift and dense noise — the image-quality transforms of the stacked-transformation
recipe (BigAug) — after amplitude mixing and before the normalisation.  No counterpart in the reference either: the
stage is defined in fixed point, `quality_host` (numpy int64) is its specification and the device equals it byte for byte
(tests/test_quality_gpu.py).
"""
import math

import numpy as np

QUALITY_RADIUS = 8                      # the largest blur radius: taps w[0..8]
QUALITY_COLS = 4 + QUALITY_RADIUS + 1    # a parameter row: a, c, beta, k, w[0..8]
QUALITY_MAX_SIZE = 512                   # 3 * 512^2 * 255 < 2^32: a sample's byte sum fits 32 bits
QUALITY_A, QUALITY_C, QUALITY_BETA, QUALITY_K = (-256, 512), (0, 512), (-16320, 16320), (0, 181000)
_NOISE_STD = math.sqrt(21845.0)          # of g = b0 + b1 + b2 + b3 - 510 over the four bytes of a uniform 32-bit word: 147.80


def _check_quality_size(S):
    if not 1 <= int(S) <= QUALITY_MAX_SIZE:
        raise ValueError("the image-quality stage takes samples of side 1 .. %d, got %r" % (QUALITY_MAX_SIZE, S))


def quality_taps(sigma):
    """Gaussian taps in Q12 -> [9] int32 with w[0] + 2 (w[1] + .. + w[8]) = 4096: radius = min(8, int(4 sigma + 0.5)), phi =
    exp(-0.5 x^2 / sigma^2) normalised in float64 over -radius .. radius, w[j] = rint(4096 phi_j) for j >= 1, w[0] = what is left of
    4096, w[j] = 0 beyond the radius.  sigma <= 0 (and every sigma whose radius is 0): the identity [4096, 0, ...]."""
    sigma = float(sigma)
    w = np.zeros(QUALITY_RADIUS + 1, np.int64)
    radius = min(QUALITY_RADIUS, int(4.0 * sigma + 0.5)) if sigma > 0.0 else 0
    if radius > 0:
        x = np.arange(-radius, radius + 1, dtype=np.float64)
        phi = np.exp(-0.5 * x * x / (sigma * sigma))
        phi = phi / phi.sum()
        w[1:radius + 1] = np.rint(4096.0 * phi[radius + 1:]).astype(np.int64)
    w[0] = 4096 - 2 * int(w[1:].sum())
    return w.astype(np.int32)


def quality_neutral(n):
    """The parameter table [n,13] int32 that leaves every sample alone: a = 0, c = 256, beta = 0, k = 0, w = [4096, 0, ...]."""
    params = np.zeros((int(n), QUALITY_COLS), np.int32)
    params[:, 1] = 256
    params[:, 4] = 4096
    return params


def _range2(name, value, lo, hi):
    try:
        a, b = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError("ImageQuality: %s must be a (low, high) pair, got %r" % (name, value))
    if not lo <= a <= b <= hi:
        raise ValueError("ImageQuality: %s must satisfy %g <= low <= high <= %g, got %r" % (name, lo, hi, value))
    return a, b


class ImageQuality:
    """The image-quality stage's parameters: what differs between two fundus cameras besides geometry and illumination — the
    sharpness, contrast, brightness and noise transforms of the stacked-transformation recipe (BigAug).

    p_focus: the probability that a sample is blurred or sharpened (an even coin picks which).  Blur: the picture is replaced by
    its Gaussian blur, sigma = uniform(*blur_sigma) pixels.  Sharpen: unsharp masking, x + amount (x - blur(x)) with sigma =
    uniform(*sharpen_sigma) and amount = uniform(*sharpen_amount).  sigma <= 2.0 (the taps reach 8 pixels), amount <= 2.0.
    p_contrast: s -> mean + c (s - mean) about the sample's own mean over all channels, c = uniform(*contrast) within [0, 2].
    p_brightness: a shift by uniform(-brightness, brightness) of the full range 255; brightness <= 0.25.
    p_noise: additive noise per pixel and channel, mean 0, standard deviation uniform(0, noise) of 255; noise <= 0.1.  (The sum of
    four uniform bytes: bell-shaped, bounded by 3.45 standard deviations.)
    A probability of 0 disables an operation, and the operation then draws nothing."""

    def __init__(self, p_focus=0.5, blur_sigma=(0.25, 1.5), sharpen_sigma=(0.5, 1.5), sharpen_amount=(0.5, 2.0),
                 p_contrast=0.5, contrast=(0.75, 1.25), p_brightness=0.5, brightness=0.1, p_noise=0.5, noise=0.05):
        for name, p in (("p_focus", p_focus), ("p_contrast", p_contrast), ("p_brightness", p_brightness), ("p_noise", p_noise)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError("ImageQuality: %s must lie in [0, 1], got %r" % (name, p))
        self.p_focus, self.p_contrast = float(p_focus), float(p_contrast)
        self.p_brightness, self.p_noise = float(p_brightness), float(p_noise)
        self.blur_sigma = _range2("blur_sigma", blur_sigma, 0.0, 2.0)
        self.sharpen_sigma = _range2("sharpen_sigma", sharpen_sigma, 0.0, 2.0)
        self.sharpen_amount = _range2("sharpen_amount", sharpen_amount, 0.0, 2.0)
        self.contrast = _range2("contrast", contrast, 0.0, 2.0)
        if not 0.0 <= float(brightness) <= 0.25:
            raise ValueError("ImageQuality: brightness must lie in [0, 0.25] (of 255), got %r" % (brightness,))
        if not 0.0 <= float(noise) <= 0.1:
            raise ValueError("ImageQuality: noise must lie in [0, 0.1] (of 255), got %r" % (noise,))
        self.brightness, self.noise = float(brightness), float(noise)


def draw_quality(np_rng, n, q):
    """The stage's draws for a batch of n samples from the run's numpy generator, sample by sample in batch order.  Focus: a coin
    `random_sample() < p_focus`; if it fires, `random_sample() < 0.5` picks blur (sigma = `uniform(*blur_sigma)`, a = -256),
    otherwise sharpen (sigma = `uniform(*sharpen_sigma)`, a = rint(256 `uniform(*sharpen_amount)`)).  Then the contrast coin with
    c = rint(256 `uniform(*contrast)`), the brightness coin with beta = rint(65280 `uniform(-brightness, brightness)`), the noise coin
    with k = rint(`uniform(0, noise)` * 65280 * 4096 / sqrt(21845)).  A coin that does not fire draws nothing else; an operation
    whose probability is 0 draws nothing at all.  -> the parameter table [n,13] int32 (a, c, beta, k, w[0..8])."""
    params = quality_neutral(n)
    for i in range(int(n)):
        if q.p_focus > 0.0 and np_rng.random_sample() < q.p_focus:
            if np_rng.random_sample() < 0.5:
                sigma, a = np_rng.uniform(*q.blur_sigma), -256
            else:
                sigma = np_rng.uniform(*q.sharpen_sigma)
                a = int(np.rint(256.0 * np_rng.uniform(*q.sharpen_amount)))
            params[i, 0] = a
            params[i, 4:] = quality_taps(sigma)
        if q.p_contrast > 0.0 and np_rng.random_sample() < q.p_contrast:
            params[i, 1] = int(np.rint(256.0 * np_rng.uniform(*q.contrast)))
        if q.p_brightness > 0.0 and np_rng.random_sample() < q.p_brightness:
            params[i, 2] = int(np.rint(65280.0 * np_rng.uniform(-q.brightness, q.brightness)))
        if q.p_noise > 0.0 and np_rng.random_sample() < q.p_noise:
            params[i, 3] = int(np.rint(np_rng.uniform(0.0, q.noise) * 65280.0 * 4096.0 / _NOISE_STD))
    return params


def check_quality_params(params, N):
    """-> params as [N,13] int64 after the range checks the device arithmetic rests on (ValueError otherwise)."""
    p = np.asarray(params)
    if p.shape != (N, QUALITY_COLS) or p.dtype.kind not in "iu":
        raise ValueError("image quality: params must be [%d,%d] integers, got %s %s" % (N, QUALITY_COLS, p.shape, p.dtype))
    p = p.astype(np.int64)
    for col, name, (lo, hi) in ((0, "a", QUALITY_A), (1, "c", QUALITY_C), (2, "beta", QUALITY_BETA), (3, "k", QUALITY_K)):
        if N and (p[:, col].min() < lo or p[:, col].max() > hi):
            raise ValueError("image quality: %s must lie in %d .. %d" % (name, lo, hi))
    if N and (p[:, 4:].min() < 0 or np.any(p[:, 4] + 2 * p[:, 5:].sum(1) != 4096)):
        raise ValueError("image quality: the taps must be non-negative with w[0] + 2 (w[1] + .. + w[8]) = 4096")
    return p


def quality_is_neutral(params):
    """[N] bool: the rows the stage copies (a = 0, c = 256, beta = 0, k = 0)."""
    p = np.asarray(params)
    return (p[:, 0] == 0) & (p[:, 1] == 256) & (p[:, 2] == 0) & (p[:, 3] == 0)


def quality_positions(params, S, pos):
    """The base position of every sample in the noise stream: a sample with k > 0 consumes S * S positions (one Philox block per
    pixel), in batch order, starting at `pos`.  -> ([N] uint64, the position behind the batch)."""
    noisy = np.asarray(params)[:, 3] > 0
    before = np.concatenate([[0], np.cumsum(noisy)[:-1]]) if len(noisy) else np.zeros(0)
    table = np.array([int(pos) + int(b) * S * S for b in before], np.uint64)
    return table, int(pos) + int(noisy.sum()) * S * S


def _philox_words(ctr, seed):
    """Words 0, 1, 2 of the Philox4x32-10 blocks with counters (ctr lo, ctr hi, 0, 1) and key (seed lo, seed hi); ctr: uint64 array.
    -> [..., 3] int64."""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    ctr = np.asarray(ctr, np.uint64)
    m, s32 = np.uint64(MASK), np.uint64(32)
    c0, c1 = ctr & m, ctr >> s32
    c2, c3 = np.zeros_like(ctr), np.ones_like(ctr)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2               # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2], -1).astype(np.int64)


def quality_noise_host(S, seed, pos):
    """g [S,S,3] int64 of one sample whose noise starts at stream position `pos`: the four bytes of word `channel` of block
    pos + y S + x, summed, minus 510 (mean 0, variance 4 (256^2 - 1) / 12 = 21845)."""
    ctr = np.uint64(int(pos)) + np.arange(S * S, dtype=np.uint64)
    words = _philox_words(ctr, seed)
    g = (words & 255) + ((words >> 8) & 255) + ((words >> 16) & 255) + ((words >> 24) & 255) - 510
    return g.reshape(S, S, 3)


def quality_host(images_u8, params, seed=0, pos=0, ranges=None):
    """The specification of the device stage (csrc/quality.hip) in numpy int64, which the device equals byte for byte: images
    [N,S,S,3] uint8, params [N,13] integers (a, c, beta, k, w[0..8]: `draw_quality`, `quality_taps`), the noise stream `seed` from
    position `pos` on (`quality_positions`).  Per pixel and channel, x the input byte, `>>` the arithmetic (floor) shift:
        H[y][x] = sum_{j=-8..8} w[|j|] X[y][clamp(x + j)]            (Q12, edge replicated)
        B[y][x] = sum_{j=-8..8} w[|j|] H[clamp(y + j)][x]            (Q24: up to 255 * 2^24, unsigned 32 bits)
        b8 = (B + 32768) >> 16;  x8 = x << 8
        s  = x8 + ((a (x8 - b8) + 128) >> 8)                         (a = -256: the blur; 0: x; > 0: unsharp masking)
        m8 = (256 SUM + n // 2) // n, SUM = the sum of the n = 3 S S bytes of the sample
        t  = m8 + ((c (s - m8) + 128) >> 8) + beta
        u  = t + ((k g + 2048) >> 12) when k > 0                     (g: `quality_noise_host`)
        out = clip((u + 128) >> 8, 0, 255)
    ranges: a dict that receives name -> (min, max) of every intermediate over the batch (the 32-bit claim is tested with it)."""
    img = np.asarray(images_u8)
    if img.ndim != 4 or img.shape[1] != img.shape[2] or img.shape[3] != 3 or img.dtype != np.uint8:
        raise ValueError("image quality takes a [N,S,S,3] uint8 batch, got %s %s" % (img.shape, img.dtype))
    N, S = img.shape[:2]
    if not 1 <= S <= QUALITY_MAX_SIZE:
        raise ValueError("image quality takes samples of side 1 .. %d, got %d" % (QUALITY_MAX_SIZE, S))
    p = check_quality_params(params, N)
    table, _ = quality_positions(p, S, pos)

    def note(name, v):
        if ranges is not None:
            lo, hi = int(np.min(v)), int(np.max(v))
            old = ranges.get(name, (lo, hi))
            ranges[name] = (min(lo, old[0]), max(hi, old[1]))

    out = np.empty_like(img)
    idx = np.clip(np.arange(S)[:, None] + np.arange(-QUALITY_RADIUS, QUALITY_RADIUS + 1)[None, :], 0, S - 1)    # [S,17]
    for n in range(N):
        a, c, beta, k = (int(v) for v in p[n, :4])
        x = img[n].astype(np.int64)
        x8 = x << 8
        if a != 0:
            w = p[n, 4 + np.abs(np.arange(-QUALITY_RADIUS, QUALITY_RADIUS + 1))]                                # [17]
            H = np.einsum("yxjc,j->yxc", x[:, idx, :], w)
            B = np.einsum("yjxc,j->yxc", H[idx, :, :], w)
            note("H", H); note("B", B)
            b8 = (B + 32768) >> 16
            prod = a * (x8 - b8)
            note("a*(x8-b8)+128", prod + 128)
            s = x8 + ((prod + 128) >> 8)
        else:
            s = x8
        note("s", s)
        cnt = 3 * S * S
        m8 = (256 * int(x.sum()) + cnt // 2) // cnt
        prod = c * (s - m8)
        note("c*(s-m8)+128", prod + 128)
        t = m8 + ((prod + 128) >> 8) + beta
        note("t", t)
        if k > 0:
            prod = k * quality_noise_host(S, seed, table[n])
            note("k*g+2048", prod + 2048)
            t = t + ((prod + 2048) >> 12)
            note("u", t)
        note("u+128", t + 128)
        out[n] = np.clip((t + 128) >> 8, 0, 255).astype(np.uint8)
    return out
