"""Device-side training input pipeline: the MI355X counterpart of the reference's per-sample host transforms
Compose([Resize(256), RandomScaleCrop(256), Normalize_tf(), ToTensor()]) (train.py:58-62; custom_transforms.py:375-391,
330-354,139-176,455-499,581-599) and of get_multi_batch's stack + .cuda() (Trainer.py:45-55).

The decoded uint8 samples are copied to the GPU as they are; resampling, cropping, normalisation and the mask thresholds run
there (csrc/pipeline.hip) and produce the [N,3,S,S] / [N,1,S,S] fp32 batch the training step takes.  The result equals the
reference's bit for bit (tests/test_input_pipeline_gpu.py, fixtures generated from the reference's own classes).

What stays on the host: PNG decoding and the random draws.  The reference draws from Python's `random` module
(`seed = random.random()`, two `random.uniform(1, 1.5)`, two `random.randint` for the crop); `draw()` makes the same draws
in the same order from any `random.Random`-like generator, so a seeded run crops exactly like the reference.

Optional augmentation stage (`Augment`, `draw_augment`, `augment_host`; csrc/augment.hip): the reference's RandomRotate,
RandomFlip, elastic_transform, add_salt_pepper_noise, adjust_light and eraser (custom_transforms.py:310-327,204-217,87-132,22-43,
45-55,58-85), in that order, between the crop and the normalisation.  Again the draws are made on the host, in the reference's
order, and the pixels are produced on the GPU, bit for bit; `augment_host` is the numpy specification of the device stage.

Optional amplitude-mixing stage (`AmplitudeMix`, `draw_mix`, `amplitude_mix_host`; csrc/spectrum.hip): a sample keeps the phase of its
2-D spectrum and moves the amplitude of a low-frequency window towards that of a sample from another source domain of the same
batch (FDA; FedDG's continuous frequency space interpolation; FACT's amplitude mix — PAPERS.md), after the augmentations and before
the normalisation.  This stage has no counterpart in the reference: `amplitude_mix_host` (float64) is its specification, and the
device stage is held to it within the error of an fp32 transform (tests/test_amplitude_mix_gpu.py).

Optional random appearance networks (`AppearanceNets`, `draw_appearance`, `appearance_host`; csrc/appearance.hip): a sample is
centred on its mean and pushed through one or two shallow convolutional networks whose weights are drawn anew for every sample,
scaled back to its energy and, with two networks, blended through a smooth random field (GIN / IPA, RandConv — PAPERS.md) — after
amplitude mixing and before the image-quality stage.  No counterpart in the reference: the stage is defined in fixed point,
`appearance_host` (numpy int64) is its specification and the device equals it byte for byte (tests/test_appearance_gpu.py).  Its
effect on the Dice / HD95 of a held-out domain has not been measured.

Optional image-quality stage (`ImageQuality`, `draw_quality`, `quality_host`; csrc/quality.hip): Gaussian blur or unsharp masking,
contrast about the sample's mean, a brightness shift and dense noise — the image-quality transforms of the stacked-transformation
recipe (BigAug) — after amplitude mixing and before the normalisation.  No counterpart in the reference either: the
stage is defined in fixed point, `quality_host` (numpy int64) is its specification and the device equals it byte for byte
(tests/test_quality_gpu.py).

Optional JPEG compression stage (`JpegCompression`, `draw_jpeg`, `jpeg_host`; csrc/jpeg.hip): baseline JPEG's round trip of the
pixels — colour conversion, 4:2:0 or 4:4:4 chroma, libjpeg's "islow" DCTs around the quantiser, "fancy" upsampling — without the
entropy coder, after the image-quality stage and before CLAHE: the file the camera writes last.  The sides are multiples of 16.
Unlike the other stages' specifications `jpeg_host` (numpy int64) is not this project's own: it equals, byte for byte, what Pillow
reads back from the file it writes (tests/test_jpeg_cpu.py), and the device equals it byte for byte (tests/test_jpeg_gpu.py).  Its
effect on the Dice / HD95 of a held-out domain has not been measured.

Optional CLAHE preprocessing (`Clahe`, `clahe_host`, `clahe_axis_table`; csrc/clahe.hip): contrast-limited adaptive histogram
equalisation of the uint8 batch, the last step before the normalisation — not an augmentation: it draws nothing, and the same
`Clahe` belongs in front of the networks at validation and prediction time (labelled_split.ClaheTestBatches, segment.Segmenter; a run's
checkpoints record it).  Defined in integers after OpenCV's createCLAHE, not byte-equal to it; `clahe_host` (numpy int64) is the
specification and the device equals it byte for byte (tests/test_clahe_gpu.py).

The coefficient tables are Pillow's (src/libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc; Geometry.c
ImagingScaleAffine for NEAREST), computed here with the same double-precision operations in the same order.
"""
import math

import numpy as np
import torch

from . import ops

PRECISION_BITS = 22
_FILTER_SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    """Resample.c lanczos_filter: sinc(x) * sinc(x / 3) on -3 <= x < 3.  One coefficient at a time through math.sin — libm's sine,
    the one Pillow's C calls; a vectorised sine may differ from it in the last bit, which a rounded 22-bit coefficient can show."""
    flat = [_sinc(v) * _sinc(v / 3) if -3.0 <= v < 3.0 else 0.0 for v in x.ravel().tolist()]
    return np.array(flat, np.float64).reshape(x.shape)


def _filter(name, x):
    if name == "lanczos":
        return _lanczos(x)
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_table(in_size, out_size, filt, first=0, count=None):
    """Pillow's coefficients for resizing an axis in_size -> out_size, for output positions [first, first+count).
    -> (bounds [count,2] int32 (first source index, taps), kk [count,ksize] int32, ksize)."""
    count = out_size - first if count is None else count
    scale = float(in_size) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = _FILTER_SUPPORT[filt] * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(first, first + count, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C (int) cast: truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < n[:, None]
    w = np.where(live, _filter(filt, (x + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(count, np.float64)
    for i in range(ksize):                                                   # sequential sum, as the C loop
        ww = ww + w[:, i]
    k = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    p = k * float(1 << PRECISION_BITS)
    kk = np.where(k < 0, (-0.5 + p).astype(np.int64), (0.5 + p).astype(np.int64)).astype(np.int32)
    kk = np.where(live, kk, 0).astype(np.int32)
    bounds = np.stack([xmin, n], 1).astype(np.int32)
    return bounds, kk, ksize


def nearest_table(in_size, out_size, first=0, count=None):
    """Source index of output positions [first, first+count) of Image.resize(..., NEAREST) (accumulated `xo += a0`)."""
    count = out_size - first if count is None else count
    a0 = float(in_size) / out_size
    steps = np.full(out_size, a0, np.float64)
    steps[0] = a0 * 0.5
    xo = np.add.accumulate(steps)                                            # sequential adds, as the C loop
    idx = np.clip(xo.astype(np.int64), 0, in_size - 1)
    return idx[first:first + count].astype(np.int32)


def draw(rng, size=256):
    """The draws of RandomScaleCrop + RandomCrop (custom_transforms.py:342-346,167-168) from `rng`, in their order.
    -> (scaled width, scaled height, crop x1, crop y1); (size, size, 0, 0) when the sample is not scaled."""
    seed = rng.random()
    nw = nh = size
    if seed > 0.5:
        nw = int(rng.uniform(1, 1.5) * size)
        nh = int(rng.uniform(1, 1.5) * size)
    if nw == size and nh == size:
        return nw, nh, 0, 0
    return nw, nh, rng.randint(0, nw - size), rng.randint(0, nh - size)


class Augment:
    """Which of the six training augmentations run, in the reference's order: rotate (RandomRotate), flip (RandomFlip), elastic
    (elastic_transform), salt_pepper (add_salt_pepper_noise), light (adjust_light), erase (eraser).  A disabled one draws nothing.

    rotate_degree: the reference draws its angle ONCE, in RandomRotate's constructor (`randint(1, 4) * 90`, custom_transforms.py:
    312), so a whole run rotates by one angle or not at all; 90 / 180 / 270 / 360 reproduce that.  The default "random" draws
    `randint(1, 4) * 90` per sample, right after a coin that fired — a deliberate deviation from the reference (no reference output
    exists for it; it is pinned against `augment_host` only)."""

    def __init__(self, rotate=True, rotate_degree="random", flip=True, elastic=True, salt_pepper=True, light=True, erase=True):
        if rotate_degree not in ("random", 90, 180, 270, 360):
            raise ValueError("rotate_degree must be 'random', 90, 180, 270 or 360, got %r" % (rotate_degree,))
        self.rotate, self.rotate_degree, self.flip, self.elastic = bool(rotate), rotate_degree, bool(flip), bool(elastic)
        self.salt_pepper, self.light, self.erase = bool(salt_pepper), bool(light), bool(erase)


def gamma_table(gamma):
    """adjust_light's table (custom_transforms.py:51-52), element by element in double precision as the reference builds it."""
    inv = 1.0 / gamma
    return np.array([((i / 255.0) ** inv) * 255 for i in np.arange(0, 256)]).astype(np.uint8)


def draw_augment(py_rng, np_rng, size, aug):
    """The random draws of the enabled augmentations for ONE sample, in the reference's order, from `py_rng` (where the reference
    uses the `random` module) and `np_rng` (where it uses `np.random`): a `random.Random(s)` and a `RandomState(s)` reproduce a run
    that seeded the two global generators with s.  -> plain data:
        k        quarter turns counter-clockwise, 0..3 (0: no rotation, or 360 degrees)
        flip_lr, flip_tb, elastic   flags
        sp       None or (value, rows, cols): the noise points; value 1 = salt — the reference writes 1, not 255, into the uint8
                 image (custom_transforms.py:37), kept — or 0 = pepper.  The third coordinate array (channels) the reference draws
                 and never uses is drawn and dropped.
        lut      None or adjust_light's 256-entry uint8 table
        rect     None or (top, left, h, w, fill): the eraser's rectangle after its rejection loop, fill = uniform(0, 255) truncated"""
    S = int(size)
    d = {"k": 0, "flip_lr": False, "flip_tb": False, "elastic": False, "sp": None, "lut": None, "rect": None}
    if aug.rotate and py_rng.random() > 0.5:
        degree = py_rng.randint(1, 4) * 90 if aug.rotate_degree == "random" else aug.rotate_degree
        d["k"] = (degree // 90) % 4
    if aug.flip:
        d["flip_lr"] = py_rng.random() < 0.5
        d["flip_tb"] = py_rng.random() < 0.5
    if aug.elastic:
        d["elastic"] = py_rng.random() > 0.5
    if aug.salt_pepper:
        n_px = S * S * 3
        num_salt = np.ceil(0.004 * n_px * 0.2)
        num_pepper = np.ceil(0.004 * n_px * (1.0 - 0.2))
        seed = py_rng.random()
        if seed > 0.5:
            value, num = (1, num_salt) if seed > 0.75 else (0, num_pepper)
            coords = [np_rng.randint(0, i - 1, int(num)) for i in (S, S, 3)]
            d["sp"] = (value, coords[0].astype(np.int32), coords[1].astype(np.int32))
    if aug.light and py_rng.random() > 0.5:
        d["lut"] = gamma_table(py_rng.random() * 3 + 0.5)
    if aug.erase and not py_rng.random() > 0.5:
        while True:
            s = np_rng.uniform(0.02, 0.06) * S * S
            r = np_rng.uniform(0.3, 0.6)
            w, h = int(np.sqrt(s / r)), int(np.sqrt(s * r))
            left, top = np_rng.randint(0, S), np_rng.randint(0, S)
            if left + w <= S and top + h <= S:
                break
        d["rect"] = (int(top), int(left), h, w, int(np_rng.uniform(0, 255)))
    return d


def gaussian_weights(sigma):
    """scipy.ndimage.gaussian_filter's 1-D kernel for `sigma` (truncate = 4), with scipy's operations: -> (w [radius + 1] = the
    centre and one half of the symmetric kernel, radius)."""
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:]), radius


def _blur_axis(x, w, axis):
    """One pass of gaussian_filter(mode="constant", cval=0) along `axis` in correlate1d's summation order for a symmetric kernel:
    acc = x[0] * w[0]; for j = radius .. 1: acc += (x[-j] + x[+j]) * w[j]."""
    r, n = len(w) - 1, x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r, r)
    p = np.moveaxis(np.pad(x, pad), axis, -1)
    acc = p[..., r:r + n] * w[0]
    for j in range(r, 0, -1):
        acc = acc + (p[..., r - j:r - j + n] + p[..., r + j:r + j + n]) * w[j]
    return np.moveaxis(acc, -1, axis)


def elastic_displacement(noise, size):
    """noise [2,S,S] uniform doubles in [0,1) -> the two displacement fields of elastic_transform (custom_transforms.py:99-112):
    gaussian_filter(noise * 2 - 1, 0.08 * S, mode="constant", cval=0) * (2 * S)."""
    S = int(size)
    w, _ = gaussian_weights(S * 0.08)
    f = np.asarray(noise, np.float64) * 2 - 1
    return _blur_axis(_blur_axis(f, w, 1), w, 2) * float(S * 2)


def _bilinear(src, cx, cy):
    """map_coordinates(order=1) at in-range coordinates, rounded into uint8 as scipy's uint8 output is: floor(v + 0.5)."""
    S = src.shape[0]
    fx, fy = np.floor(cx), np.floor(cy)
    tx, ty = cx - fx, cy - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)          # reached with weight 0 only
    g = src.astype(np.float64)
    if g.ndim == 3:
        tx, ty = tx[..., None], ty[..., None]
    v = (1.0 - tx) * ((1.0 - ty) * g[x0, y0] + ty * g[x0, y1]) + tx * ((1.0 - ty) * g[x1, y0] + ty * g[x1, y1])
    return np.floor(v + 0.5).astype(np.uint8)


def augment_host(image_u8, mask_u8, aug_draw, noise=None):
    """The specification of the device stage in numpy: image [S,S,3] uint8 and disc mask [S,S] uint8 (scaled and cropped), one
    `draw_augment` result, noise [2,S,S] uniform doubles in [0,1) (needed when aug_draw["elastic"]) -> (image, mask) uint8.
    Equal, bit for bit, to the reference's classes applied in the order rotate, flip, elastic, salt and pepper, light, erase with
    'label' = the disc mask (tests/golden/augment.npz), and to what DeviceInputPipeline computes on the GPU."""
    d = aug_draw
    img, mask = np.asarray(image_u8), np.asarray(mask_u8)
    S = img.shape[0]
    assert img.shape == (S, S, 3) and mask.shape == (S, S) and img.dtype == np.uint8 and mask.dtype == np.uint8
    if d["k"]:
        img, mask = np.rot90(img, d["k"]), np.rot90(mask, d["k"])
    if d["flip_lr"]:
        img, mask = img[:, ::-1], mask[:, ::-1]
    if d["flip_tb"]:
        img, mask = img[::-1], mask[::-1]
    if d["elastic"]:
        disp = elastic_displacement(noise, S)
        rows, cols = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        cx, cy = rows + disp[0], cols + disp[1]
        last = float(S - 1)
        inside = (cx >= 0.0) & (cx <= last) & (cy >= 0.0) & (cy <= last)
        cxc, cyc = np.clip(cx, 0.0, last), np.clip(cy, 0.0, last)
        img = np.where(inside[..., None], _bilinear(img, cxc, cyc), 0).astype(np.uint8)      # mode="constant": 0 outside
        mask = _bilinear(mask, cxc, cyc)                                                     # mode="nearest": clamped
    img = np.array(img)                                                                      # a writable copy
    if d["sp"] is not None:
        value, rows, cols = d["sp"]
        img[rows, cols, :] = value
    if d["lut"] is not None:
        img = d["lut"][img]
    if d["rect"] is not None:
        top, left, h, w, fill = d["rect"]
        img[top:top + h, left:left + w, :] = fill
    return img, np.ascontiguousarray(mask)

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


def _check_mix_args(images_u8, partner, lam, b):
    img = np.asarray(images_u8)
    if img.ndim != 4 or img.shape[1] != img.shape[2] or img.shape[3] != 3 or img.dtype != np.uint8:
        raise ValueError("amplitude mixing takes a [N,S,S,3] uint8 batch, got %s %s" % (img.shape, img.dtype))
    N, S = img.shape[:2]
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
    return img, partner.astype(np.int64), lam, int(b)


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


# ------------------------------------------------------------------------------------------ random appearance networks
APPEARANCE_CHANNELS = (3, 2, 2, 2, 3)    # four layers: the picture's three channels, a hidden width of two, three channels out
APPEARANCE_LAYERS = 4
APPEARANCE_W_OFF = (0, 54, 90, 126)      # a layer's weights [co][ci][3][3] within a net's 180
APPEARANCE_B_OFF = (0, 2, 4, 6)          # a layer's biases [co] within a net's 9
APPEARANCE_NET_COLS = 4 + 180 + 9        # a net: k[4], the weights, the biases
APPEARANCE_COLS = 3 + 2 * APPEARANCE_NET_COLS    # a parameter row: flags, alpha_0, alpha_1, net 0, net 1
APPEARANCE_CL = (1 << 19) - 1            # every layer's output and both g_j are clipped to -CL .. CL
APPEARANCE_W_MAX, APPEARANCE_BIAS_MAX, APPEARANCE_R_MAX = 16384, 1 << 19, 1 << 20
APPEARANCE_MAX_SIZE = 512                # 3 * 512^2 * 2^30 < 2^53: an energy converts to float64 exactly
APPEARANCE_SPACING = (4, 512)
APPEARANCE_SELECTED, APPEARANCE_BLEND = 1, 2     # the bits of a row's flags


def appearance_grid(S, spacing):
    """G = ceil(S / spacing) + 3: control values per axis of the blend field."""
    return -(-int(S) // int(spacing)) + 3


def _check_appearance_size(S, spacing):
    if not 1 <= int(S) <= APPEARANCE_MAX_SIZE:
        raise ValueError("the appearance stage takes samples of side 1 .. %d, got %r" % (APPEARANCE_MAX_SIZE, S))
    if isinstance(spacing, bool) or int(spacing) != spacing or not APPEARANCE_SPACING[0] <= int(spacing) <= APPEARANCE_SPACING[1]:
        raise ValueError("the appearance stage's spacing must be an integer in %d .. %d, got %r" % (APPEARANCE_SPACING + (spacing,)))


def appearance_axis_table(S, spacing):
    """-> [S,5] int64: per pixel x of an axis the first control index i = x // spacing and the four cubic B-spline weights of
    t = x / spacing - i in Q12 — (1 - t)^3 / 6, (3 t^3 - 6 t^2 + 4) / 6, (-3 t^3 + 3 t^2 + 3 t + 1) / 6, t^3 / 6 in float64, each
    rounded (rint), then the largest (the first of equals) moved by what the four lack of 4096.  All four are >= 0 and i + 3 <= G - 1."""
    _check_appearance_size(S, spacing)
    S, spacing = int(S), int(spacing)
    x = np.arange(S, dtype=np.int64)
    i = x // spacing
    t = (x - i * spacing).astype(np.float64) / float(spacing)
    w = np.stack([(1.0 - t) ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0,
                  (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0, t ** 3 / 6.0], 1)
    q = np.rint(w * 4096.0).astype(np.int64)
    q[np.arange(S), np.argmax(q, 1)] += 4096 - q.sum(1)
    return np.concatenate([i[:, None], q], 1)


def appearance_field_host(field, S, spacing):
    """Control values [N,G,G] in 0 .. 256 -> the blend field b [N,S,S] int64 in 0 .. 256: with (i, w) of `appearance_axis_table`,
    hx_r = (sum_c wx[c] P[iy + r][ix + c] + 8) >> 4 for the four control rows r, b = (sum_r wy[r] hx_r + 2^19) >> 20."""
    tab = appearance_axis_table(S, spacing)
    P = np.asarray(field).astype(np.int64)
    idx = tab[:, :1] + np.arange(4)[None, :]                              # [S,4]
    hx = ((P[:, :, idx] * tab[None, None, :, 1:]).sum(-1) + 8) >> 4       # [N,G,S]
    return ((hx[:, idx, :] * tab[None, :, 1:, None]).sum(2) + (1 << 19)) >> 20


class AppearanceNets:
    """The random appearance stage's parameters (GIN / IPA of Ouyang et al. 2022, RandConv of Xu et al. 2021): a sample
    is pushed through a shallow convolutional network whose weights are drawn anew for every sample — a random non-linear remapping
    of intensities and local texture that leaves shapes, and therefore labels, alone.

    p: the probability that a sample is remapped.  blend: a remapped sample gets TWO networks, blended through a smooth random field
    (IPA: the appearance changes differently in different parts of the picture); False: one network.  spacing: pixels between the
    control values of that field, 4 .. 512.  bias_sigma: the standard deviation of the biases in grey levels, 0 .. 2048.  p_k3: the
    probability that a layer is 3x3 and not 1x1.  The effect on the Dice / HD95 of a held-out domain has not been measured."""

    def __init__(self, p=0.5, blend=True, spacing=32, bias_sigma=32.0, p_k3=0.5):
        for name, v in (("p", p), ("p_k3", p_k3)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError("AppearanceNets: %s must lie in [0, 1], got %r" % (name, v))
        if isinstance(spacing, bool) or int(spacing) != spacing or not APPEARANCE_SPACING[0] <= int(spacing) <= APPEARANCE_SPACING[1]:
            raise ValueError("AppearanceNets: spacing must be an integer in %d .. %d, got %r" % (APPEARANCE_SPACING + (spacing,)))
        if not 0.0 <= float(bias_sigma) <= APPEARANCE_BIAS_MAX / 256.0:
            raise ValueError("AppearanceNets: bias_sigma must lie in [0, %g] grey levels, got %r" % (APPEARANCE_BIAS_MAX / 256.0, bias_sigma))
        self.p, self.blend, self.spacing = float(p), bool(blend), int(spacing)
        self.bias_sigma, self.p_k3 = float(bias_sigma), float(p_k3)


def appearance_neutral(n, S, spacing):
    """-> (params [n,389] int32, field [n,G,G] int32) that leave every sample alone: flags 0 (not selected: a copy), alpha = 256,
    k = 1, weights and biases 0, the field 256 everywhere."""
    _check_appearance_size(S, spacing)
    params = np.zeros((int(n), APPEARANCE_COLS), np.int32)
    params[:, 1:3] = 256
    for j in range(2):
        params[:, 3 + j * APPEARANCE_NET_COLS:7 + j * APPEARANCE_NET_COLS] = 1
    G = appearance_grid(S, spacing)
    return params, np.full((int(n), G, G), 256, np.int32)


def appearance_net_row(k, weights, biases):
    """One net's 193 columns from k [4], weights = four arrays [co,ci,3,3] and biases = four arrays [co] (integers)."""
    row = np.zeros(APPEARANCE_NET_COLS, np.int64)
    row[:4] = k
    for l in range(APPEARANCE_LAYERS):
        ci, co = APPEARANCE_CHANNELS[l], APPEARANCE_CHANNELS[l + 1]
        row[4 + APPEARANCE_W_OFF[l]:4 + APPEARANCE_W_OFF[l] + co * ci * 9] = np.asarray(weights[l]).reshape(co * ci * 9)
        row[184 + APPEARANCE_B_OFF[l]:184 + APPEARANCE_B_OFF[l] + co] = np.asarray(biases[l]).reshape(co)
    return row


def appearance_net_of(row):
    """The inverse of `appearance_net_row`: 193 columns -> (k [4], [W_l [co,ci,3,3]], [bias_l [co]]) int64."""
    row = np.asarray(row).astype(np.int64)
    W, B = [], []
    for l in range(APPEARANCE_LAYERS):
        ci, co = APPEARANCE_CHANNELS[l], APPEARANCE_CHANNELS[l + 1]
        W.append(row[4 + APPEARANCE_W_OFF[l]:4 + APPEARANCE_W_OFF[l] + co * ci * 9].reshape(co, ci, 3, 3))
        B.append(row[184 + APPEARANCE_B_OFF[l]:184 + APPEARANCE_B_OFF[l] + co])
    return row[:4], W, B


def _draw_appearance_net(np_rng, nets):
    k, W, B = [], [], []
    for l in range(APPEARANCE_LAYERS):
        ci, co = APPEARANCE_CHANNELS[l], APPEARANCE_CHANNELS[l + 1]
        k.append(3 if np_rng.random_sample() < nets.p_k3 else 1)
        w = np_rng.normal(0.0, 1.0, (co, ci, 3, 3)) / math.sqrt(ci * k[-1] * k[-1])
        W.append(np.clip(np.rint(w * 4096.0), -APPEARANCE_W_MAX, APPEARANCE_W_MAX).astype(np.int64))
        b = np_rng.normal(0.0, 1.0, co) * nets.bias_sigma
        B.append(np.clip(np.rint(b * 256.0), -APPEARANCE_BIAS_MAX, APPEARANCE_BIAS_MAX).astype(np.int64))
    return appearance_net_row(k, W, B)


def draw_appearance(np_rng, n, S, nets):
    """The stage's draws for a batch of n samples of side S from the run's numpy generator, sample by sample in batch order: a coin
    `random_sample() < p`; if it fires, for net 0 and (with `blend`) net 1: alpha = `randint(0, 257)`, then layer by layer the size
    coin `random_sample() < p_k3` (3x3, else 1x1), co * ci * 9 standard normals scaled by 1 / sqrt(fan_in) (fan_in = ci k k; the
    eight taps a 1x1 layer ignores are drawn all the same, so the stream does not depend on the coin) and quantised to Q12
    (rint, clipped to +-16384), co standard normals times bias_sigma grey levels quantised to Q8 (clipped to +-2^19); then, with
    `blend`, the G * G control values `randint(0, 257)`.  A coin that does not fire draws nothing else.
    -> (params [n,389] int32, field [n,G,G] int32)."""
    params, field = appearance_neutral(n, S, nets.spacing)
    for i in range(int(n)):
        if not np_rng.random_sample() < nets.p:
            continue
        params[i, 0] = APPEARANCE_SELECTED | (APPEARANCE_BLEND if nets.blend else 0)
        for j in range(2 if nets.blend else 1):
            params[i, 1 + j] = int(np_rng.randint(0, 257))
            params[i, 3 + j * APPEARANCE_NET_COLS:3 + (j + 1) * APPEARANCE_NET_COLS] = _draw_appearance_net(np_rng, nets)
        if nets.blend:
            field[i] = np_rng.randint(0, 257, field.shape[1:])
    return params, field


def check_appearance_params(params, field, N, S, spacing):
    """-> (params [N,389], field [N,G,G]) as int64 after the range checks the device arithmetic rests on (ValueError otherwise):
    flags 0 .. 3, alpha 0 .. 256, k 1 or 3, |W| <= 16384, |bias| <= 2^19, control values 0 .. 256."""
    _check_appearance_size(S, spacing)
    p, f = np.asarray(params), np.asarray(field)
    G = appearance_grid(S, spacing)
    if p.shape != (N, APPEARANCE_COLS) or p.dtype.kind not in "iu":
        raise ValueError("appearance: params must be [%d,%d] integers, got %s %s" % (N, APPEARANCE_COLS, p.shape, p.dtype))
    if f.shape != (N, G, G) or f.dtype.kind not in "iu":
        raise ValueError("appearance: the field must be [%d,%d,%d] integers, got %s %s" % (N, G, G, f.shape, f.dtype))
    p, f = p.astype(np.int64, order="C"), f.astype(np.int64, order="C")
    if not N:
        return p, f
    if p[:, 0].min() < 0 or p[:, 0].max() > 3:
        raise ValueError("appearance: flags must lie in 0 .. 3")
    if p[:, 1:3].min() < 0 or p[:, 1:3].max() > 256:
        raise ValueError("appearance: alpha must lie in 0 .. 256")
    for j in range(2):
        net = p[:, 3 + j * APPEARANCE_NET_COLS:3 + (j + 1) * APPEARANCE_NET_COLS]
        if not np.all((net[:, :4] == 1) | (net[:, :4] == 3)):
            raise ValueError("appearance: a layer's kernel size must be 1 or 3")
        if np.abs(net[:, 4:184]).max() > APPEARANCE_W_MAX:
            raise ValueError("appearance: weights must lie in -%d .. %d" % (APPEARANCE_W_MAX, APPEARANCE_W_MAX))
        if np.abs(net[:, 184:]).max() > APPEARANCE_BIAS_MAX:
            raise ValueError("appearance: biases must lie in -%d .. %d" % (APPEARANCE_BIAS_MAX, APPEARANCE_BIAS_MAX))
    if f.min() < 0 or f.max() > 256:
        raise ValueError("appearance: the field's control values must lie in 0 .. 256")
    return p, f


def appearance_is_neutral(params):
    """[N] bool: the rows the stage copies (not selected)."""
    return (np.asarray(params)[:, 0] & APPEARANCE_SELECTED) == 0


def appearance_layer_host(h, W, bias, k, leak):
    """One layer: h [ci,S,S] int64 -> [co,S,S].  v = ((sum_{ci,dy,dx} W[co][ci][dy][dx] h[ci][y + dy - 1][x + dx - 1] + 2048) >> 12)
    + bias[co] with h = 0 outside the picture (k = 1: the centre tap alone); with `leak`, v < 0 -> (3 v + 128) >> 8; clip to +-CL."""
    ci, S = h.shape[0], h.shape[1]
    pad = np.zeros((ci, S + 2, S + 2), np.int64)
    pad[:, 1:-1, 1:-1] = h
    acc = np.zeros((W.shape[0], S, S), np.int64)
    for dy in range(3):
        for dx in range(3):
            if k == 3 or (dy == 1 and dx == 1):
                acc += np.einsum("oc,cyx->oyx", W[:, :, dy, dx], pad[:, dy:dy + S, dx:dx + S])
    v = ((acc + 2048) >> 12) + bias[:, None, None]
    if leak:
        v = np.where(v < 0, (3 * v + 128) >> 8, v)
    return np.clip(v, -APPEARANCE_CL, APPEARANCE_CL)


def _energy_q4(v):
    q = (v + 8) >> 4
    return int((q * q).sum())


def appearance_gain(E_in, E_j):
    """R_j in Q12: min(rint(sqrt(float64(E_in) / float64(E_j)) * 4096), 2^20); 4096 when E_j = 0."""
    if E_j == 0:
        return 4096
    return int(min(np.rint(np.sqrt(np.float64(E_in) / np.float64(E_j)) * 4096.0), float(APPEARANCE_R_MAX)))


def appearance_host(images_u8, params, field, spacing, detail=None):
    """The specification of the device stage (csrc/appearance.hip) in numpy int64, which the device equals byte for byte: images
    [N,S,S,3] uint8, (params [N,389], field [N,G,G]) as `draw_appearance` makes them.  The definition is this project's own, in
    fixed point, after GIN / IPA; it is NOT byte-equal to anyone's float code.  Per selected sample, `>>` the arithmetic
    (floor) shift, CL = 2^19 - 1, x an input byte:
        m8 = (256 SUM + cnt // 2) // cnt, cnt = 3 S S, SUM the sum of the sample's bytes;  c0 = (x << 8) - m8  (Q8; 0 outside)
        y_j = net j on c0: four layers 3 -> 2 -> 2 -> 2 -> 3 (`appearance_layer_host`: Q12 weights, Q8 biases, 64-bit sums, zero
              padding at EVERY layer, a leaky ReLU behind layers 0 .. 2, the clip to +-CL behind every layer)
        z_j = (alpha_j c0 + (256 - alpha_j) y_j + 128) >> 8
        E_in = sum ((c0 + 8) >> 4)^2,  E_j = sum ((z_j + 8) >> 4)^2  over the sample (exact; below 2^53)
        R_j = `appearance_gain`(E_in, E_j);  E_j = 0: R_j = 4096 and z_j := c0
        g_j = clip((R_j z_j + 2048) >> 12, -CL, CL)
        b   = `appearance_field_host` (0 .. 256) with the blend flag, 256 without (net 0 alone; net 1 is not evaluated)
        out = clip((m8 + ((b g_0 + (256 - b) g_1 + 128) >> 8) + 128) >> 8, 0, 255)
    A sample that is not selected is copied.  detail: a dict that receives n -> the sample's intermediates (m8, c0, E_in, b, and per
    net the four layer outputs, z, E, R, g)."""
    img = np.asarray(images_u8)
    if img.ndim != 4 or img.shape[1] != img.shape[2] or img.shape[3] != 3 or img.dtype != np.uint8:
        raise ValueError("the appearance stage takes a [N,S,S,3] uint8 batch, got %s %s" % (img.shape, img.dtype))
    N, S = img.shape[:2]
    p, f = check_appearance_params(params, field, N, S, spacing)
    out = img.copy()
    CL = APPEARANCE_CL
    for n in range(N):
        flags = int(p[n, 0])
        if not flags & APPEARANCE_SELECTED:
            continue
        x = img[n].astype(np.int64)
        cnt = 3 * S * S
        m8 = (256 * int(x.sum()) + cnt // 2) // cnt
        c0 = (x << 8) - m8                                                    # [S,S,3]
        E_in = _energy_q4(c0)
        blend = bool(flags & APPEARANCE_BLEND)
        d = {"m8": m8, "c0": c0, "E_in": E_in, "nets": []}
        g = []
        for j in range(2 if blend else 1):
            alpha = int(p[n, 1 + j])
            k, W, B = appearance_net_of(p[n, 3 + j * APPEARANCE_NET_COLS:3 + (j + 1) * APPEARANCE_NET_COLS])
            h, layers = c0.transpose(2, 0, 1), []
            for l in range(APPEARANCE_LAYERS):
                h = appearance_layer_host(h, W[l], B[l], int(k[l]), l < APPEARANCE_LAYERS - 1)
                layers.append(h)
            z = (alpha * c0 + (256 - alpha) * h.transpose(1, 2, 0) + 128) >> 8
            E = _energy_q4(z)
            R = appearance_gain(E_in, E)
            if E == 0:
                z = c0
            g.append(np.clip((R * z + 2048) >> 12, -CL, CL))
            d["nets"].append({"layers": layers, "z": z, "E": E, "R": R, "g": g[-1]})
        if blend:
            b = appearance_field_host(f[n:n + 1], S, spacing)[0][..., None]
            t = (b * g[0] + (256 - b) * g[1] + 128) >> 8
            d["b"] = b[..., 0]
        else:
            t = (256 * g[0] + 128) >> 8
        out[n] = np.clip((m8 + t + 128) >> 8, 0, 255).astype(np.uint8)
        if detail is not None:
            detail[n] = d
    return out


# ------------------------------------------------------------------------------------------ image-quality augmentation
QUALITY_RADIUS = 8                      # the largest blur radius: taps w[0..8]
QUALITY_COLS = 4 + QUALITY_RADIUS + 1    # a parameter row: a, c, beta, k, w[0..8]
QUALITY_MAX_SIZE = 512                   # 3 * 512^2 * 255 < 2^32: a sample's byte sum fits 32 bits
QUALITY_A, QUALITY_C, QUALITY_BETA, QUALITY_K = (-256, 512), (0, 512), (-16320, 16320), (0, 181000)
_NOISE_STD = math.sqrt(21845.0)          # of g = b0 + b1 + b2 + b3 - 510 over the four bytes of a uniform 32-bit word: 147.80


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


# ------------------------------------------------------------------------------------------ JPEG compression augmentation
JPEG_MAX_SIZE = 4096
# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), in natural (row-major) order
_JPEG_BASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32], np.int64)


def _check_jpeg_size(S):
    if int(S) != S or not 16 <= int(S) <= JPEG_MAX_SIZE or int(S) % 16:
        raise ValueError("the JPEG stage takes samples whose side is a multiple of 16 in 16 .. %d (whole MCUs), got %r" % (JPEG_MAX_SIZE, S))


def jpeg_tables(quality):
    """libjpeg's quantisation tables at `quality` (1 .. 100) -> [2,64] int32, luma and chroma in natural (row-major) order: the
    Annex K tables scaled by `jpeg_quality_scaling` (5000 // q below 50, else 200 - 2 q), each entry clip((base * scale + 50) // 100,
    1, 255) — what `jpeg_set_quality(..., force_baseline=TRUE)` installs and Pillow's `save(quality=q)` writes."""
    if int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError("JPEG quality must be an integer in 1 .. 100, got %r" % (quality,))
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((_JPEG_BASE * scale + 50) // 100, 1, 255).astype(np.int32)


def jpeg_reciprocals(tables):
    """The device quantiser's multipliers: ceil(2^32 / (8 Q)) per table entry (int32: Q >= 1 keeps them below 2^29).  With d = 8 Q
    and M = (2^32 + e) / d, 0 <= e < d, (n M) >> 32 = floor(n / d) whenever n e < 2^32 — n = |c| + (d >> 1) < 2^16 and e < 2^11 here;
    tests/test_jpeg_cpu.py checks every |c| in 0 .. 32767 against every divisor."""
    d = 8 * np.asarray(tables, np.int64)
    return (((1 << 32) + d - 1) // d).astype(np.int32)


class JpegCompression:
    """The JPEG stage's parameters: the file a fundus camera or an archive writes last — 8 x 8 block edges, ringing around the disc
    rim and the vessels, half-resolution chroma (ITU-T T.81; BigAug's image-quality group, the common-corruptions
    benchmarks).  p: the probability that a sample is compressed.  quality: (low, high), integers with 1 <= low <= high <= 100; a
    compressed sample gets libjpeg's tables at a quality drawn uniformly from low .. high.  p_420: the probability that a compressed
    sample is written 4:2:0 (chroma at half resolution both ways, Pillow's default below quality 100 ... and most cameras') and not
    4:4:4.  The side of the samples must be a multiple of 16."""

    def __init__(self, p=0.5, quality=(30, 95), p_420=0.75):
        for name, v in (("p", p), ("p_420", p_420)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError("JpegCompression: %s must lie in [0, 1], got %r" % (name, v))
        try:
            lo, hi = quality
            ok = int(lo) == lo and int(hi) == hi and 1 <= int(lo) <= int(hi) <= 100
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("JpegCompression: quality must be an integer pair with 1 <= low <= high <= 100, got %r" % (quality,))
        self.p, self.p_420 = float(p), float(p_420)
        self.quality = (int(lo), int(hi))


def jpeg_neutral(n):
    """(mode [n] int32, tables [n,2,64] int32) that leave every sample alone: mode 0, tables of ones (not read)."""
    return np.zeros(int(n), np.int32), np.ones((int(n), 2, 64), np.int32)


def draw_jpeg(np_rng, n, j):
    """The stage's draws for a batch of n samples from the run's numpy generator, sample by sample in batch order: a coin
    `random_sample() < p`; if it fires, quality = `randint(low, high + 1)`, then a coin `random_sample() < p_420` that picks 4:2:0
    over 4:4:4.  A coin that does not fire draws nothing else; p = 0 draws nothing at all.  -> (mode [n] int32: 0 off, 1 = 4:4:4,
    2 = 4:2:0; tables [n,2,64] int32 = `jpeg_tables(quality)`).  The device takes tables, not qualities: a caller can hand in a
    camera's own."""
    mode, tables = jpeg_neutral(n)
    for i in range(int(n)):
        if j.p > 0.0 and np_rng.random_sample() < j.p:
            tables[i] = jpeg_tables(int(np_rng.randint(j.quality[0], j.quality[1] + 1)))
            mode[i] = 2 if np_rng.random_sample() < j.p_420 else 1
    return mode, tables


def check_jpeg_params(mode, tables, N):
    """-> (mode [N] int64, tables [N,2,64] int64) after the checks the device arithmetic rests on (ValueError otherwise): modes in
    {0, 1, 2}, and table entries in 1 .. 255 wherever the mode is not 0."""
    m, t = np.asarray(mode), np.asarray(tables)
    if m.shape != (N,) or m.dtype.kind not in "iu":
        raise ValueError("jpeg: mode must be [%d] integers, got %s %s" % (N, m.shape, m.dtype))
    if t.shape != (N, 2, 64) or t.dtype.kind not in "iu":
        raise ValueError("jpeg: tables must be [%d,2,64] integers, got %s %s" % (N, t.shape, t.dtype))
    m, t = m.astype(np.int64), t.astype(np.int64)
    if N and (m.min() < 0 or m.max() > 2):
        raise ValueError("jpeg: mode must be 0 (off), 1 (4:4:4) or 2 (4:2:0)")
    on = t[m != 0]
    if on.size and (on.min() < 1 or on.max() > 255):
        raise ValueError("jpeg: table entries must lie in 1 .. 255 (baseline JPEG)")
    return m, t


def jpeg_is_neutral(mode):
    """[N] bool: the rows the stage copies (mode 0)."""
    return np.asarray(mode) == 0


def _jpeg_descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _jpeg_fdct8(d, rows):
    """libjpeg's jfdctint.c on eight arrays: the row pass (outputs 0 and 4 << 2, the others DESCALE 11) or the column pass (outputs 0
    and 4 DESCALE 2, the others DESCALE 15).  -> (the eight outputs, every sum in front of a shift: for the 32-bit claim)."""
    n = 11 if rows else 15
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1 = (t12 + t13) * 4433
    e2, e6 = z1 + t13 * 6270, z1 - t12 * 15137
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    pre = [t10 + t11, a7 + z1 + z4, e2, a6 + z2 + z3, t10 - t11, a5 + z2 + z4, e6, a4 + z1 + z3]
    out = [(pre[i] << 2 if rows else _jpeg_descale(pre[i], 2)) if i in (0, 4) else _jpeg_descale(pre[i], n) for i in range(8)]
    return out, pre + [z5, a4, a5, a6, a7, z1, z2, z3, z4]


def _jpeg_idct8(d, n):
    """libjpeg's jidctint.c on eight arrays, every output DESCALE n (11: the column pass, 18: the row pass).  -> (the eight outputs,
    every sum in front of a shift)."""
    z1 = (d[2] + d[6]) * 4433
    t2, t3 = z1 - d[6] * 15137, z1 + d[2] * 6270
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 * 2446 + z1 + z3, o1 * 16819 + z2 + z4, o2 * 25172 + z2 + z3, o3 * 12299 + z1 + z4
    pre = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return [_jpeg_descale(p, n) for p in pre], pre + [z5, z1, z2, z3, z4, o0, o1, o2, o3]


def _jpeg_plane(x, Q, note):
    """One plane [H,W] int64 of samples 0 .. 255 (H, W multiples of 8) through the codec with the table Q [64] -> the decoded plane,
    clamped to 0 .. 255."""
    H, W = x.shape
    b = (x - 128).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)              # [by,bx,row,column]
    r, pre = _jpeg_fdct8([b[..., i] for i in range(8)], True)
    note("fdct rows", pre)
    b = np.stack(r, -1)
    r, pre = _jpeg_fdct8([b[..., j, :] for j in range(8)], False)
    note("fdct columns", pre)
    c = np.stack(r, -2)
    note("coefficient", c)
    d = 8 * Q.reshape(8, 8)
    k = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    c = k * Q.reshape(8, 8)
    note("dequantised", c)
    r, pre = _jpeg_idct8([c[..., j, :] for j in range(8)], 11)
    note("idct columns", pre)
    b = np.stack(r, -2)
    r, pre = _jpeg_idct8([b[..., i] for i in range(8)], 18)
    note("idct rows", pre)
    b = np.stack(r, -1) + 128
    note("idct output", b)
    return np.clip(b, 0, 255).transpose(0, 2, 1, 3).reshape(H, W)


def _jpeg_upsample(c):
    """libjpeg's h2v2_fancy_upsample: [h,w] -> [2 h, 2 w]."""
    h, w = c.shape
    up, dn = c[np.maximum(np.arange(h) - 1, 0)], c[np.minimum(np.arange(h) + 1, h - 1)]
    cs = np.empty((2 * h, w), np.int64)
    cs[0::2], cs[1::2] = 3 * c + up, 3 * c + dn
    left, right = cs[:, np.maximum(np.arange(w) - 1, 0)], cs[:, np.minimum(np.arange(w) + 1, w - 1)]
    out = np.empty((2 * h, 2 * w), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
    return out


def jpeg_host(images_u8, mode, tables, ranges=None):
    """The specification of the device stage (csrc/jpeg.hip) in numpy int64, which the device equals byte for byte and which equals,
    byte for byte, what Pillow (libjpeg-turbo) reads back from the baseline file it writes with these tables (tests/test_jpeg_cpu.py):
    images [N,S,S,3] uint8 with S a multiple of 16, mode [N] (0: the row is copied, 1: 4:4:4, 2: 4:2:0), tables [N,2,64] (luma,
    chroma; natural order).  `>>` is the floor shift, DESCALE(x, n) = (x + (1 << (n - 1))) >> n:
        Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
        Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16;  Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
        4:2:0: chroma = (sum of the 2 x 2 cell + 1, 2, 1, 2, .. along the output columns) >> 2
        per 8 x 8 block of x - 128: jfdctint (rows, then columns; the coefficients carry a factor 8),
        k = sign(c) ((|c| + (8 Q >> 1)) // (8 Q)), c' = k Q, jidctint (columns DESCALE 11, rows DESCALE 18), + 128, clip to 0 .. 255
        4:2:0: h2v2 fancy upsampling: cs = 3 near row + far row (above for even output rows, below for odd; the near row itself at
        the top and bottom), even column (3 cs[x] + cs[x-1] + 8) >> 4, odd (3 cs[x] + cs[x+1] + 7) >> 4, with cs[-1] = cs[0] and
        cs[w] = cs[w-1]: the first column is (4 cs[0] + 8) >> 4 and the last (4 cs[w-1] + 7) >> 4
        R = Y + ((91881 cr + 32768) >> 16);  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16);  B = Y + ((116130 cb + 32768) >> 16),
        cb = Cb - 128, cr = Cr - 128, each clipped to 0 .. 255
    libjpeg's inverse DCT clamps through a table that WRAPS outside -384 .. 639 (`JPEG_IDCT_WINDOW`, about the legal range): inside
    it the table and the clip here agree, and the tests assert that their inputs stay inside.
    ranges: a dict that receives name -> (min, max) of every intermediate over the batch ("idct output": in front of the clip)."""
    img = np.asarray(images_u8)
    if img.ndim != 4 or img.shape[1] != img.shape[2] or img.shape[3] != 3 or img.dtype != np.uint8:
        raise ValueError("the JPEG stage takes a [N,S,S,3] uint8 batch, got %s %s" % (img.shape, img.dtype))
    N, S = img.shape[:2]
    _check_jpeg_size(S)
    m, t = check_jpeg_params(mode, tables, N)

    def note(name, v):
        if ranges is not None:
            vs = v if isinstance(v, list) else [v]
            lo, hi = min(int(np.min(a)) for a in vs), max(int(np.max(a)) for a in vs)
            old = ranges.get(name, (lo, hi))
            ranges[name] = (min(lo, old[0]), max(hi, old[1]))

    out = np.empty_like(img)
    for n in range(N):
        if m[n] == 0:
            out[n] = img[n]
            continue
        x = img[n].astype(np.int64)
        R, G, B = x[..., 0], x[..., 1], x[..., 2]
        pre = [19595 * R + 38470 * G + 7471 * B + 32768, -11059 * R - 21709 * G + 32768 * B + 8388608 + 32767,
               32768 * R - 27439 * G - 5329 * B + 8388608 + 32767]
        note("colour forward", pre)
        Y, Cb, Cr = (p >> 16 for p in pre)
        if m[n] == 2:
            bias = 1 + (np.arange(S // 2) & 1)
            Cb, Cr = (((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2) for c in (Cb, Cr))
        Y, Cb, Cr = _jpeg_plane(Y, t[n, 0], note), _jpeg_plane(Cb, t[n, 1], note), _jpeg_plane(Cr, t[n, 1], note)
        if m[n] == 2:
            Cb, Cr = _jpeg_upsample(Cb), _jpeg_upsample(Cr)
        cb, cr = Cb - 128, Cr - 128
        pre = [91881 * cr + 32768, -22554 * cb - 46802 * cr + 32768, 116130 * cb + 32768]
        note("colour back", pre)
        out[n] = np.clip(np.stack([Y + (p >> 16) for p in pre], -1), 0, 255).astype(np.uint8)
    return out


# libjpeg's range-limit table (jdmaster.c, prepare_range_limit_table) indexed with (x + 128) & 1023 clamps like a clip for
# x + 128 in -384 .. 639 and wraps beyond: the pre-clamp outputs of the inverse DCT ("idct output" of jpeg_host's ranges) must stay inside
JPEG_IDCT_WINDOW = (-384, 639)


# ------------------------------------------------------------------------------------------------ CLAHE preprocessing
CLAHE_MAX_SIDE = 4096                   # tile counts stay below 2^24: c[v] * 255 + n / 2 fits unsigned 32 bits
CLAHE_MAX_TILES = 16
CLAHE_MODES = ("luma", "rgb")


class Clahe:
    """Contrast-limited adaptive histogram equalisation as a PREPROCESSING step (Pizer et al. 1987, Zuiderveld 1994): the
    uint8 picture is equalised tile by tile before the normalisation, in training and wherever a picture becomes network input.
    Deterministic — nothing is drawn.  Off unless an object of this class is handed to a feed or a front.

    clip: the clip limit as a multiple of the uniform bin height n / 256 of a tile, 1 <= clip <= 256 (256: no clipping); carried as
    clip_q8 = round(256 clip).  tiles = (ty, tx): tiles along the height and the width, each 1 .. 16 and not more than the picture's
    side.  floor: a pixel belongs to the field of view when max(R, G, B) >= floor (locate's test; 0: every pixel); pixels outside it
    are neither counted nor changed.  mode: "luma" equalises Y = (77 R + 150 G + 29 B + 128) >> 8 and shifts the three channels by
    Y' - Y (chroma kept); "rgb" equalises each channel by itself.
    The definition (`clahe_host`) is this project's own integer text after OpenCV's createCLAHE; it is NOT byte-equal to OpenCV
    (tile boundaries, rounding and the field mask differ)."""

    def __init__(self, clip=2.0, tiles=(8, 8), floor=0, mode="luma"):
        try:
            clip = float(clip)
        except (TypeError, ValueError):
            raise ValueError("Clahe: clip must be a number in [1, 256], got %r" % (clip,))
        if not 1.0 <= clip <= 256.0:
            raise ValueError("Clahe: clip must lie in [1, 256], got %r" % (clip,))
        try:
            ty, tx = (int(t) for t in tiles)
            if (ty, tx) != tuple(tiles):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("Clahe: tiles must be a pair of integers (ty, tx), got %r" % (tiles,))
        if not (1 <= ty <= CLAHE_MAX_TILES and 1 <= tx <= CLAHE_MAX_TILES):
            raise ValueError("Clahe: tiles must lie in 1 .. %d each, got %r" % (CLAHE_MAX_TILES, tiles))
        if isinstance(floor, bool) or int(floor) != floor or not 0 <= int(floor) <= 255:
            raise ValueError("Clahe: floor must be an integer in 0 .. 255, got %r" % (floor,))
        if mode not in CLAHE_MODES:
            raise ValueError("Clahe: mode must be one of %s, got %r" % (", ".join(CLAHE_MODES), mode))
        self.clip, self.clip_q8 = clip, int(np.rint(clip * 256.0))
        self.tiles, self.floor, self.mode = (ty, tx), int(floor), mode

    @property
    def planes(self):
        return 1 if self.mode == "luma" else 3

    def check_size(self, H, W):
        ty, tx = self.tiles
        if not (1 <= H <= CLAHE_MAX_SIDE and 1 <= W <= CLAHE_MAX_SIDE):
            raise ValueError("clahe: the picture's sides must lie in 1 .. %d, got %d x %d" % (CLAHE_MAX_SIDE, H, W))
        if ty > H or tx > W:
            raise ValueError("clahe: tiles %s need a picture of at least that many rows and columns, got %d x %d" % (self.tiles, H, W))

    def record(self):
        """-> what a checkpoint carries as its "clahe" entry: ints and strings only."""
        return {"clip_q8": self.clip_q8, "ty": self.tiles[0], "tx": self.tiles[1], "floor": self.floor, "mode": self.mode}

    @classmethod
    def from_record(cls, d):
        try:
            c = cls(int(d["clip_q8"]) / 256.0, (int(d["ty"]), int(d["tx"])), int(d["floor"]), str(d["mode"]))
        except (KeyError, TypeError) as e:
            raise ValueError("not a Clahe record: %r (%s)" % (d, e))
        if c.clip_q8 != int(d["clip_q8"]):
            raise ValueError("not a Clahe record: clip_q8 = %r" % (d["clip_q8"],))
        return c

    def __eq__(self, other):
        return isinstance(other, Clahe) and self.record() == other.record()

    def __hash__(self):
        return hash(tuple(sorted(self.record().items())))

    def __repr__(self):
        return "Clahe(clip=%g, tiles=%r, floor=%d, mode=%r)" % (self.clip_q8 / 256.0, self.tiles, self.floor, self.mode)


def clahe_record(clahe):
    """None -> None, a Clahe -> its record()."""
    return None if clahe is None else clahe.record()


def parse_clahe(text):
    """The value of a program's --clahe switch -> "checkpoint", None ("off") or a Clahe from CLIP[:TY,TX[:FLOOR[:MODE]]]."""
    text = str(text).strip()
    if text == "checkpoint":
        return "checkpoint"
    if text == "off":
        return None
    parts = text.split(":")
    try:
        if not 1 <= len(parts) <= 4:
            raise ValueError
        kw = {"clip": float(parts[0])}
        if len(parts) > 1:
            ty, tx = parts[1].split(",")
            kw["tiles"] = (int(ty), int(tx))
        if len(parts) > 2:
            kw["floor"] = int(parts[2])
        if len(parts) > 3:
            kw["mode"] = parts[3]
    except ValueError:
        raise ValueError("--clahe takes checkpoint, off or CLIP[:TY,TX[:FLOOR[:MODE]]], got %r" % (text,))
    return Clahe(**kw)


def clahe_bounds(L, t):
    """Tile boundaries along an axis of length L: b_k = (k L) // t, k = 0 .. t -> [t + 1] int64.  Uneven tiles, no padding."""
    return (np.arange(int(t) + 1, dtype=np.int64) * int(L)) // int(t)


def clahe_axis_table(L, t):
    """-> (k0 [L], w [L]) int64: the lower tile index and the Q8 weight of tile k0 + 1 for every pixel of an axis.  Doubled tile
    centres c2_k = b_k + b_{k+1}, pixel y at p = 2 y + 1.  p <= c2_0: (0, 0); p >= c2_{t-1}: (t - 1, 0); otherwise k0 = the largest k
    with c2_k <= p and w = ((p - c2_k) 256 + den // 2) // den, den = c2_{k+1} - c2_k.  (Where two centres lie 512 or more doubled
    units apart, the last pixel in front of the upper centre rounds to w = 256: all of tile k0 + 1.)"""
    L, t = int(L), int(t)
    b = clahe_bounds(L, t)
    c2 = b[:-1] + b[1:]
    p = 2 * np.arange(L, dtype=np.int64) + 1
    k0 = np.clip(np.searchsorted(c2, p, side="right") - 1, 0, t - 1)
    w = np.zeros(L, np.int64)
    inner = (p > c2[0]) & (p < c2[t - 1])
    if inner.any():
        k = k0[inner]
        den = c2[k + 1] - c2[k]
        w[inner] = ((p[inner] - c2[k]) * 256 + den // 2) // den
    k0[p <= c2[0]] = 0
    k0[p >= c2[t - 1]] = t - 1
    return k0, w


def clahe_redistribute(hist, clip_q8):
    """One tile's histogram h [256] (n = sum h > 0) -> the clipped histogram with the excess handed back: limit = max(1, (clip_q8 n)
    >> 16), excess = sum max(h - limit, 0), h = min(h, limit) + excess // 256, and with r = excess % 256 > 0 the bins 0, step,
    2 step, ... (step = max(256 // r, 1)) get one more each until r of them have.  The counts still sum to n."""
    h = np.asarray(hist, dtype=np.int64).copy()
    n = int(h.sum())
    limit = max(1, (int(clip_q8) * n) >> 16)
    excess = int(np.maximum(h - limit, 0).sum())
    h = np.minimum(h, limit) + excess // 256
    r = excess % 256
    if r > 0:
        step = max(256 // r, 1)
        h[np.arange(r) * step] += 1
    return h


def clahe_lut(hist, clip_q8):
    """One tile's histogram [256] -> its LUT [256] int64: the identity for an empty tile, else lut[v] = min((c[v] 255 + n // 2) // n,
    255) over the inclusive prefix sum c of `clahe_redistribute`'s counts."""
    n = int(np.asarray(hist, dtype=np.int64).sum())
    if n == 0:
        return np.arange(256, dtype=np.int64)
    c = np.cumsum(clahe_redistribute(hist, clip_q8))
    return np.minimum((c * 255 + n // 2) // n, 255)


def _clahe_arg(clahe, kw):
    if clahe is None:
        return Clahe(**kw)
    if kw or not isinstance(clahe, Clahe):
        raise ValueError("clahe: pass a Clahe, or its parameters as keywords (got %r, %r)" % (clahe, kw))
    return clahe


def _clahe_planes(img, clahe):
    """img [N,H,W,3] int64 -> (planes [N,P,H,W] int64, field [N,H,W] bool)."""
    field = img.max(-1) >= clahe.floor
    if clahe.mode == "luma":
        planes = ((77 * img[..., 0] + 150 * img[..., 1] + 29 * img[..., 2] + 128) >> 8)[:, None]
    else:
        planes = img.transpose(0, 3, 1, 2)
    return planes, field


def clahe_luts_host(images_u8, clahe=None, **kw):
    """-> the tile LUTs [N,P,ty,tx,256] uint8 of `clahe_host` (P = 1 for "luma", 3 for "rgb")."""
    clahe = _clahe_arg(clahe, kw)
    img = np.asarray(images_u8)
    if img.ndim != 4 or img.shape[3] != 3 or img.dtype != np.uint8:
        raise ValueError("clahe takes a [N,H,W,3] uint8 batch, got %s %s" % (img.shape, img.dtype))
    N, H, W = img.shape[:3]
    if not 1 <= N <= 65535:
        raise ValueError("clahe takes 1 .. 65535 pictures, got %d" % N)
    clahe.check_size(H, W)
    ty, tx = clahe.tiles
    planes, field = _clahe_planes(img.astype(np.int64), clahe)
    by, bx = clahe_bounds(H, ty), clahe_bounds(W, tx)
    luts = np.empty((N, clahe.planes, ty, tx, 256), np.uint8)
    for n in range(N):
        for i in range(ty):
            for j in range(tx):
                f = field[n, by[i]:by[i + 1], bx[j]:bx[j + 1]]
                for p in range(clahe.planes):
                    v = planes[n, p, by[i]:by[i + 1], bx[j]:bx[j + 1]][f]
                    luts[n, p, i, j] = clahe_lut(np.bincount(v, minlength=256), clahe.clip_q8)
    return luts


def clahe_host(images_u8, clahe=None, **kw):
    """The specification of the device stage (csrc/clahe.hip) in numpy int64, which the device equals byte for byte: images
    [N,H,W,3] uint8 and a `Clahe` (or its parameters as keywords: clip, tiles, floor, mode) -> [N,H,W,3] uint8.
    Field: max(R, G, B) >= floor.  Planes: Y = (77 R + 150 G + 29 B + 128) >> 8 ("luma") or the three channels ("rgb").  Per tile
    (`clahe_bounds`) and plane a LUT over the tile's field pixels (`clahe_lut`).  Per pixel, with (k0y, wy), (k0x, wx) from
    `clahe_axis_table`, the upper neighbours min(k0 + 1, t - 1), and a, b, c, d the LUT values of tiles (k0y, k0x), (k0y, k0x + 1),
    (k0y + 1, k0x), (k0y + 1, k0x + 1) at the pixel's plane value:
        v' = ((256 - wy) ((256 - wx) a + wx b) + wy ((256 - wx) c + wx d) + 32768) >> 16
    "rgb": channel c becomes its own v'; "luma": every channel becomes clip(channel + (Y' - Y), 0, 255).  Pixels outside the field
    are copied."""
    clahe = _clahe_arg(clahe, kw)
    luts = clahe_luts_host(images_u8, clahe).astype(np.int64)
    img = np.asarray(images_u8).astype(np.int64)
    N, H, W = img.shape[:3]
    ty, tx = clahe.tiles
    planes, field = _clahe_planes(img, clahe)
    k0y, wy = clahe_axis_table(H, ty)
    k0x, wx = clahe_axis_table(W, tx)
    k1y, k1x = np.minimum(k0y + 1, ty - 1), np.minimum(k0x + 1, tx - 1)
    wy, wx = wy[:, None], wx[None, :]
    out = img.copy()
    for n in range(N):
        new = []
        for p in range(clahe.planes):
            v, lut = planes[n, p], luts[n, p]
            a, b = lut[k0y[:, None], k0x[None, :], v], lut[k0y[:, None], k1x[None, :], v]
            c, d = lut[k1y[:, None], k0x[None, :], v], lut[k1y[:, None], k1x[None, :], v]
            new.append(((256 - wy) * ((256 - wx) * a + wx * b) + wy * ((256 - wx) * c + wx * d) + 32768) >> 16)
        if clahe.mode == "luma":
            res = np.clip(img[n] + (new[0] - planes[n, 0])[..., None], 0, 255)
        else:
            res = np.stack(new, -1)
        out[n] = np.where(field[n][..., None], res, img[n])
    return out.astype(np.uint8)


def clahe_device_tables(H, W, clahe):
    """The axis tables as the device reads them, int32: k0 | w << 8 per pixel -> (rows [H], columns [W rounded up to 4]), and bands
    [ty + 1]: the first row whose k0 is k (k0 does not decrease and takes every value), bands[ty] = H."""
    ty, tx = clahe.tiles
    k0y, wy = clahe_axis_table(H, ty)
    k0x, wx = clahe_axis_table(W, tx)
    cols = np.zeros((W + 3) & ~3, np.int32)
    cols[:W] = k0x | (wx << 8)
    bands = np.searchsorted(k0y, np.arange(ty + 1), side="left").astype(np.int32)
    return (k0y | (wy << 8)).astype(np.int32), cols, bands


def device_uniform(n, seed, pos, device="cuda"):
    """n uniform doubles in [0,1): numbers pos .. pos + n - 1 of the Philox4x32-10 stream `seed` (wtpse_uniform_f64)."""
    out = torch.empty(int(n), dtype=torch.float64, device=device)
    ops.lib().call("wtpse_uniform_f64", out.data_ptr(), int(n), int(seed), int(pos), ops.stream_ptr())
    return out


def _dev_u8(a, device):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise ValueError("input samples must be uint8 (decoded images), got %s" % t.dtype)
    return t.to(device, non_blocking=True).contiguous()


def _dev_i32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device, non_blocking=True)


class DeviceInputPipeline:
    """batch = pipeline(images, disc_masks, draws): images [H,W,3] uint8 and disc masks [H,W] uint8 per sample (numpy or
    torch, host or device; sizes may differ between samples), draws = [draw(rng, size) per sample].

    aug_draws = [draw_augment(py_rng, np_rng, size, aug) per sample] switches the augmentation stage on (None, the default: the
    stage does not exist).  The elastic transform's uniform fields come from the device generator — stream `noise_seed`, running
    position `noise_pos` (2 * S * S numbers per sample whose elastic coin fired; run state, see trainer.FundusBatches) — unless
    `noise` [N,2,S,S] fp64 in [0,1) is given (rows of samples without an elastic transform are not read).  The reference draws
    these fields from an unseeded RandomState(None) (custom_transforms.py:108), which nothing can reproduce: the fields are this
    pipeline's own, the arithmetic on them is scipy's.

    mix_draws = (partner, lam, b) — `draw_mix`'s two arrays and `AmplitudeMix.band(size)` — switches the amplitude-mixing stage on
    (None, the default: the stage does not exist): it runs on the uint8 batch after the augmentation stage (after the crop when
    there is none) and before the normalisation; the masks are not touched.  A batch in which no coin fired launches nothing.

    quality_draws = `draw_quality`'s parameter table [N,13] switches the image-quality stage on (None, the default: the stage does
    not exist): it runs on the uint8 batch after the other two stages and before the normalisation; the masks are not touched.  Its
    noise comes from the device Philox stream `noise_seed` too — blocks of their own, which no other consumer of the seed reads — at
    the running position `quality_pos` (S * S positions per sample with k > 0, in batch order; run state like `noise_pos`).  A batch
    in which no coin fired launches nothing.

    appearance_draws = (params, field, spacing) — `draw_appearance`'s two arrays and `AppearanceNets.spacing` — switches the random
    appearance networks on (None, the default: the stage does not exist): they run on the uint8 batch after amplitude mixing and
    before the image-quality stage — appearance first, the camera simulated last; the masks are not touched.  The stage reads no
    device random stream and keeps no state.  A batch in which no coin fired launches nothing.

    clahe = a `Clahe` switches the CLAHE preprocessing on (None, the default: the stage does not exist): it runs on the uint8 batch
    after the image-quality stage and immediately before the normalisation — the camera is simulated first, then normalised; the
    masks are not touched.  It draws nothing and keeps no state.

    jpeg_draws = `draw_jpeg`'s (mode [N], tables [N,2,64]) switches the JPEG compression stage on (None, the default: the stage does
    not exist): it runs on the uint8 batch after the image-quality stage and before CLAHE — the camera writes its file last, and
    preprocessing reads it; the masks are not touched.  The side must be a multiple of 16.  The stage reads no device random stream
    and keeps no state.  A batch in which no coin fired launches nothing."""

    def __init__(self, size=256, device="cuda", noise_seed=0):
        self.noise_seed, self.noise_pos = int(noise_seed), 0
        self.quality_pos = 0
        self._gauss = None
        self.size = int(size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the device-side input pipeline runs on the GPU only (no CPU fallback)")
        self._resize_tables = {}

    def _resize_table(self, in_size):
        t = self._resize_tables.get(in_size)
        if t is None:
            b, k, ks = resample_table(in_size, self.size, "bicubic")
            t = self._resize_tables[in_size] = (_dev_i32(b, self.device), _dev_i32(k, self.device), ks)
        return t

    def _resample(self, src, bounds, kk, tab, ksize, L, vertical):
        N, H, W, C = src.shape
        out = torch.empty((N, L, W, C) if vertical else (N, H, L, C), dtype=torch.uint8, device=self.device)
        ops.lib().call("wtpse_resample_u8", src.data_ptr(), out.data_ptr(), bounds.data_ptr(), kk.data_ptr(),
                       0 if tab is None else tab.data_ptr(), ksize, N, H, W, C, L, int(vertical), ops.stream_ptr())
        return out

    def _augment(self, img, od1, xidx, yidx, aug_draws, noise):
        """img [N,S,S,3] uint8 (cropped), od1 [N,S,S,1] uint8 behind the index tables -> (img, mask [N,S,S]) uint8 augmented."""
        S, dev, call, st = self.size, self.device, ops.lib().call, ops.stream_ptr()
        N = img.shape[0]
        code = _dev_i32([d["k"] | (4 if d["flip_lr"] else 0) | (8 if d["flip_tb"] else 0) for d in aug_draws], dev)
        out = torch.empty_like(img)
        mask = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
        call("wtpse_aug_geometry", img.data_ptr(), od1.data_ptr(), xidx.data_ptr(), yidx.data_ptr(), code.data_ptr(), out.data_ptr(),
             mask.data_ptr(), N, S, st)
        img = out
        active = [i for i, d in enumerate(aug_draws) if d["elastic"]]
        if active:
            na = len(active)
            if self._gauss is None:
                w, radius = gaussian_weights(S * 0.08)
                self._gauss = (torch.from_numpy(w).to(dev), radius)
            w, radius = self._gauss
            if noise is None:
                u, index = device_uniform(na * 2 * S * S, self.noise_seed, self.noise_pos, dev), None
                self.noise_pos += na * 2 * S * S
            else:
                u = noise if isinstance(noise, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64))
                if tuple(u.shape) != (N, 2, S, S) or u.dtype != torch.float64:
                    raise ValueError("noise must be [%d,2,%d,%d] float64, got %s %s" % (N, S, S, tuple(u.shape), u.dtype))
                u, index = u.to(dev).contiguous(), _dev_i32(active, dev)
            tmp = torch.empty((na, 2, S, S), dtype=torch.float64, device=dev)
            disp = torch.empty_like(tmp)
            call("wtpse_aug_blur", u.data_ptr(), tmp.data_ptr(), w.data_ptr(), 0 if index is None else index.data_ptr(), radius,
                 na * 2, S, 0, 1, 1.0, st)
            call("wtpse_aug_blur", tmp.data_ptr(), disp.data_ptr(), w.data_ptr(), 0, radius, na * 2, S, 1, 0, float(2 * S), st)
            slot = np.full(N, -1, np.int32)
            slot[active] = np.arange(na)
            out, mask2 = torch.empty_like(img), torch.empty_like(mask)
            slot = _dev_i32(slot, dev)
            call("wtpse_aug_warp", img.data_ptr(), mask.data_ptr(), disp.data_ptr(), slot.data_ptr(), out.data_ptr(), mask2.data_ptr(), N, S, st)
            img, mask = out, mask2
        if any(d["sp"] is not None or d["lut"] is not None or d["rect"] is not None for d in aug_draws):
            ident = np.arange(256, dtype=np.uint8)
            lut = np.stack([ident if d["lut"] is None else np.asarray(d["lut"], np.uint8) for d in aug_draws])
            rect = np.array([(0, 0, 0, 0, 0) if d["rect"] is None else d["rect"] for d in aug_draws], np.int32)
            pts = [np.zeros(0, np.int32) if d["sp"] is None else d["sp"][1].astype(np.int32) * S + d["sp"][2].astype(np.int32)
                   for d in aug_draws]
            off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
            val = [0 if d["sp"] is None else int(d["sp"][0]) for d in aug_draws]
            max_pts = max(len(p) for p in pts)
            # every table stays referenced until the launch is queued: a temporary's block would be handed to the next allocation
            # and overwritten by its copy before the kernel reads it
            dpts = _dev_i32(np.concatenate(pts), dev) if max_pts else None
            lut, rect, off, val = torch.from_numpy(lut).to(dev), _dev_i32(rect, dev), _dev_i32(off, dev), _dev_i32(val, dev)
            call("wtpse_aug_photometric", img.data_ptr(), lut.data_ptr(), rect.data_ptr(), 0 if dpts is None else dpts.data_ptr(),
                 off.data_ptr(), val.data_ptr(), max_pts, N, S, st)
        return img, mask

    def __call__(self, images, disc_masks, draws, aug_draws=None, noise=None, mix_draws=None, quality_draws=None, clahe=None,
                 appearance_draws=None, jpeg_draws=None):
        S, dev = self.size, self.device
        N = len(images)
        assert len(disc_masks) == N and len(draws) == N and (aug_draws is None or len(aug_draws) == N)
        if jpeg_draws is not None:
            _check_jpeg_size(S)
            j_mode, j_tables = check_jpeg_params(jpeg_draws[0], jpeg_draws[1], N)
        if appearance_draws is not None:
            a_params, a_field, a_spacing = appearance_draws
            a_params, a_field = check_appearance_params(a_params, a_field, N, S, a_spacing)
        if quality_draws is not None:
            quality_draws = check_quality_params(quality_draws, N)
        if mix_draws is not None:
            _check_mix_size(S)
        if clahe is not None:
            if not isinstance(clahe, Clahe):
                raise ValueError("clahe must be a Clahe or None, got %r" % (clahe,))
            clahe.check_size(S, S)
        # ---- Resize(S): bicubic, horizontal pass then vertical pass, batched over samples of one input size
        img1 = torch.empty((N, S, S, 3), dtype=torch.uint8, device=dev)
        od1 = torch.empty((N, S, S, 1), dtype=torch.uint8, device=dev)
        groups = {}
        for i, im in enumerate(images):
            groups.setdefault(tuple(im.shape[:2]), []).append(i)
        for (H, W), idx in groups.items():
            im = torch.stack([_dev_u8(images[i], dev) for i in idx])
            md = torch.stack([_dev_u8(disc_masks[i], dev) for i in idx]).unsqueeze(-1)
            sel = torch.tensor(idx, device=dev)
            for src, dst in ((im, img1), (md, od1)):
                t = src
                if W != S:
                    b, k, ks = self._resize_table(W)
                    t = self._resample(t, b, k, None, ks, S, False)
                if H != S:
                    b, k, ks = self._resize_table(H)
                    t = self._resample(t, b, k, None, ks, S, True)
                dst[sel] = t
        # ---- RandomScaleCrop(S): bilinear up-scale to (nw, nh) and crop, only for the S columns / rows that survive;
        # unscaled samples get the identity table.  The disc mask's NEAREST resize + crop is an index gather.
        hb, hk, vb, vk, xi, yi = [], [], [], [], [], []
        for nw, nh, x1, y1 in draws:
            b, k, ks = resample_table(S, nw, "bilinear", x1, S)
            hb.append(b); hk.append(k)
            b, k, ks = resample_table(S, nh, "bilinear", y1, S)
            vb.append(b); vk.append(k)
            xi.append(nearest_table(S, nw, x1, S))
            yi.append(nearest_table(S, nh, y1, S))
        tab = torch.arange(N, dtype=torch.int32, device=dev)
        t = self._resample(img1, _dev_i32(np.stack(hb), dev), _dev_i32(np.stack(hk), dev), tab, 3, S, False)
        img2 = self._resample(t, _dev_i32(np.stack(vb), dev), _dev_i32(np.stack(vk), dev), tab, 3, S, True)
        image = torch.empty((N, 3, S, S), dtype=torch.float32, device=dev)
        od = torch.empty((N, 1, S, S), dtype=torch.float32, device=dev)
        oc = torch.empty((N, 1, S, S), dtype=torch.float32, device=dev)
        xidx, yidx = _dev_i32(np.stack(xi), dev), _dev_i32(np.stack(yi), dev)
        if aug_draws is not None:
            # the augmentation stage leaves the mask cropped: input_finish reads it through identity tables
            img2, od1 = self._augment(img2, od1, xidx, yidx, aug_draws, noise)
            xidx = yidx = torch.arange(S, dtype=torch.int32, device=dev).repeat(N, 1).contiguous()
        if mix_draws is not None:
            partner, lam, b = mix_draws
            if np.any(np.asarray(partner) >= 0):
                img2 = ops.amplitude_mix(img2, partner, lam, b)
        if appearance_draws is not None and not appearance_is_neutral(a_params).all():
            img2 = ops.appearance_nets(img2, a_params, a_field, a_spacing)
        if quality_draws is not None and not quality_is_neutral(quality_draws).all():
            # (the seed as the C ABI sees it: ctypes reduces wtpse_uniform_f64's modulo 2^64 too)
            img2, self.quality_pos = ops.image_quality(img2, quality_draws, self.noise_seed & ((1 << 64) - 1), self.quality_pos, want_pos=True)
        if jpeg_draws is not None and not jpeg_is_neutral(j_mode).all():
            img2 = ops.jpeg_roundtrip(img2, j_mode, j_tables)
        if clahe is not None:
            img2 = ops.clahe(img2, clahe)
        ops.lib().call("wtpse_input_finish", img2.data_ptr(), od1.data_ptr(), xidx.data_ptr(), yidx.data_ptr(), image.data_ptr(),
                       od.data_ptr(), oc.data_ptr(), N, S, ops.stream_ptr())
        return image, od, oc
