"""The resampling tables of the device input pipeline and the crop's draws.

The coefficient tables are Pillow's (src/libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc; Geometry.c
ImagingScaleAffine for NEAREST), computed here with the same double-precision operations in the same order.

The reference draws from Python's `random` module (`seed = random.random()`, two `random.uniform(1, 1.5)`, two `random.randint`
for the crop); `draw()` makes the same draws in the same order from any `random.Random`-like generator, so a seeded run crops
exactly like the reference.
"""
import math

import numpy as np

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
