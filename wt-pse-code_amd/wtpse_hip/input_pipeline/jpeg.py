"""Optional JPEG compression stage (`JpegCompression`, `draw_jpeg`, `jpeg_host`; csrc/jpeg.hip): baseline JPEG's round trip of the
pixels — colour conversion, 4:2:0 or 4:4:4 chroma, libjpeg's "islow" DCTs around the quantiser, "fancy" upsampling — without the
entropy coder, after the image-quality stage and before CLAHE: the file the camera writes last.  The sides are multiples of 16.
Unlike the other stages' specifications `jpeg_host` (numpy int64) is not this project's own: it equals, byte for byte, what Pillow
reads back from the file it writes (tests/test_jpeg_cpu.py), and the device equals it byte for byte (tests/test_jpeg_gpu.py).  Its
effect on the Dice / HD95 of a held-out domain has not been measured.
"""
import numpy as np

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
