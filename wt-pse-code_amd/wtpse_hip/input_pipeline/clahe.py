"""Optional CLAHE preprocessing (`Clahe`, `clahe_host`, `clahe_axis_table`; csrc/clahe.hip): contrast-limited adaptive histogram
equalisation of the uint8 batch, the last step before the normalisation — not an augmentation: it draws nothing, and the same
`Clahe` belongs in front of the networks at validation and prediction time (labelled_split.ClaheTestBatches, segment.Segmenter; a run's
checkpoints record it).  Defined in integers after OpenCV's createCLAHE, not byte-equal to it; `clahe_host` (numpy int64) is the
specification and the device equals it byte for byte (tests/test_clahe_gpu.py).
"""
import numpy as np

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


def check_clahe(clahe, H, W):
    """-> clahe, after the checks every front makes (ValueError otherwise): a `Clahe`, and one that fits H x W pictures."""
    if not isinstance(clahe, Clahe):
        raise ValueError("clahe must be an input_pipeline.Clahe or None, got %r" % (clahe,))
    clahe.check_size(H, W)
    return clahe


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
