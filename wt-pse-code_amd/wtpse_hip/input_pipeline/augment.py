"""Optional augmentation stage (`Augment`, `draw_augment`, `augment_host`; csrc/augment.hip): the reference's RandomRotate,
RandomFlip, elastic_transform, add_salt_pepper_noise, adjust_light and eraser (custom_transforms.py:310-327,204-217,87-132,22-43,
45-55,58-85), in that order, between the crop and the normalisation.  Again the draws are made on the host, in the reference's
order, and the pixels are produced on the GPU, bit for bit; `augment_host` is the numpy specification of the device stage.
"""
import numpy as np


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
