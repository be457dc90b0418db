"""Optional random appearance networks (`AppearanceNets`, `draw_appearance`, `appearance_host`; csrc/appearance.hip): a sample is
centred on its mean and pushed through one or two shallow convolutional networks whose weights are drawn anew for every sample,
scaled back to its energy and, with two networks, blended through a smooth random field (GIN / IPA, RandConv — PAPERS.md) — after
amplitude mixing and before the image-quality stage.  No counterpart in the reference: the stage is defined in fixed point,
`appearance_host` (numpy int64) is its specification and the device equals it byte for byte (tests/test_appearance_gpu.py).  Its
effect on the Dice / HD95 of a held-out domain has not been measured.
"""
import math

import numpy as np

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
