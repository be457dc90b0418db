"""Boundary loss (Kervadec et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019): the specification on the host
(numpy, integers / float64) of what csrc/boundary.hip computes on the device, and the weight schedule of a run.

The loss of one call is  L_B = mean(sigmoid(logit) * phi)  with phi the SIGNED DISTANCE MAP of the label: the Euclidean distance to
the label's contour, positive outside the object and negative inside, in pixels (un-normalised).  It is used on top of the region
loss with a weight alpha that grows over the run:  L = L_seg + alpha * L_B.

phi of one plane `t` (nonzero = object, the convention of `ops.seg_metrics`), with pos = {t != 0}:
    d2_out[p] = min over q in pos      of |p - q|^2      (exact integer)
    d2_in[p]  = min over q not in pos  of |p - q|^2
    phi[p]    = sqrt(d2_out[p]) outside,  1 - sqrt(d2_in[p]) inside
which is Kervadec's one_hot2dist, `edt(neg) * neg - (edt(pos) - 1) * pos` with scipy's distance_transform_edt (an object pixel next
to the background has phi = 0).  DELIBERATE DEFINITION: a plane without a contour — pos empty or pos everything — has phi = 0
everywhere.  (The reference code does the same for the empty plane; for the all-foreground plane scipy measures the distance to a
background pixel that does not exist and its answer means nothing.)  Where the set a distance is taken to is empty, the squared
distance maps hold -1.
"""
import math

import numpy as np

from .terms import WeightSchedule


def _plane(t):
    t = np.asarray(t)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("a label plane is a non-empty 2-D array, got shape %s" % (t.shape,))
    return t


def _d2_to_set(member, chunk):
    """[h, w] int32: squared distance of every pixel to the nearest True pixel of `member`, by comparing all pairs; -1 when there is none."""
    h, w = member.shape
    ys, xs = np.nonzero(member)
    if ys.size == 0:
        return np.full((h, w), -1, dtype=np.int32)
    if ys.size == h * w:                             # every pixel is its own nearest member
        return np.zeros((h, w), dtype=np.int32)
    ys, xs = ys.astype(np.int32), xs.astype(np.int32)
    py, px = np.divmod(np.arange(h * w, dtype=np.int32), np.int32(w))
    out = np.empty(h * w, dtype=np.int32)
    step = max(1, int(chunk) // ys.size)
    for i in range(0, h * w, step):
        dy = py[i:i + step, None] - ys[None, :]
        dx = px[i:i + step, None] - xs[None, :]
        out[i:i + step] = (dy * dy + dx * dx).min(axis=1)
    return out.reshape(h, w)


def squared_distances_host(t, chunk=1 << 22):
    """-> (d2_out, d2_in), int32 [h, w]: the exact squared Euclidean distance of every pixel to the nearest object pixel / to the
    nearest background pixel of the plane `t` (0 on the set itself, -1 where the set is empty).  All pairs are compared, `chunk`
    pair distances at a time: O((h w)^2) — the yardstick for small planes; `squared_distances_separable_host` gives the same
    integers for large ones."""
    pos = _plane(t) != 0
    return _d2_to_set(pos, chunk), _d2_to_set(~pos, chunk)


def _d2_separable(member):
    h, w = member.shape
    if not member.any():
        return np.full((h, w), -1, dtype=np.int32)
    big = np.int64(1) << 40
    rows = np.arange(h, dtype=np.int64)
    g2 = np.empty((h, w), dtype=np.int64)            # squared vertical distance to the nearest member of the column
    for x in range(w):
        r = rows[member[:, x]]
        g2[:, x] = big if r.size == 0 else ((rows[:, None] - r[None, :]) ** 2).min(axis=1)
    cols = np.arange(w, dtype=np.int64)
    dx2 = (cols[:, None] - cols[None, :]) ** 2       # [x, q]
    out = np.empty((h, w), dtype=np.int32)
    for y in range(h):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return out


def squared_distances_separable_host(t):
    """The same two integer maps as `squared_distances_host`, column distances first and a min-plus over each row second
    (O(h w (h + w))): no pair of pixels is skipped, so it is exact as well."""
    pos = _plane(t) != 0
    return _d2_separable(pos), _d2_separable(~pos)


def signed_distance_from_d2(d2_out, d2_in):
    """phi (float64) from the two squared-distance maps; a plane without a contour (a -1 in either map) is all zero."""
    d2_out, d2_in = np.asarray(d2_out), np.asarray(d2_in)
    if (d2_out < 0).any() or (d2_in < 0).any():
        return np.zeros(d2_out.shape, dtype=np.float64)
    inside = d2_out == 0
    return np.where(inside, 1.0 - np.sqrt(d2_in.astype(np.float64)), np.sqrt(d2_out.astype(np.float64)))


def signed_distance_host(t, chunk=1 << 22):
    """The signed distance map phi (float64 [h, w]) of one label plane: see the module's docstring.  phi = 0 on a plane whose
    object is empty or fills it (a definition: there is no contour to measure from)."""
    return signed_distance_from_d2(*squared_distances_host(t, chunk))


def _sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def boundary_loss_host(x, phi, mask=None):
    """L_B = (1/n) sum_i sigmoid(x_i m_i) phi_i over all elements, in float64 (mask None: m = 1 — the disc call; the cup call
    passes od_pred, which multiplies the logits exactly as in `ops.bce_logits_pw_fwd`).  The weight is not applied."""
    x, phi = np.asarray(x, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    z = x if mask is None else x * np.asarray(mask, dtype=np.float64)
    return float(math.fsum((_sigmoid(z) * phi).ravel()) / x.size)


def boundary_grad_host(x, phi, alpha, mask=None):
    """d(alpha L_B)/dx in float64: alpha / n * phi_i * s_i (1 - s_i) [* m_i], s = sigmoid(x m)."""
    x, phi = np.asarray(x, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    m = 1.0 if mask is None else np.asarray(mask, dtype=np.float64)
    z = x * m
    e = np.exp(-np.abs(z))
    return float(alpha) / x.size * phi * (e / (1.0 + e) ** 2) * m


class BoundaryLoss(WeightSchedule):
    """The boundary term of a run and its weight schedule: alpha = weight_at(epoch) = min(cap, weight + ramp * epoch) — Kervadec's
    "increase" strategy (start small, add a constant per epoch), capped.  `TrainStep(boundary=)` / `TrainRun(boundary=)` take one."""

    def __init__(self, weight=0.01, ramp=0.01, cap=1.0):
        self._nonneg(weight=weight, ramp=ramp, cap=cap)
        self.weight, self.ramp, self.cap = float(weight), float(ramp), float(cap)

    def config(self):
        return {"weight": self.weight, "ramp": self.ramp, "cap": self.cap}

    def __repr__(self):
        return "BoundaryLoss(weight=%r, ramp=%r, cap=%r)" % (self.weight, self.ramp, self.cap)
