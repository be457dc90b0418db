"""Lovász hinge loss (Berman, Triki & Blaschko, "The Lovász-Softmax loss", CVPR 2018: the binary form), per image: the specification
on the host (numpy: fp32 errors, integer counts, float64 sums) of what csrc/lovasz.hip computes on the device, and the weight schedule
of a run.  It is the convex surrogate of the Jaccard index itself, where the soft Dice of overlap.py is a smoothed copy of it.

Per call, x = logits [B, 1, H, W] (fp32), t = target, m = the ROI mask (od_pred) of the cup call, None for the disc call.  A pixel is
KEPT iff m is None or m_i != 0: an ignored pixel is taken out of the set (Berman's `ignore`), not multiplied in, and the logit of a
kept pixel is x_i itself.  Per plane b (one image), over its kept pixels:
    1. sign_i = +1 where t_i > 0, else -1;  e_i = 1 - x_i sign_i IN FP32 — the product is exact, so e_i is rounded once
       (fmaf(-x, sign, 1) on the device, np.float32(1) - x * sign here): the sort keys are the same bits on both sides.
    2. the kept pixels ordered by e descending, ties by ascending pixel index (np.argsort(-e, kind="stable")).
    3. G = kept foreground pixels; for position r = 1 .. n: c_r = foreground among the first r, and in float64
           J_r = 1 - (G - c_r) / (G + r - c_r)        (the denominator is >= 1)
           g_1 = J_1,  g_r = J_r - J_{r-1}            (J never decreases along the order: every g_r >= 0)
    4. L_b = sum_r max(e_(r), 0) g_r (float64, math.fsum); a plane without a kept pixel has L_b = 0.
       L_lv = mean over the B planes of L_b — per image, as validate.py averages.
    5. the gradient of w L_lv with the order and g held constant, as in the published implementation:
           d/dx_i = (w / B) (-sign_i) g_rank(i)       for a kept pixel with e_i > 0
       and exactly 0 everywhere else: ignored pixels and e_i <= 0.
    6. a kept pixel with a non-finite logit makes its plane's L_b NaN (the call's NaN test sees it); such a plane adds nothing to
       the gradient.
Pixels with e <= 0 come behind every pixel with e > 0 and add nothing to value or gradient: the device sorts the positive errors
only, while G counts every kept foreground pixel — the same numbers.
"""
import math

import numpy as np

from .terms import WeightSchedule


def _planes(x, t, mask):
    """-> x [B, n] fp32, foreground [B, n] bool, kept [B, n] bool."""
    x = np.asarray(x)
    if x.ndim < 2 or x.size == 0:
        raise ValueError("lovasz loss: logits [B, ..., H, W], got shape %s" % (x.shape,))
    B = x.shape[0]
    x = x.astype(np.float32).reshape(B, -1)
    fg = np.asarray(t).reshape(B, -1) > 0
    keep = np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask).reshape(B, -1) != 0
    if fg.shape != x.shape or keep.shape != x.shape:
        raise ValueError("lovasz loss: target and mask must have the logits' number of elements")
    return x, fg, keep


def _errors(x, fg):
    """e = 1 - x sign in fp32 (one rounding) and sign."""
    sign = np.where(fg, np.float32(1), np.float32(-1))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(1) - x * sign, sign


def _sorted_plane(e, fg, keep):
    """One plane: (idx, g): the kept pixels in the order of step 2 and their g_r (float64)."""
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(-e[idx], kind="stable")]
    n = idx.size
    G = int(fg[idx].sum())
    c = np.cumsum(fg[idx].astype(np.int64))
    r = np.arange(1, n + 1, dtype=np.int64)
    J = 1.0 - (G - c).astype(np.float64) / (G + r - c).astype(np.float64)
    g = np.diff(J, prepend=0.0)
    return idx, g


def _bad(x, keep):
    """[B] bool: the plane holds a kept pixel with a non-finite logit."""
    return (keep & ~np.isfinite(x)).any(axis=1)


def lovasz_planes_host(x, t, mask=None):
    """[B] float64: L_b of every plane (0 without a kept pixel, NaN with a non-finite kept logit)."""
    x, fg, keep = _planes(x, t, mask)
    e, _ = _errors(x, fg)
    bad = _bad(x, keep)
    out = np.zeros(x.shape[0], dtype=np.float64)
    for b in range(x.shape[0]):
        if bad[b]:
            out[b] = math.nan
            continue
        idx, g = _sorted_plane(e[b], fg[b], keep[b])
        out[b] = math.fsum(np.maximum(e[b][idx].astype(np.float64), 0.0) * g)
    return out


def lovasz_loss_host(x, t, mask=None):
    """L_lv = mean over the planes of L_b, float64.  The weight is not applied."""
    planes = lovasz_planes_host(x, t, mask)
    return float(math.fsum(planes) / planes.size) if np.isfinite(planes).all() else math.nan


def lovasz_grad_host(x, t, weight, mask=None):
    """d(weight L_lv)/dx in float64, of x's shape: (weight / B) (-sign_i) g_rank(i) at a kept pixel with e_i > 0, 0 elsewhere; all
    zero on a plane with a non-finite kept logit."""
    shape = np.asarray(x).shape
    x, fg, keep = _planes(x, t, mask)
    e, sign = _errors(x, fg)
    bad = _bad(x, keep)
    B = x.shape[0]
    out = np.zeros(x.shape, dtype=np.float64)
    for b in range(B):
        if bad[b]:
            continue
        idx, g = _sorted_plane(e[b], fg[b], keep[b])
        live = e[b][idx] > 0
        out[b][idx[live]] = (float(weight) / B) * (-sign[b][idx[live]].astype(np.float64)) * g[live]
    return out.reshape(shape)


def lovasz_ranks_host(x, t, mask=None):
    """int32, of x's shape: the 0-based place in its plane's order of every kept pixel with e > 0, -1 elsewhere."""
    shape = np.asarray(x).shape
    x, fg, keep = _planes(x, t, mask)
    e, _ = _errors(x, fg)
    out = np.full(x.shape, -1, dtype=np.int32)
    for b in range(x.shape[0]):
        idx = np.flatnonzero(keep[b] & (e[b] > 0))
        idx = idx[np.argsort(-e[b][idx], kind="stable")]
        out[b][idx] = np.arange(idx.size, dtype=np.int32)
    return out.reshape(shape)


class LovaszLoss(WeightSchedule):
    """The Lovász hinge term of a run and its weight schedule: w = weight_at(epoch) = min(cap, weight + ramp * epoch) (cap None: no
    cap).  The loss itself has no parameters.  `TrainStep(lovasz=)` / `TrainRun(lovasz=)` take one."""

    def __init__(self, weight=1.0, ramp=0.0, cap=None):
        self._nonneg(weight=weight, ramp=ramp, **({} if cap is None else {"cap": cap}))
        self.weight, self.ramp, self.cap = float(weight), float(ramp), None if cap is None else float(cap)

    def config(self):
        return {"weight": self.weight, "ramp": self.ramp, "cap": self.cap}

    def __repr__(self):
        return "LovaszLoss(weight=%r, ramp=%r, cap=%r)" % (self.weight, self.ramp, self.cap)
