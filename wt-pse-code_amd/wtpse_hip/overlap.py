"""Soft Dice / Tversky / focal Tversky overlap loss, per image: the specification on the host (numpy, float64) of what
csrc/overlap.hip computes on the device, and the weight schedule of a run.

Per call, x = logits [B, 1, H, W], t = target, m = the ROI mask (od_pred) of the cup call, m = 1 for the disc call:
    z_i = x_i m_i,   s_i = sigmoid(z_i)  (from e = exp(-|z|), as boundary._sigmoid)
and per plane b (one image), over its H W pixels,
    TP = sum m s t,   FP = sum m s (1 - t),   FN = sum m (1 - s) t
    TI_b = (TP + eps) / (TP + a FP + b FN + eps)                  (a = fp, b = fn, eps = smooth)
    L_b  = (1 - TI_b)^g                                           (g = focal)
    L_ov = mean over the B planes of L_b — per image, as validate.py averages Dice.
a = b = 0.5 is soft Dice (Milletari et al. 2016): TI = (2 TP + 2 eps) / (sum m s + sum m t + 2 eps).  Other a, b: the Tversky index
(Salehi et al. 2017); b > a punishes false negatives more — the tool for a small structure such as the cup.  g != 1: focal Tversky.
`focal` is the exponent APPLIED to 1 - TI.  Abraham & Khan (2019) write (1 - TI)^(1/gamma) with gamma in [1, 3]: their gamma = 4/3
is focal = 0.75 here.  (The other published convention raises to gamma itself; that gamma is `focal` unchanged.)

DELIBERATE DEFINITIONS
1. All three sums carry the factor m.  Outside the ROI the masked logit is 0 and s = 0.5 whatever the network does: left in, those
   pixels would add a constant 0.5 each to FP and swamp the cup's own sums.  Cup pixels outside the predicted disc are left out of FN
   for the same reason: the cup call cannot reach them.
2. Where 1 - TI_b <= 0 — in exact arithmetic only == 0 can happen: an empty target with s underflowed to 0, an all-foreground target
   with s = 1, a plane with m = 0 everywhere (TI = eps / eps) — the plane's loss and its whole gradient are 0.  This is decided before
   any power with exponent g - 1 < 0 is taken: no inf * 0.  (A NaN is not <= 0 and goes through.)

The device accumulates sum m s t, sum m s and sum m t and takes FP and FN as differences; for t in [0, 1] that is the same number
up to float64 rounding.
"""
import math

import numpy as np

from .boundary import _sigmoid
from .terms import WeightSchedule


def _params(fp, fn, focal, smooth):
    a, b, g, eps = float(fp), float(fn), float(focal), float(smooth)
    if not (a >= 0 and b >= 0 and a + b > 0 and g > 0 and eps > 0 and all(math.isfinite(v) for v in (a, b, g, eps))):
        raise ValueError("overlap loss: fp, fn >= 0 with fp + fn > 0, focal > 0, smooth > 0 (finite), got %r" % ((fp, fn, focal, smooth),))
    return a, b, g, eps


def _planes(x, t, mask):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim < 2 or x.size == 0:
        raise ValueError("overlap loss: logits [B, ..., H, W], got shape %s" % (x.shape,))
    B = x.shape[0]
    x = x.reshape(B, -1)
    t = np.asarray(t, dtype=np.float64).reshape(B, -1)
    m = np.ones_like(x) if mask is None else np.asarray(mask, dtype=np.float64).reshape(B, -1)
    if t.shape != x.shape or m.shape != x.shape:
        raise ValueError("overlap loss: target and mask must have the logits' number of elements")
    return x, t, m


def _index(x, t, m, a, b, eps):
    """Per plane: s, N = TP + eps, D = TP + a FP + b FN + eps, u = 1 - N / D."""
    s = _sigmoid(x * m)
    tp = np.array([math.fsum(r) for r in m * s * t])
    fp = np.array([math.fsum(r) for r in m * s * (1.0 - t)])
    fn = np.array([math.fsum(r) for r in m * (1.0 - s) * t])
    N = tp + eps
    D = tp + a * fp + b * fn + eps
    return s, N, D, 1.0 - N / D


def overlap_planes_host(x, t, mask=None, fp=0.5, fn=0.5, focal=1.0, smooth=1.0):
    """[B] float64: L_b = (1 - TI_b)^focal of every plane (0 where 1 - TI_b <= 0)."""
    a, b, g, eps = _params(fp, fn, focal, smooth)
    x, t, m = _planes(x, t, mask)
    _, _, _, u = _index(x, t, m, a, b, eps)
    out = np.zeros(x.shape[0], dtype=np.float64)
    for k, uk in enumerate(u):
        if not uk <= 0.0:
            out[k] = uk if g == 1.0 else uk ** g
    return out


def overlap_loss_host(x, t, mask=None, fp=0.5, fn=0.5, focal=1.0, smooth=1.0):
    """L_ov = mean over the planes of L_b, float64.  The weight is not applied."""
    planes = overlap_planes_host(x, t, mask, fp, fn, focal, smooth)
    return float(math.fsum(planes) / planes.size)


def overlap_grad_host(x, t, weight, mask=None, fp=0.5, fn=0.5, focal=1.0, smooth=1.0):
    """d(weight L_ov)/dx in float64, of x's shape.  With N = TP + eps, D = TP + a FP + b FN + eps:
        dTI/ds_i  = m_i [t_i D - N (t_i + a (1 - t_i) - b t_i)] / D^2
        dL_b/dTI  = -g (1 - TI)^(g - 1)
        d(w L_ov)/dx_i = (w / B) dL_b/dTI dTI/ds_i s_i (1 - s_i) m_i
    and all zero on a plane with 1 - TI <= 0."""
    a, b, g, eps = _params(fp, fn, focal, smooth)
    shape = np.asarray(x).shape
    x, t, m = _planes(x, t, mask)
    B = x.shape[0]
    s, N, D, u = _index(x, t, m, a, b, eps)
    e = np.exp(-np.abs(x * m))
    ds = e / (1.0 + e) ** 2                          # s (1 - s), without the cancellation of 1 - s
    out = np.zeros_like(x)
    for k in range(B):
        if u[k] <= 0.0:
            continue
        dL = -g * (1.0 if g == 1.0 else u[k] ** (g - 1.0))
        dTI = m[k] * (t[k] * D[k] - N[k] * (t[k] + a * (1.0 - t[k]) - b * t[k])) / (D[k] * D[k])
        out[k] = (float(weight) / B) * dL * dTI * ds[k] * m[k]
    return out.reshape(shape)


class OverlapLoss(WeightSchedule):
    """The overlap term of a run and its weight schedule: w = weight_at(epoch) = min(cap, weight + ramp * epoch) (cap None: no cap).
    fp / fn weigh false positives / false negatives (0.5, 0.5: soft Dice), focal is the exponent of 1 - TI, smooth the eps of the
    index.  `TrainStep(overlap=)` / `TrainRun(overlap=)` take one."""

    def __init__(self, weight=1.0, fp=0.5, fn=0.5, focal=1.0, smooth=1.0, ramp=0.0, cap=None):
        self._nonneg(weight=weight, fp=fp, fn=fn, focal=focal, smooth=smooth, ramp=ramp, **({} if cap is None else {"cap": cap}))
        if fp + fn <= 0:
            raise ValueError("OverlapLoss: fp + fn must be > 0, got fp=%r, fn=%r" % (fp, fn))
        for name, v in (("focal", focal), ("smooth", smooth)):
            if v <= 0:
                raise ValueError("OverlapLoss: %s must be > 0, got %r" % (name, v))
        self.weight, self.fp, self.fn, self.focal, self.smooth = float(weight), float(fp), float(fn), float(focal), float(smooth)
        self.ramp, self.cap = float(ramp), None if cap is None else float(cap)

    def config(self):
        return {"weight": self.weight, "fp": self.fp, "fn": self.fn, "focal": self.focal, "smooth": self.smooth, "ramp": self.ramp,
                "cap": self.cap}

    def __repr__(self):
        return "OverlapLoss(weight=%r, fp=%r, fn=%r, focal=%r, smooth=%r, ramp=%r, cap=%r)" % (
            self.weight, self.fp, self.fn, self.focal, self.smooth, self.ramp, self.cap)
