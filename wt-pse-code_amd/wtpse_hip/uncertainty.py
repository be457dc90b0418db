"""Sampled shape latents: how far to trust a prediction.

The student shape network predicts a mean and a log-variance per pixel; the deterministic prediction (WT_PSE.predict) uses the
mean alone.  Drawing K latents z_k = mu + scale * exp(logvar / 2) * eps_k — the teacher's reparameterisation (reference
algorithms.py:1068-1075), the form the segmentation head was trained under — and pushing each through the attention, the fusion
and the 1x1 output convolution gives K predictions per pixel, from which follow their mean, their spread, a vote count and, per
sample, the cup-to-disc ratios.  Everything behind the latent is pointwise, so the device does all K in ONE launch
(ops.shape_samples, csrc/uncertainty.hip) behind a single pass of the two U-Nets (WT_PSE.predict_samples,
validate.predict_pair_samples, segment.Segmenter(samples=K)).

This module holds the host side: `shape_samples_host`, the numpy fp64 specification of the launch (it sits beside the device path as
augment_host, overlay_host and mask_geometry_host do), the result record, and the arithmetic of uncertainty.csv.
"""
import os

import numpy as np

from . import tables as T

RATIOS = ("vcdr", "hcdr", "acdr")
STATS = ("mean", "std", "p05", "p95")
CSV_COLUMNS = ("index", "name", "n_samples", "n_defined") + tuple("%s_%s" % (r, s) for r in RATIOS for s in STATS) + \
    ("disc_disagree_px", "cup_disagree_px", "disc_std_mean", "cup_std_mean")
INT_COLUMNS = ("index", "n_samples", "n_defined", "disc_disagree_px", "cup_disagree_px")


class ShapeSamples:
    """What WT_PSE.predict_samples returns: mean, std [B,1,H,W] fp32 and votes [B,1,H,W] uint8 over the K sampled predictions,
    logits [B,K,H,W] (None unless asked for), and the deterministic `logit` [B,1,H,W] / `pre` (pre-sigmoid attention) of predict()
    from the same U-Net pass.  n_samples, seed, offset, scale: the draw."""
    __slots__ = ("mean", "std", "votes", "logits", "logit", "pre", "n_samples", "seed", "offset", "scale")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def shape_samples_host(emb, mu, logvar, w, b, coef, wout, bout, wz, eps, scale=1.0, threshold=0.75):
    """The specification of wtpse_shape_samples in float64.  emb [B,CE,...], mu / logvar [B,...] or [B,1,...], eps [B,K,...] standard
    normals (trailing dimensions of equal size); w, b: the attention layer; wout [CE], bout: the output convolution; wz: the latent's
    own weight of a cat_shape head or None.  Per sample
        z = mu + scale * std * eps,  std = exp(logvar / 2) with non-finite values set to 0
        a = sigmoid(w z + b),  fuse[c] = coef emb[c] + a emb[c],  logit = sum_c wout[c] fuse[c] + bout (+ wz z),  p = sigmoid(logit)
    -> {"logits" [B,K,...], "mean", "std" [B,...] (population standard deviation by a running Welford update: K equal samples give
    exactly 0), "votes" [B,...] uint8 = #{k: p > threshold}}."""
    emb = np.asarray(emb, np.float64)
    B, CE = emb.shape[:2]
    emb = emb.reshape(B, CE, -1)
    mu = np.asarray(mu, np.float64).reshape(B, -1)
    logvar = np.asarray(logvar, np.float64).reshape(B, -1)
    eps = np.asarray(eps, np.float64)
    K, tail = eps.shape[1], eps.shape[2:]
    eps = eps.reshape(B, K, -1)
    wout = np.asarray(wout, np.float64).reshape(-1)
    if not (emb.shape[2] == mu.shape[1] == logvar.shape[1] == eps.shape[2] and wout.shape[0] == CE and K >= 1 and scale >= 0):
        raise ValueError("shape_samples_host: emb %s, mu %s, logvar %s, eps %s, wout %s" % (emb.shape, mu.shape, logvar.shape, eps.shape, wout.shape))
    with np.errstate(over="ignore", invalid="ignore"):
        std = np.exp(logvar / 2)
    std = np.where(np.isfinite(std), std, 0.0)
    logits = np.empty_like(eps)
    mean, m2, votes = np.zeros_like(mu), np.zeros_like(mu), np.zeros(mu.shape, np.int64)
    for k in range(K):
        z = mu + float(scale) * std * eps[:, k]
        a = _sigmoid(float(w) * z + float(b))
        fuse = float(coef) * emb + a[:, None] * emb
        logit = np.tensordot(fuse, wout, axes=([1], [0])) + float(bout)
        if wz is not None:
            logit = logit + float(wz) * z
        logits[:, k] = logit
        p = _sigmoid(logit)
        d = p - mean
        mean = mean + d / (k + 1)
        m2 = m2 + d * (p - mean)
        votes += p > threshold
    shape = (B,) + tuple(tail)
    return {"logits": logits.reshape((B, K) + tuple(tail)), "mean": mean.reshape(shape), "std": np.sqrt(np.maximum(m2, 0.0) / K).reshape(shape),
            "votes": votes.astype(np.uint8).reshape(shape)}


# ---- uncertainty.csv ------------------------------------------------------------------------------------------------------
def ratio_statistics(samples):
    """samples: the `segment.measure` rows of one image's K samples -> {n_samples, n_defined, <ratio>_mean / _std / _p05 / _p95}.  A
    sample with an empty disc has no ratio: it is left out and n_defined counts the others; with none left every statistic is nan.
    std is the population standard deviation, the percentiles numpy.percentile's (linear interpolation), all in float64."""
    keep = [s for s in samples if s["disc_area"] > 0]
    out = {"n_samples": len(samples), "n_defined": len(keep)}
    for r in RATIOS:
        v = np.array([s[r] for s in keep], np.float64)
        if len(v):
            vals = (float(v.mean()), float(v.std()), float(np.percentile(v, 5)), float(np.percentile(v, 95)))
        else:
            vals = (float("nan"),) * 4
        out.update({"%s_%s" % (r, s): x for s, x in zip(STATS, vals)})
    return out


def map_statistics(votes, std, n_samples):
    """One image's vote map (uint8) and spread map of one class -> (pixels the samples disagree on: 0 < votes < K, mean spread)."""
    votes = np.asarray(votes)
    return int(((votes > 0) & (votes < n_samples)).sum()), float(np.asarray(std, np.float64).mean())


def std_picture(std_disc, std_cup):
    """Two spread maps [h,w] -> the RGB picture [h,w,3] uint8: R = round(255 min(1, 2 std_disc)), G the same for the cup, B = 0 (a
    population standard deviation of values in [0, 1] is at most 0.5)."""
    chan = lambda s: np.rint(255.0 * np.minimum(1.0, 2.0 * np.maximum(np.asarray(s, np.float64), 0.0))).astype(np.uint8)
    r = chan(std_disc)
    return np.stack((r, chan(std_cup), np.zeros_like(r)), -1)


def write_csv(out_dir, rows):
    """rows: [{CSV_COLUMNS}] -> out_dir/uncertainty.csv (tables.write_csv's form)."""
    T.write_csv(os.path.join(out_dir, "uncertainty.csv"), CSV_COLUMNS, rows, INT_COLUMNS)


def read_csv(out_dir):
    return T.read_csv(os.path.join(out_dir, "uncertainty.csv"), INT_COLUMNS)
