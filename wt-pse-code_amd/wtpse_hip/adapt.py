"""Adapting BatchNorm statistics to an unlabelled target site: the label-free first step of test-time adaptation (AdaBN, Li et al.
2016; prediction-time BatchNorm, Nado et al. 2020; source / target blending with a pseudo-count, Schneider et al. 2020 — PAPERS.md).

An eval-mode BatchNorm normalises by the running ("source") statistics.  Under a `BlendState` (HipNet.bn_blend, set by `blended`) it
normalises by the TARGET images' own statistics instead, pooled over what was seen and blended with the source's:

    mean_t = (A1 + s1) / (AM + M)         var_t = max((A2 + s2) / (AM + M) - mean_t^2, 0)         (biased, as train mode normalises)
    w      = n_seen / (N0 + n_seen)        n_seen: target IMAGES pooled, this call included; N0 >= 0: the prior strength in images
    mean_b = (1 - w) mean_s + w mean_t     var_b = (1 - w) var_s + w var_t
    scale  = gamma / sqrt(var_b + eps)     shift = beta - mean_b scale

with (s1, s2) the call's per-channel sum and sum of squares over its M = n H W values — the partials the convolutions' and the
upsampling's epilogues leave in train mode, folded in float64 — and (A1, A2, AM) the sums and count of earlier calls.  The device side
is one launch per layer (csrc/bn.hip, wtpse_bn_finalize_blend) that never writes the running buffers; this module holds the float64
host specification (`target_host`, `blend_host`, `coeffs_host`, `divergence_host`, `bound_host`, `blend_weight`) and the modes:

    batch    no history: every call is normalised by its own statistics blended with the source, n_seen = the call's batch size.
    stream   history persists: a call is normalised by everything seen so far, itself included.  Works at batch size 1; depends on the
             order of the images.
    site     `SiteStatistics.fit`: ONE stream pass of validate.predict_pair over a folder, then every layer's final blend is written
             into COPIES of the buffers (running_mean = mean_b, running_var = var_b) and returned as a checkpoint like a best-Dice one.
             The live networks are not touched.  One pass is an approximation of AdaBN: a layer's statistics were gathered while the
             layers in front of it still ran on their evolving ones.  More passes are not run.

`batch` and `stream` predictions depend on the images that share the call (and, for `stream`, on those before it); a `site` checkpoint
is an ordinary checkpoint, its predictions depend on the image alone.

    python -m wtpse_hip.adapt --images DIR --checkpoint CK --out OUT [--prior 16] [--batch-size 9] [--clahe checkpoint]

    OUT/adapted_checkpoint.pth.tar   loads wherever checkpoint_<epoch>.pth.tar does (test_run.load_checkpoint); extra entry "site",
                                     and "clahe" — the CLAHE preprocessing the statistics were fitted under — when CK has one
                                     (--clahe checkpoint, the default) or --clahe names one
    OUT/shift.csv                    SHIFT_COLUMNS, one row per BatchNorm module of the four networks: KL(N_target || N_source) per
                                     channel, its mean and maximum (images = 0: the layer does not run at prediction time, kept as is)
    OUT/shift.json                   prior, images, source, the mean divergence per network and overall: "how far is this site"

For whole photographs run wtpse_hip.locate first and pass its crop/ folder.  `segment` / `locate` take --adapt {batch,stream} --prior N0,
Segmenter the keywords adapt= / prior=.  For a labelled test split `AdaptedTestRun` is test_run.TestRun with the same two keywords;
the `test_run` and `morphometry_run` programs have no switch — give them a site checkpoint, as `calibration_run`.
Whether any of this improves Dice on a held-out domain is the user's experiment.
"""
import contextlib
import json
import os

import numpy as np
import torch

from . import ops
from . import tables as T
from .test_run import CHECKPOINT_KEYS, TestRun

EPS = float(np.float32(1e-5))          # nn.BatchNorm2d's eps as the kernels take it: a float, widened
DEFAULT_PRIOR = 16.0                   # Schneider et al.'s N
MODES = ("batch", "stream")
BOUND_HEADROOM = 2.0                   # one binade over the Samuelson bound: E[x^2] - mean^2 can undershoot the variance
SHIFT_COLUMNS = ("network", "name", "channels", "images", "div_mean", "div_max")


# ---- the specification (float64, host) ------------------------------------------------------------------------------------------
def blend_weight(n_seen, prior=DEFAULT_PRIOR):
    """w = n_seen / (N0 + n_seen): the weight of the target statistics after n_seen target images under a prior worth N0 images."""
    n, p = float(n_seen), float(prior)
    if not (n >= 0.0 and p >= 0.0) or n + p == 0.0:
        raise ValueError("blend_weight: n_seen and prior must not be negative and not both zero (got %r, %r)" % (n_seen, prior))
    return n / (p + n)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def target_host(s1, s2, count, a1=0.0, a2=0.0, acc_count=0.0):
    """Per-channel sums of this call (s1, s2 over `count` values) pooled with those of earlier calls -> (mean_t, var_t), biased."""
    n = float(acc_count) + float(count)
    mean = (_f64(a1) + _f64(s1)) / n
    var = np.maximum((_f64(a2) + _f64(s2)) / n - mean * mean, 0.0)
    return mean, var


def blend_host(mean_s, var_s, mean_t, var_t, w):
    """-> (mean_b, var_b) = (1 - w) source + w target, float64."""
    w = float(w)
    if not 0.0 <= w <= 1.0:
        raise ValueError("blend_host: w must lie in [0, 1] (got %r)" % (w,))
    return (1.0 - w) * _f64(mean_s) + w * _f64(mean_t), (1.0 - w) * _f64(var_s) + w * _f64(var_t)


def coeffs_host(gamma, beta, mean_b, var_b, eps=EPS):
    """-> float32 [C,2] = (scale, shift): float64 throughout, rounded once."""
    scale = _f64(gamma) / np.sqrt(_f64(var_b) + float(eps))
    return np.stack((scale, _f64(beta) - _f64(mean_b) * scale), axis=-1).astype(np.float32)


def divergence_host(mean_s, var_s, mean_t, var_t, eps=EPS):
    """KL(N(mean_t, var_t + eps) || N(mean_s, var_s + eps)) per channel, float64: the shift report."""
    vs, vt = _f64(var_s) + float(eps), _f64(var_t) + float(eps)
    dm = _f64(mean_t) - _f64(mean_s)
    return 0.5 * (np.log(vs / vt) + (vt + dm * dm) / vs - 1.0)


def bound_host(gamma, beta, mean_b, var_b, mean_call, var_call, count, eps=EPS, headroom=BOUND_HEADROOM):
    """A bound of |scale y + shift| over the `count` values of a call whose own (biased) statistics are (mean_call, var_call):
    |y - mean_call| <= sqrt(var_call (count - 1)) (Samuelson), so |gamma| invstd (sqrt(var_call (count - 1)) + |mean_call - mean_b|)
    + |beta|, times `headroom`.  Per channel, float64; the kernel leaves the maximum over the channels in the amax table."""
    invstd = 1.0 / np.sqrt(_f64(var_b) + float(eps))
    dev = np.sqrt(_f64(var_call) * max(float(count) - 1.0, 1.0)) + np.abs(_f64(mean_call) - _f64(mean_b))
    return float(headroom) * (np.abs(_f64(gamma)) * invstd * dev + np.abs(_f64(beta)))


# ---- the state behind HipNet.bn_blend ---------------------------------------------------------------------------------------------
class _Slot:
    """One BatchNorm module's buffers, float64 on the device: acc [C,2] (pooled sum, sum of squares; stream mode only, else None) and,
    where the state reports, moments [C,4] = (mean_t, var_t, mean_b, var_b) and div [C] of its last call (else None); images / pixels
    pooled so far (stream mode), w and count of the last call."""
    __slots__ = ("acc", "moments", "div", "images", "pixels", "w", "count", "calls")

    def __init__(self, C, device, stream, report):
        self.acc = torch.zeros((C, 2), dtype=torch.float64, device=device) if stream else None
        self.moments = torch.empty((C, 4), dtype=torch.float64, device=device) if report else None
        self.div = torch.empty((C,), dtype=torch.float64, device=device) if report else None
        self.images, self.pixels, self.w, self.count, self.calls = 0, 0, None, 0, 0


class BlendState:
    """What HipNet.bn_blend holds: the prior N0, the mode and, per BatchNorm module (allocated at its first call), a `_Slot`.
    `finalize` is what nn._bn_coeffs calls in place of ops.bn_eval_coeffs.  A state may serve several networks at once: every
    module has its own slot, its own image and pixel counts.  report=True: every launch also leaves the layer's moments and its
    divergence from the source in the slot (the shift report; off, the launch writes the coefficients and the bound alone)."""

    def __init__(self, prior=DEFAULT_PRIOR, mode="batch", report=False):
        if mode not in MODES:
            raise ValueError("mode must be one of %s (got %r)" % (", ".join(MODES), mode))
        if not float(prior) >= 0.0:
            raise ValueError("prior must not be negative (got %r)" % (prior,))
        self.prior, self.mode, self.report, self.slots = float(prior), mode, bool(report), {}

    @property
    def n_seen(self):
        """Target images pooled so far (stream mode: the most any layer has seen; batch mode keeps no history: 0)."""
        return max((s.images for s in self.slots.values()), default=0)

    def reset(self):
        self.slots = {}

    def slot(self, bn):
        s = self.slots.get(bn)
        if s is None:
            s = self.slots[bn] = _Slot(bn.weight.numel(), bn.weight.device, self.mode == "stream", self.report)
        return s

    def finalize(self, bn, y, stats, act_amax=None):
        """-> ss [C,2] of BatchNorm `bn` over the conv output y [B,C,H,W] whose (sum, sum^2) partials are `stats`."""
        B, _, H, W = y.shape
        s, count = self.slot(bn), B * H * W
        stream = self.mode == "stream"
        n_seen = s.images + B if stream else B
        s.w, s.count = blend_weight(n_seen, self.prior), count
        ss = ops.bn_finalize_blend(stats, count, bn.weight, bn.bias, bn.running_mean, bn.running_var, s.w, EPS,
                                   s.acc if stream else None, s.pixels if stream else 0, s.moments, s.div, act_amax)
        if stream:
            s.images, s.pixels = n_seen, s.pixels + count
        s.calls += 1
        return ss


def make_state(adapt, prior=DEFAULT_PRIOR):
    """The `adapt=` keyword of Segmenter / the --adapt switch -> a fresh BlendState, or None for None / "none"."""
    if adapt is None or adapt == "none":
        return None
    return BlendState(prior, adapt)


@contextlib.contextmanager
def blended(nets, state):
    """bn_blend = state on every network of `nets` for the duration of the block, what it was before restored whatever ends it.
    state None: nothing is set.  Composes with validate.eval_mode (train-mode networks ignore the switch)."""
    nets = [n for n in nets if n is not None]
    if state is None:
        yield None
        return
    before = [n.bn_blend for n in nets]
    for n in nets:
        object.__setattr__(n, "bn_blend", state)
    try:
        yield state
    finally:
        for n, b in zip(nets, before):
            object.__setattr__(n, "bn_blend", b)


def check_adapt(adapt, views=None):
    """The (adapt, views) pair a driver was given: stream mode would pool every view of an image as if it were another image."""
    if adapt not in (None, "none") + MODES:
        raise ValueError("adapt must be one of none, %s (got %r)" % (", ".join(MODES), adapt))
    if adapt == "stream" and views is not None:
        raise ValueError("--adapt stream cannot be combined with --views: every view of an image would be pooled as one more image "
                         "(use --adapt batch, or a site checkpoint from wtpse_hip.adapt)")
    return None if adapt == "none" else adapt


# ---- a labelled test split under adaptation ------------------------------------------------------------------------------------------
class AdaptedTestRun(TestRun):
    """test_run.TestRun with Segmenter's two keywords: adapt="batch" / "stream" (prior: N0) holds the networks' eval-mode BatchNorm
    layers on the batches' own statistics blended with the checkpoint's for the duration of `run` — per batch, or pooled over the
    split in its order — and bn_blend is what it was afterwards, whatever ends the run.  summary.json (and the returned means) then
    also name adapt and prior.  adapt=None, the default: TestRun itself, nothing more runs and nothing more is written."""
    __test__ = False

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, adapt=None, prior=DEFAULT_PRIOR, **kw):
        super().__init__(model, model_shape, model_oc, model_shape_oc, out_dir, **kw)
        self.adapt, self.prior = check_adapt(adapt), float(prior)
        if self.adapt is not None and not self.prior >= 0.0:
            raise ValueError("prior must not be negative (got %r)" % (prior,))

    def run(self, batches):
        if self.adapt is None:
            return super().run(batches)
        with blended(self.nets, make_state(self.adapt, self.prior)):
            means = dict(super().run(batches), adapt=self.adapt, prior=self.prior)
        T.write_json(os.path.join(self.out_dir, "summary.json"), means, allow_nan=True)
        return means


# ---- the adapted checkpoint -------------------------------------------------------------------------------------------------------
def _checkpoint_keys():
    return CHECKPOINT_KEYS


def site_checkpoint(state_dicts, updates, site, clahe=None):
    """state_dicts: the four networks' state_dicts in CHECKPOINT_KEYS order; updates: {key: {BatchNorm module name: (mean_b, var_b)}}
    -> the four-key checkpoint dict with every tensor CLONED, `<name>.running_mean / .running_var` replaced by the float32 roundings
    of the updates, plus "site" = `site` and, when `clahe` (a `Clahe.record()`) is not None, "clahe" = a copy of it.  The inputs are
    not modified."""
    out = {}
    for key, sd in zip(_checkpoint_keys(), state_dicts):
        new = {k: v.detach().clone() for k, v in sd.items()}
        for name, (mean_b, var_b) in updates.get(key, {}).items():
            for buf, val in ((name + ".running_mean", mean_b), (name + ".running_var", var_b)):
                old = new[buf]
                val = torch.from_numpy(np.asarray(val, dtype=np.float64).astype(np.float32))
                if tuple(val.shape) != tuple(old.shape):
                    raise ValueError("%s.%s: %s values for a buffer of %s" % (key, buf, tuple(val.shape), tuple(old.shape)))
                new[buf] = val.to(old.device)
        out[key] = new
    out["site"] = site
    if clahe is not None:
        out["clahe"] = dict(clahe)
    return out


def shift_rows(site):
    """The "site" entry of an adapted checkpoint -> shift.csv's rows, in the networks' module order."""
    return [dict(network=key, name=name, channels=len(layer["divergence"]), images=layer["images"],
                 div_mean=float(np.mean(layer["divergence"])) if layer["divergence"] else 0.0,
                 div_max=float(np.max(layer["divergence"])) if layer["divergence"] else 0.0)
            for key in _checkpoint_keys() for name, layer in site["layers"].get(key, {}).items()]


def shift_summary(site):
    """-> {prior, images, source, networks: {key: mean divergence}, mean_divergence}: the means run over the channels of the layers
    the pass visited (None where it visited none)."""
    per, pooled = {}, []
    for key in _checkpoint_keys():
        vals = [d for layer in site["layers"].get(key, {}).values() if layer["images"] for d in layer["divergence"]]
        per[key] = float(np.mean(vals)) if vals else None
        pooled += vals
    return dict(prior=site["prior"], images=site["images"], source=site["source"], networks=per,
                mean_divergence=float(np.mean(pooled)) if pooled else None)


def write_shift(out_dir, site):
    """-> OUT/shift.csv and OUT/shift.json (tables.py's forms); returns the summary."""
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, "shift.csv"), SHIFT_COLUMNS, shift_rows(site), ("channels", "images"), ("network", "name"))
    summary = shift_summary(site)
    T.write_json(os.path.join(out_dir, "shift.json"), summary, allow_nan=False)
    return summary


def read_shift(out_dir):
    return (T.read_csv(os.path.join(out_dir, "shift.csv"), ("channels", "images"), ("network", "name")),
            T.read_json(os.path.join(out_dir, "shift.json")))


class SiteStatistics:
    """fit(folder or batches) -> the adapted checkpoint dict of the module docstring; `self.state` keeps the pass's BlendState (its
    slots hold every visited layer's pooled sums and last moments), `self.site` the "site" entry.
    clahe: the `input_pipeline.Clahe` the source checkpoint was trained under (None: none): the folder's images pass through it on
    their way in, and the adapted checkpoint carries its record as "clahe" like its source."""

    def __init__(self, model, model_shape, model_oc, model_shape_oc, prior=DEFAULT_PRIOR, batch_size=9, size=256, clahe=None):
        self.clahe = clahe
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        self.nets = [model, model_shape, model_oc, model_shape_oc]
        self.prior, self.batch_size, self.size = float(prior), int(batch_size), int(size)
        self.state, self.site = BlendState(self.prior, "stream", report=True), None

    def _batches(self, source):
        from .segment import ImageFolder, Segmenter
        if isinstance(source, (str, os.PathLike)):
            source = ImageFolder(source)
        if not isinstance(source, ImageFolder):
            yield from source
            return
        device = next(self.nets[0].parameters()).device
        front = Segmenter(None, None, None, None, out_dir=None, size=self.size, clahe=self.clahe).front   # `segment`'s and `locate`'s loader
        for first in range(0, len(source), self.batch_size):
            yield front([source.load(i) for i in range(first, min(first + self.batch_size, len(source)))], device)

    def fit(self, source, source_name=None):
        """source: a folder / segment.ImageFolder of region-of-interest crops, or an iterable of network inputs [B,3,S,S] on the
        device.  One stream pass of validate.predict_pair in eval mode; modes and bn_blend are restored, nothing else of the live
        networks is written."""
        from . import nn as E
        from . import validate as V
        from .packed import fetch
        self.state, images = BlendState(self.prior, "stream", report=True), 0
        with V.eval_mode(self.nets), blended(self.nets, self.state):
            for image in self._batches(source):
                V.predict_pair(*self.nets, image)
                images += int(image.shape[0])
        if images < 1:
            raise ValueError("SiteStatistics.fit: no target image")
        found = [(key, name, m) for key, net in zip(_checkpoint_keys(), self.nets) for name, m in net.named_modules() if isinstance(m, E.BNP)]
        seen = [(key, name, m, self.state.slots[m]) for key, name, m in found if m in self.state.slots]
        host = iter(fetch([t for _, _, m, s in seen for t in (s.acc, m.running_mean, m.running_var)]))       # the one copy
        updates, layers = {}, {key: {} for key in _checkpoint_keys()}
        stats = {}
        for key, name, m, s in seen:
            acc, mean_s, var_s = next(host), next(host), next(host)
            mean_t, var_t = target_host(acc[:, 0], acc[:, 1], s.pixels)
            updates.setdefault(key, {})[name] = blend_host(mean_s, var_s, mean_t, var_t, blend_weight(s.images, self.prior))
            stats[(key, name)] = (s.images, divergence_host(mean_s, var_s, mean_t, var_t))
        for key, name, m in found:                      # every BatchNorm module has its row, visited or not
            n, div = stats.get((key, name), (0, np.zeros(m.weight.numel())))
            layers[key][name] = dict(images=int(n), divergence=[float(d) for d in div])
        self.site = dict(prior=self.prior, images=images, source=source_name, layers=layers)
        torch.cuda.synchronize()
        return site_checkpoint([n.state_dict() for n in self.nets], updates, self.site,
                               None if self.clahe is None else self.clahe.record())


# ---- command line -----------------------------------------------------------------------------------------------------------------
def parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip.adapt", description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", required=True, help="a directory of the target site's region-of-interest crops, no labels")
    ap.add_argument("--checkpoint", required=True, help="the source checkpoint: checkpoint_<epoch>.pth.tar, swad_checkpoint.pth.tar, ...")
    ap.add_argument("--out", required=True)
    ap.add_argument("--prior", type=float, default=DEFAULT_PRIOR, help="N0: how many target images the source statistics are worth")
    ap.add_argument("--batch-size", type=int, default=9)
    from .programs import add_clahe_argument
    add_clahe_argument(ap)
    return ap


def add_adapt_arguments(ap):
    """--adapt / --prior on a run program's parser (segment, locate, test_run, morphometry_run)."""
    ap.add_argument("--adapt", choices=("none",) + MODES, default="none",
                    help="BatchNorm on the target images' own statistics blended with the checkpoint's: per batch, or pooled over the run")
    ap.add_argument("--prior", type=float, default=DEFAULT_PRIOR, help="--adapt: how many target images the checkpoint's statistics are worth")


def main(argv=None):
    from .programs import load_networks, require_gpu, resolve_clahe
    from .segment import EXTENSIONS, ImageFolder
    ap = parser()
    args = ap.parse_args(argv)
    if args.prior < 0 or args.batch_size < 1:
        ap.error("--prior must not be negative and --batch-size must be positive")
    require_gpu("adapt")
    folder = ImageFolder(args.images)
    if len(folder) < 1:
        raise SystemExit("no image (%s) under %s" % (" ".join(EXTENSIONS), args.images))
    nets, _, record = load_networks(args.checkpoint, want_clahe=True)
    fit = SiteStatistics(*nets, prior=args.prior, batch_size=args.batch_size, clahe=resolve_clahe(ap, args.clahe, record))
    ckpt = fit.fit(folder, source_name=os.path.basename(args.checkpoint))
    os.makedirs(args.out, exist_ok=True)
    torch.save({k: ({n: v.cpu() for n, v in d.items()} if k in _checkpoint_keys() else d) for k, d in ckpt.items()},
               os.path.join(args.out, "adapted_checkpoint.pth.tar"))
    summary = write_shift(args.out, fit.site)
    print(json.dumps(summary, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
