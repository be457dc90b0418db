"""Test-time entropy minimisation on an unlabelled target site: TENT (Wang et al., ICLR 2021) with EATA's sample filter (Niu et al.,
ICML 2022) — PAPERS.md.  One gradient step per batch on the prediction entropy, updating ONLY the scale and shift of the BatchNorm
layers of the two segmentation networks; adapt.py re-estimates their statistics, this module moves their affines.

THE OBJECTIVE (host specification here, device: csrc/entropy.hip through ops.entropy_loss).  Per call, x = logits [B, 1, H, W],
m = the ROI mask (od_pred, as in overlap.py) of the cup call, m = 1 for the disc call.  Per pixel z = x m, e = exp(-|z|):
    h(z)  = log1p(e) + |z| e / (1 + e)        (= -s ln s - (1 - s) ln(1 - s), s = sigmoid(z); stable, symmetric in z; nats)
    h'(z) = -z e / (1 + e)^2                  (= -z s (1 - s))
per plane b (one image):
    M_b = sum m,    H_b = (sum m h(z)) / M_b,    H_b = 0 where M_b = 0
    c_b = [M_b > 0 and H_b < margin]          (margin in nats; +inf: plain TENT; EATA's default for two classes: 0.4 ln 2 = EATA_MARGIN;
                                               a NaN or +inf plane fails `<` and is not selected)
    w_b = exp(margin - H_b) when `reweight` is on and the margin is finite, else 1         (a constant: EATA detaches it)
    L       = (1 / B) sum_b c_b w_b H_b
    dL/dx_i = (c_b w_b / (B M_b)) m_i^2 h'(z_i)

DELIBERATE DEFINITIONS
1. The mean runs over all B planes, not over the selected ones: a plane's bits then depend on that plane alone, not on its neighbours
   in the batch.
2. Masked pixels contribute neither to H_b nor to the gradient.  Left in, every pixel outside the ROI (z = 0) would add a constant
   ln 2 to the sum and pull every cup plane's entropy towards ln 2 whatever the network does.

THE STEP.  `TentStep.step(image)`: per stage (disc, then cup on the ROI of the FIRST disc forward), `steps` times: the prediction
path with a tape (WT_PSE._forward_predict), ops.entropy_loss, WT_PSE._backward_predict, one Adam launch over the index list of the
BatchNorm affines (ops.adam_index; compact moments).  The returned logits are those of the first forward of each stage — the
prediction is made while adapting, as TENT does.  stats="batch": the two segmentation networks run in train mode (the batch's own
statistics: the paper's form; their running buffers advance as in any train-mode forward); stats="frozen": eval mode on the
checkpoint's statistics — a site-fitted checkpoint of wtpse_hip.adapt composes this way.  The two shape networks are in eval mode and
are never written.  steps=0 adapts nothing, statistics included: the networks predict in eval mode (validate.predict_pair) and only the
entropies are reported.  Eager only; no host synchronisation inside `step`.

lr = 1e-3 and betas = (0.9, 0.999) are TENT's published defaults.  Their effect on Dice or HD95 of a held-out fundus domain is NOT
MEASURED HERE, as for every optional term of this project; whether a step helps on a given site is the user's experiment.  Out of
scope: EATA's Fisher regulariser, CoTTA, any update of the convolution weights.

    python -m wtpse_hip.tent --images DIR --checkpoint CK --out OUT [--lr 1e-3] [--steps 1] [--epochs 1] [--margin inf] [--reweight]
                             [--stats batch] [--batch-size 9] [--size 256] [--clahe checkpoint]

    OUT/tent_checkpoint.pth.tar   loads wherever adapted_checkpoint.pth.tar does; extra entry "tent" (the arguments, the image count,
                                  the source) and "clahe" carried over.  --steps 0 reproduces the source's tensors bitwise.
    OUT/tent.csv                  TENT_COLUMNS, one row per step: mean entropy and selected count of both stages
    OUT/drift.csv                 DRIFT_COLUMNS, one row per BatchNorm module of the two segmentation networks: max and mean |change|
                                  of gamma and of beta against the source
"""
import contextlib
import json
import math
import os

import numpy as np
import torch

from . import ops
from . import tables as T
from .test_run import CHECKPOINT_KEYS, TestRun

EATA_MARGIN = 0.4 * math.log(2.0)
STATS = ("batch", "frozen")
TENT_COLUMNS = ("epoch", "step", "images", "ent_od", "sel_od", "ent_oc", "sel_oc")
DRIFT_COLUMNS = ("network", "name", "channels", "gamma_max", "gamma_mean", "beta_max", "beta_mean")
SEG_KEYS = (CHECKPOINT_KEYS[0], CHECKPOINT_KEYS[2])
EMBEDDING_BLOCKS = ("inc", "down1", "down2", "down3", "down4", "up1", "up2", "up3", "up4")      # what WT_PSE._embedding runs


# ---- the specification (float64, host) ------------------------------------------------------------------------------------------
def _planes(x, mask):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim < 2 or x.size == 0:
        raise ValueError("entropy: logits [B, ..., H, W], got shape %s" % (x.shape,))
    B = x.shape[0]
    x = x.reshape(B, -1)
    m = np.ones_like(x) if mask is None else np.asarray(mask, dtype=np.float64).reshape(B, -1)
    if m.shape != x.shape:
        raise ValueError("entropy: the mask must have the logits' number of elements")
    return x, m


def _margin(margin):
    margin = float(margin)
    if not margin > 0.0:
        raise ValueError("margin must be positive (nats; inf: no filter), got %r" % (margin,))
    return margin


def entropy_pixels_host(z):
    """h(z), float64, elementwise."""
    with np.errstate(invalid="ignore"):
        az = np.abs(np.asarray(z, dtype=np.float64))
        e = np.exp(-az)
        return np.log1p(e) + az * e / (1.0 + e)


def entropy_planes_host(x, mask=None, margin=float("inf"), reweight=False):
    """-> (H [B], selected [B] bool, w [B]) in float64: the per-plane mean entropies, the selection c_b and the coefficients w_b."""
    margin = _margin(margin)
    x, m = _planes(x, mask)
    B = x.shape[0]
    H, sel, w = np.zeros(B), np.zeros(B, dtype=bool), np.ones(B)
    h = entropy_pixels_host(x * m)
    for b in range(B):
        M = math.fsum(m[b])
        if M > 0.0:
            H[b] = math.fsum(m[b] * h[b]) / M
        sel[b] = bool(M > 0.0 and H[b] < margin)
        if reweight and math.isfinite(margin):
            with np.errstate(over="ignore", invalid="ignore"):
                w[b] = np.exp(margin - H[b])
    return H, sel, w


def tent_loss_host(x, mask=None, margin=float("inf"), reweight=False):
    """L = (1 / B) sum_b c_b w_b H_b, float64."""
    H, sel, w = entropy_planes_host(x, mask, margin, reweight)
    return float(math.fsum(w[b] * H[b] for b in range(H.size) if sel[b]) / H.size)


def tent_grad_host(x, mask=None, margin=float("inf"), reweight=False):
    """dL/dx in float64, of x's shape: (c_b w_b / (B M_b)) m_i^2 h'(z_i); exactly +0.0 on an unselected plane."""
    shape = np.asarray(x).shape
    H, sel, w = entropy_planes_host(x, mask, margin, reweight)
    x, m = _planes(x, mask)
    B = x.shape[0]
    out = np.zeros_like(x)
    for b in range(B):
        if not sel[b]:
            continue
        z = x[b] * m[b]
        e = np.exp(-np.abs(z))
        out[b] = (w[b] / (B * math.fsum(m[b]))) * (m[b] * m[b]) * (-z * e / (1.0 + e) ** 2)
    return out.reshape(shape)


def entropy_fp32(x, mask=None, margin=float("inf"), reweight=False):
    """The same formulas in float32 throughout (numpy, sums in index order by np.add.reduce on float32): the tests' yardstick of what
    a plain fp32 implementation would give -> (H [B], loss, grad of x's shape), float32."""
    f = np.float32
    margin = _margin(margin)
    shape = np.asarray(x).shape
    x64, m64 = _planes(x, mask)
    x, m = x64.astype(f), m64.astype(f)
    B = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        z = x * m
        az = np.abs(z)
        e = np.exp(-az).astype(f)
        h = (np.log1p(e).astype(f) + az * e / (f(1) + e)).astype(f)
        M = m.sum(axis=1, dtype=f)
        H = np.where(M > 0, (m * h).sum(axis=1, dtype=f) / np.where(M > 0, M, f(1)), f(0)).astype(f)
        sel = (M > 0) & (H < f(margin))
        w = np.exp(f(margin) - H).astype(f) if (reweight and math.isfinite(margin)) else np.ones(B, dtype=f)
        loss = f(np.where(sel, w * H, f(0)).astype(f).sum(dtype=f) / f(B))
        K = np.where(sel, w / (f(B) * np.where(M > 0, M, f(1))), f(0)).astype(f)
        g = (K[:, None] * (m * m) * (-z * e / ((f(1) + e) * (f(1) + e)))).astype(f)
        g[~sel] = f(0)
    return H, loss, g.reshape(shape)


# ---- which elements a step moves ------------------------------------------------------------------------------------------------------
def affine_modules(net):
    """[(name, BNP)] of the BatchNorm modules WT_PSE._embedding runs — inc and the U-Net body — in the network's module order.  The
    teacher (prior_dist) is left out: prediction never runs it."""
    from . import nn as E
    return [(name, m) for name, m in net.named_modules() if isinstance(m, E.BNP) and name.split(".")[0] in EMBEDDING_BLOCKS]


def affine_index(net):
    """The positions in `net`'s flat parameter buffer of the weight and bias of every module of affine_modules(net): a sorted host
    int64 array of distinct positions, built from param_offset (the network must have been flattened: ensure_ready)."""
    idx = []
    for _, m in affine_modules(net):
        for p in (m.weight, m.bias):
            off = net.param_offset(p)
            idx.extend(range(off, off + p.numel()))
    idx = np.asarray(sorted(idx), dtype=np.int64)
    if idx.size == 0 or len(set(idx.tolist())) != idx.size or idx[0] < 0 or idx[-1] >= net._flat.numel():
        raise RuntimeError("affine_index: the BatchNorm affines do not map to distinct positions of the flat buffer")
    return idx


def check_arguments(lr=1e-3, betas=(0.9, 0.999), steps=1, margin=float("inf"), reweight=False, stats="batch", eps=1e-8):
    """The arguments of TentStep / the command line -> a dict of their checked values; ValueError names the offender."""
    if not (isinstance(lr, (int, float)) and math.isfinite(lr) and lr > 0):
        raise ValueError("lr must be a positive finite number (got %r)" % (lr,))
    try:
        b1, b2 = (float(b) for b in betas)
    except (TypeError, ValueError):
        raise ValueError("betas must be two numbers in [0, 1) (got %r)" % (betas,))
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError("betas must be two numbers in [0, 1) (got %r)" % (betas,))
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
        raise ValueError("steps must be a non-negative integer (got %r)" % (steps,))
    if stats not in STATS:
        raise ValueError("stats must be one of %s (got %r)" % (", ".join(STATS), stats))
    if not (isinstance(eps, (int, float)) and math.isfinite(eps) and eps > 0):
        raise ValueError("eps must be a positive finite number (got %r)" % (eps,))
    return dict(lr=float(lr), betas=[b1, b2], steps=int(steps), margin=_margin(margin), reweight=bool(reweight), stats=stats, eps=float(eps))


class _AffineAdam:
    """Adam over the BatchNorm affines of one network: the device index list, compact moments, a device step count and rate."""

    def __init__(self, net, lr):
        net.ensure_ready()
        dev = net._flat.device
        self.net = net
        self.idx = torch.from_numpy(affine_index(net).astype(np.int32)).to(dev)
        n = self.idx.numel()
        self.m = ops.zero_(torch.empty(n, dtype=torch.float32, device=dev))
        self.v = ops.zero_(torch.empty(n, dtype=torch.float32, device=dev))
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        # episodic: what the network was at construction — parameters (a step moves the affines alone) and every buffer
        self.saved_flat = net._flat.clone()
        self.saved_buffers = [(b, b.detach().clone()) for b in net.buffers()]

    def step(self, g, betas, eps):
        ops.adam_index(self.net._flat, g, self.m, self.v, self.idx, self.lr_dev, betas[0], betas[1], eps, 1, self.t_dev)
        ops.counter_add(self.t_dev, 1)

    def restore(self):
        with torch.no_grad():
            self.net._flat.copy_(self.saved_flat)
            for b, saved in self.saved_buffers:
                b.copy_(saved)
        ops.zero_(self.m)
        ops.zero_(self.v)
        ops.zero_(self.t_dev)
        self.net.invalidate_packed()


class TentStep:
    """The step of the module docstring over (model, model_shape, model_oc, model_shape_oc).  episodic=True: after every `step` the two
    segmentation networks' parameters, buffers and the optimiser state are put back to what they were at construction (device copies)
    — every batch is adapted from the source.  affine_only=False issues the weight-gradient launches as well (nothing reads them: the
    comparison of tools/bench_tent.py)."""

    def __init__(self, model, model_shape, model_oc, model_shape_oc, lr=1e-3, betas=(0.9, 0.999), steps=1, margin=float("inf"),
                 reweight=False, stats="batch", episodic=False, affine_only=True, eps=1e-8):
        self.args = check_arguments(lr, betas, steps, margin, reweight, stats, eps)
        self.lr, self.betas, self.steps, self.eps = self.args["lr"], tuple(self.args["betas"]), self.args["steps"], self.args["eps"]
        self.margin, self.reweight, self.stats = self.args["margin"], self.args["reweight"], stats
        self.episodic, self.affine_only = bool(episodic), bool(affine_only)
        self.args.update(episodic=self.episodic, affine_only=self.affine_only)
        self.nets = [model, model_shape, model_oc, model_shape_oc]
        for n in self.nets:
            if n is None or not hasattr(n, "ensure_ready"):
                raise ValueError("TentStep needs the four networks (model, model_shape, model_oc, model_shape_oc)")
        for n in (model, model_oc):
            if not (hasattr(n, "_forward_predict") and n.n_classes == 1):
                raise ValueError("TentStep: the segmentation networks must be single-class WT_PSE networks")
        self.opt = [_AffineAdam(model, self.lr), _AffineAdam(model_oc, self.lr)]

    @contextlib.contextmanager
    def _modes(self):
        """Segmentation networks in train mode under stats="batch" (eval under "frozen", and with steps = 0), shape networks in eval
        mode; the previous modes restored whatever ends the block."""
        before = [n.training for n in self.nets]
        train = self.stats == "batch" and self.steps > 0
        for n, seg in zip(self.nets, (True, False, True, False)):
            n.train(train and seg)
        try:
            yield
        finally:
            for n, mode in zip(self.nets, before):
                n.train(mode)

    def _stage(self, net, shape, x, mask, opt):
        """-> (the first forward's logits, mean plane entropy, selected count) of one stage; device scalars."""
        first = None
        for k in range(max(self.steps, 1)):
            (logits, _), tape = net._forward_predict(shape, x, want_tape=self.steps > 0)
            loss, dx, planes, sel = ops.entropy_loss(logits, mask, self.margin, self.reweight, want_planes=True, want_grad=self.steps > 0)
            if self.steps > 0:
                attach = net._attach_grads
                object.__setattr__(net, "_attach_grads", False)         # the gradient is read from the flat buffer below
                try:
                    net._backward_predict(tape, dx, affine_only=self.affine_only)
                finally:
                    object.__setattr__(net, "_attach_grads", attach)
                opt.step(net._gtarget, self.betas, self.eps)
            if first is None:
                ent = torch.empty((), dtype=torch.float32, device=planes.device)
                ops.lib().call("wtpse_reduce_rows", planes.data_ptr(), planes.numel(), 1, ent.data_ptr(), 0, 1.0 / planes.numel(),
                               ops.stream_ptr())
                first = (logits, ent, sel.sum())
        return first

    def step(self, image):
        """image [B,3,S,S] on the device -> (logits_od, logits_oc * od_pred, {ent_od, ent_oc, sel_od, sel_oc}): the pair as
        validate.predict_pair shapes it, from the first forward of each stage; the dict holds device scalars (mean plane entropy in
        nats, number of selected planes)."""
        image = image.detach().to(torch.float32).contiguous()
        with torch.no_grad(), self._modes():
            pred, ent_od, sel_od = self._stage(self.nets[0], self.nets[1], image, None, self.opt[0])
            roi, od_pred = ops.roi(image, pred)
            pred_oc, ent_oc, sel_oc = self._stage(self.nets[2], self.nets[3], torch.stack((roi, roi), 0), od_pred, self.opt[1])
            pred_oc = ops.relu_mask(pred_oc, od_pred)
        if self.episodic:
            self.reset()
        return pred, pred_oc, dict(ent_od=ent_od, ent_oc=ent_oc, sel_od=sel_od, sel_oc=sel_oc)

    def reset(self):
        """The two segmentation networks and the optimiser state back to construction time."""
        for o in self.opt:
            o.restore()


# ---- a labelled test split scored while adapting ------------------------------------------------------------------------------------
class TentTestRun(TestRun):
    """test_run.TestRun whose predictions are made by a TentStep while it adapts, in the split's order: every batch is predicted by
    the first forward of its step and the networks carry the step on to the next batch (episodic=True: every batch from the source).
    summary.json (and the returned means) also hold the TentStep arguments under "tent".  The networks ARE modified by the run."""
    __test__ = False

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, overlay="device", metrics="device", **tent):
        super().__init__(model, model_shape, model_oc, model_shape_oc, out_dir, overlay=overlay, metrics=metrics)
        self.tent = TentStep(model, model_shape, model_oc, model_shape_oc, **tent)

    def predict(self, image, size):
        """validate.predict_pair's pair at the label size, from the step's first forwards."""
        pred, pred_oc, _ = self.tent.step(image)
        if size is not None and tuple(size) != tuple(pred.shape[2:]):
            pred, pred_oc = ops.resize_bilinear(pred, size), ops.resize_bilinear(pred_oc, size)
        return pred, pred_oc

    def batch(self, image, label_od, label_oc):
        """TestRun.batch takes its two logit maps from validate.predict_pair, looked up in that module at the call: for the duration
        of the batch the name answers with `predict` (this run's four networks only; anything else is refused), and is put back
        whatever ends the batch.  Everything behind the logits — masks, metrics, pictures — is TestRun's own code."""
        from . import validate as V
        plain = V.predict_pair

        def adapting(model, model_shape, model_oc, model_shape_oc, data, label_size=None):
            if [model, model_shape, model_oc, model_shape_oc] != self.nets:
                raise RuntimeError("TentTestRun.batch: predict_pair was called for other networks than the run's")
            return self.predict(data, label_size)

        V.predict_pair = adapting
        try:
            return super().batch(image, label_od, label_oc)
        finally:
            V.predict_pair = plain

    def run(self, batches):
        means = dict(super().run(batches), tent=dict(self.tent.args))
        T.write_json(os.path.join(self.out_dir, "summary.json"), means, allow_nan=True)
        return means


# ---- the checkpoint and the tables ------------------------------------------------------------------------------------------------------
def tent_checkpoint(state_dicts, tent, clahe=None):
    """state_dicts: the four networks' state_dicts in CHECKPOINT_KEYS order -> the four-key checkpoint dict with every tensor CLONED,
    plus "tent" = `tent` (the arguments, the image count, the source) and, when `clahe` (a `Clahe.record()`) is not None, "clahe" = a
    copy of it.  The inputs are not modified."""
    state_dicts = list(state_dicts)
    if len(state_dicts) != len(CHECKPOINT_KEYS):
        raise ValueError("tent_checkpoint: %d state_dicts for the keys %s" % (len(state_dicts), ", ".join(CHECKPOINT_KEYS)))
    out = {key: {k: v.detach().clone() for k, v in sd.items()} for key, sd in zip(CHECKPOINT_KEYS, state_dicts)}
    out["tent"] = dict(tent)
    if clahe is not None:
        out["clahe"] = dict(clahe)
    return out


def drift_rows(source, final):
    """source / final: {key: state_dict} holding at least SEG_KEYS -> drift.csv's rows: per BatchNorm module (a `<name>.running_mean`
    entry) of the two segmentation networks, in state_dict order, the max and mean |final - source| of gamma and of beta (float64)."""
    rows = []
    for key in SEG_KEYS:
        src, fin = source[key], final[key]
        for k in src:
            if not k.endswith(".running_mean"):
                continue
            name = k[:-len(".running_mean")]
            d = [np.abs(np.asarray(fin[name + s].detach().cpu(), dtype=np.float64) - np.asarray(src[name + s].detach().cpu(), dtype=np.float64))
                 for s in (".weight", ".bias")]
            rows.append(dict(network=key, name=name, channels=int(d[0].size), gamma_max=float(d[0].max()), gamma_mean=float(d[0].mean()),
                             beta_max=float(d[1].max()), beta_mean=float(d[1].mean())))
    return rows


def write_tables(out_dir, step_rows, drift):
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, "tent.csv"), TENT_COLUMNS, step_rows, ("epoch", "step", "images", "sel_od", "sel_oc"))
    T.write_csv(os.path.join(out_dir, "drift.csv"), DRIFT_COLUMNS, drift, ("channels",), ("network", "name"))


def read_tables(out_dir):
    return (T.read_csv(os.path.join(out_dir, "tent.csv"), ("epoch", "step", "images", "sel_od", "sel_oc")),
            T.read_csv(os.path.join(out_dir, "drift.csv"), ("channels",), ("network", "name")))


class TentRun:
    """fit(folder or batches) -> the tent checkpoint dict: `epochs` passes of TentStep.step over the images, in their order;
    `self.rows` keeps tent.csv's rows, `self.info` the "tent" entry.  The live networks ARE adapted (that is the result); the loader
    and CLAHE handling are adapt.SiteStatistics'."""

    def __init__(self, model, model_shape, model_oc, model_shape_oc, epochs=1, batch_size=9, size=256, clahe=None, **tent):
        if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 1:
            raise ValueError("epochs must be a positive integer (got %r)" % (epochs,))
        from .adapt import SiteStatistics
        self.loader = SiteStatistics(model, model_shape, model_oc, model_shape_oc, batch_size=batch_size, size=size, clahe=clahe)
        self.nets, self.epochs, self.clahe = self.loader.nets, int(epochs), clahe
        self.step = TentStep(model, model_shape, model_oc, model_shape_oc, **tent)
        self.rows, self.info = [], None

    def fit(self, source, source_name=None):
        from .packed import fetch
        source_sd = {key: {k: v.detach().clone() for k, v in n.state_dict().items()} for key, n in zip(CHECKPOINT_KEYS, self.nets)}
        scalars, counts, images = [], [], 0
        for epoch in range(self.epochs):
            images = 0
            for image in self.loader._batches(source):
                _, _, s = self.step.step(image)
                scalars.extend((s["ent_od"], s["sel_od"].to(torch.float32), s["ent_oc"], s["sel_oc"].to(torch.float32)))
                counts.append((epoch, int(image.shape[0])))
                images += int(image.shape[0])
        if images < 1:
            raise ValueError("TentRun.fit: no target image")
        host = fetch([torch.stack([t.reshape(()) for t in scalars])])[0].reshape(-1, 4)          # the one copy
        self.rows = [dict(epoch=e, step=i, images=n, ent_od=float(r[0]), sel_od=int(r[1]), ent_oc=float(r[2]), sel_oc=int(r[3]))
                     for i, ((e, n), r) in enumerate(zip(counts, host))]
        self.info = dict(self.step.args, epochs=self.epochs, images=images, source=source_name)
        torch.cuda.synchronize()
        ckpt = tent_checkpoint([n.state_dict() for n in self.nets], self.info, None if self.clahe is None else self.clahe.record())
        self.drift = drift_rows(source_sd, ckpt)
        return ckpt


# ---- command line -----------------------------------------------------------------------------------------------------------------
def parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip.tent", description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", required=True, help="a directory of the target site's region-of-interest crops, no labels")
    ap.add_argument("--checkpoint", required=True, help="the source checkpoint: checkpoint_<epoch>.pth.tar, adapted_checkpoint.pth.tar, ...")
    ap.add_argument("--out", required=True)
    ap.add_argument("--lr", type=float, default=1e-3, help="Adam's rate on the BatchNorm affines (TENT's default)")
    ap.add_argument("--steps", type=int, default=1, help="gradient steps per batch and stage; 0: adapt nothing")
    ap.add_argument("--epochs", type=int, default=1, help="passes over the folder")
    ap.add_argument("--margin", type=float, default=float("inf"),
                    help="select the images whose mean entropy is below this many nats (EATA: 0.4 ln 2 = %.4f); inf: all (TENT)" % EATA_MARGIN)
    ap.add_argument("--reweight", action="store_true", help="EATA's coefficient exp(margin - entropy) on the selected images")
    ap.add_argument("--stats", choices=STATS, default="batch", help="BatchNorm on the batch's statistics (train mode) or on the checkpoint's")
    ap.add_argument("--batch-size", type=int, default=9)
    ap.add_argument("--size", type=int, default=256, help="the side the crops are resized to")
    from .programs import add_clahe_argument
    add_clahe_argument(ap)
    return ap


def main(argv=None):
    from .programs import load_networks, require_gpu, resolve_clahe
    from .segment import EXTENSIONS, ImageFolder
    ap = parser()
    args = ap.parse_args(argv)
    if args.batch_size < 1 or args.epochs < 1 or args.size < 1:
        ap.error("--batch-size, --epochs and --size must be positive")
    try:
        check_arguments(lr=args.lr, steps=args.steps, margin=args.margin, reweight=args.reweight, stats=args.stats)
    except ValueError as e:
        ap.error(str(e))
    require_gpu("tent")
    folder = ImageFolder(args.images)
    if len(folder) < 1:
        raise SystemExit("no image (%s) under %s" % (" ".join(EXTENSIONS), args.images))
    nets, _, record = load_networks(args.checkpoint, want_clahe=True)
    run = TentRun(*nets, epochs=args.epochs, batch_size=args.batch_size, size=args.size, clahe=resolve_clahe(ap, args.clahe, record),
                  lr=args.lr, steps=args.steps, margin=args.margin, reweight=args.reweight, stats=args.stats)
    ckpt = run.fit(folder, source_name=os.path.basename(args.checkpoint))
    os.makedirs(args.out, exist_ok=True)
    torch.save({k: ({n: v.cpu() for n, v in d.items()} if k in CHECKPOINT_KEYS else d) for k, d in ckpt.items()},
               os.path.join(args.out, "tent_checkpoint.pth.tar"))
    write_tables(args.out, run.rows, run.drift)
    print(json.dumps(dict(run.info, steps_run=len(run.rows)), sort_keys=True, default=str))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
