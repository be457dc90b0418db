"""Validation front half: counterpart of Trainer.validate (reference Trainer.py:137-256) — SURVEY.md §8f row 2.

Device part (HIP kernels): OD predict -> od_pred = sigmoid > 0.75 -> ROI -> OC predict on the stacked (roi, roi) input
-> predictions_oc * od_pred -> bilinear resize of both logit maps to the label size (Trainer.py:170-209).
Host part (as in the reference, which does it in numpy/scipy/skimage on the CPU): threshold 0.75 on the sigmoid,
largest connected component + hole filling (utils.py:267-329), Dice = (2|A&B| + 1)/(|A| + |B| + 1) (metrics.py:68-97),
ASD / HD95 (Trainer.py:226-239), the per-epoch means, the validation objective and the best-Dice checkpoint (Trainer.py:242-288).

ASD / HD95 come from the un-vendored `medpy==0.5.2` in the reference (requirements.txt:2; `medpy.metric.binary.asd / hd95`), which is
not installed here: `asd` / `hd95` below restate its PUBLISHED algorithm — surface = object XOR its erosion by the
connectivity-1 structuring element, distances = Euclidean distance transform of the complement of the other surface sampled on
this surface; asd = their mean (result -> reference, ONE direction, as medpy's `asd`; its `assd` is the symmetric one), hd95 = the
95th percentile of both directions' distances pooled.  **Parity unpinned** (no medpy run to compare with); pinned instead to an
independent brute-force surface-distance oracle on small masks (oracle/metrics_cpu.py, tests/test_validate_cpu.py).

`metrics="device"` (validate_epoch / validate / Validator) runs that host back half on the GPU instead (csrc/postprocess.hip):
ops.postprocess_masks is `postprocess` bit for bit, ops.seg_metrics leaves per image the Dice counts, the two order statistics of
the squared surface distances HD95 interpolates between and the ASD sum, and `device_metrics` finishes them in float64 as `dice` /
`hd95` / `asd` do: Dice and HD95 are bitwise the host path's, ASD agrees within 1e-12 relative (a fixed-order fp64 sum where
numpy's mean sums pairwise).  One device -> host copy per batch; both classes in one set of launches.  The default stays "host".
"""
import contextlib

import numpy as np
import torch

from . import ops


@contextlib.contextmanager
def eval_mode(nets):
    """The networks in eval mode for the duration of the block, their previous modes restored whatever ends it (Trainer.py:138-141,
    289-311)."""
    modes = [n.training for n in nets]
    for n in nets:
        n.eval()
    try:
        yield
    finally:
        for n, mode in zip(nets, modes):
            n.train(mode)


def noise_share(n_samples, size, n_views=1):
    """An image's share of the noise stream, in elements: 2 V K S^2 — both stages, V views, K samples of S x S normals
    (predict_pair_samples / predict_pair_views' stream layouts).  The image at index i of a run draws from position i times this."""
    return 2 * int(n_views) * int(n_samples) * int(size) * int(size)


def predict_pair(model, model_shape, model_oc, model_shape_oc, data, label_size=None):
    """-> (logits_od, logits_oc*od_pred), each [B,1,h,w] resized to `label_size` when given.  Does not modify `data`."""
    with torch.no_grad():
        pred, _ = model.predict(model_shape, data)
        roi, od_pred = ops.roi(data.contiguous(), pred)
        pred_oc, _ = model_oc.predict(model_shape_oc, torch.stack((roi, roi), 0))
        # predictions_oc * od_pred: od_pred is {0,1}; reuse the ReLU-mask kernel (out = ref > 0 ? v : 0)
        pred_oc = ops.relu_mask(pred_oc, od_pred)
        if label_size is not None and tuple(label_size) != tuple(pred.shape[2:]):
            pred = ops.resize_bilinear(pred, label_size)
            pred_oc = ops.resize_bilinear(pred_oc, label_size)
    return pred, pred_oc


def predict_pair_samples(model, model_shape, model_oc, model_shape_oc, data, n_samples, seed=0, offset=0, scale=1.0, want_logits=False,
                         image_stride=None):
    """predict_pair at the network size plus n_samples sampled predictions of each stage from the same two U-Net passes
    (WT_PSE.predict_samples).  Stage 1 samples the disc; the ROI is built from the DETERMINISTIC disc logit exactly as predict_pair
    builds it (a cup U-Net pass per sample is not run); stage 2 samples the cup on that ROI, and the cup's samples are multiplied by
    od_pred as the deterministic cup logit is (outside it: logit 0, mean 0.5, std 0, no vote).
    -> (pred, pred_oc, disc, cup): the pair bitwise predict_pair's, disc / cup the uncertainty.ShapeSamples of the two stages.

    Stream layout: both stages draw from the ops.randn stream `seed`.  With N = n_samples * H * W, image b of the batch owns the
    2 N elements from offset + 2 N b on: the disc's samples take the first N (sample k at + k H W), the cup's the second N.  An
    image's numbers therefore depend on (seed, offset + 2 N b) alone, not on the batch it is in: a caller that walks a folder
    passes offset = 2 N * (index of the batch's first image).  offset must be a multiple of 4.
    image_stride (elements; None: the 2 N above): image b owns the 2 N elements from offset + image_stride * b on instead — for a
    caller that interleaves several draws per image in one stream (predict_pair_views)."""
    B, _, H, W = data.shape
    N = int(n_samples) * H * W
    stride = 2 * N if image_stride is None else int(image_stride)
    with torch.no_grad():
        disc = model.predict_samples(model_shape, data, n_samples, seed, int(offset), scale, None, want_logits, image_stride=stride)
        pred = disc.logit
        roi, od_pred = ops.roi(data.contiguous(), pred)
        cup = model_oc.predict_samples(model_shape_oc, torch.stack((roi, roi), 0), n_samples, seed, int(offset) + N, scale, None,
                                       want_logits, image_stride=stride)
        pred_oc = ops.relu_mask(cup.logit, od_pred)
        ops.shape_samples_mask_(od_pred, cup.mean, cup.std, cup.votes, cup.logits)
        cup.logit = pred_oc
    return pred, pred_oc, disc, cup


def predict_pair_views(model, model_shape, model_oc, model_shape_oc, data, views, n_samples=0, seed=0, offset=0, scale=1.0):
    """predict_pair under test-time views (views.py): `views` is what views.parse takes and not None — V codes, 0 first.  The V views
    of `data` come from one ops.dihedral_views launch (view 0 is `data` itself); each view runs through predict_pair (n_samples = 0)
    or predict_pair_samples as a call of its own, with its own ROI and its cup masked by its own od_pred — so the identity view is
    predict_pair bit for bit — and one ops.views_merge per structure turns the maps back and merges them.
    -> (pred, pred_oc, disc, cup) like predict_pair_samples: pred / pred_oc are the float32 means of the views' un-viewed deterministic
    logits (views.merge_host's mean_logit); disc / cup are uncertainty.ShapeSamples with their logits [B,n,S,S], n = V maps (the
    views' deterministic logits; sample v) when n_samples = 0 and n = V K maps (sample v K + k) when n_samples = K > 0; .logit is
    pred / pred_oc, .pre None.  The merged cup is restricted to the merged disc as predict_pair restricts it: od_pred from the merged
    disc logit (ops.roi), outside it logit 0, mean 0.5, std 0, no vote.

    Stream layout (n_samples = K > 0): with N = K S S, image b owns the 2 V N elements from offset + 2 V N b on; inside them view v
    owns the 2 N from + 2 N v on, disc first and cup second as in predict_pair_samples.  A caller that walks a folder passes
    offset = 2 V N * (index of the batch's first image): an image's draws depend on (seed, its index) alone."""
    from . import views as VW
    from .uncertainty import ShapeSamples
    codes = VW.parse(views)
    if codes is None:
        raise ValueError("predict_pair_views needs at least the identity view; without views call predict_pair / predict_pair_samples")
    V, K = len(codes), int(n_samples)
    B, _, H, W = data.shape
    if H != W or K < 0 or V * K > VW.MAX_MAPS:
        raise ValueError("predict_pair_views: square inputs and views * n_samples <= %d (got %s, %d x %d)" % (VW.MAX_MAPS, tuple(data.shape), V, K))
    N = K * H * W
    with torch.no_grad():
        planes = ops.dihedral_views(data.contiguous(), codes)
        det, det_oc, smp, smp_oc = [], [], [], []
        for v in range(V):
            x = data if v == 0 else planes[v]
            if K == 0:
                p, p_oc = predict_pair(model, model_shape, model_oc, model_shape_oc, x)
            else:
                p, p_oc, d, c = predict_pair_samples(model, model_shape, model_oc, model_shape_oc, x, K, seed, int(offset) + 2 * N * v, scale,
                                                     want_logits=True, image_stride=2 * V * N)
                smp.append(d.logits)
                smp_oc.append(c.logits)
            det.append(p)
            det_oc.append(p_oc)
        out = []
        for logits, sampled in ((det, smp), (det_oc, smp_oc)):
            mean, std, votes, maps, merged = ops.views_merge(torch.stack(logits, 0), codes, 0.75, K == 0, True)
            if K:
                mean, std, votes, maps, _ = ops.views_merge(torch.stack(sampled, 0), codes, 0.75, True, False)
            out.append(ShapeSamples(mean=mean, std=std, votes=votes, logits=maps, logit=merged, pre=None, n_samples=V * max(K, 1),
                                    seed=int(seed), offset=int(offset), scale=float(scale)))
        disc, cup = out
        pred = disc.logit
        od_pred = ops.roi(data.contiguous(), pred)[1]
        pred_oc = ops.relu_mask(cup.logit, od_pred)
        ops.shape_samples_mask_(od_pred, cup.mean, cup.std, cup.votes, cup.logits)
        cup.logit = pred_oc
    return pred, pred_oc, disc, cup


def largest_fillhole(binary):
    """utils.get_largest_fillhole (utils.py:267-276): keep the largest 8-connected component (skimage.measure.label's
    default connectivity in 2-D), then fill holes."""
    from scipy import ndimage
    binary = np.asarray(binary).copy()
    lab, n = ndimage.label(binary, structure=np.ones((3, 3), dtype=int))
    if n:
        areas = ndimage.sum(binary > 0, lab, index=np.arange(1, n + 1))
        binary[lab != int(np.argmax(areas)) + 1] = 0
    return ndimage.binary_fill_holes(binary.astype(int))


def postprocess(logits, threshold=0.75):
    """utils.postprocessing, label != None branch (utils.py:306-323): [1,h,w] logits -> uint8 mask [1,h,w]."""
    prob = torch.sigmoid(logits).detach().cpu().numpy()
    mask = (prob > threshold).astype(np.uint8)
    mask[0] = largest_fillhole(mask[0]).astype(np.uint8)
    return mask


def dice(seg, gt):
    seg = np.asarray(seg, dtype=np.bool_)
    gt = np.asarray(gt, dtype=np.bool_)
    inter = float(np.logical_and(seg, gt).sum())
    return (2 * inter + 1.0) / (1.0 + float(seg.sum()) + float(gt.sum()))


def _surface_distances(result, reference):
    """medpy.metric.binary.__surface_distances (0.5.2), voxelspacing None, connectivity 1: distances from every surface pixel of
    `result` to the nearest surface pixel of `reference`.  RuntimeError on an empty mask, as medpy raises."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    result = np.atleast_1d(np.asarray(result).astype(np.bool_))
    reference = np.atleast_1d(np.asarray(reference).astype(np.bool_))
    footprint = generate_binary_structure(result.ndim, 1)
    if not result.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not reference.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border)
    return dt[result_border]


def asd(result, reference):
    """medpy.metric.binary.asd: mean distance from the surface of `result` to the surface of `reference` (pixels)."""
    return float(_surface_distances(result, reference).mean())


def hd95(result, reference):
    """medpy.metric.binary.hd95: 95th percentile of the surface distances of both directions, pooled."""
    return float(np.percentile(np.hstack((_surface_distances(result, reference), _surface_distances(reference, result))), 95))


def surface_metrics(pred_mask, label):
    """(hd95, asd) of one image as Trainer.validate scores them (Trainer.py:218-239): 100 / 100 for an empty prediction."""
    pred_mask = np.asarray(pred_mask)
    if np.sum(pred_mask) < 1e-4:
        return 100.0, 100.0
    p, r = np.asarray(pred_mask, dtype=np.bool_), np.asarray(label, dtype=np.bool_)
    return hd95(p, r), asd(p, r)


# ---- the back half on the device ---------------------------------------------------------------------------------------
_EMPTY_LABEL = "The second supplied array does not contain any binary object."


def _check_metrics(metrics):
    if metrics not in ("host", "device"):
        raise ValueError("metrics must be 'host' or 'device', got %r" % (metrics,))


def percentile95_position(n):
    """numpy.percentile(a, 95) of n sorted float64 values restated (numpy/lib/_function_base_impl.py: q = 95 / float64(100); the
    linear method's virtual index (n - 1) * q — _QuantileMethods["linear"], not the generic _compute_virtual_index, whose other
    operation order rounds differently; then _get_indexes / _get_gamma): -> (rank_lo, rank_hi, gamma).  The device's
    percentile_ranks computes the same ranks."""
    q = np.true_divide(95, np.float64(100))
    vi = (n - 1) * q
    if vi >= n - 1:
        prev, lo, hi = -1, n - 1, n - 1
    elif vi < 0:
        prev, lo, hi = 0, 0, 0
    else:
        prev = int(np.floor(vi))
        lo, hi = prev, prev + 1
    return lo, hi, vi - np.intp(prev)


def hd95_from_order_stats(n, d2_lo, d2_hi):
    """np.percentile(distances, 95) from the two order statistics of the n pooled squared distances: numpy's _lerp on
    sqrt(d2) (what distance_transform_edt returns)."""
    _, _, t = percentile95_position(n)
    a, b = np.sqrt(np.float64(d2_lo)), np.sqrt(np.float64(d2_hi))
    diff_b_a = b - a
    r = a + diff_b_a * t
    if t >= 0.5:
        r = b - diff_b_a * (1 - t)
    return float(r)


def _finish_surface(r):
    """(hd95, asd) from one record, with surface_metrics' conventions."""
    if r[1] == 0:
        return 100.0, 100.0
    if r[2] == 0:
        raise RuntimeError(_EMPTY_LABEL)
    hd = hd95_from_order_stats(int(r[3] + r[4]), int(r[5]), int(r[6]))
    asd_sum = np.int64(r[7]).view(np.float64)
    return hd, float(asd_sum / np.float64(r[3]))


def _finish_dice(r):
    return (2 * float(r[0]) + 1.0) / (1.0 + float(r[1]) + float(r[2]))


def _device_records(pred, pred_oc, label_od, label_oc, threshold=0.75):
    """ops.seg_metrics of both classes in one set of launches -> host int64 [2B, 8]: disc images first, then cup."""
    ts = (pred, pred_oc, label_od, label_oc)
    if not torch.cuda.is_available() or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise RuntimeError("metrics='device' needs the GPU and device tensors (predictions and labels); there is no CPU fallback")
    masks = ops.postprocess_masks(torch.cat((pred, pred_oc), 0).contiguous(), threshold)
    labels = torch.cat((label_od, label_oc), 0).to(torch.float32).contiguous()
    return ops.seg_metrics(masks, labels).cpu().numpy()         # the one device -> host copy


METRIC_KEYS = ("disc_dice", "cup_dice", "disc_hd", "disc_asd", "cup_hd", "cup_asd")


def finish_records(rec, B):
    """Host records [2B, 8] (disc images first, then cup) -> per-image {disc_dice, cup_dice, disc_hd, disc_asd, cup_hd, cup_asd}
    (lists, batch order).  Raises the host path's RuntimeError for an empty label under a non-empty prediction (cup before disc,
    image by image)."""
    out = {k: [] for k in METRIC_KEYS}
    for i in range(B):
        out["disc_dice"].append(_finish_dice(rec[i]))
        out["cup_dice"].append(_finish_dice(rec[B + i]))
        hd, a = _finish_surface(rec[B + i])
        out["cup_hd"].append(hd)
        out["cup_asd"].append(a)
        hd, a = _finish_surface(rec[i])
        out["disc_hd"].append(hd)
        out["disc_asd"].append(a)
    return out


def device_metrics(pred, pred_oc, label_od, label_oc, threshold=0.75):
    """Per-image {disc_dice, cup_dice, disc_hd, disc_asd, cup_hd, cup_asd} (lists, batch order) of one validation batch computed
    on the GPU: pred / pred_oc [B,1,h,w] logits, label_od / label_oc [B,1,h,w] labels (nonzero = object), all device tensors.
    Raises the host path's RuntimeError for an empty label under a non-empty prediction (cup before disc, image by image)."""
    return finish_records(_device_records(pred, pred_oc, label_od, label_oc, threshold), pred.shape[0])


def host_metrics(pred, pred_oc, label_od, label_oc, masks=None):
    """The same per-image lists on the host, as Trainer.validate's inner loop scores an image (Trainer.py:214-239): post-processing,
    Dice of both classes, then the cup's surface metrics, then the disc's.  masks: [(post, post_oc)] per image when the caller has
    post-processed already (the test run paints them too)."""
    lod, loc = label_od.cpu().numpy(), label_oc.cpu().numpy()
    out = {k: [] for k in METRIC_KEYS}
    for i in range(pred.shape[0]):
        post, post_oc = masks[i] if masks is not None else (postprocess(pred[i])[0], postprocess(pred_oc[i])[0])
        out["disc_dice"].append(dice(post, lod[i, 0]))
        out["cup_dice"].append(dice(post_oc, loc[i, 0]))
        hd, a = surface_metrics(post_oc, loc[i, 0])
        out["cup_hd"].append(hd)
        out["cup_asd"].append(a)
        hd, a = surface_metrics(post, lod[i, 0])
        out["disc_hd"].append(hd)
        out["disc_asd"].append(a)
    return out


def batch_metrics(pred, pred_oc, label_od, label_oc, metrics="host"):
    """Per-image metric lists of one batch on the chosen side: what validate_epoch sums and test_run.TestRun tabulates."""
    if metrics == "device":
        return device_metrics(pred, pred_oc, label_od, label_oc)
    return host_metrics(pred, pred_oc, label_od, label_oc)


class MetricMeans:
    """Running per-image sums in arrival order -> the means validate_epoch returns (sum / max(n, 1), plus n)."""

    def __init__(self):
        self.acc = dict(cup_dice=0.0, disc_dice=0.0, cup_hd=0.0, disc_hd=0.0, cup_asd=0.0, disc_asd=0.0)
        self.total = 0

    def add(self, m):
        for i in range(len(m["disc_dice"])):
            for k in self.acc:
                self.acc[k] += m[k][i]
            self.total += 1

    def means(self):
        out = {k: v / max(self.total, 1) for k, v in self.acc.items()}
        out["n"] = self.total
        return out


def validate_epoch(model, model_shape, model_oc, model_shape_oc, batches, metrics="host"):
    """One pass of Trainer.validate's loop (Trainer.py:152-249) -> per-image means
    {cup_dice, disc_dice, cup_hd, disc_hd, cup_asd, disc_asd, n}.  batches: iterable of (image [B,3,H,W] device,
    label_od [B,1,h,w], label_oc [B,1,h,w]).  Eval mode for the duration, the previous modes restored (Trainer.py:138-141,289-311).
    metrics="device": post-processing and metrics on the GPU (device_metrics; the labels must be device tensors)."""
    _check_metrics(metrics)
    acc = MetricMeans()
    with eval_mode([model, model_shape, model_oc, model_shape_oc]):
        for image, label_od, label_oc in batches:
            pred, pred_oc = predict_pair(model, model_shape, model_oc, model_shape_oc, image, label_od.shape[2:])
            acc.add(batch_metrics(pred, pred_oc, label_od, label_oc, metrics))
    return acc.means()


def best_checkpoint(model, model_shape, model_oc, model_shape_oc):
    """The dict Trainer.validate saves on a new best (Trainer.py:282-288); test_visulization.py:132-193 loads it back."""
    return {"model": model.state_dict(), "model_shape": model_shape.state_dict(), "model_oc": model_oc.state_dict(),
            "model_oc_shape": model_shape_oc.state_dict()}


class Validator:
    """The per-epoch bookkeeping of Trainer.validate (Trainer.py:258-311): the validation objective ('OD' -> disc Dice, 'OC' -> cup
    Dice, anything else their mean), best_mean_dice / best_epoch, and on a new best the four-state_dict checkpoint (returned; saved
    with torch.save when `out_dir` is given, as checkpoint_<best_epoch>.pth.tar, with the score line appended to score.txt).
    clahe: the `Clahe.record()` of the preprocessing the networks are trained under (TrainRun sets it from its feed); when it is not
    None the checkpoint carries it as a fifth entry "clahe", which the reference's filtered load ignores."""

    clahe = None

    def __init__(self, objective="OD_OC", out_dir=None, metrics="host"):
        _check_metrics(metrics)
        self.objective, self.out_dir, self.metrics = objective, out_dir, metrics
        self.best_mean_dice, self.best_epoch = 0.0, -1

    def __call__(self, epoch, model, model_shape, model_oc, model_shape_oc, batches):
        """-> (is_best, cup_dice, cup_hd, cup_asd, disc_dice, disc_hd, disc_asd) on a new best, (0, 0, 0, 0, 0, 0, 0) otherwise —
        Trainer.validate's return values — plus `self.last` = the epoch's means and `self.checkpoint` = the dict just built."""
        if self.metrics == "host":
            m = validate_epoch(model, model_shape, model_oc, model_shape_oc, batches)
        else:
            m = validate_epoch(model, model_shape, model_oc, model_shape_oc, batches, self.metrics)
        self.last = m
        mean_dice = m["disc_dice"] if self.objective == "OD" else m["cup_dice"] if self.objective == "OC" else \
            (m["cup_dice"] + m["disc_dice"]) / 2
        if not mean_dice > self.best_mean_dice:
            return 0, 0, 0, 0, 0, 0, 0
        self.best_epoch, self.best_mean_dice = epoch + 1, mean_dice
        self.checkpoint = best_checkpoint(model, model_shape, model_oc, model_shape_oc)
        if self.clahe is not None:
            self.checkpoint["clahe"] = dict(self.clahe)
        if self.out_dir is not None:
            import os
            with open(os.path.join(self.out_dir, "score.txt"), "a") as f:
                f.write("cd:{} dd:{} c_hd:{} d_hd:{} c_asd:{} d_asd:{}\n".format(m["cup_dice"], m["disc_dice"], m["cup_hd"], m["disc_hd"],
                                                                               m["cup_asd"], m["disc_asd"]))
            torch.save(self.checkpoint, os.path.join(self.out_dir, "checkpoint_%d.pth.tar" % self.best_epoch))
        return 1, m["cup_dice"], m["cup_hd"], m["cup_asd"], m["disc_dice"], m["disc_hd"], m["disc_asd"]


def validate(model, model_shape, model_oc, model_shape_oc, batches, metrics="host"):
    """batches: iterable of (image [B,3,H,W] device, label_od [B,1,h,w], label_oc [B,1,h,w]) -> (mean cup Dice, mean disc Dice).
    Puts the four networks in eval mode for the duration (Trainer.py:138-141) and restores the previous mode.
    metrics="device": post-processing and Dice on the GPU (the labels must be device tensors)."""
    _check_metrics(metrics)
    cup, disc, total = 0.0, 0.0, 0
    with eval_mode([model, model_shape, model_oc, model_shape_oc]):
        for image, label_od, label_oc in batches:
            pred, pred_oc = predict_pair(model, model_shape, model_oc, model_shape_oc, image, label_od.shape[2:])
            if metrics == "device":
                B = pred.shape[0]
                rec = _device_records(pred, pred_oc, label_od, label_oc)
                for i in range(B):
                    disc += _finish_dice(rec[i])
                    cup += _finish_dice(rec[B + i])
                    total += 1
                continue
            lod, loc = label_od.cpu().numpy(), label_oc.cpu().numpy()
            for i in range(pred.shape[0]):
                disc += dice(postprocess(pred[i])[0], lod[i, 0])
                cup += dice(postprocess(pred_oc[i])[0], loc[i, 0])
                total += 1
    return cup / max(total, 1), disc / max(total, 1)
