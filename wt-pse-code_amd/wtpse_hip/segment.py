"""Segmenting unlabelled images: a trained checkpoint and any folder of region-of-interest crops — no ground truth, no naming rule,
any mix of sizes — through both stages, and per image the segmentation as a label file, the contours on the picture and the
cup-to-disc ratios.  The test run (test_run.py) scores a labelled split; this is the path for images that have no label.

    python -m wtpse_hip.segment --images DIR --checkpoint C --out O [--batch-size 9] [--no-overlay] [--samples K --seed S --sample-scale X]
                                [--morphometry [--sectors N] [--eye right|left]] [--views none|id|hflip|flips|d4|<codes>]
                                [--adapt none|batch|stream [--prior 16]] [--gradability [--min-focus-ratio X ...]]

    O/mask/<stem>.png        mode 'L', the image's own size, grey levels 0 (cup) / 128 (disc) / 255 (background): the dataset's
                             label encoding — FundusTree and FundusTestBatches read it as a label
    O/overlay/<stem>.png     the contours on the resized network input: disc-or-cup green, cup blue (--no-overlay: not written)
    O/measurements.csv       CSV_COLUMNS, one row per image
    O/summary.json           n, n_empty_disc, n_empty_cup and the means of the three ratios over the images where they are defined

With --samples K (Segmenter(samples=K); 0, the default, changes nothing and writes none of these) every image is also predicted under
K sampled shape latents (uncertainty.py, validate.predict_pair_samples) from the same two U-Net passes:

    O/uncertainty/<stem>.png the spread of the K predictions at the image's own size, RGB: R = round(255 min(1, 2 std_disc)), G the
                             same for the cup, B = 0
    O/uncertainty.csv        uncertainty.CSV_COLUMNS, one row per image: mean / std / 5th / 95th percentile of each ratio over the
                             samples whose disc is not empty (n_defined of n_samples; nan when none is), the pixels the samples'
                             votes disagree on and the mean spread per class
    O/summary.json           gains n_samples and mean_vcdr_std (the mean of vcdr_std over the images where it is defined)

The per-sample ratios are taken from the samples' masks at the network's 256 x 256 (post-processed like the deterministic ones; the
ratios are scale-free), not at the native size.  The image at folder index i draws its 2 K S^2 normals from position 2 K S^2 i of the
stream `seed` whatever the batch size (`Segmenter.sample_offsets`), so a folder segmented twice draws the same numbers.

With --morphometry (Segmenter(morphometry=True, sectors=N, eye=E); off, the default, changes nothing and writes none of these) every
pair of native-size masks also goes through ops.onh_profile (morphometry.py: ellipse fits, the rim width per angular sector, ISNT):

    O/morphometry.csv        morphometry.MORPH_COLUMNS, one row per image
    O/rim_profile.csv        index, name, rim_000 .. rim_{N-1}: the rim width per sector in pixels at the image's own size
    O/summary.json           gains sectors, mean_vcdr_ellipse, mean_rim_min_rel and, with --eye, n_isnt_violations
    O/morphometry_uncertainty.csv   with --samples K as well: morphometry.STAT_COLUMNS and the per-sector spread of the relative rim
                             width over the K sampled masks (at the network's 256 x 256, like uncertainty.csv)

measurements.csv and CSV_COLUMNS are the same with and without it.

With --views (Segmenter(views=...); views.parse names the sets; none, the default, changes nothing) every image is predicted under V
flipped / rotated views of itself and the views' predictions, turned back, are merged (validate.predict_pair_views, ops.views_merge):
the mask, the overlay and measurements.csv come from the merged logits, and uncertainty/ and uncertainty.csv are written as above —
over the V views' deterministic predictions with --samples 0, over the V K sampled ones otherwise (n_samples in the table and in
summary.json is the number of maps merged; sample v K + k is sample k of view v).  summary.json gains views, the code list.  The
image at folder index i draws from position 2 V K S^2 i of the stream; the cost is V passes of both U-Nets.

With --clahe (Segmenter(clahe=Clahe(...)); `checkpoint`, the default, applies what the checkpoint records as "clahe" and changes
nothing for a checkpoint without the entry; `off`; or CLIP[:TY,TX[:FLOOR[:MODE]]]) the resized crops pass through the CLAHE
preprocessing (csrc/clahe.hip; the project's own integer definition, not byte-equal to OpenCV; effect on held-out Dice / HD95
unmeasured) before the normalisation: a checkpoint trained under the stage needs it, one trained without must not get it.

With --adapt batch|stream (Segmenter(adapt=..., prior=N0); none, the default, changes nothing) the eval-mode BatchNorm layers run on the
images' own statistics blended with the checkpoint's (adapt.py): per network batch, or pooled over the run in folder order.  The
predictions then depend on the images that share the batch (and, for stream, on those before it); --adapt stream refuses --views,
whose every view would be pooled as one more image.  summary.json gains adapt and prior.  A checkpoint from wtpse_hip.adapt needs no switch.

With --gradability (Segmenter(gradability=Gradability(...)); off, the default, changes nothing and writes none of these) every decoded
image, at its own size and while `front` has it on the device, also goes through ops.gradability_record (every pixel in the field:
t = 0) and ops.locate_cells at the cell side gradability.crop_cell(h, w); gradability.py finishes the records:

    O/gradability.csv        gradability.columns(): focus, exposure and field measures per image, then the flags of the thresholds
                             given (--min-focus, --min-focus-ratio, --max-dark, --max-bright, --max-cv, --min-fov-fill; none by
                             default, on purpose), then focus_rank, the image's percentile rank by focus_ratio within the run
    O/summary.json           gains gradability: the thresholds and levels, n_judged, n_gradable

The masks and measurements.csv are the same with and without it.

Front (`Segmenter.front`): the decoded uint8 images go to the GPU as they are; the LANCZOS resize to 256 x 256 — FundusTree's
Image.resize((S, S), Image.LANCZOS), bit for bit — is two passes of wtpse_resample_u8 with `resample_table(..., "lanczos")`, batched
over the images of one size, a pass whose axis already has the target length skipped as Pillow skips it; wtpse_image_finish
normalises.  A network batch is `batch_size` consecutive images whatever their sizes: the networks only see 256 x 256.

Back (`Segmenter.back`): per native size, both logit maps resized bilinearly (ops.resize_bilinear), ops.postprocess_masks,
ops.label_map, ops.mask_geometry and — on the network input resized bilinearly to the native size, the test run's picture —
ops.overlay without a ground truth.  Everything a size group produces comes back in ONE device -> host copy.

Host specifications beside the device path: `label_map_host`, `mask_geometry_host`; `measure` finishes a table row from the two
geometry records in float64.  The ratios: vcdr = cup height / disc height and hcdr = cup width / disc width of the bounding boxes,
acdr = cup area / disc area; nan when the disc is empty, 0.0 when only the cup is.  The cup is NOT clipped to the disc: the table
reports what the post-processing produced.
"""
import json
import os

import numpy as np
import torch

from . import adapt as A
from . import gradability as GR
from . import morphometry as M
from . import ops
from . import tables as T
from . import uncertainty as U
from . import validate as V
from . import views as VW
from .input_pipeline import DeviceInputPipeline, _dev_i32, resample_table
from .packed import fetch

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")
INT_COLUMNS = ("height", "width", "disc_area", "cup_area", "disc_top", "disc_bottom", "disc_left", "disc_right",
               "cup_top", "cup_bottom", "cup_left", "cup_right")
FLOAT_COLUMNS = ("disc_cy", "disc_cx", "cup_cy", "cup_cx", "vcdr", "hcdr", "acdr")
CSV_COLUMNS = ("index", "name") + INT_COLUMNS + FLOAT_COLUMNS
RATIOS = ("vcdr", "hcdr", "acdr")


# ---- the host specifications ----------------------------------------------------------------------------------------------
def label_map_host(disc, cup):
    """Two masks (nonzero = object) -> uint8 grey levels: 0 where cup, else 128 where disc, else 255.  The inverse of
    test_run.label_thresholds_host: read back, oc == (cup != 0) and od == ((disc | cup) != 0)."""
    disc, cup = np.asarray(disc) != 0, np.asarray(cup) != 0
    return np.where(cup, 0, np.where(disc, 128, 255)).astype(np.uint8)


def mask_geometry_host(mask):
    """[..., h, w] masks -> int64 [..., 8] = (area, top, bottom, left, right, sum_r, sum_c, 0) over the nonzero pixels; an empty mask:
    (0, h, -1, w, -1, 0, 0, 0).  ops.mask_geometry's records."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape[-2:]
    out = np.zeros(mask.shape[:-2] + (8,), np.int64)
    for idx in np.ndindex(*mask.shape[:-2]):
        r, c = np.nonzero(mask[idx])
        if len(r):
            out[idx] = (len(r), r.min(), r.max(), c.min(), c.max(), r.astype(np.int64).sum(), c.astype(np.int64).sum(), 0)
        else:
            out[idx] = (0, h, -1, w, -1, 0, 0, 0)
    return out


def _ratio(num, den):
    return float("nan") if den == 0 else float(np.float64(num) / np.float64(den))


def measure(rec_disc, rec_cup, h, w):
    """The two geometry records of one image -> its table row without index and name (INT_COLUMNS as int, FLOAT_COLUMNS as float)."""
    d, c = [int(v) for v in rec_disc], [int(v) for v in rec_cup]
    row = {"height": int(h), "width": int(w), "disc_area": d[0], "cup_area": c[0]}
    ext = {}
    for name, r in (("disc", d), ("cup", c)):
        row.update({name + "_top": r[1], name + "_bottom": r[2], name + "_left": r[3], name + "_right": r[4]})
        ext[name] = (r[2] - r[1] + 1, r[4] - r[3] + 1) if r[0] else (0, 0)
        row[name + "_cy"], row[name + "_cx"] = _ratio(r[5], r[0]), _ratio(r[6], r[0])
    row["vcdr"] = _ratio(ext["cup"][0], ext["disc"][0])
    row["hcdr"] = _ratio(ext["cup"][1], ext["disc"][1])
    row["acdr"] = _ratio(c[0], d[0])
    return row


def summarise(rows):
    """-> {n, n_empty_disc, n_empty_cup, mean_vcdr, mean_hcdr, mean_acdr}: a mean over the rows where the ratio is defined, None
    when there is none."""
    out = {"n": len(rows), "n_empty_disc": sum(1 for r in rows if r["disc_area"] == 0),
           "n_empty_cup": sum(1 for r in rows if r["cup_area"] == 0)}
    for k in RATIOS:
        vals = [r[k] for r in rows if r[k] == r[k]]
        out["mean_" + k] = float(np.mean(np.array(vals, np.float64))) if vals else None
    return out


# ---- the table ------------------------------------------------------------------------------------------------------------
def write_measurements(out_dir, rows, summary):
    """rows: [{CSV_COLUMNS}] -> out_dir/measurements.csv (floats as repr: they read back to the same float64; nan as "nan") and
    out_dir/summary.json (an undefined mean as null)."""
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, "measurements.csv"), CSV_COLUMNS, rows, ("index",) + INT_COLUMNS)
    T.write_json(os.path.join(out_dir, "summary.json"), summary, allow_nan=False)


def read_measurements(out_dir):
    """-> (rows, summary) as write_measurements wrote them."""
    return T.read_csv(os.path.join(out_dir, "measurements.csv"), ("index",) + INT_COLUMNS), T.read_json(os.path.join(out_dir, "summary.json"))


# ---- the feed -------------------------------------------------------------------------------------------------------------
class ImageFolder:
    """A directory — its files with one of EXTENSIONS, case-insensitive, sorted by file name — or an explicit list of paths, in its
    order.  No naming rule, no mask.  `names[i]` is the output name of image i: its stem plus ".png"; two inputs with one stem raise
    ValueError here, before anything runs."""

    def __init__(self, path_or_list):
        if isinstance(path_or_list, (str, os.PathLike)):
            root = os.fspath(path_or_list)
            files = sorted(f for f in os.listdir(root)
                           if os.path.splitext(f)[1].lower() in EXTENSIONS and os.path.isfile(os.path.join(root, f)))
            self.paths = [os.path.join(root, f) for f in files]
        else:
            self.paths = [os.fspath(p) for p in path_or_list]
        self.names = [os.path.splitext(os.path.basename(p))[0] + ".png" for p in self.paths]
        seen = {}
        for p, n in zip(self.paths, self.names):
            if n in seen:
                raise ValueError("%s and %s would both be written as %s" % (seen[n], p, n))
            seen[n] = p

    def __len__(self):
        return len(self.paths)

    def load(self, i):
        """-> [h,w,3] uint8, decoded as FundusTree decodes: Image.open(p).convert("RGB")."""
        from PIL import Image
        return np.array(Image.open(self.paths[i]).convert("RGB"))


def _groups(sizes):
    """{(h, w): [positions]} in order of first appearance."""
    g = {}
    for i, s in enumerate(sizes):
        g.setdefault((int(s[0]), int(s[1])), []).append(i)
    return g


# ---- the driver -----------------------------------------------------------------------------------------------------------
class BackResult:
    """What Segmenter.back_result returns: per-image lists in the images' order — labels, overlays (entries None without overlay),
    rows (`measure`), spreads (None unless a spread was passed) and morph (`morphometry.finish` rows; None with morphometry off)."""
    __slots__ = ("labels", "overlays", "rows", "spreads", "morph")

    def __init__(self, labels, overlays, rows, spreads=None, morph=None):
        self.labels, self.overlays, self.rows, self.spreads, self.morph = labels, overlays, rows, spreads, morph


class Segmenter:
    """run(folder) segments every image of an ImageFolder (or of what ImageFolder takes) in batches of `batch_size` consecutive
    images and writes the files of the module docstring; -> the summary, `self.rows` keeps the table.  Eval mode for the duration, the
    previous modes restored.  front / back are the two halves around validate.predict_pair.
    clahe: an `input_pipeline.Clahe` puts the CLAHE preprocessing into `front`, after the resize and before the normalisation (None,
    the default: nothing changes) — for a checkpoint trained under the same Clahe (its "clahe" entry).  Overlays show the network
    input, hence the equalised picture."""

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, batch_size=9, overlay=True, size=256, samples=0, seed=0,
                 scale=1.0, morphometry=False, sectors=24, eye=None, views=None, adapt=None, prior=A.DEFAULT_PRIOR, clahe=None,
                 gradability=None):
        if gradability is not None and not isinstance(gradability, GR.Gradability):
            raise ValueError("gradability must be a gradability.Gradability or None, got %r" % (gradability,))
        # (None, the default: nothing changes.  write_gradability: finish() writes gradability.csv — locate.py, which joins these rows
        # to the photographs', turns it off)
        self.gradability, self.write_gradability, self.grad_rows, self._grad_pending = gradability, True, [], []
        if clahe is not None:
            from .input_pipeline import Clahe
            if not isinstance(clahe, Clahe):
                raise ValueError("clahe must be an input_pipeline.Clahe or None, got %r" % (clahe,))
            clahe.check_size(int(size), int(size))
        self.clahe = clahe
        self.morphometry, self.sectors, self.eye = bool(morphometry), M.check_sectors(sectors), M.check_eye(eye)
        self.morph_rows, self.morph_sample_rows = [], []
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        if not 0 <= int(samples) <= 64 or not float(scale) >= 0.0:
            raise ValueError("samples must lie in 0..64 and scale must not be negative (got %r, %r)" % (samples, scale))
        if 2 * int(batch_size) * int(samples) >= 8192:
            raise ValueError("batch_size * samples must stay below 4096 (one set of post-processing launches per batch)")
        self.views = VW.parse(views)
        self.adapt, self.prior = A.check_adapt(adapt, self.views), float(prior)
        if self.adapt is not None and not self.prior >= 0.0:
            raise ValueError("prior must not be negative (got %r)" % (prior,))
        if self.views is not None:
            n_views = len(self.views)
            if n_views * int(samples) > VW.MAX_MAPS:
                raise ValueError("views * samples must not exceed %d (got %d x %d)" % (VW.MAX_MAPS, n_views, int(samples)))
            if 2 * int(batch_size) * n_views * max(int(samples), 1) >= 8192:
                raise ValueError("batch_size * views * max(samples, 1) must stay below 4096 (one set of post-processing launches per batch)")
        self.samples, self.seed, self.scale = int(samples), int(seed), float(scale)
        # the maps behind uncertainty.csv: the K samples, or with views the V views' predictions (samples = 0) / the V K samples
        self.n_maps = self.samples if self.views is None else len(self.views) * max(self.samples, 1)
        self.sample_rows, self.sample_offsets = [], []
        self.nets = [model, model_shape, model_oc, model_shape_oc]
        self.out_dir, self.batch_size, self.overlay, self.size = out_dir, int(batch_size), bool(overlay), int(size)
        self._pipe, self._tables, self.rows = None, {}, []

    def _lanczos_pass(self, src, vertical):
        """One pass of Pillow's LANCZOS resize to `size` along the width (vertical = False) or the height of src [N,H,W,3] uint8:
        DeviceInputPipeline's resampling launch with the "lanczos" table of the axis' length."""
        in_size = src.shape[1] if vertical else src.shape[2]
        if self._pipe is None or self._pipe.device != src.device:
            self._pipe, self._tables = DeviceInputPipeline(self.size, src.device), {}
        t = self._tables.get(in_size)
        if t is None:
            b, k, ks = resample_table(in_size, self.size, "lanczos")
            t = self._tables[in_size] = (_dev_i32(b, src.device), _dev_i32(k, src.device), ks)
        return self._pipe._resample(src, t[0], t[1], None, t[2], self.size, vertical)

    def front(self, images, device="cuda"):
        """images: decoded [h,w,3] uint8 arrays of any sizes -> [B,3,S,S] fp32 on the device, in their order: FundusTree's LANCZOS
        resize, then (with clahe) ops.clahe, then FundusTestBatches.host_sample's normalisation, bit for bit.  An image may also be a [h,w,3] uint8 tensor that is
        already on the device (locate.py's crops): it takes the same path without visiting the host."""
        S, dev = self.size, torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the segmentation front runs on the GPU only (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        images = [im.contiguous() if isinstance(im, torch.Tensor) else np.ascontiguousarray(im) for im in images]
        for im in images:
            on_device = isinstance(im, torch.Tensor)
            if im.dtype != (torch.uint8 if on_device else np.uint8) or im.ndim != 3 or im.shape[2] != 3 or (on_device and im.device != dev):
                raise ValueError("images must be decoded [h,w,3] uint8 arrays, or such tensors on %s (got %s %s)" % (dev, tuple(im.shape), im.dtype))
        groups = _groups([im.shape[:2] for im in images])
        small = torch.empty((len(images), S, S, 3), dtype=torch.uint8, device=dev)
        for (H, W), idx in groups.items():
            if any(isinstance(images[i], torch.Tensor) for i in idx):
                t = torch.stack([images[i] if isinstance(images[i], torch.Tensor) else torch.from_numpy(images[i]).to(dev) for i in idx])
            else:
                t = torch.from_numpy(np.stack([images[i] for i in idx])).to(dev)
            if self.gradability is not None:                           # the decoded pictures at their own size, every pixel in the field
                c = GR.crop_cell(H, W)
                self._grad_pending.append((idx, c, ops.gradability_record(t, 0, self.gradability.sat), ops.locate_cells(t, c, 0)))
            if W != S:
                t = self._lanczos_pass(t, False)
            if H != S:
                t = self._lanczos_pass(t, True)
            if len(groups) == 1:
                small = t
            else:
                small[torch.tensor(idx, device=dev)] = t
        small = small.contiguous()
        if self.clahe is not None:
            small = ops.clahe(small, self.clahe)
        return ops.image_finish(small)

    def take_gradability(self, names):
        """What the `front` calls since the last take left on the device (one copy) -> the images' gradability.csv rows without flags
        and rank, in the images' order; they join `self.grad_rows` with their index and name."""
        pending, self._grad_pending = self._grad_pending, []
        host = iter(fetch([t for _, _, rec, cells in pending for t in (rec, cells)]))
        rows = [None] * len(names)
        for idx, c, _, _ in pending:
            rec, cells = next(host), next(host)
            for j, i in enumerate(idx):
                rows[i] = self.gradability.measures(rec[j], cells[j], c)
        for name, row in zip(names, rows):
            self.grad_rows.append(dict(row, index=len(self.grad_rows) + 1, name=name))
        return rows

    def back(self, image, logits_od, logits_oc, sizes, spread=None):
        """image [B,3,S,S] (the network input) and the two logit maps [B,1,S,S] on the device, sizes = [(h, w)] per image ->
        (label maps [h,w] uint8, overlays [h,w,3] uint8 or None, rows = `measure` dicts), lists in the images' order.
        spread = (std_disc, std_cup) [B,1,S,S] fp32: resized to the native sizes like the logits, they ride in each size group's copy
        and come back as a fourth list of [2,h,w] fp32 arrays.  The first fields of `back_result`, whatever the switches."""
        r = self.back_result(image, logits_od, logits_oc, sizes, spread)
        return (r.labels, r.overlays, r.rows) if spread is None else (r.labels, r.overlays, r.rows, r.spreads)

    def back_result(self, image, logits_od, logits_oc, sizes, spread=None):
        """`back` as one BackResult: labels, overlays, rows, spreads (None without `spread`) and morph — with morphometry on,
        ops.onh_profile runs on each size group's masks, its two records ride in the group's one copy, and morph is the list of the
        images' `morphometry.finish` rows; None when it is off."""
        B, S = image.shape[0], self.size
        if len(sizes) != B or tuple(logits_od.shape) != (B, 1, S, S) or tuple(logits_oc.shape) != (B, 1, S, S):
            raise ValueError("back: %d sizes, logits %s / %s for an image batch %s"
                             % (len(sizes), tuple(logits_od.shape), tuple(logits_oc.shape), tuple(image.shape)))
        labels, overlays, rows, spreads, morph = [None] * B, [None] * B, [None] * B, [None] * B, [None] * B
        groups = _groups(sizes)
        for (h, w), idx in groups.items():
            n = len(idx)
            if len(groups) == 1:
                img, lod, loc = image.contiguous(), logits_od.contiguous(), logits_oc.contiguous()
            else:
                sel = torch.tensor(idx, device=image.device)
                img, lod, loc = image[sel], logits_od[sel], logits_oc[sel]
            if spread is not None:
                sp = torch.cat((spread[0], spread[1]), 0) if len(groups) == 1 else torch.cat((spread[0][sel], spread[1][sel]), 0)
                if (h, w) != (S, S):
                    sp = ops.resize_bilinear(sp.contiguous(), (h, w))
            if (h, w) != (S, S):
                lod, loc = ops.resize_bilinear(lod, (h, w)), ops.resize_bilinear(loc, (h, w))
            masks = ops.postprocess_masks(torch.cat((lod, loc), 0))
            disc, cup = masks[:n], masks[n:]
            geom = ops.mask_geometry(masks)
            out = [geom, ops.label_map(disc, cup).reshape(n, h, w)]
            if self.overlay:
                if (h, w) != (S, S):
                    img = ops.resize_bilinear(img, (h, w))              # the test run's picture (test_visulization.py:231-232)
                out.append(ops.overlay(img, disc, cup, None, None)[1])
            if spread is not None:
                out.append(sp.reshape(2, n, h, w))
            if self.morphometry:
                out.extend(ops.onh_profile(disc, cup, geom[:n], self.sectors))
            host = iter(fetch(out))                                    # the one copy; taken in the order it was filled
            rec, lm = next(host), next(host)
            ov = next(host) if self.overlay else None
            sm = next(host) if spread is not None else None
            if self.morphometry:
                prof, mom = next(host), next(host)
                mrows = M.finish_batch(rec, mom, prof.view(np.uint32), h, w, self.eye)
            for j, i in enumerate(idx):
                labels[i], rows[i] = lm[j], measure(rec[j], rec[n + j], h, w)
                overlays[i] = ov[j] if self.overlay else None
                spreads[i] = sm[:, j] if spread is not None else None
                morph[i] = mrows[j] if self.morphometry else None
        return BackResult(labels, overlays, rows, spreads if spread is not None else None, morph if self.morphometry else None)

    def back_samples(self, disc, cup):
        """The uncertainty.ShapeSamples of the two stages (with their [B,K,S,S] logits) -> per image the uncertainty.csv row without
        index and name.  Both classes' B K sampled logit maps go through ops.postprocess_masks and ops.mask_geometry at the network
        size in one set of launches; the records, the vote maps and the spread maps come back in one copy; `measure` per sample and
        the statistics (uncertainty.ratio_statistics / map_statistics) are the host's."""
        return self.back_samples_result(disc, cup)[0]

    def back_samples_result(self, disc, cup):
        """-> (the rows of `back_samples`, morph): with morphometry on, the same 2 B K masks go through ops.onh_profile, its records
        ride in that copy, and morph is per image `morphometry.sample_statistics` of its K samples; None when it is off."""
        B, K, S = disc.logits.shape[0], disc.logits.shape[1], self.size
        masks = ops.postprocess_masks(torch.cat((disc.logits.reshape(B * K, 1, S, S), cup.logits.reshape(B * K, 1, S, S)), 0))
        geom = ops.mask_geometry(masks)
        out = [geom.reshape(2, B, K, 8), disc.votes.reshape(B, S, S), cup.votes.reshape(B, S, S),
               torch.cat((disc.std, cup.std), 0).reshape(2, B, S, S)]
        if self.morphometry:
            out.extend(ops.onh_profile(masks[:B * K], masks[B * K:], geom[:B * K], self.sectors))
        rec, votes_disc, votes_cup, std, *morph = fetch(out)           # the one copy
        votes = (votes_disc, votes_cup)
        rows = []
        for b in range(B):
            row = U.ratio_statistics([measure(rec[0, b, k], rec[1, b, k], S, S) for k in range(K)])
            for c, name in enumerate(("disc", "cup")):
                row[name + "_disagree_px"], row[name + "_std_mean"] = U.map_statistics(votes[c][b], std[c, b], K)
            rows.append(row)
        if not self.morphometry:
            return rows, None
        N = self.sectors
        prof, mom = morph[0].view(np.uint32).reshape(B, K, N, 4), morph[1].reshape(B, K, 2, 4)
        return rows, [M.sample_statistics([M.finish(rec[0, b, k], rec[1, b, k], mom[b, k], prof[b, k], S, S, self.eye) for k in range(K)])
                      for b in range(B)]

    def write_samples(self, names, spreads, rows, morph=None):
        """One batch of sampled results -> O/uncertainty under `names`; the rows join `self.sample_rows` with their index and name (the
        morphometry statistics, when given, `self.morph_sample_rows`)."""
        from PIL import Image
        os.makedirs(os.path.join(self.out_dir, "uncertainty"), exist_ok=True)
        for name, sp, row in zip(names, spreads, rows):
            Image.fromarray(U.std_picture(sp[0], sp[1])).save(os.path.join(self.out_dir, "uncertainty", name))
            self.sample_rows.append(dict(row, index=len(self.sample_rows) + 1, name=name))
        for name, row in zip(names, morph or ()):
            self.morph_sample_rows.append(dict(row, index=len(self.morph_sample_rows) + 1, name=name))

    def write(self, names, labels, overlays, rows, morph=None):
        """One batch of `back` results -> O/mask and O/overlay under `names`; the rows join `self.rows` with their index and name (the
        morphometry rows, when given, `self.morph_rows`)."""
        from PIL import Image
        for sub in ("mask",) + (("overlay",) if self.overlay else ()):
            os.makedirs(os.path.join(self.out_dir, sub), exist_ok=True)
        for name, lm, ov, row in zip(names, labels, overlays, rows):
            Image.fromarray(lm, "L").save(os.path.join(self.out_dir, "mask", name))
            if ov is not None:
                Image.fromarray(ov).save(os.path.join(self.out_dir, "overlay", name))
            self.rows.append(dict(row, index=len(self.rows) + 1, name=name))
        for name, row in zip(names, morph or ()):
            self.morph_rows.append(dict(row, index=len(self.morph_rows) + 1, name=name))

    def finish(self):
        """-> the summary of `self.rows`, written with them (measurements.csv, summary.json)."""
        summary = summarise(self.rows)
        if self.n_maps:
            vals = [r["vcdr_std"] for r in self.sample_rows if r["vcdr_std"] == r["vcdr_std"]]
            summary.update(n_samples=self.n_maps, mean_vcdr_std=float(np.mean(np.array(vals, np.float64))) if vals else None)
        if self.views is not None:
            summary.update(views=list(self.views))
        if self.adapt is not None:
            summary.update(adapt=self.adapt, prior=self.prior)
        if self.morphometry:
            summary.update(M.summarise(self.morph_rows, self.eye), sectors=self.sectors)
        if self.gradability is not None and self.write_gradability:
            self.grad_rows = GR.finish_rows(self.grad_rows, self.gradability)
            summary.update(gradability=GR.summarise(self.grad_rows, self.gradability))
        write_measurements(self.out_dir, self.rows, summary)
        if self.gradability is not None and self.write_gradability:
            GR.write_csv(self.out_dir, self.grad_rows)
        if self.n_maps:
            U.write_csv(self.out_dir, self.sample_rows)
        if self.morphometry:
            M.write_csv(self.out_dir, self.morph_rows)
            if self.n_maps:
                M.write_uncertainty_csv(self.out_dir, self.morph_sample_rows)
        return summary

    def run(self, folder):
        if not isinstance(folder, ImageFolder):
            folder = ImageFolder(folder)
        device = next(self.nets[0].parameters()).device
        self.rows, self.sample_rows, self.sample_offsets = [], [], []
        self.morph_rows, self.morph_sample_rows = [], []
        self.grad_rows, self._grad_pending = [], []
        per_image = V.noise_share(self.samples, self.size, len(self.views) if self.views is not None else 1)
        with V.eval_mode(self.nets), A.blended(self.nets, A.make_state(self.adapt, self.prior)):
            for first in range(0, len(folder), self.batch_size):
                idx = range(first, min(first + self.batch_size, len(folder)))
                images = [folder.load(i) for i in idx]
                image = self.front(images, device)
                names, sizes = [folder.names[i] for i in idx], [im.shape[:2] for im in images]
                if self.gradability is not None:
                    self.take_gradability(names)
                if not self.n_maps:
                    pred, pred_oc = V.predict_pair(*self.nets, image)
                    r = self.back_result(image, pred, pred_oc, sizes)
                    self.write(names, r.labels, r.overlays, r.rows, r.morph)
                    continue
                if self.views is not None:
                    pred, pred_oc, disc, cup = V.predict_pair_views(*self.nets, image, self.views, self.samples, self.seed, first * per_image,
                                                                    self.scale)
                else:
                    pred, pred_oc, disc, cup = V.predict_pair_samples(*self.nets, image, self.samples, self.seed, first * per_image,
                                                                      self.scale, want_logits=True)
                self.sample_offsets += [i * per_image for i in idx]
                r = self.back_result(image, pred, pred_oc, sizes, (disc.std, cup.std))
                self.write(names, r.labels, r.overlays, r.rows, r.morph)
                self.write_samples(names, r.spreads, *self.back_samples_result(disc, cup))
        return self.finish()


# ---- command line -----------------------------------------------------------------------------------------------------------
def add_arguments(ap, images_help=None):
    """The switches of `python -m wtpse_hip.segment` on an argparse parser (wtpse_hip.locate takes every one of them too)."""
    ap.add_argument("--images", required=True, help=images_help or "a directory of region-of-interest crops (%s)" % " ".join(EXTENSIONS))
    ap.add_argument("--checkpoint", required=True, help="checkpoint_<epoch>.pth.tar as validate.Validator saves it")
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch-size", type=int, default=9)
    ap.add_argument("--no-overlay", action="store_true", help="write the masks and the table only")
    ap.add_argument("--samples", type=int, default=0, help="K sampled shape latents per image: uncertainty/ and uncertainty.csv (0: none)")
    ap.add_argument("--seed", type=int, default=0, help="the noise stream of --samples")
    ap.add_argument("--sample-scale", type=float, default=1.0, help="multiplies the predicted standard deviation of the latent")
    ap.add_argument("--morphometry", action="store_true", help="ellipse fits, rim profile and ISNT: morphometry.csv, rim_profile.csv")
    ap.add_argument("--sectors", type=int, default=24, help="angular sectors of the rim profile: a multiple of 8 in 8..360")
    ap.add_argument("--eye", choices=("right", "left"), default=None, help="which eye the crops show: fills nasal / temporal / isnt")
    ap.add_argument("--views", default="none", help="test-time views to merge: none, id, hflip, flips, d4 or a comma list of codes 0..7 "
                                                    "(0 first): uncertainty/ and uncertainty.csv over the views")
    A.add_adapt_arguments(ap)
    from .programs import add_clahe_argument
    add_clahe_argument(ap)
    GR.add_arguments(ap)


def segmenter_arguments(ap, args):
    """The parsed switches of `add_arguments` -> Segmenter's keywords (without the networks and out_dir)."""
    M.check_sectors(args.sectors)
    try:
        views = VW.parse(args.views)
        adapt = A.check_adapt(args.adapt, views)
        if args.prior < 0:
            raise ValueError("--prior must not be negative")
    except ValueError as e:
        ap.error(str(e))
    kw = dict(batch_size=args.batch_size, overlay=not args.no_overlay, samples=args.samples, seed=args.seed, scale=args.sample_scale,
              morphometry=args.morphometry, sectors=args.sectors, eye=args.eye, views=views)
    if adapt is not None:                   # (off: the keywords are what they were)
        kw.update(adapt=adapt, prior=args.prior)
    try:
        grad = GR.from_arguments(args)
    except ValueError as e:
        ap.error(str(e))
    if grad is not None:                    # (off: the keywords are what they were)
        kw["gradability"] = grad
    return kw


def main(argv=None):
    import argparse
    from .programs import load_networks, require_gpu, resolve_clahe
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip.segment", description=__doc__.split("\n\n")[0])
    add_arguments(ap)
    args = ap.parse_args(argv)
    kw = segmenter_arguments(ap, args)
    require_gpu("segment")
    folder = ImageFolder(args.images)
    if len(folder) < 1:
        raise SystemExit("no image (%s) under %s" % (" ".join(EXTENSIONS), args.images))
    nets, _, record = load_networks(args.checkpoint, want_clahe=True)
    clahe = resolve_clahe(ap, args.clahe, record)
    if clahe is not None:                   # (off: the keywords are what they were)
        kw["clahe"] = clahe
    summary = Segmenter(*nets, out_dir=args.out, **kw).run(folder)
    torch.cuda.synchronize()
    print(json.dumps(summary, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
