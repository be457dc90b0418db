"""Test run: counterpart of the reference's second program, test_visulization.py — a trained checkpoint, the target domain's `test`
split through both stages, and per image the input picture plus an overlay of the predicted cup / disc contours and the ground
truth's (red) at the label's original resolution (test_visulization.py:100-269, utils.save_per_img utils.py:371-454).  On top of the
pictures this run writes what the reference never did: a per-image metric table and its means (the numbers of Trainer.validate).

    python -m wtpse_hip.test_run --data-dir D --datasetTest 3 --checkpoint C --out O [--batch-size 9]

    O/original_image/<n>.png      the image, untransformed, at the label size           n = 1, 2, ... over the whole run
    O/overlay/<n>.png             the same with the contours painted
    O/per_image.csv               index, name, disc_dice, cup_dice, disc_hd, disc_asd, cup_hd, cup_asd
    O/summary.json                their means and n — equal to validate.validate_epoch on the same batches
    O/morphometry_errors.csv      TestRun(morphometry=True) only — the command line of that switch is wtpse_hip.morphometry_run

Pieces: `FundusTestBatches` (the feed: FundusSegmentation(phase='test', state='prediction') under Resize(256) / Normalize_tf /
ToTensor with the original-size labels, fundus_dataloader.py:100-135), `load_checkpoint` (the filtered load_state_dict sequence,
test_visulization.py:132-193), `TestRun` (the driver) and `overlay_host`, the readable specification of the pictures in numpy whose
device form is ops.overlay (csrc/overlay.hip) — the pair validate.postprocess / ops.postprocess_masks once more.

The pictures, restated (overlay_host):
  * untransform (utils.py:460-463): (img + 1) * 127.5 in fp32, truncated by astype(np.uint8); `original` is saved before painting.
  * composite (test_visulization.py:243-256): channel 0 = cup, channel 1 = disc OR cup.  save_per_img names channel 0 `disc_map` and
    channel 1 `cup_map` (utils.py:385-386) — swapped against the content — and the colours follow the names: the cup's contour comes
    out blue, the disc-or-cup contour green.  Kept.  The ground truth's composite is built the same way and each of its channels goes
    through get_largest_fillhole (utils.py:426-427).
  * the two prediction channels get their first / last row and column zeroed (utils.py:388-396); the ground truth does not.
  * measure.find_contours(map, 0.5) on a 0/1 map has a vertex at the midpoint of every horizontally or vertically adjacent pixel pair
    whose values differ; every vertex (r, c) paints int(r + dr), int(c + dc) for seven offsets (utils.py:408-448), int truncating
    towards zero.  Painted last wins: prediction channel 1 (green), channel 0 (blue), ground truth channel 1, channel 0 (both red).
  * an index of -1 (ground truth touching the first row / column) wraps to the last row / column, as numpy indexing does.
  * DEVIATION, the only one: an index equal to h or w (ground truth touching the last row / column) makes the reference raise
    IndexError and end the program; here that single paint is dropped and the run goes on.

**Contour parity unpinned**: `skimage` is not installed, so there is no run of save_per_img to compare with.  The restatement is pinned
instead to an independent marching-squares enumeration (all 16 cases of every 2 x 2 cell with the (level - a) / (b - a)
interpolation, painted in the reference's statement order: tests/test_test_run_cpu.py), and ops.overlay to overlay_host byte for byte.
"""
import json
import os

import numpy as np
import torch

from . import morphometry as M
from . import ops
from . import tables as T
from . import validate as V
from .packed import fetch

PAINT_OFFSETS = ((0, 0), (1, 0), (1, 1), (0, 1), (-1, 0), (-1, -1), (0, -1))       # utils.py:409-415, in statement order
GREEN, BLUE, RED = (0, 255, 0), (0, 0, 255), (255, 0, 0)
CSV_COLUMNS = ("index", "name") + V.METRIC_KEYS


# ---- the pictures on the host: the specification --------------------------------------------------------------------------
def contour_vertices(m):
    """The vertex set of measure.find_contours(m, 0.5) on a 0/1 map -> (rows, cols), float64: (i, j + 0.5) where m[i, j] != m[i, j+1],
    (i + 0.5, j) where m[i, j] != m[i+1, j]."""
    m = np.asarray(m) != 0
    hr, hc = np.nonzero(m[:, :-1] != m[:, 1:])
    vr, vc = np.nonzero(m[:-1, :] != m[1:, :])
    return np.concatenate((hr.astype(np.float64), vr + 0.5)), np.concatenate((hc + 0.5, vc.astype(np.float64)))


def paint_contours(canvas, m, colour):
    """utils.py:408-448 for one map: every vertex paints its seven pixels.  Negative indices wrap (numpy); an index of h or w — where
    the reference raises IndexError — is dropped."""
    h, w = m.shape
    rr, cc = contour_vertices(m)
    for dr, dc in PAINT_OFFSETS:
        r, c = (rr + dr).astype(int), (cc + dc).astype(int)
        keep = (r < h) & (c < w)
        canvas[r[keep], c[keep], :] = colour


def composite(od, oc):
    """test_visulization.py:243-256 -> (channel 0, channel 1) = (cup, disc OR cup), uint8 0 / 1."""
    od, oc = np.asarray(od) == 1, np.asarray(oc) == 1
    return oc.astype(np.uint8), (od | oc).astype(np.uint8)


def overlay_host(img, pred_od, pred_oc, gt_od, gt_oc):
    """One image: img [3,h,w] fp32 (normalised, at the label size), the four masks [h,w] with values 0 / 1 ->
    (original, overlay), uint8 [h,w,3]."""
    img = np.asarray(img, dtype=np.float32)
    patch = ((img + np.float32(1)) * np.float32(127.5)).transpose(1, 2, 0)         # untransform, then HWC (test_visulization.py:265-266)
    assert patch.dtype == np.float32
    original = patch.astype(np.uint8)
    canvas = patch.copy()
    p0, p1 = composite(pred_od, pred_oc)
    for p in (p0, p1):
        p[:, 0] = p[:, -1] = 0
        p[0, :] = p[-1, :] = 0
    g0, g1 = composite(gt_od, gt_oc)
    g0, g1 = V.largest_fillhole(g0).astype(np.uint8), V.largest_fillhole(g1).astype(np.uint8)
    paint_contours(canvas, p1, GREEN)          # `contours_cup` of `cup_map` = channel 1
    paint_contours(canvas, p0, BLUE)           # `contours_disc` of `disc_map` = channel 0
    paint_contours(canvas, g1, RED)
    paint_contours(canvas, g0, RED)
    return original, canvas.astype(np.uint8)


def overlay_host_batch(img, pred_od, pred_oc, gt_od, gt_oc):
    """[B,3,h,w] and four [B,1,h,w] arrays -> (original, overlay) uint8 [B,h,w,3]: ops.overlay's shapes."""
    outs = [overlay_host(img[i], pred_od[i, 0], pred_oc[i, 0], gt_od[i, 0], gt_oc[i, 0]) for i in range(len(img))]
    return np.stack([o for o, _ in outs]), np.stack([o for _, o in outs])


# ---- the feed -----------------------------------------------------------------------------------------------------------
def label_thresholds_host(mask):
    """fundus_dataloader.py:112-134: grey levels -> (original_od, original_oc) uint8: 1 where the byte is <= 200 / <= 50."""
    mask = np.asarray(mask)
    return (mask <= 200).astype(np.uint8), (mask <= 50).astype(np.uint8)


class FundusTestBatches:
    """The reference's test loader — DataLoader(FundusSegmentation(phase='test', state='prediction', transform=Compose([Resize(256),
    Normalize_tf(), ToTensor()])), shuffle=False) — over a `FundusTree(..., phase="test", state="prediction")`: index order over the
    first pool, the last batch short.  Iterating yields (image [B,3,256,256] fp32, original_od, original_oc [B,1,h,w] fp32, names),
    device tensors; `triples()` yields the same without the names — what validate_epoch and TrainRun(val_batches=...) take.
    The images of one batch must share a label size (the reference's collate stacks them): ValueError otherwise."""

    def __init__(self, tree, batch_size, device="cuda"):
        if tree.phase != "test" or tree.state != "prediction":
            raise ValueError("FundusTestBatches needs FundusTree(..., phase='test', state='prediction') (got %r, %r)"
                             % (tree.phase, tree.state))
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        keys = tree.keys()
        self.images, self.masks, self.names = tree.pools[keys[0]] if keys else ([], [], [])
        self.size, self.batch_size, self.device = tree.size, int(batch_size), device

    def __len__(self):
        return (len(self.images) + self.batch_size - 1) // self.batch_size

    def host_sample(self, i):
        """-> (image [3,S,S] fp32, mask [h,w] uint8 grey levels, name)."""
        img = self.images[i].resize((self.size, self.size))     # Resize(256) on the 256 x 256 pool image: Pillow's copy
        a = np.array(img).astype(np.float32)                    # Normalize_tf (custom_transforms.py:468-472)
        a /= 127.5
        a -= 1.0
        return np.ascontiguousarray(a.transpose(2, 0, 1)), np.array(self.masks[i]).astype(np.uint8), self.names[i]

    def host_batch(self, b):
        """Batch b on the host -> (images [B,3,S,S] fp32, masks [B,1,h,w] uint8, names)."""
        idx = range(b * self.batch_size, min((b + 1) * self.batch_size, len(self.images)))
        samples = [self.host_sample(i) for i in idx]
        for _, m, name in samples[1:]:
            if m.shape != samples[0][1].shape:
                raise ValueError("images of one batch must share a label size: %s is %s, %s is %s"
                                 % (samples[0][2], samples[0][1].shape, name, m.shape))
        return np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples])[:, None], [s[2] for s in samples]

    def __iter__(self):
        for b in range(len(self)):
            image, mask, names = self.host_batch(b)
            od, oc = ops.label_thresholds(torch.from_numpy(mask).to(self.device))
            yield torch.from_numpy(image).to(self.device), od, oc, names

    def triples(self):
        for image, od, oc, _ in self:
            yield image, od, oc


# ---- checkpoint ---------------------------------------------------------------------------------------------------------
CHECKPOINT_KEYS = ("model", "model_shape", "model_oc", "model_oc_shape")


def load_checkpoint(path_or_dict, model, model_shape, model_oc, model_shape_oc):
    """test_visulization.py:122,132-193: for each of the four networks keep the checkpoint's entries the network has, overwrite its
    own state_dict with them and load that."""
    ckpt = path_or_dict
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
    for net, key in zip((model, model_shape, model_oc, model_shape_oc), CHECKPOINT_KEYS):
        model_dict = net.state_dict()
        pretrained_dict = {k: v for k, v in ckpt[key].items() if k in model_dict}
        model_dict.update(pretrained_dict)
        net.load_state_dict(model_dict)
    return ckpt


# ---- the table ----------------------------------------------------------------------------------------------------------
def write_table(out_dir, rows, means):
    """rows: [{index, name, <METRIC_KEYS>}] -> out_dir/per_image.csv (floats as repr: they read back to the same float64) and
    out_dir/summary.json (the means and n)."""
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, "per_image.csv"), CSV_COLUMNS, rows, ("index",))
    T.write_json(os.path.join(out_dir, "summary.json"), means, allow_nan=True)           # (the only summary that may hold NaN)


def read_table(out_dir):
    """-> (rows, means) as write_table wrote them."""
    return T.read_csv(os.path.join(out_dir, "per_image.csv"), ("index",)), T.read_json(os.path.join(out_dir, "summary.json"))


# ---- the driver -----------------------------------------------------------------------------------------------------------
def _check_side(what, v):
    if v not in ("host", "device"):
        raise ValueError("%s must be 'host' or 'device', got %r" % (what, v))


class TestRun:
    """The loop of test_visulization.py:201-269 plus the metric table.  overlay / metrics pick the side the pictures / the numbers are
    computed on; both sides consume the same device predictions and the same device-resized image, so their pictures, Dice and HD95
    are identical and ASD agrees within validate.py's 1e-12 relative.

    morphometry=True (sectors, eye: morphometry.py) also runs ops.mask_geometry + ops.onh_profile on the prediction's masks and on the
    label's masks: `batch` appends the batch's `morphometry.finish` rows to `self.morph_pred` / `self.morph_label`, and `run` writes
    O/morphometry_errors.csv (`self.morph_rows`, `self.morph_means`).  Off, the default, nothing more runs and nothing more is written."""
    __test__ = False                        # (the name starts with "Test": not a pytest class)

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, overlay="device", metrics="device", morphometry=False,
                 sectors=24, eye=None):
        _check_side("overlay", overlay)
        _check_side("metrics", metrics)
        self.morphometry, self.sectors, self.eye = bool(morphometry), M.check_sectors(sectors), M.check_eye(eye)
        self.morph_pred, self.morph_label, self.morph_rows, self.morph_means = [], [], [], None
        self.nets = [model, model_shape, model_oc, model_shape_oc]
        self.out_dir, self.overlay, self.metrics = out_dir, overlay, metrics

    def batch(self, image, label_od, label_oc):
        """One batch -> (per-image metric lists, original [B,h,w,3] uint8, overlay [B,h,w,3] uint8) on the host.  Everything the device
        sides leave — the metric records, the pictures, with morphometry the two mask sets' geometry, profile and moment records —
        comes back in ONE device -> host copy."""
        size = tuple(label_od.shape[2:])
        B = image.shape[0]
        pred, pred_oc = V.predict_pair(*self.nets, image, size)
        img = image.contiguous()
        if size != tuple(img.shape[2:]):
            img = ops.resize_bilinear(img, size)                # test_visulization.py:231-232
        out, masks = [], None
        if self.morphometry or "device" in (self.overlay, self.metrics):
            masks = ops.postprocess_masks(torch.cat((pred, pred_oc), 0).contiguous())
        if self.metrics == "device":
            labels = torch.cat((label_od, label_oc), 0).to(torch.float32).contiguous()
            out.append(ops.seg_metrics(masks, labels))
        if self.overlay == "device":
            gt = [(t == 1).to(torch.uint8).contiguous() for t in (label_od, label_oc)]
            out.extend(ops.overlay(img, masks[:B], masks[B:], gt[0], gt[1]))
        if self.morphometry:
            lab = torch.cat([(t == 1).to(torch.uint8) for t in (label_od, label_oc)], 0).contiguous()
            for mk in (masks, lab):
                geom = ops.mask_geometry(mk)
                out.extend((geom,) + tuple(ops.onh_profile(mk[:B], mk[B:], geom[:B], self.sectors)))
        host = iter(fetch(out))                                 # the one copy; taken below in the order it was filled above
        host_masks = None
        if "host" in (self.overlay, self.metrics):
            host_masks = [(V.postprocess(pred[i])[0], V.postprocess(pred_oc[i])[0]) for i in range(B)]
        if self.metrics == "device":
            m = V.finish_records(next(host), B)
        else:
            m = V.host_metrics(pred, pred_oc, label_od, label_oc, masks=host_masks)
        if self.overlay == "device":
            original, over = next(host), next(host)
        else:
            lod, loc = label_od.cpu().numpy(), label_oc.cpu().numpy()
            original, over = overlay_host_batch(img.cpu().numpy(), np.stack([a for a, _ in host_masks])[:, None],
                                                np.stack([b for _, b in host_masks])[:, None], lod, loc)
        if self.morphometry:
            for rows in (self.morph_pred, self.morph_label):
                rec, prof, mom = next(host), next(host), next(host)
                rows.extend(M.finish_batch(rec, mom, prof.view(np.uint32), size[0], size[1], self.eye))
        return m, original, over

    def run(self, batches):
        """batches: iterable of (image, original_od, original_oc[, names]) device tensors (FundusTestBatches) -> the means;
        `self.rows` keeps the per-image table.  Eval mode for the duration, the previous modes restored, as validate_epoch does."""
        from PIL import Image
        for sub in ("original_image", "overlay"):
            os.makedirs(os.path.join(self.out_dir, sub), exist_ok=True)
        acc, self.rows = V.MetricMeans(), []
        self.morph_pred, self.morph_label, self.morph_rows, self.morph_means = [], [], [], None
        with V.eval_mode(self.nets):
            for item in batches:
                image, label_od, label_oc = item[:3]
                names = item[3] if len(item) > 3 else [""] * image.shape[0]
                m, original, over = self.batch(image, label_od, label_oc)
                acc.add(m)
                for i in range(image.shape[0]):
                    n = len(self.rows) + 1                      # num_name_global (test_visulization.py:240)
                    Image.fromarray(original[i]).save(os.path.join(self.out_dir, "original_image", "%d.png" % n))
                    Image.fromarray(over[i]).save(os.path.join(self.out_dir, "overlay", "%d.png" % n))
                    self.rows.append(dict({k: m[k][i] for k in V.METRIC_KEYS}, index=n, name=names[i]))
        means = acc.means()
        write_table(self.out_dir, self.rows, means)
        if self.morphometry:
            self.morph_rows = [dict(M.error_row(p, l), index=r["index"], name=r["name"])
                               for r, p, l in zip(self.rows, self.morph_pred, self.morph_label)]
            self.morph_means = M.write_errors_csv(self.out_dir, self.morph_rows)
        return means


# ---- command line -------------------------------------------------------------------------------------------------------
def build_networks(device):
    """The four networks of test_visulization.py:123-197 at the default hparams (per_domain_batch 3, three source domains)."""
    import algorithms
    import shape_networks
    from .synth import default_hparams
    hp = default_hparams(True)
    mk = lambda two_step: algorithms.WT_PSE(n_channels=3, n_classes=1, hparams=hp, device=device, two_step=two_step, per_domain_batch=3,
                                            source_domain_num=3).to(device)
    mks = lambda: shape_networks.ShapeVariationalDist_x(hp, device, n_classes=1, number_source_domain=3, batch_size=3).to(device)
    return mk(False), mks(), mk(True), mks()


def main(argv=None):
    from .programs import open_test_split, test_run_parser
    args = test_run_parser("test_run", __doc__).parse_args(argv)
    nets, batches = open_test_split("test_run", args)
    run = TestRun(*nets, out_dir=args.out, overlay=args.overlay, metrics=args.metrics)
    means = run.run(batches)
    torch.cuda.synchronize()
    print(json.dumps(means, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
