"""Test run: counterpart of the reference's second program, test_visulization.py — a trained checkpoint, the target domain's `test`
split through both stages, and per image the input picture plus an overlay of the predicted cup / disc contours and the ground
truth's (red) at the label's original resolution (test_visulization.py:100-269, utils.save_per_img utils.py:371-454).  On top of the
pictures this run writes what the reference never did: a per-image metric table and its means (the numbers of Trainer.validate).

    python -m wtpse_hip.test_run --data-dir D --datasetTest 3 --checkpoint C --out O [--batch-size 9]

    O/original_image/<n>.png      the image, untransformed, at the label size           n = 1, 2, ... over the whole run
    O/overlay/<n>.png             the same with the contours painted
    O/per_image.csv               index, name, disc_dice, cup_dice, disc_hd, disc_asd, cup_hd, cup_asd
    O/summary.json                their means and n — equal to validate.validate_epoch on the same batches

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

from . import ops
from . import validate as V

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
    with open(os.path.join(out_dir, "per_image.csv"), "w") as f:
        f.write(",".join(CSV_COLUMNS) + "\n")
        for r in rows:
            name = str(r["name"])
            if any(ch in name for ch in ',"\n'):
                name = '"' + name.replace('"', '""') + '"'
            f.write(",".join([str(int(r["index"])), name] + [repr(float(r[k])) for k in V.METRIC_KEYS]) + "\n")
    with open(os.path.join(out_dir, "summary.json"), "w") as f:
        json.dump(means, f, indent=1, sort_keys=True)
        f.write("\n")


def read_table(out_dir):
    """-> (rows, means) as write_table wrote them."""
    import csv
    with open(os.path.join(out_dir, "per_image.csv"), newline="") as f:
        rows = [dict(r, index=int(r["index"]), **{k: float(r[k]) for k in V.METRIC_KEYS}) for r in csv.DictReader(f)]
    with open(os.path.join(out_dir, "summary.json")) as f:
        return rows, json.load(f)


# ---- the driver -----------------------------------------------------------------------------------------------------------
def _check_side(what, v):
    if v not in ("host", "device"):
        raise ValueError("%s must be 'host' or 'device', got %r" % (what, v))


class TestRun:
    """The loop of test_visulization.py:201-269 plus the metric table.  overlay / metrics pick the side the pictures / the numbers are
    computed on; both sides consume the same device predictions and the same device-resized image, so their pictures, Dice and HD95
    are identical and ASD agrees within validate.py's 1e-12 relative."""
    __test__ = False                        # (the name starts with "Test": not a pytest class)

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, overlay="device", metrics="device"):
        _check_side("overlay", overlay)
        _check_side("metrics", metrics)
        self.nets = [model, model_shape, model_oc, model_shape_oc]
        self.out_dir, self.overlay, self.metrics = out_dir, overlay, metrics

    def batch(self, image, label_od, label_oc):
        """One batch -> (per-image metric lists, original [B,h,w,3] uint8, overlay [B,h,w,3] uint8) on the host.  With both sides on the
        device everything comes back in ONE device -> host copy."""
        size = tuple(label_od.shape[2:])
        B = image.shape[0]
        pred, pred_oc = V.predict_pair(*self.nets, image, size)
        img = image.contiguous()
        if size != tuple(img.shape[2:]):
            img = ops.resize_bilinear(img, size)                # test_visulization.py:231-232
        blob, masks = [], None
        if "device" in (self.overlay, self.metrics):
            masks = ops.postprocess_masks(torch.cat((pred, pred_oc), 0).contiguous())
        if self.metrics == "device":
            labels = torch.cat((label_od, label_oc), 0).to(torch.float32).contiguous()
            blob.append(ops.seg_metrics(masks, labels).view(torch.uint8).reshape(-1))
        if self.overlay == "device":
            gt = [(t == 1).to(torch.uint8).contiguous() for t in (label_od, label_oc)]
            blob.extend(t.reshape(-1) for t in ops.overlay(img, masks[:B], masks[B:], gt[0], gt[1]))
        host = (torch.cat(blob) if len(blob) > 1 else blob[0]).cpu().numpy() if blob else None      # the one copy
        host_masks = None
        if "host" in (self.overlay, self.metrics):
            host_masks = [(V.postprocess(pred[i])[0], V.postprocess(pred_oc[i])[0]) for i in range(B)]
        off = 0
        if self.metrics == "device":
            m = V.finish_records(host[:2 * B * 64].view(np.int64).reshape(2 * B, 8), B)
            off = 2 * B * 64
        else:
            m = V.host_metrics(pred, pred_oc, label_od, label_oc, masks=host_masks)
        if self.overlay == "device":
            n = B * size[0] * size[1] * 3
            original, over = host[off:off + n].reshape(B, size[0], size[1], 3), host[off + n:off + 2 * n].reshape(B, size[0], size[1], 3)
        else:
            lod, loc = label_od.cpu().numpy(), label_oc.cpu().numpy()
            original, over = overlay_host_batch(img.cpu().numpy(), np.stack([a for a, _ in host_masks])[:, None],
                                                np.stack([b for _, b in host_masks])[:, None], lod, loc)
        return m, original, over

    def run(self, batches):
        """batches: iterable of (image, original_od, original_oc[, names]) device tensors (FundusTestBatches) -> the means;
        `self.rows` keeps the per-image table.  Eval mode for the duration, the previous modes restored, as validate_epoch does."""
        from PIL import Image
        modes = [n.training for n in self.nets]
        for n in self.nets:
            n.eval()
        for sub in ("original_image", "overlay"):
            os.makedirs(os.path.join(self.out_dir, sub), exist_ok=True)
        acc, self.rows = V.MetricMeans(), []
        try:
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
        finally:
            for n, mode in zip(self.nets, modes):
                n.train(mode)
        means = acc.means()
        write_table(self.out_dir, self.rows, means)
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
    import argparse
    from .fundus_data import FundusTree
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip.test_run", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--datasetTest", type=int, required=True, help="the target domain: Domain<N>/test is read")
    ap.add_argument("--checkpoint", required=True, help="checkpoint_<epoch>.pth.tar as validate.Validator saves it")
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch-size", type=int, default=9)
    ap.add_argument("--overlay", choices=("device", "host"), default="device")
    ap.add_argument("--metrics", choices=("device", "host"), default="device")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("wtpse_hip.test_run needs the GPU: the networks have no CPU path")
    device = "cuda:0"
    torch.cuda.set_device(0)
    nets = build_networks(device)
    load_checkpoint(args.checkpoint, *nets)
    tree = FundusTree(args.data_dir, phase="test", splitid=(args.datasetTest,), state="prediction")
    if len(tree) < 1:
        raise SystemExit("no test images under %s" % os.path.join(args.data_dir, "Domain%d" % args.datasetTest, "test"))
    run = TestRun(*nets, out_dir=args.out, overlay=args.overlay, metrics=args.metrics)
    means = run.run(FundusTestBatches(tree, args.batch_size, device))
    torch.cuda.synchronize()
    print(json.dumps(means, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
