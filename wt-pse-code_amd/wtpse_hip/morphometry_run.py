"""The test run with optic-disc morphometry: test_run.TestRun plus, per image, the moment-based cup-to-disc ratios and the rim minimum
(morphometry.py) of the prediction and of the label, side by side — the place to see how good those numbers are against ground truth.

    python -m wtpse_hip.morphometry_run --data-dir D --datasetTest 3 --checkpoint C --out O [--batch-size 9] [--sectors 24] [--eye right|left]

writes everything `python -m wtpse_hip.test_run` writes, byte for byte, and

    O/morphometry_errors.csv      index, name, {vcdr_ellipse,hcdr_ellipse,rim_min_rel}_{pred,label,abs_diff}, closed by a row of means

`MorphometryTestRun(..., morphometry=False)` is TestRun: nothing more runs and nothing more is written.  On, the same pass
(ops.mask_geometry + ops.onh_profile) runs on the prediction's masks and on the label's masks — both are on the device there — and
their records ride in the batch's one device -> host copy.  It lives beside test_run.py as a subclass so that module stays as it is:
`batch` restates TestRun.batch with the pass added before the copy (tests/test_morphometry_gpu.py holds the two to the same metrics
and pictures).  The switch belongs in TestRun itself; a change that edits test_run.py should move it there and drop this module.
"""
import json
import os

import numpy as np
import torch

from . import morphometry as M
from . import ops
from . import validate as V
from .test_run import FundusTestBatches, TestRun, build_networks, load_checkpoint, overlay_host_batch


class MorphometryTestRun(TestRun):
    """TestRun(..., morphometry=False, sectors=24, eye=None).  On: `batch` also appends the batch's `morphometry.finish` rows to
    `self.morph_pred` / `self.morph_label`, and `run` writes O/morphometry_errors.csv (`self.morph_rows`, `self.morph_means`)."""
    __test__ = False

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, overlay="device", metrics="device", morphometry=False,
                 sectors=24, eye=None):
        self.morphometry, self.sectors, self.eye = bool(morphometry), M.check_sectors(sectors), M.check_eye(eye)
        self.morph_pred, self.morph_label, self.morph_rows, self.morph_means = [], [], [], None
        super().__init__(model, model_shape, model_oc, model_shape_oc, out_dir, overlay=overlay, metrics=metrics)

    def batch(self, image, label_od, label_oc):
        """TestRun.batch, and with morphometry on the two mask sets' geometry, profile and moment records in the same single copy."""
        if not self.morphometry:
            return super().batch(image, label_od, label_oc)
        size = tuple(label_od.shape[2:])
        B, N = image.shape[0], self.sectors
        pred, pred_oc = V.predict_pair(*self.nets, image, size)
        img = image.contiguous()
        if size != tuple(img.shape[2:]):
            img = ops.resize_bilinear(img, size)
        blob = []
        masks = ops.postprocess_masks(torch.cat((pred, pred_oc), 0).contiguous())
        if self.metrics == "device":
            labels = torch.cat((label_od, label_oc), 0).to(torch.float32).contiguous()
            blob.append(ops.seg_metrics(masks, labels).view(torch.uint8).reshape(-1))
        if self.overlay == "device":
            gt = [(t == 1).to(torch.uint8).contiguous() for t in (label_od, label_oc)]
            blob.extend(t.reshape(-1) for t in ops.overlay(img, masks[:B], masks[B:], gt[0], gt[1]))
        lab = torch.cat([(t == 1).to(torch.uint8) for t in (label_od, label_oc)], 0).contiguous()
        for mk in (masks, lab):
            geom = ops.mask_geometry(mk)
            blob.append(geom.view(torch.uint8).reshape(-1))
            blob.extend(t.view(torch.uint8).reshape(-1) for t in ops.onh_profile(mk[:B], mk[B:], geom[:B], N))
        host = torch.cat(blob).cpu().numpy()                             # the one copy
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
        per_set = (192 + 16 * N) * B                                     # records 128 B, profile 16 N B, moments 64 B per image
        off = len(host) - 2 * per_set                                    # the last entries of the blob
        for rows in (self.morph_pred, self.morph_label):
            rec = host[off:off + 128 * B].copy().view(np.int64).reshape(2 * B, 8)
            prof = host[off + 128 * B:off + (128 + 16 * N) * B].copy().view(np.uint32).reshape(B, N, 4)
            mom = host[off + (128 + 16 * N) * B:off + per_set].copy().view(np.int64).reshape(B, 2, 4)
            rows.extend(M.finish_batch(rec, mom, prof, size[0], size[1], self.eye))
            off += per_set
        return m, original, over

    def run(self, batches):
        self.morph_pred, self.morph_label, self.morph_rows, self.morph_means = [], [], [], None
        means = super().run(batches)
        if self.morphometry:
            self.morph_rows = [dict(M.error_row(p, l), index=r["index"], name=r["name"])
                               for r, p, l in zip(self.rows, self.morph_pred, self.morph_label)]
            self.morph_means = M.write_errors_csv(self.out_dir, self.morph_rows)
        return means


# ---- command line -------------------------------------------------------------------------------------------------------------
def main(argv=None):
    import argparse
    from .fundus_data import FundusTree
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip.morphometry_run", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--datasetTest", type=int, required=True, help="the target domain: Domain<N>/test is read")
    ap.add_argument("--checkpoint", required=True, help="checkpoint_<epoch>.pth.tar as validate.Validator saves it")
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch-size", type=int, default=9)
    ap.add_argument("--overlay", choices=("device", "host"), default="device")
    ap.add_argument("--metrics", choices=("device", "host"), default="device")
    ap.add_argument("--sectors", type=int, default=24, help="angular sectors of the rim profile: a multiple of 8 in 8..360")
    ap.add_argument("--eye", choices=("right", "left"), default=None)
    args = ap.parse_args(argv)
    M.check_sectors(args.sectors)
    if not torch.cuda.is_available():
        raise SystemExit("wtpse_hip.morphometry_run needs the GPU: the networks have no CPU path")
    device = "cuda:0"
    torch.cuda.set_device(0)
    nets = build_networks(device)
    load_checkpoint(args.checkpoint, *nets)
    tree = FundusTree(args.data_dir, phase="test", splitid=(args.datasetTest,), state="prediction")
    if len(tree) < 1:
        raise SystemExit("no test images under %s" % os.path.join(args.data_dir, "Domain%d" % args.datasetTest, "test"))
    run = MorphometryTestRun(*nets, out_dir=args.out, overlay=args.overlay, metrics=args.metrics, morphometry=True, sectors=args.sectors,
                             eye=args.eye)
    means = run.run(FundusTestBatches(tree, args.batch_size, device))
    torch.cuda.synchronize()
    print(json.dumps(dict(means, **run.morph_means), sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
