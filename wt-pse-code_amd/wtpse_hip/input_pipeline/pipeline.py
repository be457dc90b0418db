"""The device pipeline: decoded uint8 samples and the host's draws in, the fp32 training batch out (csrc/pipeline.hip,
csrc/augment.hip, and the optional stages of `stages.RUN_ORDER`)."""
import numpy as np
import torch

from .. import ops
from .augment import gaussian_weights
from .resample import nearest_table, resample_table
from .stages import RUN_ORDER


def device_uniform(n, seed, pos, device="cuda"):
    """n uniform doubles in [0,1): numbers pos .. pos + n - 1 of the Philox4x32-10 stream `seed` (wtpse_uniform_f64)."""
    out = torch.empty(int(n), dtype=torch.float64, device=device)
    ops.lib().call("wtpse_uniform_f64", out.data_ptr(), int(n), int(seed), int(pos), ops.stream_ptr())
    return out


def _dev_u8(a, device):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise ValueError("input samples must be uint8 (decoded images), got %s" % t.dtype)
    return t.to(device, non_blocking=True).contiguous()


def _dev_i32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device, non_blocking=True)


class DeviceInputPipeline:
    """batch = pipeline(images, disc_masks, draws): images [H,W,3] uint8 and disc masks [H,W] uint8 per sample (numpy or
    torch, host or device; sizes may differ between samples), draws = [draw(rng, size) per sample].

    aug_draws = [draw_augment(py_rng, np_rng, size, aug) per sample] switches the augmentation stage on (None, the default: the
    stage does not exist).  The elastic transform's uniform fields come from the device generator — stream `noise_seed`, running
    position `noise_pos` (2 * S * S numbers per sample whose elastic coin fired; run state, see trainer.FundusBatches) — unless
    `noise` [N,2,S,S] fp64 in [0,1) is given (rows of samples without an elastic transform are not read).  The reference draws
    these fields from an unseeded RandomState(None) (custom_transforms.py:108), which nothing can reproduce: the fields are this
    pipeline's own, the arithmetic on them is scipy's.

    mix_draws, appearance_draws, quality_draws, jpeg_draws, clahe: one keyword per optional stage of `stages.RUN_ORDER`, each the
    value that stage's `draw` makes for the batch (stages.py says what each holds).  A keyword left at None, the default, means the
    stage does not exist: no check, no launch, no allocation.  The stages that are on run in `stages.RUN_ORDER` on the uint8 batch,
    after the augmentation stage (after the crop when there is none) and before the normalisation; the masks are not touched.  All
    of them are checked before anything is launched or allocated, and a stage whose batch is neutral throughout — no coin fired —
    launches nothing.  Only the image-quality stage keeps state here: the running position `quality_pos` of its noise in the stream
    `noise_seed` (run state like `noise_pos`)."""

    def __init__(self, size=256, device="cuda", noise_seed=0):
        self.noise_seed, self.noise_pos = int(noise_seed), 0
        self.quality_pos = 0
        self._gauss = None
        self.size = int(size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the device-side input pipeline runs on the GPU only (no CPU fallback)")
        self._resize_tables = {}

    def _resize_table(self, in_size):
        t = self._resize_tables.get(in_size)
        if t is None:
            b, k, ks = resample_table(in_size, self.size, "bicubic")
            t = self._resize_tables[in_size] = (_dev_i32(b, self.device), _dev_i32(k, self.device), ks)
        return t

    def _resample(self, src, bounds, kk, tab, ksize, L, vertical):
        N, H, W, C = src.shape
        out = torch.empty((N, L, W, C) if vertical else (N, H, L, C), dtype=torch.uint8, device=self.device)
        ops.lib().call("wtpse_resample_u8", src.data_ptr(), out.data_ptr(), bounds.data_ptr(), kk.data_ptr(),
                       0 if tab is None else tab.data_ptr(), ksize, N, H, W, C, L, int(vertical), ops.stream_ptr())
        return out

    def _augment(self, img, od1, xidx, yidx, aug_draws, noise):
        """img [N,S,S,3] uint8 (cropped), od1 [N,S,S,1] uint8 behind the index tables -> (img, mask [N,S,S]) uint8 augmented."""
        S, dev, call, st = self.size, self.device, ops.lib().call, ops.stream_ptr()
        N = img.shape[0]
        code = _dev_i32([d["k"] | (4 if d["flip_lr"] else 0) | (8 if d["flip_tb"] else 0) for d in aug_draws], dev)
        out = torch.empty_like(img)
        mask = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
        call("wtpse_aug_geometry", img.data_ptr(), od1.data_ptr(), xidx.data_ptr(), yidx.data_ptr(), code.data_ptr(), out.data_ptr(),
             mask.data_ptr(), N, S, st)
        img = out
        active = [i for i, d in enumerate(aug_draws) if d["elastic"]]
        if active:
            na = len(active)
            if self._gauss is None:
                w, radius = gaussian_weights(S * 0.08)
                self._gauss = (torch.from_numpy(w).to(dev), radius)
            w, radius = self._gauss
            if noise is None:
                u, index = device_uniform(na * 2 * S * S, self.noise_seed, self.noise_pos, dev), None
                self.noise_pos += na * 2 * S * S
            else:
                u = noise if isinstance(noise, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64))
                if tuple(u.shape) != (N, 2, S, S) or u.dtype != torch.float64:
                    raise ValueError("noise must be [%d,2,%d,%d] float64, got %s %s" % (N, S, S, tuple(u.shape), u.dtype))
                u, index = u.to(dev).contiguous(), _dev_i32(active, dev)
            tmp = torch.empty((na, 2, S, S), dtype=torch.float64, device=dev)
            disp = torch.empty_like(tmp)
            call("wtpse_aug_blur", u.data_ptr(), tmp.data_ptr(), w.data_ptr(), 0 if index is None else index.data_ptr(), radius,
                 na * 2, S, 0, 1, 1.0, st)
            call("wtpse_aug_blur", tmp.data_ptr(), disp.data_ptr(), w.data_ptr(), 0, radius, na * 2, S, 1, 0, float(2 * S), st)
            slot = np.full(N, -1, np.int32)
            slot[active] = np.arange(na)
            out, mask2 = torch.empty_like(img), torch.empty_like(mask)
            slot = _dev_i32(slot, dev)
            call("wtpse_aug_warp", img.data_ptr(), mask.data_ptr(), disp.data_ptr(), slot.data_ptr(), out.data_ptr(), mask2.data_ptr(), N, S, st)
            img, mask = out, mask2
        if any(d["sp"] is not None or d["lut"] is not None or d["rect"] is not None for d in aug_draws):
            ident = np.arange(256, dtype=np.uint8)
            lut = np.stack([ident if d["lut"] is None else np.asarray(d["lut"], np.uint8) for d in aug_draws])
            rect = np.array([(0, 0, 0, 0, 0) if d["rect"] is None else d["rect"] for d in aug_draws], np.int32)
            pts = [np.zeros(0, np.int32) if d["sp"] is None else d["sp"][1].astype(np.int32) * S + d["sp"][2].astype(np.int32)
                   for d in aug_draws]
            off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
            val = [0 if d["sp"] is None else int(d["sp"][0]) for d in aug_draws]
            max_pts = max(len(p) for p in pts)
            # every table stays referenced until the launch is queued: a temporary's block would be handed to the next allocation
            # and overwritten by its copy before the kernel reads it
            dpts = _dev_i32(np.concatenate(pts), dev) if max_pts else None
            lut, rect, off, val = torch.from_numpy(lut).to(dev), _dev_i32(rect, dev), _dev_i32(off, dev), _dev_i32(val, dev)
            call("wtpse_aug_photometric", img.data_ptr(), lut.data_ptr(), rect.data_ptr(), 0 if dpts is None else dpts.data_ptr(),
                 off.data_ptr(), val.data_ptr(), max_pts, N, S, st)
        return img, mask

    def __call__(self, images, disc_masks, draws, aug_draws=None, noise=None, mix_draws=None, quality_draws=None, clahe=None,
                 appearance_draws=None, jpeg_draws=None):
        S, dev = self.size, self.device
        N = len(images)
        assert len(disc_masks) == N and len(draws) == N and (aug_draws is None or len(aug_draws) == N)
        given = {"mix_draws": mix_draws, "appearance_draws": appearance_draws, "quality_draws": quality_draws,
                 "jpeg_draws": jpeg_draws, "clahe": clahe}
        on = [(stage, stage.check(given[stage.pipe_kw], N, S)) for stage in RUN_ORDER if given[stage.pipe_kw] is not None]
        # ---- Resize(S): bicubic, horizontal pass then vertical pass, batched over samples of one input size
        img1 = torch.empty((N, S, S, 3), dtype=torch.uint8, device=dev)
        od1 = torch.empty((N, S, S, 1), dtype=torch.uint8, device=dev)
        groups = {}
        for i, im in enumerate(images):
            groups.setdefault(tuple(im.shape[:2]), []).append(i)
        for (H, W), idx in groups.items():
            im = torch.stack([_dev_u8(images[i], dev) for i in idx])
            md = torch.stack([_dev_u8(disc_masks[i], dev) for i in idx]).unsqueeze(-1)
            sel = torch.tensor(idx, device=dev)
            for src, dst in ((im, img1), (md, od1)):
                t = src
                if W != S:
                    b, k, ks = self._resize_table(W)
                    t = self._resample(t, b, k, None, ks, S, False)
                if H != S:
                    b, k, ks = self._resize_table(H)
                    t = self._resample(t, b, k, None, ks, S, True)
                dst[sel] = t
        # ---- RandomScaleCrop(S): bilinear up-scale to (nw, nh) and crop, only for the S columns / rows that survive;
        # unscaled samples get the identity table.  The disc mask's NEAREST resize + crop is an index gather.
        hb, hk, vb, vk, xi, yi = [], [], [], [], [], []
        for nw, nh, x1, y1 in draws:
            b, k, ks = resample_table(S, nw, "bilinear", x1, S)
            hb.append(b); hk.append(k)
            b, k, ks = resample_table(S, nh, "bilinear", y1, S)
            vb.append(b); vk.append(k)
            xi.append(nearest_table(S, nw, x1, S))
            yi.append(nearest_table(S, nh, y1, S))
        tab = torch.arange(N, dtype=torch.int32, device=dev)
        t = self._resample(img1, _dev_i32(np.stack(hb), dev), _dev_i32(np.stack(hk), dev), tab, 3, S, False)
        img2 = self._resample(t, _dev_i32(np.stack(vb), dev), _dev_i32(np.stack(vk), dev), tab, 3, S, True)
        image = torch.empty((N, 3, S, S), dtype=torch.float32, device=dev)
        od = torch.empty((N, 1, S, S), dtype=torch.float32, device=dev)
        oc = torch.empty((N, 1, S, S), dtype=torch.float32, device=dev)
        xidx, yidx = _dev_i32(np.stack(xi), dev), _dev_i32(np.stack(yi), dev)
        if aug_draws is not None:
            # the augmentation stage leaves the mask cropped: input_finish reads it through identity tables
            img2, od1 = self._augment(img2, od1, xidx, yidx, aug_draws, noise)
            xidx = yidx = torch.arange(S, dtype=torch.int32, device=dev).repeat(N, 1).contiguous()
        for stage, value in on:
            if not stage.idle(value):
                img2 = stage.run(self, img2, value)
        ops.lib().call("wtpse_input_finish", img2.data_ptr(), od1.data_ptr(), xidx.data_ptr(), yidx.data_ptr(), image.data_ptr(),
                       od.data_ptr(), oc.data_ptr(), N, S, ops.stream_ptr())
        return image, od, oc
