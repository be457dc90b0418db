#!/usr/bin/env python3
"""Any CPU box (TEST INFRASTRUCTURE): what a `FundusBatches` with the augmentations and all five input stages on hands its
pipeline over two consecutive batches -> tests/golden/input_stage_draws.npz, the fixture of tests/test_input_stages_cpu.py.

    python tools/make_golden_stage_draws.py

The feed runs over the synthetic tree (oracle.fundus_tree.make_tree, seed 5; three source domains, batch 6, side 64) with a
recording object in the pipeline's place and both generators seeded 11.  Stored per batch b (numbers only), as `b<b>_<name>`: the
crop draws, the augmentation draws flattened to arrays (`flatten_aug`), and every stage's value as the pipeline receives it.  The
fixture pins the random stream of every stage: it was written before the stages were given one protocol and must not change
when a stage is added (tests/test_input_stages_cpu.py compares array for array).
"""
import os
import random
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

OUT = os.path.join(ROOT, "tests", "golden", "input_stage_draws.npz")
SEED, BATCH, SIZE, BATCHES = 11, 6, 64, 2


class RecordingPipe:
    """Stands in for DeviceInputPipeline: keeps the arguments of every call."""

    def __init__(self):
        self.noise_seed, self.noise_pos, self.quality_pos, self.calls = 0, 0, 0, []

    def __call__(self, images, masks, draws, *args, **kw):
        self.calls.append((draws, args, kw))


def stage_configs():
    """The feed keywords of the all-stages feed."""
    from wtpse_hip.input_pipeline import AmplitudeMix, AppearanceNets, Clahe, ImageQuality, JpegCompression
    return {"style": AmplitudeMix(), "quality": ImageQuality(), "clahe": Clahe(tiles=(4, 4)),
            "appearance": AppearanceNets(p=0.8, spacing=16), "jpeg": JpegCompression()}


def make_sets(root):
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    make_tree(root, seed=5)
    return [FundusTree(root, "train", (i,), size=SIZE) for i in (1, 2, 3)]


def flatten_aug(aug_draws):
    """[draw_augment result per sample] -> name -> array.  An absent part is -1 (sp value, rect) or the identity table (lut, with
    has_lut 0); the noise points of all samples lie one behind the other, sp_off [N + 1] delimiting them."""
    pts = [np.zeros((2, 0), np.int32) if d["sp"] is None else np.stack([d["sp"][1], d["sp"][2]]) for d in aug_draws]
    return {
        "aug_flags": np.array([(d["k"], d["flip_lr"], d["flip_tb"], d["elastic"]) for d in aug_draws], np.int32),
        "aug_sp_value": np.array([-1 if d["sp"] is None else d["sp"][0] for d in aug_draws], np.int32),
        "aug_sp_off": np.concatenate([[0], np.cumsum([p.shape[1] for p in pts])]).astype(np.int32),
        "aug_sp_points": np.concatenate(pts, 1).astype(np.int32),
        "aug_has_lut": np.array([d["lut"] is not None for d in aug_draws], np.int32),
        "aug_lut": np.stack([np.arange(256, dtype=np.uint8) if d["lut"] is None else d["lut"] for d in aug_draws]),
        "aug_rect": np.array([(-1,) * 5 if d["rect"] is None else d["rect"] for d in aug_draws], np.int32),
    }


def flatten_call(call):
    """One recorded call of the all-stages feed -> name -> array."""
    draws, args, kw = call
    (aug_draws,) = args
    out = {"draws": np.array(draws, np.int32)}
    out.update(flatten_aug(aug_draws))
    partner, lam, band = kw["mix_draws"]
    out.update(mix_partner=partner, mix_lam=lam, mix_band=np.array(band))
    out["quality"] = kw["quality_draws"]
    params, field, spacing = kw["appearance_draws"]
    out.update(appearance_params=params, appearance_field=field, appearance_spacing=np.array(spacing))
    mode, tables = kw["jpeg_draws"]
    out.update(jpeg_mode=mode, jpeg_tables=tables)
    r = kw["clahe"].record()
    out["clahe"] = np.array([r["clip_q8"], r["ty"], r["tx"], r["floor"], ("luma", "rgb").index(r["mode"])], np.int32)
    return out


def record(root):
    """Run the all-stages feed for BATCHES batches over a tree made under `root` -> name -> array."""
    from wtpse_hip.input_pipeline import Augment
    from wtpse_hip.trainer import FundusBatches
    pipe = RecordingPipe()
    feed = FundusBatches(make_sets(root), BATCH, "cpu", size=SIZE, augment=Augment(), pipe=pipe, **stage_configs())
    py_rng, np_rng = random.Random(SEED), np.random.RandomState(SEED)
    out = {}
    for b in range(BATCHES):
        feed(py_rng, np_rng)
        out.update({"b%d_%s" % (b, k): np.asarray(v) for k, v in flatten_call(pipe.calls[-1]).items()})
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        arrays = record(os.path.join(tmp, "tree"))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
