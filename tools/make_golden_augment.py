#!/usr/bin/env python3
"""BUILD CONTAINER / any CPU box with the reference checked out (TEST INFRASTRUCTURE): the reference's OWN augmentation classes
(custom_transforms.py through oracle/ref_import.load_transforms) -> tests/golden/augment.npz, the fixture of
tests/test_augment_cpu.py and tests/test_augment_gpu.py.

    python tools/make_golden_augment.py

The classes are applied in the order the device stage uses — RandomRotate, RandomFlip, elastic_transform,
add_salt_pepper_noise, adjust_light, eraser — with 'label' = the disc mask, on one synthetic square sample per size (S = 64 and
S = 96, in the style of oracle/make_golden_transforms.synth_sample), after `random.seed(py_seed)` and `np.random.seed(np_seed)`.

Two shims, neither touching arithmetic:
  * cv2 is not installed; `cv2.LUT = lambda img, table: table[img]` is what LUT does on uint8;
  * elastic_transform draws its two fields from `np.random.RandomState(None)`: for the duration of that call RandomState returns a
    seeded generator (noise_seed) that records the two fields it hands out.
The eraser reads `image.shape`, so a PIL image that reaches it (no numpy-producing class in front) is turned into an array first.

Cases (per size; seeds are searched with the product's own `draw_augment`, so that every branch is hit, and asserted here):
each class alone with its coin firing — all four degrees, both flips, salt and pepper, an eraser with at least one rejected
rectangle — all six together, and one where all six run and nothing fires.  RandomRotate draws its angle in the constructor: the
constructor runs after `random.seed(ctor_seed)`, and the angle is stored.

Stored per case (numbers only): the seeds, which classes ran, the angle, the recorded fields, the outputs, and the next
`random.random()` / `np.random.random()` after the chain (pins the number of draws).
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

from oracle import ref_import  # noqa: E402
from oracle.make_golden_transforms import synth_sample  # noqa: E402
from wtpse_hip.input_pipeline import Augment, draw_augment  # noqa: E402

NAMES = ("rotate", "flip", "elastic", "salt_pepper", "light", "erase")
ONLY = {n: {m: m == n for m in NAMES} for n in NAMES}
ALL = {m: True for m in NAMES}


def count_rejections(np_seed, S, sp):
    """How many rectangles the eraser's loop rejects after `np.random.seed(np_seed)` (and after the noise points' draws, if any)."""
    rs = np.random.RandomState(np_seed)
    if sp:
        n = int(np.ceil(0.004 * S * S * 3 * (0.2 if sp == 1 else (1.0 - 0.2))))
        for i in (S, S, 3):
            rs.randint(0, i - 1, n)
    k = 0
    while True:
        s = rs.uniform(0.02, 0.06) * S * S
        r = rs.uniform(0.3, 0.6)
        w, h = int(np.sqrt(s / r)), int(np.sqrt(s * r))
        left, top = rs.randint(0, S), rs.randint(0, S)
        if left + w <= S and top + h <= S:
            return k
        k += 1


def find(S, enabled, degree, want, np_want=None):
    """The first (py_seed, np_seed) whose draws satisfy `want(draw, py_seed)` (and np_want(np_seed, draw))."""
    aug = Augment(rotate_degree=degree or "random", **enabled)
    for py_seed in range(100000):
        d = draw_augment(random.Random(py_seed), np.random.RandomState(0), S, aug)
        if not want(d, py_seed):
            continue
        for np_seed in range(1000):
            if np_want is None or np_want(np_seed, d):
                return py_seed, np_seed
    raise RuntimeError("no seed found")


def ctor_seed_for(degree):
    for s in range(1000):
        if random.Random(s).randint(1, 4) * 90 == degree:
            return s


def cases_for(S):
    first = S == 64
    k_of = lambda deg: (deg // 90) % 4
    out = []
    for deg in ((90, 180) if first else (270, 360)):
        out.append(("rot%d" % deg, ONLY["rotate"], deg, lambda d, s, deg=deg: d["k"] == k_of(deg) and random.Random(s).random() > 0.5, None))
    out.append(("flip", ONLY["flip"], 0, lambda d, s: d["flip_lr"] and d["flip_tb"], None))
    out.append(("flip_lr" if first else "flip_tb", ONLY["flip"], 0,
                (lambda d, s: d["flip_lr"] and not d["flip_tb"]) if first else (lambda d, s: d["flip_tb"] and not d["flip_lr"]), None))
    out.append(("elastic", ONLY["elastic"], 0, lambda d, s: d["elastic"], None))
    sp = 1 if first else 0                    # salt alone at 64, pepper alone at 96; the other one in the all-six case
    out.append(("salt" if first else "pepper", ONLY["salt_pepper"], 0, lambda d, s: d["sp"] is not None and d["sp"][0] == sp, None))
    out.append(("light", ONLY["light"], 0, lambda d, s: d["lut"] is not None, None))
    out.append(("erase", ONLY["erase"], 0, lambda d, s: d["rect"] is not None, lambda s, d: count_rejections(s, S, None) >= 1))
    deg = 270 if first else 90
    out.append(("all", ALL, deg,
                lambda d, s, deg=deg: d["k"] == k_of(deg) and d["flip_lr"] and d["flip_tb"] and d["elastic"] and d["sp"] is not None
                and d["sp"][0] == 1 - sp and d["lut"] is not None and d["rect"] is not None,
                lambda s, d: count_rejections(s, S, 2 if d["sp"][0] == 0 else 1) >= 1))
    out.append(("none", ALL, 180,
                lambda d, s: not (d["k"] or d["flip_lr"] or d["flip_tb"] or d["elastic"]) and d["sp"] is None and d["lut"] is None
                and d["rect"] is None, None))
    return out


def main():
    tr = ref_import.load_transforms()
    from PIL import Image
    tr.cv2.LUT = lambda img, table: table[img]
    real_rs = np.random.RandomState

    def run_reference(img, mask, enabled, degree, py_seed, np_seed, noise_seed):
        chain, fields = [], []
        if enabled["rotate"]:
            random.seed(ctor_seed_for(degree))
            rot = tr.RandomRotate()
            assert rot.degree == degree
            chain.append(("rotate", rot))
        for name, cls in (("flip", tr.RandomFlip), ("elastic", tr.elastic_transform), ("salt_pepper", tr.add_salt_pepper_noise),
                          ("light", tr.adjust_light), ("erase", tr.eraser)):
            if enabled[name]:
                chain.append((name, cls()))

        class Recording:
            def __init__(self, seed=None):
                self.rs = real_rs(noise_seed)

            def rand(self, *shape):
                f = self.rs.rand(*shape)
                fields.append(f.copy())
                return f

        sample = {"image": Image.fromarray(img), "label": Image.fromarray(mask), "img_name": "synthetic"}
        random.seed(py_seed)
        np.random.seed(np_seed)
        for name, t in chain:
            if name == "erase" and not isinstance(sample["image"], np.ndarray):
                sample["image"] = np.array(sample["image"])
            if name == "elastic":
                np.random.RandomState = Recording
            try:
                sample = t(sample)
            finally:
                np.random.RandomState = real_rs
        nxt = (random.random(), np.random.random())
        assert len(fields) in (0, 2)
        return np.array(sample["image"]).astype(np.uint8), np.array(sample["label"]).astype(np.uint8), fields, nxt

    out = {"sizes": np.array([64, 96], np.int64), "names": np.array(NAMES)}
    for S in (64, 96):
        img, mask, _ = synth_sample(np.random.RandomState(700 + S), S, S)
        out["s%d_img" % S], out["s%d_mask" % S] = img, mask
        tags = []
        for ci, (tag, enabled, degree, want, np_want) in enumerate(cases_for(S)):
            py_seed, np_seed = find(S, enabled, degree, want, np_want)
            noise_seed = 4000 + 10 * S + ci
            o_img, o_mask, fields, nxt = run_reference(img, mask, enabled, degree, py_seed, np_seed, noise_seed)
            key = "s%d_%s_" % (S, tag)
            out[key + "seeds"] = np.array([py_seed, np_seed, noise_seed, degree], np.int64)
            out[key + "enabled"] = np.array([enabled[n] for n in NAMES])
            out[key + "img"], out[key + "mask"] = o_img, o_mask
            out[key + "next"] = np.array(nxt, np.float64)
            if fields:
                out[key + "noise"] = np.stack(fields)
            tags.append(tag)
            print("S=%d %-8s py_seed %5d np_seed %3d changed pixels: image %d mask %d" %
                  (S, tag, py_seed, np_seed, int((o_img != img).any(-1).sum()), int((o_mask != mask).sum())))
        out["s%d_cases" % S] = np.array(tags)
    dst = os.path.join(ROOT, "tests", "golden", "augment.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if not ref_import.available():
        sys.exit("reference not present at %s — this fixture can only be generated where it is" % ref_import.REFERENCE_ROOT)
    main()
