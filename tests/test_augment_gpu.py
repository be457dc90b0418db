"""The device-side augmentation stage (csrc/augment.hip) — everything here is bitwise, there is no tolerance:
(a) against the reference's own classes (tests/golden/augment.npz), (b) against `augment_host` at the production geometry and at a
ragged size, (c) switched off against today's batches, (d) the device uniform against its restatement, (e) a resumed feed."""
import os
import random

import numpy as np
import pytest
import torch

from test_augment_cpu import fixture_cases, philox_uniform
from wtpse_hip.input_pipeline import (Augment, DeviceInputPipeline, augment_host, device_uniform, draw, draw_augment, gamma_table)

pytestmark = pytest.mark.gpu

NO_AUG = {"k": 0, "flip_lr": False, "flip_tb": False, "elastic": False, "sp": None, "lut": None, "rect": None}


def finish_host(img_u8, mask_u8):
    """Normalize_tf + ToTensor on the cropped uint8 sample, as wtpse_input_finish: two fp32 roundings, (mask <= 200), (mask <= 50)."""
    a = img_u8.astype(np.float32)
    a /= 127.5
    a -= 1.0
    return a.transpose(2, 0, 1), (mask_u8 <= 200).astype(np.float32)[None], (mask_u8 <= 50).astype(np.float32)[None]


def assert_batch(batch, i, want, what):
    for t, w, name in zip(batch, want, ("image", "od", "oc")):
        got = t[i].cpu().numpy()
        assert got.dtype == w.dtype and np.array_equal(got, w), "%s: %s differs in %d places" % (what, name, int((got != w).sum()))


@pytest.mark.parametrize("S", [64, 96])
def test_device_equals_reference_fixture(S, golden_dir):
    """(a) every fixture case of one size in one batch: image and both masks after input_finish."""
    cases = [c for c in fixture_cases(golden_dir) if c[0] == S]
    assert len(cases) == 10
    draws, noise = [], np.zeros((len(cases), 2, S, S))
    for i, (_, tag, aug, py_seed, np_seed, img, mask, nz, _, _, _) in enumerate(cases):
        draws.append(draw_augment(random.Random(py_seed), np.random.RandomState(np_seed), S, aug))
        if nz is not None:
            noise[i] = nz
    pipe = DeviceInputPipeline(S, "cuda")
    batch = pipe([c[5] for c in cases], [c[6] for c in cases], [(S, S, 0, 0)] * len(cases), draws, noise)
    assert pipe.noise_pos == 0                                       # explicit noise leaves the generator where it was
    for i, c in enumerate(cases):
        assert_batch(batch, i, finish_host(c[8], c[9]), "S=%d %s" % (S, c[1]))


def cropped_u8(img, od, crop, S):
    """Resize(S) + RandomScaleCrop(S) of one sample on the host (oracle/transforms_cpu.py): the uint8 picture the stage works on."""
    from oracle import transforms_cpu as T
    img, od = T.resample_u8(img, S, S, "bicubic"), T.resample_u8(od, S, S, "bicubic")
    nw, nh, x1, y1 = crop
    if (nw, nh) != (S, S):
        img, od = T.resample_u8(img, nw, nh, "bilinear"), T.nearest_u8(od, nw, nh)
    return np.ascontiguousarray(img[y1:y1 + S, x1:x1 + S]), np.ascontiguousarray(od[y1:y1 + S, x1:x1 + S])


@pytest.mark.parametrize("S", [256, 50])
def test_device_equals_host(S):
    """(b) N = 3 with mixed flags at S = 256 (radius 82, the production geometry) and S = 50 (radius 16; no tile of any kernel is
    full), through real resize and crop tables, with the device generator's noise.  Sample 1 has nothing active and must come out as
    the un-augmented pipeline leaves it."""
    rs = np.random.RandomState(8 + S)
    sizes = [(S + 40, S + 21), (S, S), (2 * S - 3, S + 9)]
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    yy = [np.mgrid[0:h, 0:w] for h, w in sizes]
    masks = [np.where(np.hypot(y - h * 0.45, x - w * 0.55) < min(h, w) * 0.15, 0,
                      np.where(np.hypot(y - h * 0.45, x - w * 0.55) < min(h, w) * 0.3, 128, 255)).astype(np.uint8)
             for (y, x), (h, w) in zip(yy, sizes)]
    crops = [(int(1.3 * S), int(1.2 * S), 5, 7), (S, S, 0, 0), (int(1.1 * S), int(1.45 * S), 3, 2)]
    n_pts = int(np.ceil(0.004 * S * S * 3 * 0.8))
    pts = lambda: (rs.randint(0, S - 1, n_pts).astype(np.int32), rs.randint(0, S - 1, n_pts).astype(np.int32))
    aug_draws = [
        dict(NO_AUG, k=1, flip_tb=True, elastic=True, sp=(0,) + pts(), lut=gamma_table(0.7), rect=(S // 3, S // 5, S // 6, S // 4, 201)),
        dict(NO_AUG),
        dict(NO_AUG, k=3, flip_lr=True, elastic=True, sp=(1,) + pts(), rect=(S - S // 7, 0, S // 7, S, 0)),
    ]
    pipe = DeviceInputPipeline(S, "cuda", noise_seed=11)
    pipe.noise_pos = 12345                                            # an odd position: the stream is addressable anywhere
    plain = pipe(imgs, masks, crops)
    assert pipe.noise_pos == 12345
    batch = pipe(imgs, masks, crops, aug_draws)
    assert pipe.noise_pos == 12345 + 2 * 2 * S * S
    noise = device_uniform(2 * 2 * S * S, 11, 12345).cpu().numpy().reshape(2, 2, S, S)
    assert noise.min() >= 0.0 and noise.max() < 1.0
    slot = {0: 0, 2: 1}
    for i, d in enumerate(aug_draws):
        img, mask = cropped_u8(imgs[i], masks[i], crops[i], S)
        assert_batch(plain, i, finish_host(img, mask), "un-augmented sample %d" % i)
        got = augment_host(img, mask, d, noise[slot[i]] if i in slot else None)
        assert_batch(batch, i, finish_host(*got), "S=%d sample %d" % (S, i))
        assert (i == 1) == all(torch.equal(a[i], b[i]) for a, b in zip(plain, batch))
    # the same stage with the noise handed in equals the generator's path
    again = pipe(imgs, masks, crops, aug_draws, np.stack([noise[0], np.zeros((2, S, S)), noise[1]]))
    assert all(torch.equal(a, b) for a, b in zip(batch, again))


def test_default_path_is_unchanged(golden_dir):
    """(c) no aug_draws, and draws in which nothing fires, both give today's batches: the transforms.npz fixture."""
    g = np.load(os.path.join(golden_dir, "transforms.npz"))
    size, n = int(g["size"]), int(g["n"])
    pipe = DeviceInputPipeline(size, "cuda")
    draws = [draw(random.Random(int(g["seed%d" % i])), size) for i in range(n)]
    assert any(d[:2] != (size, size) for d in draws)
    imgs, ods = [g["in%d_img" % i] for i in range(n)], [g["in%d_od" % i] for i in range(n)]
    for aug_draws in (None, [dict(NO_AUG) for _ in range(n)]):
        batch = pipe(imgs, ods, draws, aug_draws)
        for i in range(n):
            assert_batch(batch, i, (g["out%d_img" % i], g["out%d_od" % i], g["out%d_oc" % i]), "sample %d" % i)
    assert pipe.noise_pos == 0


def test_device_uniform_equals_restatement():
    """(d) bitwise at two positions (one odd, one beyond 2^32), and a continued call equals one longer call."""
    for seed, pos in ((1234, 0), (77, (1 << 33) + 12345)):
        got = device_uniform(700, seed, pos).cpu().numpy()
        assert np.array_equal(got, philox_uniform(seed, pos, 700)), (seed, pos)
    whole = device_uniform(5001, 9, 40)
    first, second = device_uniform(2001, 9, 40), device_uniform(3000, 9, 40 + 2001)
    assert torch.equal(torch.cat([first, second]), whole)
    assert float(whole.min()) >= 0.0 and float(whole.max()) < 1.0


def test_feed_resumes_bitwise(tmp_path):
    """(e) FundusBatches with augmentations on the synthetic PNG tree: a feed interrupted after two batches, saved and rebuilt, hands
    out the third batch of the uninterrupted feed — same samples, crops, augmentation draws and elastic noise."""
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.trainer import FundusBatches
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    sets = [FundusTree(root, "train", (i,), size=64) for i in (1, 2, 3)]

    def feed():
        f = FundusBatches(sets, 6, "cuda", size=64, augment=Augment())
        f.set_seed(3)
        return f

    a, py_a, np_a = feed(), random.Random(3), np.random.RandomState(3)
    batches_a = [a(py_a, np_a) for _ in range(3)]
    b, py_b, np_b = feed(), random.Random(3), np.random.RandomState(3)
    for k in range(2):
        assert all(torch.equal(x, y) for x, y in zip(b(py_b, np_b), batches_a[k]))
    saved = (b.state(), py_b.getstate(), np_b.get_state())
    assert saved[0]["noise_pos"] > 0 and saved[0]["noise_pos"] % (2 * 64 * 64) == 0       # an elastic transform has fired
    c, py_c, np_c = feed(), random.Random(0), np.random.RandomState(0)
    c.load_state(saved[0])
    py_c.setstate(saved[1])
    np_c.set_state(saved[2])
    third = c(py_c, np_c)
    assert all(torch.equal(x, y) for x, y in zip(third, batches_a[2]))
    assert c.state() == a.state()
    assert not torch.equal(batches_a[2][0], batches_a[1][0])
