"""The device's amplitude-mixing stage (csrc/spectrum.hip) against `amplitude_mix_host`, the float64 specification.

The bar for the unrounded fp32 output: the device's largest deviation from the specification is at most 4 times that of the float32
`torch.fft` restatement on the CPU (test_amplitude_mix_cpu.mix_float32) for the same inputs — the factor covers a different but
equally valid summation order.  The uint8 output equals the specification's except where the specification's unrounded value lies
within that bar of a half-integer; there it may differ by one level, and such pixels may be at most 1 % of a case.  Rows without a
partner, with lam = 0 and with themselves as partner come back bit for bit.  Every case prints its two deviations before it asserts
(profiles/amplitude_mix.md records them)."""
import random

import numpy as np
import pytest
import torch

from test_amplitude_mix_cpu import mix_float32, noisy_images
from wtpse_hip import ops
from wtpse_hip.input_pipeline import AmplitudeMix, Augment, amplitude_mix_host, draw_mix

pytestmark = pytest.mark.gpu

PARTNER5 = [3, -1, 0, 4, 1]
_IMAGES = {}


def images(S, N):
    """The seeded noisy batch of one size, made once and shared (nobody writes to it)."""
    if (S, N) not in _IMAGES:
        img = noisy_images(100 + S, N, S)
        img.setflags(write=False)
        _IMAGES[(S, N)] = (img, torch.from_numpy(img.copy()).cuda())
    return _IMAGES[(S, N)]


def device_mix(dimg, partner, lam, b):
    u8, f32 = ops.amplitude_mix(dimg, np.asarray(partner), np.asarray(lam, np.float64), b, want_float=True)
    return u8.cpu().numpy(), f32.cpu().numpy()


def check_against_spec(img, partner, lam, b, got_u8, got_f32, what):
    """-> (device deviation, restatement's deviation) after asserting the fp32 bar and the uint8 rule."""
    lam = np.asarray(lam, np.float64)
    spec = amplitude_mix_host(img, partner, lam, b, as_float=True)    # lam in float64; device and restatement both take it in fp32
    ref_dev = float(np.abs(mix_float32(img, partner, lam, b).astype(np.float64) - spec).max())
    dev = float(np.abs(got_f32.astype(np.float64) - spec).max())
    print("%s: device deviation %.3e, float32 torch.fft restatement %.3e grey levels" % (what, dev, ref_dev))
    tol = 4.0 * ref_dev
    assert dev <= tol, "%s: device %.3e against 4 x %.3e" % (what, dev, ref_dev)
    clipped = np.clip(spec, 0.0, 255.0)
    want_u8 = np.rint(clipped).astype(np.uint8)
    near_tie = np.abs(clipped - np.floor(clipped) - 0.5) <= tol
    assert near_tie.mean() <= 0.01, "%s: %.3f %% of the pixels lie within %.1e of a tie" % (what, 100 * near_tie.mean(), tol)
    diff = np.abs(got_u8.astype(np.int16) - want_u8.astype(np.int16))
    assert not np.any(diff[~near_tie]), "%s: %d uint8 pixels differ away from a tie" % (what, int((diff[~near_tie] != 0).sum()))
    assert diff.max() <= 1, "%s: a uint8 pixel differs by %d" % (what, int(diff.max()))
    return dev, ref_dev


def bands(S):
    return [0, 1, S // 10, S // 2 - 1, S // 2]


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("S", [32, 64, 256])
def test_output_against_spec(S, which):
    """32 runs the closing radix-2 pass, 64 and 256 the pure radix-4 path; b = 0 is the mean alone, b = S/2 touches the Nyquist
    lines; N = 5 is odd (the last workgroup of a launch is ragged) and row 1 is copied through."""
    b = bands(S)[which]
    img, dimg = images(S, 5)
    for lam in (0.0, 0.3, 0.8, 1.0):
        u8, f32 = device_mix(dimg, PARTNER5, [lam] * 5, b)
        check_against_spec(img, PARTNER5, [lam] * 5, b, u8, f32, "S=%d b=%d lam=%g" % (S, b, lam))
        assert np.array_equal(u8[1], img[1]) and np.array_equal(f32[1], img[1].astype(np.float32))
        if lam == 0.0:
            assert np.array_equal(u8, img)
        else:
            assert not np.array_equal(u8[0], img[0])


@pytest.mark.parametrize("S,b", [(128, 12), (128, 64), (512, 256)])
def test_output_against_spec_other_sizes(S, b):
    """128 (three radix-4 passes and the radix-2 pass) and 512 (four and one: the largest transform, two per workgroup), N = 2."""
    img, dimg = images(S, 2)
    u8, f32 = device_mix(dimg, [1, 0], [0.8, 0.3], b)
    check_against_spec(img, [1, 0], [0.8, 0.3], b, u8, f32, "S=%d b=%d N=2" % (S, b))


@pytest.mark.parametrize("S", [32, 256, 512])
def test_exact_identities(S):
    """No partner, lam = 0 and partner = self return the input bit for bit — in the same launch as a row that is really mixed."""
    N = 5 if S < 512 else 4
    img, dimg = images(S, N)
    partner = [0, -1, 3, 2, 0][:N]            # row 0: itself; row 1: none; row 2: lam = 0; row 3 (and 4): mixed
    lam = [0.9, 0.5, 0.0, 0.7, 1.0][:N]
    for b in (S // 10, S // 2):
        u8, f32 = device_mix(dimg, partner, lam, b)
        for n in (0, 1, 2):
            assert np.array_equal(u8[n], img[n]), "row %d changed at b = %d" % (n, b)
            assert np.array_equal(f32[n], img[n].astype(np.float32))
        assert not np.array_equal(u8[3], img[3])


def test_two_calls_are_bitwise_equal():
    img, dimg = images(256, 5)
    lam = [0.3, 0.0, 0.8, 1.0, 0.55]
    a = device_mix(dimg, PARTNER5, lam, 25)
    other = device_mix(dimg, [1, 2, 3, 4, 0], lam, 128)        # the workspace is reused in between
    b = device_mix(dimg, PARTNER5, lam, 25)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], other[0])


def test_black_own_image():
    """|F| = 0 everywhere: the phase is taken as 1, the result is lam |G| on zero phase."""
    img = np.array(images(64, 5)[0][:2])
    img[0] = 0
    u8, f32 = device_mix(torch.from_numpy(img).cuda(), [1, -1], [0.6, 0.0], 6)
    assert np.all(np.isfinite(f32))
    check_against_spec(img, [1, -1], [0.6, 0.0], 6, u8, f32, "black own image")
    assert u8[0].max() > 0


def test_refusals_on_the_device():
    dimg = images(64, 5)[1]
    with pytest.raises(ValueError):
        ops.amplitude_mix(torch.zeros((2, 48, 48, 3), dtype=torch.uint8, device="cuda"), [1, 0], [0.5, 0.5], 4)
    with pytest.raises(ValueError):
        ops.amplitude_mix(dimg, [5, 0, 0, 0, 0], [0.5] * 5, 4)
    with pytest.raises(ValueError):
        ops.amplitude_mix(dimg, PARTNER5, [0.5] * 5, 33)


# ---------------------------------------------------------------------------------------------------------------- the feed
def _sets(tmp_path):
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    return [FundusTree(root, "train", (i,), size=64) for i in (1, 2, 3)]


def test_feed_with_the_stage_on(tmp_path):
    """FundusBatches on the synthetic PNG tree (three domains, two samples each, S = 64), style = AmplitudeMix(p = 1) against style =
    None from the same seeds: the masks are bitwise the same, and the image is the unmixed batch's uint8 — recovered exactly as
    rint((image + 1) * 127.5) — pushed through amplitude_mix_host with the same draws and normalised, ties as above.  Only the uint8
    output is the feed's own (a feed hands out no unrounded values): the fp32 values the bar is measured with come from a second,
    stand-alone call of the stage on the recovered uint8 batch with the same draws — the stage is deterministic, so that call's
    uint8 output is asserted equal to the feed's."""
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)
    mix = AmplitudeMix(p=1.0)
    py_p, np_p = random.Random(3), np.random.RandomState(3)
    plain = FundusBatches(sets, 6, "cuda", size=64)(py_p, np_p)
    py_s, np_s = random.Random(3), np.random.RandomState(3)
    styled = FundusBatches(sets, 6, "cuda", size=64, style=mix)(py_s, np_s)
    assert torch.equal(plain[1], styled[1]) and torch.equal(plain[2], styled[2])
    # the stage's draws come after all the others: the plain feed's generator stands where they start
    partner, lam = draw_mix(np_p, 3, 2, mix)
    assert py_p.getstate() == py_s.getstate()
    assert all(np.array_equal(x, y) for x, y in zip(np_p.get_state()[1:3], np_s.get_state()[1:3]))
    assert (partner >= 0).all()

    def to_u8(image):
        v = (image.cpu().numpy().astype(np.float64) + 1.0) * 127.5
        u = np.rint(v)
        assert np.abs(v - u).max() < 1e-4
        return np.ascontiguousarray(u.astype(np.uint8).transpose(0, 2, 3, 1))

    src, got = to_u8(plain[0]), to_u8(styled[0])
    renorm = got.astype(np.float32)
    renorm /= 127.5
    renorm -= 1.0
    assert np.array_equal(renorm.transpose(0, 3, 1, 2), styled[0].cpu().numpy())          # normalised as every batch is
    b = mix.band(64)
    assert b == 6
    again_u8, f32 = device_mix(torch.from_numpy(src).cuda(), partner, lam, b)
    assert np.array_equal(again_u8, got)
    check_against_spec(src, partner, lam, b, got, f32, "feed batch")
    assert not np.array_equal(src, got)


def test_feed_resumes_bitwise(tmp_path):
    """A feed with augmentations AND the stage, interrupted after two batches, saved and rebuilt, hands out the third batch of the
    uninterrupted feed: the stage adds no state beyond the generators the run checkpoints."""
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)

    def feed():
        f = FundusBatches(sets, 6, "cuda", size=64, augment=Augment(), style=AmplitudeMix(p=0.6))
        f.set_seed(3)
        return f

    a, py_a, np_a = feed(), random.Random(3), np.random.RandomState(3)
    batches_a = [a(py_a, np_a) for _ in range(3)]
    b, py_b, np_b = feed(), random.Random(3), np.random.RandomState(3)
    for k in range(2):
        assert all(torch.equal(x, y) for x, y in zip(b(py_b, np_b), batches_a[k]))
    saved = (b.state(), py_b.getstate(), np_b.get_state())
    c, py_c, np_c = feed(), random.Random(0), np.random.RandomState(0)
    c.load_state(saved[0])
    py_c.setstate(saved[1])
    np_c.set_state(saved[2])
    third = c(py_c, np_c)
    assert all(torch.equal(x, y) for x, y in zip(third, batches_a[2]))
    assert c.state() == a.state()
    # the stage did something: the same feed without it hands out other pictures, but the same masks
    d = FundusBatches(sets, 6, "cuda", size=64, augment=Augment())
    d.set_seed(3)
    first = d(random.Random(3), np.random.RandomState(3))
    assert torch.equal(first[1], batches_a[0][1]) and not torch.equal(first[0], batches_a[0][0])


def test_run_with_the_stage_trains_and_resumes(tmp_path):
    """TrainRun on a feed with style = AmplitudeMix(): two epochs against one epoch, save, load into fresh networks and a new feed, one
    more epoch — the same batches and the same bits at the end."""
    from test_trainer_gpu import B, RATES, _assert_same, _setup, _snapshot
    from wtpse_hip.trainer import FundusBatches, TrainRun
    sets = _sets(tmp_path)
    seen = {"a": [], "b": []}

    def feed(dev, key):
        class Recorded(FundusBatches):
            def __call__(self, py_rng, np_rng):
                batch = super().__call__(py_rng, np_rng)
                seen[key].append([t.clone() for t in batch])
                return batch
        return Recorded(sets, B, dev, size=64, style=AmplitudeMix())

    kw = dict(iter_per_epoch=2, max_epoch=2, lr=RATES, graph="plan", seed=3)
    dev, hp, nets = _setup()
    a = TrainRun(*nets, hp, feed(dev, "a"), **kw)
    a.train_epoch()
    ea = a.train_epoch()
    sa = _snapshot(a.train_step, nets)

    dev, hp, nets1 = _setup()
    b1 = TrainRun(*nets1, hp, feed(dev, "b"), **kw)
    b1.train_epoch()
    path = str(tmp_path / "run.pth.tar")
    b1.save(path)
    del b1
    dev, hp, nets2 = _setup(seed=5, noise=None)
    b2 = TrainRun.load(path, *nets2, hp, feed(dev, "b"))
    eb = b2.train_epoch()
    sb = _snapshot(b2.train_step, nets2)
    assert len(seen["a"]) == len(seen["b"]) == 4
    for ba, bb in zip(seen["a"], seen["b"]):
        assert all(torch.equal(x, y) for x, y in zip(ba, bb))
    _assert_same(sa, sb)
    assert ea["sums"] == eb["sums"] and all(v == v for v in ea["sums"].values())
