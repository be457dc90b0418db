"""The device's random appearance networks (csrc/appearance.hip) against `appearance_host`, the integer specification: every
comparison is np.array_equal.  The tile is 32 rows x 64 pixels with a 4-pixel halo, one ring per layer: S = 3 is smaller than the halo
(every layer pads on all sides at once), S = 20 lies inside one tile, S = 71 has odd 213-byte rows and partial tiles on both axes,
S = 128 has seams on both axes."""
import random

import numpy as np
import pytest
import torch

from test_appearance_cpu import checkerboard, net_row, param_row, random_field, rows_of, spike_net
from test_quality_cpu import pictures
from test_quality_gpu import _inputs, _sets, normalised, to_u8
from wtpse_hip import ops
from wtpse_hip.input_pipeline import (AmplitudeMix, AppearanceNets, Augment, DeviceInputPipeline, ImageQuality, appearance_grid,
                                      appearance_host, appearance_neutral, draw, draw_appearance, draw_augment, draw_mix,
                                      draw_quality, quality_host)

pytestmark = pytest.mark.gpu

_PICTURES = {}
K3, K1, KMIX0, KMIX1 = (3, 3, 3, 3), (1, 1, 1, 1), (3, 1, 3, 1), (1, 1, 3, 3)


def batch(S, N):
    """The seeded batch of one size, made once and shared (nobody writes to it) -> (host, device)."""
    if (S, N) not in _PICTURES:
        img = pictures(300 + S, N, S)
        img.setflags(write=False)
        _PICTURES[(S, N)] = (img, torch.from_numpy(img.copy()).cuda())
    return _PICTURES[(S, N)]


def check(img, dimg, params, field, spacing, what=""):
    """Device against specification, bit for bit; the input buffer is left as it was.  -> the device's bytes."""
    got = ops.appearance_nets(dimg, params, field, spacing).cpu().numpy()
    want = appearance_host(img, params, field, spacing)
    bad = got != want
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        delta = got.astype(np.int16) - want.astype(np.int16)
        raise AssertionError("%s: %d bytes differ (per sample %s), the first at %s: device %d, specification %d; differences from %d to %d"
                             % (what, int(bad.sum()), bad.reshape(len(bad), -1).sum(1).tolist(), first, got[first], want[first],
                                delta.min(), delta.max()))
    assert np.array_equal(dimg.cpu().numpy(), img), "%s: the input was written" % what
    return got


def test_smaller_than_the_halo():
    img, dimg = batch(3, 2)
    params = rows_of(param_row(net_row(1, K3), net_row(2, K3)), param_row(net_row(3, K3, bias_sigma=200.0), alpha=(0, 0)))
    got = check(img, dimg, params, random_field(1, 2, 3, 4), 4, "S=3")
    assert not np.array_equal(got, img)


def test_inside_one_tile():
    img, dimg = batch(20, 2)
    params = rows_of(param_row(net_row(4, K3), net_row(5, KMIX0), alpha=(30, 200)), param_row(net_row(6, KMIX1), alpha=(0, 0)))
    got = check(img, dimg, params, random_field(2, 2, 20, 8), 8, "S=20")
    assert not np.array_equal(got[0], img[0]) and not np.array_equal(got[1], img[1])


@pytest.mark.parametrize("ks", [(K3, K3), (K1, K1), (KMIX0, KMIX1)], ids=["k3", "k1", "mixed"])
def test_odd_side_mixed_batch(ks):
    """S = 71, N = 3: one sample copied, one with a single net, one blended."""
    img, dimg = batch(71, 3)
    params = rows_of(param_row(selected=False), param_row(net_row(7, ks[0], bias_sigma=100.0), alpha=(20, 0)),
                     param_row(net_row(8, ks[0]), net_row(9, ks[1]), alpha=(100, 0)))
    got = check(img, dimg, params, random_field(3, 3, 71, 32), 32, "S=71 %r" % (ks,))
    assert np.array_equal(got[0], img[0]) and not np.array_equal(got[1], img[1]) and not np.array_equal(got[2], img[2])


def test_seams_between_tiles():
    """S = 128, N = 2: 4 x 2 tiles per sample, all layers 3x3: the full 4-pixel halo."""
    img, dimg = batch(128, 2)
    params = rows_of(param_row(net_row(10, K3, w_scale=2.0), net_row(11, K3), alpha=(0, 0)), param_row(net_row(12, K3, bias_sigma=500.0), alpha=(0, 0)))
    check(img, dimg, params, random_field(4, 2, 128, 32), 32, "S=128")


def test_extremes():
    S = 33
    img = np.concatenate([checkerboard(2, S), batch(S, 2)[0]])
    dimg = torch.from_numpy(img).cuda()
    neutral = appearance_neutral(4, S, 32)[1]
    # the ends of the weight and bias ranges: the layers' clips fire
    for sign_w, sign_b in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        net = net_row(0, const_w=sign_w * 16384, const_b=sign_b * (1 << 19))
        params = rows_of(param_row(net, net, alpha=(0, 256)), param_row(net, alpha=(0, 0)), param_row(net, net_row(1), alpha=(256, 0)),
                         param_row(net, alpha=(256, 0)))
        got = check(img, dimg, params, random_field(5, 4, S, 32), 32, "extremes %d %d" % (sign_w, sign_b))
        assert np.array_equal(got[3], img[3])                       # alpha_0 = 256 without blend: the input
    # g's clip at both ends, and the E_j = 0 branch (alone, and as one of two blended nets)
    zero = net_row(0, const_w=0, const_b=0)
    params = rows_of(param_row(spike_net(1), alpha=(0, 0)), param_row(spike_net(-1), spike_net(1), alpha=(0, 0)),
                     param_row(zero, alpha=(0, 0)), param_row(net_row(2), zero, alpha=(10, 0)))
    got = check(img, dimg, params, random_field(6, 4, S, 32), 32, "gain")
    assert np.array_equal(got[2], img[2])
    # the field: all 0, all 256, a checkerboard of 0 and 256; spacing 4 and spacing > S
    params = rows_of(*[param_row(net_row(20 + i), net_row(30 + i, KMIX0), alpha=(0, 40)) for i in range(4)])
    for spacing in (4, 32, 512):
        G = appearance_grid(S, spacing)
        yy, xx = np.mgrid[0:G, 0:G]
        board = np.broadcast_to(np.where(((yy + xx) & 1) == 1, 256, 0)[None], (4, G, G)).astype(np.int32)
        for name, field in (("0", np.zeros((4, G, G), np.int32)), ("256", np.full((4, G, G), 256, np.int32)), ("board", board),
                            ("random", random_field(7, 4, S, spacing))):
            check(img, dimg, params, field, spacing, "field %s spacing %d" % (name, spacing))


def test_buffers_and_repeatability():
    img, dimg = batch(71, 3)
    params, field = draw_appearance(np.random.RandomState(12), 3, 71, AppearanceNets(p=1.0, spacing=16))
    first = check(img, dimg, params, field, 16, "drawn")
    second = ops.appearance_nets(dimg, params, field, 16)
    assert np.array_equal(second.cpu().numpy(), first) and second.data_ptr() != dimg.data_ptr()
    assert np.array_equal(dimg.cpu().numpy(), img)


def test_refusals_on_the_device():
    dimg = batch(20, 2)[1]
    p, f = appearance_neutral(2, 20, 8)
    with pytest.raises(ValueError):
        ops.appearance_nets(dimg, p[:1], f[:1], 8)
    with pytest.raises(ValueError):
        ops.appearance_nets(dimg, p, f, 16)                          # the field of another spacing
    bad = p.copy()
    bad[0, 1] = 257
    with pytest.raises(ValueError):
        ops.appearance_nets(dimg, bad, f, 8)
    with pytest.raises(ValueError):
        ops.appearance_nets(dimg.to(torch.float32), p, f, 8)
    with pytest.raises(ValueError):
        ops.appearance_nets(torch.zeros((2, 20, 24, 3), dtype=torch.uint8, device="cuda"), p, f, 8)


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def test_pipeline_stage_order():
    """augment, mix, appearance, quality: the batch with all four equals the batch of the first two pushed through the two
    specifications in that order; appearance_draws=None gives what the pipeline gave without the argument."""
    S, N = 32, 4
    imgs, masks = _inputs(S, N)
    py_rng, np_rng = random.Random(5), np.random.RandomState(5)
    draws = [draw(py_rng, S) for _ in range(N)]
    aug_draws = [draw_augment(py_rng, np_rng, S, Augment()) for _ in range(N)]
    mix = AmplitudeMix(p=1.0)
    partner, lam = draw_mix(np_rng, 2, 2, mix)
    mix_draws = (partner, lam, mix.band(S))
    quality = draw_quality(np_rng, N, ImageQuality(p_focus=1, p_contrast=1, p_brightness=1, p_noise=1))
    nets = AppearanceNets(p=1.0, spacing=8)
    a_params, a_field = draw_appearance(np_rng, N, S, nets)
    a_params[1] = appearance_neutral(1, S, 8)[0][0]
    pipe = lambda: DeviceInputPipeline(S, "cuda", noise_seed=9)
    two = pipe()(imgs, masks, draws, aug_draws, mix_draws=mix_draws)
    three = pipe()(imgs, masks, draws, aug_draws, mix_draws=mix_draws, quality_draws=quality)
    three_none = pipe()(imgs, masks, draws, aug_draws, mix_draws=mix_draws, quality_draws=quality, appearance_draws=None)
    three_neutral = pipe()(imgs, masks, draws, aug_draws, mix_draws=mix_draws, quality_draws=quality,
                           appearance_draws=appearance_neutral(N, S, 8) + (8,))
    assert all(torch.equal(a, b) for a, b in zip(three, three_none)) and all(torch.equal(a, b) for a, b in zip(three, three_neutral))
    four = pipe()(imgs, masks, draws, aug_draws, mix_draws=mix_draws, quality_draws=quality, appearance_draws=(a_params, a_field, 8))
    assert torch.equal(two[1], four[1]) and torch.equal(two[2], four[2])             # the masks are not touched
    want = quality_host(appearance_host(to_u8(two[0]), a_params, a_field, 8), quality, 9, 0)
    assert np.array_equal(four[0].cpu().numpy(), normalised(want))
    assert not torch.equal(three[0], four[0])
    # the stage alone, behind the crop
    alone = pipe()(imgs, masks, draws, appearance_draws=(a_params, a_field, 8))
    plain = pipe()(imgs, masks, draws)
    assert np.array_equal(alone[0].cpu().numpy(), normalised(appearance_host(to_u8(plain[0]), a_params, a_field, 8)))
    assert torch.equal(alone[0][1], plain[0][1]) and not torch.equal(alone[0][0], plain[0][0])


# ---------------------------------------------------------------------------------------------------------------- the feed
def test_feed_resumes_bitwise(tmp_path):
    """FundusBatches(appearance=AppearanceNets()) on the synthetic PNG tree: two batches, the state saved, one batch more; a fresh feed
    loaded from that state reproduces the third batch bit for bit — and the state has no entry of the stage's."""
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)
    nets = AppearanceNets(p=0.7, spacing=16)

    def feed():
        f = FundusBatches(sets, 6, "cuda", size=64, appearance=nets)
        f.set_seed(3)
        return f

    a, py_a, np_a = feed(), random.Random(3), np.random.RandomState(3)
    first, second = a(py_a, np_a), a(py_a, np_a)
    saved = (a.state(), py_a.getstate(), np_a.get_state())
    assert set(saved[0]) == {"order"}
    third = a(py_a, np_a)
    b, py_b, np_b = feed(), random.Random(0), np.random.RandomState(0)
    b.load_state(saved[0])
    py_b.setstate(saved[1])
    np_b.set_state(saved[2])
    again = b(py_b, np_b)
    assert all(torch.equal(x, y) for x, y in zip(again, third))
    assert b.state() == a.state()
    # the stage did something, to the pictures alone
    d = FundusBatches(sets, 6, "cuda", size=64)
    plain = d(random.Random(3), np.random.RandomState(3))
    assert torch.equal(plain[1], first[1]) and torch.equal(plain[2], first[2]) and not torch.equal(plain[0], first[0])
    assert not torch.equal(first[0], second[0])
