"""Random appearance networks, host side: `appearance_host` (the integer specification of csrc/appearance.hip) against an independent
restatement of its convolutions through torch's conv2d in float64 (exact: every sum is below 2^53), its identities, the energy
matching, the axis table, the validator's ranges, `draw_appearance`'s stream and the feed's draws.  `net_row`, `param_row` and
`rows_of` are shared with tests/test_appearance_gpu.py.  Every comparison with the specification is np.array_equal."""
import random

import numpy as np
import pytest
import torch

from test_quality_cpu import RecordingPipe, _sets, pictures
from wtpse_hip.input_pipeline import (APPEARANCE_BIAS_MAX, APPEARANCE_BLEND, APPEARANCE_CHANNELS, APPEARANCE_CL, APPEARANCE_COLS,
                                      APPEARANCE_NET_COLS, APPEARANCE_SELECTED, APPEARANCE_W_MAX, AppearanceNets, ImageQuality,
                                      appearance_axis_table, appearance_field_host, appearance_gain, appearance_grid,
                                      appearance_host, appearance_is_neutral, appearance_net_of, appearance_net_row,
                                      appearance_neutral, check_appearance_params, draw_appearance, draw_quality)

CL = APPEARANCE_CL


def net_row(seed, k=(3, 3, 3, 3), w_scale=1.0, bias_sigma=32.0, const_w=None, const_b=None):
    """One net's 193 columns: seeded normal weights of standard deviation w_scale / sqrt(fan_in) in Q12 and biases of bias_sigma grey
    levels in Q8 — or every weight const_w and every bias const_b.  The dead taps of a 1x1 layer are filled like the others."""
    rng = np.random.RandomState(seed)
    W, B = [], []
    for l in range(4):
        ci, co = APPEARANCE_CHANNELS[l], APPEARANCE_CHANNELS[l + 1]
        w = np.rint(rng.normal(0, 1, (co, ci, 3, 3)) * w_scale / np.sqrt(ci * k[l] ** 2) * 4096.0)
        b = np.rint(rng.normal(0, 1, co) * bias_sigma * 256.0)
        W.append(np.full_like(w, const_w) if const_w is not None else np.clip(w, -APPEARANCE_W_MAX, APPEARANCE_W_MAX))
        B.append(np.full_like(b, const_b) if const_b is not None else np.clip(b, -APPEARANCE_BIAS_MAX, APPEARANCE_BIAS_MAX))
    return appearance_net_row(k, W, B)


def param_row(net0=None, net1=None, alpha=(64, 64), blend=None, selected=True):
    """A parameter row: two nets -> blended unless blend=False."""
    row = appearance_neutral(1, 8, 4)[0][0].astype(np.int64)
    if not selected:
        return row
    blend = (net1 is not None) if blend is None else blend
    row[0] = APPEARANCE_SELECTED | (APPEARANCE_BLEND if blend else 0)
    row[1:3] = alpha
    if net0 is not None:
        row[3:3 + APPEARANCE_NET_COLS] = net0
    if net1 is not None:
        row[3 + APPEARANCE_NET_COLS:] = net1
    return row


def rows_of(*rows):
    return np.stack(rows).astype(np.int32)


def random_field(seed, N, S, spacing):
    G = appearance_grid(S, spacing)
    return np.random.RandomState(seed).randint(0, 257, (N, G, G)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the convolution
def layer_by_conv2d(h, W, bias, k, leak):
    """One layer a second way: the sums through conv2d(padding=1) in float64 — exact on these integers — then the integer shift,
    bias, leak and clip.  h [ci,S,S] int64 -> [co,S,S] int64."""
    w = W.astype(np.float64)
    if k == 1:
        centre = np.zeros_like(w)
        centre[:, :, 1, 1] = w[:, :, 1, 1]
        w = centre
    acc = torch.nn.functional.conv2d(torch.from_numpy(h.astype(np.float64))[None], torch.from_numpy(w), padding=1)[0].numpy()
    assert np.abs(acc).max() < 2.0 ** 53
    acc = acc.astype(np.int64)
    assert np.array_equal(acc.astype(np.float64), acc)
    v = ((acc + 2048) >> 12) + bias[:, None, None]
    if leak:
        v = np.where(v < 0, (3 * v + 128) >> 8, v)
    return np.clip(v, -CL, CL)


@pytest.mark.parametrize("k", [(3, 3, 3, 3), (1, 1, 1, 1), (3, 1, 1, 3), (1, 3, 3, 1)])
def test_layers_equal_conv2d(k):
    """Tap order, zero padding at EVERY layer and the 1x1 layers: the restatement is chained on its own outputs, so a layer that
    padded with anything but 0 (the bias makes the out-of-picture value non-zero) would show in the next."""
    S = 13
    img = pictures(5, 2, S)
    nets = [net_row(10 + i, k, w_scale=3.0, bias_sigma=300.0) for i in range(4)]
    params = rows_of(param_row(nets[0], nets[1]), param_row(nets[2], nets[3]))
    detail = {}
    appearance_host(img, params, random_field(1, 2, S, 4), 4, detail)
    for n in range(2):
        h0 = detail[n]["c0"].transpose(2, 0, 1)
        assert np.array_equal(h0, (img[n].astype(np.int64).transpose(2, 0, 1) << 8) - detail[n]["m8"])
        for j in range(2):
            kk, W, B = appearance_net_of(params[n, 3 + j * APPEARANCE_NET_COLS:3 + (j + 1) * APPEARANCE_NET_COLS])
            h = h0
            for l in range(4):
                h = layer_by_conv2d(h, W[l], B[l], int(kk[l]), l < 3)
                assert np.array_equal(h, detail[n]["nets"][j]["layers"][l]), (n, j, l)
            assert np.abs(h).max() > 0


def test_border_is_zero_padded_not_bias_padded():
    """All weights 0 but the last layer's: layer 2's output is its bias everywhere inside the picture; a 3x3 last layer must see 0,
    not that bias, beyond the border."""
    S = 6
    W = [np.zeros((APPEARANCE_CHANNELS[l + 1], APPEARANCE_CHANNELS[l], 3, 3), np.int64) for l in range(4)]
    B = [np.zeros(APPEARANCE_CHANNELS[l + 1], np.int64) for l in range(4)]
    B[2][:] = 10 * 256
    W[3][:] = 4096
    net = appearance_net_row((1, 1, 1, 3), W, B)
    detail = {}
    appearance_host(pictures(1, 1, S), rows_of(param_row(net, alpha=(0, 0))), appearance_neutral(1, S, 4)[1], 4, detail)
    y = detail[0]["nets"][0]["layers"][3]
    assert y[0, 2, 2] == 18 * 2560 and y[0, 0, 0] == 8 * 2560 and y[0, 0, 2] == 12 * 2560 and y[2, S - 1, S - 1] == 8 * 2560


# ---------------------------------------------------------------------------------------------------------------- identities
def test_identities():
    S, sp = 21, 8
    img = pictures(7, 3, S)
    n0, n1 = net_row(1), net_row(2, (1, 3, 1, 3))
    neutral_p, neutral_f = appearance_neutral(3, S, sp)
    assert appearance_is_neutral(neutral_p).all()
    assert np.array_equal(appearance_host(img, neutral_p, neutral_f, sp), img)
    # alpha_0 = 256 without blend returns the input, whatever the net
    p = rows_of(*[param_row(n0, alpha=(256, 0))] * 3)
    assert not appearance_is_neutral(p).any()
    assert np.array_equal(appearance_host(img, p, neutral_f, sp), img)
    # blend off = a field of 256 everywhere
    single = appearance_host(img, rows_of(*[param_row(n0, n1, blend=False)] * 3), random_field(3, 3, S, sp), sp)
    both256 = appearance_host(img, rows_of(*[param_row(n0, n1)] * 3), neutral_f, sp)
    assert np.array_equal(single, both256) and not np.array_equal(single, img)
    # a field of 0 everywhere = net 1 alone
    both0 = appearance_host(img, rows_of(*[param_row(n0, n1)] * 3), np.zeros_like(neutral_f), sp)
    alone1 = appearance_host(img, rows_of(*[param_row(n1, alpha=(64, 64))] * 3), neutral_f, sp)
    assert np.array_equal(both0, alone1) and not np.array_equal(both0, both256)
    # a row that is not selected is copied beside rows that are not
    mixed = appearance_host(img, rows_of(param_row(n0), param_row(selected=False), param_row(n0, n1)), random_field(4, 3, S, sp), sp)
    assert np.array_equal(mixed[1], img[1]) and not np.array_equal(mixed[0], img[0]) and not np.array_equal(mixed[2], img[2])


def test_typical_draws_stay_unsaturated():
    S = 64
    img = pictures(11, 4, S)
    params, field = draw_appearance(np.random.RandomState(4), 4, S, AppearanceNets(p=1.0))
    out = appearance_host(img, params, field, 32)
    sat = np.mean((out == 0) | (out == 255))
    assert sat < 0.25 and out.std() > 0.25 * img.std() and not np.array_equal(out, img)


# ---------------------------------------------------------------------------------------------------------------- energy
def test_energy_is_matched():
    """‖q(g_j)‖ against sqrt(E_in), q(v) = (v + 8) >> 4 and ‖.‖ the root of the sum of squares over the M = 3 S S values.  With
    r = sqrt(E_in / E_j): R_j / 4096 = r + d, |d| <= 2^-13 (R_j is rounded to 2^-12); g = (R_j / 4096) z + e, |e| <= 1/2 (g is rounded
    to an integer); q(v) = v / 16 + h, |h| <= 1/2.  So q(g) = (R_j / 4096) (q(z) - h') + e / 16 + h, and by the triangle inequality
        | ‖q(g)‖ - sqrt(E_in) | <= 2^-13 sqrt(E_j) + sqrt(M) (R_j / 8192 + 1/32 + 1/2)
    as long as neither the cap of R_j nor the clip of g fired (asserted)."""
    S = 40
    img = pictures(21, 4, S)
    params, field = draw_appearance(np.random.RandomState(8), 4, S, AppearanceNets(p=1.0, spacing=16))
    detail = {}
    appearance_host(img, params, field, 16, detail)
    M = 3 * S * S
    for n in range(4):
        E_in = detail[n]["E_in"]
        assert E_in == int((((detail[n]["c0"] + 8) >> 4) ** 2).sum())
        for net in detail[n]["nets"]:
            assert net["E"] > 0 and net["R"] < 1 << 20 and np.abs(net["g"]).max() < CL
            assert net["R"] == appearance_gain(E_in, net["E"])
            got = np.sqrt(float((((net["g"] + 8) >> 4) ** 2).sum()))
            bound = 2.0 ** -13 * np.sqrt(net["E"]) + np.sqrt(M) * (net["R"] / 8192.0 + 1.0 / 32 + 0.5)
            assert abs(got - np.sqrt(E_in)) <= bound * (1 + 1e-12), (n, got, np.sqrt(E_in), bound)
            assert bound < 0.01 * np.sqrt(E_in)                      # the bound says something: within 1 % here


def test_zero_energy_branch():
    """All weights and biases 0, alpha = 0: z = 0, E_j = 0 -> R = 4096 and z := c0: the input comes back."""
    S = 9
    img = pictures(2, 2, S)
    zero = net_row(0, const_w=0, const_b=0)
    detail = {}
    out = appearance_host(img, rows_of(param_row(zero, alpha=(0, 0)), param_row(zero, zero, alpha=(0, 0))), random_field(5, 2, S, 4), 4, detail)
    assert np.array_equal(out, img)
    assert all(net["E"] == 0 and net["R"] == 4096 for n in range(2) for net in detail[n]["nets"])
    assert appearance_gain(0, 5) == 0 and appearance_gain(1 << 50, 1) == 1 << 20 and appearance_gain(9, 4) == 6144


# ---------------------------------------------------------------------------------------------------------------- the axis table
@pytest.mark.parametrize("S", [1, 5, 33, 256, 512])
@pytest.mark.parametrize("spacing", [4, 32, 512])
def test_axis_table(S, spacing):
    tab = appearance_axis_table(S, spacing)
    G = appearance_grid(S, spacing)
    assert tab.shape == (S, 5) and G == -(-S // spacing) + 3
    assert tab[:, 1:].min() >= 0 and np.all(tab[:, 1:].sum(1) == 4096)
    assert tab[:, 0].min() == 0 and tab[:, 0].max() + 3 <= G - 1
    # close to the float weights, and exactly the B-spline's values at a knot
    t = (np.arange(S) % spacing) / float(spacing)
    assert np.abs(tab[:, 4] - 4096.0 * t ** 3 / 6.0).max() <= 2.0
    assert tuple(tab[0, 1:]) == (683, 2730, 683, 0)
    for value in (0, 256):
        b = appearance_field_host(np.full((1, G, G), value, np.int64), S, spacing)
        assert b.shape == (1, S, S) and np.all(b == value)
    b = appearance_field_host(np.random.RandomState(S).randint(0, 257, (2, G, G)), S, spacing)
    assert b.min() >= 0 and b.max() <= 256


# ---------------------------------------------------------------------------------------------------------------- the validator
def test_ranges_are_refused_one_past_their_end():
    S, sp = 8, 4
    good_p, good_f = appearance_neutral(2, S, sp)
    good_p = rows_of(param_row(net_row(1), net_row(2)), param_row(net_row(3)))
    check_appearance_params(good_p, good_f, 2, S, sp)
    w0, b0 = 3 + 4, 3 + 184

    def bad(col, value, field=None):
        p = good_p.copy()
        if col is not None:
            p[1, col] = value
        with pytest.raises(ValueError):
            check_appearance_params(p, good_f if field is None else field, 2, S, sp)

    def good(col, value):
        p = good_p.copy()
        p[1, col] = value
        check_appearance_params(p, good_f, 2, S, sp)

    for col, lo, hi in ((0, 0, 3), (1, 0, 256), (2, 0, 256), (w0, -16384, 16384), (w0 + 179, -16384, 16384),
                        (w0 + APPEARANCE_NET_COLS, -16384, 16384), (b0, -(1 << 19), 1 << 19), (b0 + 8, -(1 << 19), 1 << 19),
                        (b0 + 8 + APPEARANCE_NET_COLS, -(1 << 19), 1 << 19)):
        good(col, lo), good(col, hi)
        bad(col, lo - 1), bad(col, hi + 1)
    for col in (3, 6, 3 + APPEARANCE_NET_COLS):
        good(col, 1), good(col, 3)
        for v in (0, 2, 4):
            bad(col, v)
    for v in (-1, 257):
        f = good_f.copy()
        f[0, 1, 2] = v
        bad(None, 0, f)
    with pytest.raises(ValueError):
        check_appearance_params(good_p[:, :-1], good_f, 2, S, sp)
    with pytest.raises(ValueError):
        check_appearance_params(good_p, good_f[:, :-1], 2, S, sp)
    with pytest.raises(ValueError):
        check_appearance_params(good_p.astype(np.float32), good_f, 2, S, sp)
    for size, spacing in ((0, 4), (513, 4), (8, 3), (8, 513)):
        with pytest.raises(ValueError):
            appearance_neutral(1, size, spacing)
    appearance_neutral(1, 512, 512), appearance_neutral(1, 1, 4)
    with pytest.raises(ValueError):
        appearance_host(np.zeros((1, 8, 9, 3), np.uint8), good_p[:1], good_f[:1], sp)


def test_stage_parameters_are_checked():
    AppearanceNets(p=0, blend=False, spacing=4, bias_sigma=0, p_k3=0), AppearanceNets(p=1, spacing=512, bias_sigma=2048, p_k3=1)
    for kw in (dict(p=-0.1), dict(p=1.1), dict(p_k3=-0.1), dict(p_k3=1.5), dict(spacing=3), dict(spacing=513), dict(spacing=7.5),
               dict(bias_sigma=-1), dict(bias_sigma=2049)):
        with pytest.raises(ValueError):
            AppearanceNets(**kw)


def test_extreme_parameters_hit_the_clips():
    """|W| = 16384 everywhere, |bias| = 2^19, bytes 0 / 255 in a checkerboard: over the four sign combinations both ends of the layers' clip
    and of g's are reached, and the largest sum the specification forms — 27 products of 2^14 x CL plus the rounding — is nowhere near the end of int64 (it is 2^37.8)."""
    S = 12
    img = checkerboard(2, S)
    assert 27 * 16384 * CL + 2048 < 2 ** 38 and (1 << 20) * CL + 2048 < 2 ** 40
    lo, hi = [], []
    for sign_w, sign_b in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        net = net_row(0, const_w=sign_w * 16384, const_b=sign_b * (1 << 19))
        detail = {}
        out = appearance_host(img, rows_of(param_row(net, net, alpha=(0, 256)), param_row(net, alpha=(0, 0))),
                              random_field(2, 2, S, 4), 4, detail)
        assert out.dtype == np.uint8
        for n in range(2):
            for entry in detail[n]["nets"]:
                assert all(np.abs(h).max() <= CL for h in entry["layers"]) and np.abs(entry["g"]).max() <= CL
                lo.append(min(h.min() for h in entry["layers"])), hi.append(max(h.max() for h in entry["layers"]))
    assert min(lo) == -CL and max(hi) == CL


def checkerboard(N, S):
    yy, xx = np.mgrid[0:S, 0:S]
    board = np.where(((yy + xx) & 1) == 1, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(board[None, :, :, None], (N, S, S, 3)))


def spike_net(sign):
    """A net whose output is large at the picture's four corners and nearly 0 elsewhere, through the zero padding alone: layer 0 is
    the constant 1000, a 3x3 layer 1 with every tap -0.5 and bias 6000 gives 2000 at the corners (4 taps inside), 0 on the edges (6)
    and -3000 -> -35 behind the leak inside (9); two 1x1 layers of weight 4 over two channels multiply by 8 each: 128000 x sign at
    the corners, -24 x sign inside.  Energy matching then scales the corners beyond g's clip."""
    W = [np.zeros((APPEARANCE_CHANNELS[l + 1], APPEARANCE_CHANNELS[l], 3, 3), np.int64) for l in range(4)]
    B = [np.zeros(APPEARANCE_CHANNELS[l + 1], np.int64) for l in range(4)]
    B[0][:], W[1][:], B[1][:], W[2][:], W[3][:] = 1000, -2048, 6000, 16384, sign * 16384
    return appearance_net_row((1, 3, 1, 1), W, B)


def test_gain_clip_fires():
    S = 33
    detail = {}
    appearance_host(checkerboard(2, S), rows_of(param_row(spike_net(1), alpha=(0, 0)), param_row(spike_net(-1), alpha=(0, 0))),
                    appearance_neutral(2, S, 32)[1], 32, detail)
    y = detail[0]["nets"][0]["layers"][3]
    assert y[0, 0, 0] == 128000 and y[1, 0, 5] == 0 and y[2, 7, 7] == -24
    assert detail[0]["nets"][0]["g"].max() == CL and detail[1]["nets"][0]["g"].min() == -CL
    assert 4096 < detail[0]["nets"][0]["R"] < 1 << 20


def test_energies_stay_below_2_53():
    """S = 512 with every value at CL: the largest energy the stage can form converts to float64 exactly."""
    E = 3 * 512 * 512 * ((CL + 8) >> 4) ** 2
    assert E < 2 ** 53 and int(np.float64(E)) == E and int(np.float64(E - 1)) == E - 1
    assert appearance_gain(E, E) == 4096 and appearance_gain(E, 1) == 1 << 20


# ---------------------------------------------------------------------------------------------------------------- the draws
def test_draw_appearance_is_deterministic_and_legal():
    nets = AppearanceNets(p=0.7, spacing=8, bias_sigma=2048.0)
    a = draw_appearance(np.random.RandomState(5), 12, 40, nets)
    b = draw_appearance(np.random.RandomState(5), 12, 40, nets)
    c = draw_appearance(np.random.RandomState(6), 12, 40, nets)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    assert a[0].shape == (12, APPEARANCE_COLS) and a[0].dtype == np.int32 and a[1].shape == (12, 8, 8) and a[1].dtype == np.int32
    check_appearance_params(a[0], a[1], 12, 40, 8)
    sel = ~appearance_is_neutral(a[0])
    assert 0 < sel.sum() < 12 and np.all(a[0][sel, 0] == 3) and np.all(a[1][~sel] == 256)
    # a coin that does not fire draws nothing else; p = 0 draws one coin per sample
    rng, ref = np.random.RandomState(1), np.random.RandomState(1)
    p, f = draw_appearance(rng, 5, 16, AppearanceNets(p=0.0))
    ref.random_sample(5)
    assert appearance_is_neutral(p).all() and rng.random_sample() == ref.random_sample()
    # blend off: one net, no field
    p, f = draw_appearance(np.random.RandomState(2), 6, 16, AppearanceNets(p=1.0, blend=False))
    assert np.all(p[:, 0] == 1) and np.all(f == 256)
    # weights follow 1 / fan_in: a 3x3 first layer has standard deviation 4096 / sqrt(27) in Q12
    p, _ = draw_appearance(np.random.RandomState(3), 400, 8, AppearanceNets(p=1.0, p_k3=1.0, blend=False))
    assert abs(p[:, 7:7 + 54].std() - 4096 / np.sqrt(27.0)) < 20


def test_feed_draws_come_last(tmp_path):
    """appearance=None: `_stage_draws` returns what it returned (no new key) and the pipeline is called as it was.  With the stage on,
    the other stages' draws are those of the stage-off run, and the stage's own start where that run's generator stands."""
    from wtpse_hip.input_pipeline import AmplitudeMix, Augment
    from wtpse_hip.trainer import FundusBatches
    sets = _sets(tmp_path)
    nets = AppearanceNets(p=0.8, spacing=16)
    for augment in (None, Augment()):
        for style, quality in ((None, None), (AmplitudeMix(), ImageQuality())):
            plain_pipe, pipe = RecordingPipe(), RecordingPipe()
            plain = FundusBatches(sets, 6, "cuda", size=64, augment=augment, style=style, quality=quality, pipe=plain_pipe)
            feed = FundusBatches(sets, 6, "cuda", size=64, augment=augment, style=style, quality=quality, appearance=nets, pipe=pipe)
            assert set(plain._stage_draws(np.random.RandomState(0), 6)) == {k for k, v in (("mix_draws", style), ("quality_draws", quality)) if v}
            py_p, np_p = random.Random(3), np.random.RandomState(3)
            py_q, np_q = random.Random(3), np.random.RandomState(3)
            for _ in range(2):
                plain(py_p, np_p)
                feed(py_q, np_q)
                want = draw_appearance(np_p, 6, 64, nets)
                n, args, kw = pipe.calls[-1]
                _, pargs, pkw = plain_pipe.calls[-1]
                got = kw["appearance_draws"]
                assert n == 6 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == 16
                assert py_p.getstate() == py_q.getstate()
                assert all(np.array_equal(x, y) for x, y in zip(np_p.get_state()[1:3], np_q.get_state()[1:3]))
                assert "appearance_draws" not in pkw and len(pargs) == len(args) and set(kw) - {"appearance_draws"} == set(pkw)
                if style is not None:
                    assert np.array_equal(kw["mix_draws"][0], pkw["mix_draws"][0]) and np.array_equal(kw["mix_draws"][1], pkw["mix_draws"][1])
                    assert np.array_equal(kw["quality_draws"], pkw["quality_draws"])
                if style is None and augment is None:
                    assert pargs == () and pkw == {}
            assert feed.state() == plain.state()                   # the stage adds no entry
    with pytest.raises(ValueError):
        FundusBatches(sets, 6, "cuda", size=1024, appearance=nets, pipe=RecordingPipe())
    with pytest.raises(ValueError):
        FundusBatches(sets, 6, "cuda", size=64, appearance=ImageQuality(), pipe=RecordingPipe())


def test_entry_points_refuse_bad_shapes_without_a_gpu():
    from wtpse_hip.lib import lib
    q = lib().query
    assert q("wtpse_appearance_workspace", 32, 256) == 7 * 32 + 6 * 32 * 256 * 256
    assert q("wtpse_appearance_workspace", 3, 71) == 24 + 6 * 3 * 71 * 71
    for N, S in ((0, 64), (65536, 64), (2, 0), (2, 513), (2000, 512)):
        assert q("wtpse_appearance_workspace", N, S) == -1
    assert lib().raw("wtpse_appearance_nets")(0, 0, 0, 2, 64, 0) == -1
    assert lib().raw("wtpse_appearance_finish")(0, 0, 0, 0, 0, 0, 2, 64, 5, 0) == -1
    assert len(lib().protos["wtpse_appearance_finish"]) == 10
