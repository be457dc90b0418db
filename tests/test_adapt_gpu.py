"""wtpse_hip/adapt.py on the device (-m gpu): wtpse_bn_finalize_blend against the float64 specification and against its sibling
wtpse_bn_finalize, then the switch HipNet.bn_blend through whole networks: nothing changes while it is off, a blended call equals a
plain call on networks that carry the emitted statistics, prior 0 equals train-mode normalisation, stream mode pools, and the site
program end to end."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from oracle.fundus_tree import _sample
from oracle.inputs import make_inputs
from test_parity_gpu import build_nets, close, HP

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ordered(a):
    """float32 array -> int64 whose order and spacing are the floats' (one step = one ulp, across zero too)."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(a, b):
    return int(np.abs(_ordered(a) - _ordered(b)).max())


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max())


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 5), (257, 16), (2304, 32)]              # (nblk, C); 2304 >= 2048: the 1024-thread form


@functools.lru_cache(maxsize=None)
def _case(nblk, C):
    """Two real tensors [nblk, C, L] (this call's and an earlier call's), |mean| / std <= 10 per channel, and their per-chunk
    (sum, sum^2) partials rounded to fp32 as a producer's epilogue leaves them; BatchNorm parameters and source statistics."""
    rng = np.random.default_rng(1000 * nblk + C)
    L = 37 if nblk < 2048 else 8
    out = []
    for _ in range(2):
        std = rng.uniform(0.3, 3.0, size=(1, C, 1))
        mean = std * rng.uniform(-10.0, 10.0, size=(1, C, 1))
        x = (mean + std * rng.normal(size=(nblk, C, L))).astype(np.float32)
        x64 = x.astype(np.float64)
        part = np.stack((x64.sum(2), (x64 * x64).sum(2)), axis=-1).astype(np.float32)
        out.append((x, part))
    p = dict(gamma=rng.normal(size=C).astype(np.float32) * 2, beta=rng.normal(size=C).astype(np.float32),
             rmean=rng.normal(size=C).astype(np.float32) * 3, rvar=rng.uniform(0.2, 5.0, size=C).astype(np.float32))
    return out, p, nblk * L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _spec(part, count, p, w, hist=None):
    """The float64 specification on fp32 partials: -> (ss, moments [C,4], div, (s1, s2))."""
    from wtpse_hip import adapt as A
    s = part.astype(np.float64).sum(0)
    a1, a2, an = (hist[0][:, 0], hist[0][:, 1], hist[1]) if hist is not None else (0.0, 0.0, 0.0)
    mt, vt = A.target_host(s[:, 0], s[:, 1], count, a1, a2, an)
    mb, vb = A.blend_host(p["rmean"], p["rvar"], mt, vt, w)
    return A.coeffs_host(p["gamma"], p["beta"], mb, vb), np.stack((mt, vt, mb, vb), 1), A.divergence_host(p["rmean"], p["rvar"], mt, vt), s


@pytest.mark.parametrize("with_acc", [False, True], ids=["noacc", "acc"])
@pytest.mark.parametrize("w", [0.0, 0.36, 1.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_finalize_blend_matches_the_specification(shape, w, with_acc):
    from wtpse_hip import ops
    nblk, C = shape
    ((x, part), (x0, part0)), p, count = _case(nblk, C)
    d = {k: _dev(v) for k, v in p.items()}
    rmean0, rvar0 = d["rmean"].clone(), d["rvar"].clone()
    moments = torch.full((C, 4), float("nan"), dtype=torch.float64, device=DEV)
    div = torch.full((C,), float("nan"), dtype=torch.float64, device=DEV)
    tab = torch.zeros(ops.AMAX_WORDS, dtype=torch.int32, device=DEV)
    acc, hist = None, None
    if with_acc:                                          # an earlier call leaves its sums; this one pools with them
        acc = torch.zeros((C, 2), dtype=torch.float64, device=DEV)
        ss0 = ops.bn_finalize_blend(_dev(part0), count, d["gamma"], d["beta"], d["rmean"], d["rvar"], w, acc=acc, acc_count=0)
        want0, _, _, s0 = _spec(part0, count, p, w)
        assert ulps(ss0.cpu().numpy(), want0) <= 1
        assert rel(acc.cpu().numpy(), s0) <= 1e-12
        hist = (s0, count)
    ss = ops.bn_finalize_blend(_dev(part), count, d["gamma"], d["beta"], d["rmean"], d["rvar"], w, acc=acc,
                               acc_count=count if with_acc else 0, moments=moments, div=div, act_amax=tab)
    torch.cuda.synchronize()
    want_ss, want_m, want_div, s = _spec(part, count, p, w, hist)
    got = ss.cpu().numpy()
    print("ulps", ulps(got, want_ss), "moments", rel(moments.cpu().numpy(), want_m), "div", rel(div.cpu().numpy(), want_div))
    assert ulps(got, want_ss) <= 1
    assert rel(moments.cpu().numpy(), want_m) <= 1e-9
    assert rel(div.cpu().numpy(), want_div) <= 1e-9
    if with_acc:
        assert rel(acc.cpu().numpy(), hist[0] + s) <= 1e-12       # after two calls: the float64 sums of both
    # the running statistics are read, never written
    assert torch.equal(d["rmean"], rmean0) and torch.equal(d["rvar"], rvar0)
    # the bound: finite and at least the largest |scale y + shift| over this call's values
    z = np.abs(got[None, :, :1].astype(np.float64) * x.astype(np.float64) + got[None, :, 1:].astype(np.float64)).max()
    bound = float(tab.cpu().numpy().max().astype(np.int32).view(np.float32))
    print("bound", bound, "max|z|", z)
    assert np.isfinite(bound) and bound >= z
    assert int((tab != 0).sum()) <= min(C, 64)            # one shard per channel at most, nothing else touched


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_weight_one_without_history_is_the_train_mode_finalize(shape):
    from wtpse_hip import ops
    nblk, C = shape
    ((x, part), _), p, count = _case(nblk, C)
    d = {k: _dev(v) for k, v in p.items()}
    ss = ops.bn_finalize_blend(_dev(part), count, d["gamma"], d["beta"], d["rmean"], d["rvar"], 1.0)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    sib, mean, invstd = ops.bn_finalize(_dev(part), count, d["gamma"], d["beta"], d["rmean"].clone(), d["rvar"].clone(), nbt)
    assert torch.equal(ss, sib)                           # bit for bit: one fold, one expression
    assert int(nbt) == 1


def test_finalize_blend_argument_checks():
    from wtpse_hip import ops
    from wtpse_hip.lib import WtpseError
    ((x, part), _), p, count = _case(3, 5)
    d = {k: _dev(v) for k, v in p.items()}
    args = (_dev(part), count, d["gamma"], d["beta"], d["rmean"], d["rvar"])
    for w in (-0.01, 1.01):
        with pytest.raises(WtpseError):
            ops.bn_finalize_blend(*args, w)
    with pytest.raises(WtpseError):
        ops.bn_finalize_blend(*args, 0.5, acc_count=10)                                    # history without its sums
    with pytest.raises(ValueError):
        ops.bn_finalize_blend(*args, 0.5, moments=torch.zeros((5, 4), device=DEV))         # float32
    with pytest.raises(ValueError):
        ops.bn_finalize_blend(*args, 0.5, acc=torch.zeros((5, 4), dtype=torch.float64, device=DEV))


# ---- the networks -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    """Seeded networks one training step away from the filler: BatchNorm's running statistics have moved."""
    from wtpse_hip.step import TrainStep
    nets = build_nets(1)
    img, od, oc = make_inputs(41, 3, 64, 64)
    ts = TrainStep(nets[0], nets[1], nets[2], nets[3], HP)
    for n in nets:
        n.seed_noise(5)
    ts.step(img.to(DEV), od.to(DEV), oc.to(DEV))
    torch.cuda.synchronize()
    return nets


@pytest.fixture(scope="module")
def data():
    return make_inputs(43, 3, 64, 64)[0].to(DEV)


def _snapshot(nets):
    return [dict(sd={k: v.detach().clone() for k, v in n.state_dict().items()}, modes=[m.training for m in n.modules()],
                 ctr=n._noise_ctr.clone() if n._noise_ctr is not None else None) for n in nets]


def _assert_unchanged(nets, snap):
    for n, s in zip(nets, snap):
        sd = n.state_dict()
        assert list(sd) == list(s["sd"])
        for k, v in sd.items():
            assert torch.equal(v, s["sd"][k]), k
        assert [m.training for m in n.modules()] == s["modes"]
        assert n.bn_blend is None
        if s["ctr"] is not None:
            assert torch.equal(n._noise_ctr, s["ctr"])


def _clones(nets):
    new = build_nets(1)
    for a, b in zip(new, nets):
        a.load_state_dict(b.state_dict())
    return new


def _bn_modules(net):
    from wtpse_hip import nn as E
    return [(name, m) for name, m in net.named_modules() if isinstance(m, E.BNP)]


def _predict(nets, x, state=None, train=False):
    from wtpse_hip import adapt as A, validate as V
    if train:
        for n in nets:
            n.train()
        return V.predict_pair(*nets, x)
    with V.eval_mode(nets), A.blended(nets, state):
        return V.predict_pair(*nets, x)


def test_switch_off_changes_nothing_and_a_blended_call_leaves_no_trace(nets, data):
    from wtpse_hip import adapt as A
    snap = _snapshot(nets)
    before = _predict(nets, data)
    state = A.BlendState(2, "batch")
    blended = _predict(nets, data, state)
    torch.cuda.synchronize()
    _assert_unchanged(nets, snap)                                   # parameters, buffers, modes, Philox counters; bn_blend None again
    after = _predict(nets, data)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert not torch.equal(blended[0], before[0])                   # (and the switch did something)
    # every BatchNorm layer that runs at prediction time was visited once, with the batch's weight
    visited = [m for n in nets for _, m in _bn_modules(n) if m in state.slots]
    assert len(visited) == len(state.slots) >= 4 * 20
    assert all(state.slots[m].calls == 1 and state.slots[m].w == 3.0 / 5.0 and state.slots[m].images == 0 for m in visited)


def test_adapted_test_run_is_the_wrapped_test_run(nets, data, tmp_path, monkeypatch):
    """AdaptedTestRun(adapt="batch") writes the table a TestRun inside `blended` writes, names the mode in summary.json and leaves
    bn_blend at None; adapt=None is TestRun itself."""
    from wtpse_hip import adapt as A, validate as V
    from wtpse_hip.test_run import TestRun, read_table
    seen, inner = [], V.predict_pair

    def recording(*a, **kw):                                        # the logits every run predicts (the fixture's networks are a step
        out = inner(*a, **kw)                                       # from the filler: their masks, and so the tables, say little)
        seen.append([t.clone() for t in out])
        return out
    monkeypatch.setattr(V, "predict_pair", recording)
    yy, xx = np.mgrid[0:64, 0:64]
    disc = ((yy - 30) ** 2 + (xx - 33) ** 2 <= 20 ** 2).astype(np.float32)
    cup = ((yy - 30) ** 2 + (xx - 33) ** 2 <= 9 ** 2).astype(np.float32)
    od, oc = (_dev(np.broadcast_to(m, (3, 1, 64, 64))) for m in (disc, cup))
    batches = [(data[:2].contiguous(), od[:2], oc[:2], ["a", "b"]), (data[2:3].contiguous(), od[2:3], oc[2:3], ["c"])]
    snap = _snapshot(nets)
    outs = [str(tmp_path / n) for n in ("adapted", "wrapped", "plain", "off")]
    means = A.AdaptedTestRun(*nets, out_dir=outs[0], adapt="batch", prior=2).run(batches)
    _assert_unchanged(nets, snap)                                   # bn_blend None again, modes restored, nothing written
    with A.blended(nets, A.BlendState(2, "batch")):
        want = TestRun(*nets, out_dir=outs[1]).run(batches)
    plain = TestRun(*nets, out_dir=outs[2]).run(batches)
    off = A.AdaptedTestRun(*nets, out_dir=outs[3]).run(batches)
    rows, summary = read_table(outs[0])
    assert rows == read_table(outs[1])[0] and len(rows) == 3
    assert means == dict(want, adapt="batch", prior=2.0) and summary == means
    assert off == plain and read_table(outs[3]) == read_table(outs[2]) and "adapt" not in off
    adapted, wrapped, plain_p, off_p = (seen[2 * i:2 * i + 2] for i in range(4))          # two batches per run
    for a, b in ((adapted, wrapped), (off_p, plain_p)):
        assert all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    assert not torch.equal(adapted[0][0], plain_p[0][0])            # (and the switch did something)
    with pytest.raises(ZeroDivisionError):                          # restored whatever ends the run
        A.AdaptedTestRun(*nets, out_dir=outs[0], adapt="stream", prior=2).run(iter(lambda: 1 // 0, None))
    _assert_unchanged(nets, snap)
    for bad in (dict(adapt="site"), dict(adapt="batch", prior=-1)):
        with pytest.raises(ValueError):
            A.AdaptedTestRun(*nets, out_dir=outs[0], **bad)


def _carry_emitted_statistics(nets, state):
    """Clones of `nets` whose running buffers hold the (mean_b, var_b) the blended call emitted per layer."""
    new = _clones(nets)
    for net, clone in zip(nets, new):
        targets = dict(_bn_modules(clone))
        for name, m in _bn_modules(net):
            if m in state.slots:
                mom = state.slots[m].moments
                with torch.no_grad():
                    targets[name].running_mean.copy_(mom[:, 2].float())
                    targets[name].running_var.copy_(mom[:, 3].float())
    return new


@pytest.mark.parametrize("cast", ["plain", "far"])
def test_blended_call_is_a_plain_call_on_the_emitted_statistics(nets, data, cast):
    """Identity, batch mode, N0 = 2: at the bar test_parity_gpu.py holds logits to (|a - b| <= 1e-4 + 1e-4 |b|).  "far": 8 x + 3, a
    cast far from the running statistics — pre-BatchNorm maps several times the source's scale with large mean offsets, where an x2h
    input scale taken from the source statistics would overflow."""
    from wtpse_hip import adapt as A
    x = data if cast == "plain" else (8.0 * data + 3.0).contiguous()
    state = A.BlendState(2, "batch", report=True)
    got = _predict(nets, x, state)
    want = _predict(_carry_emitted_statistics(nets, state), x)
    for g, w_, what in zip(got, want, ("disc", "cup")):
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(w_).all())
        print(cast, what, "max |diff|", float((g - w_).abs().max()), "scale", float(w_.abs().max()))
        close(g, w_, atol=1e-4, what="%s logits, %s" % (what, cast))


def test_prior_zero_is_train_mode_normalisation(nets, data):
    from wtpse_hip import adapt as A
    got = _predict(nets, data, A.BlendState(0, "batch"))
    want = _predict(_clones(nets), data, train=True)
    for g, w_, what in zip(got, want, ("disc", "cup")):
        print(what, "max |diff|", float((g - w_).abs().max()), "scale", float(w_.abs().max()))
        close(g, w_, atol=1e-4, what=what + " logits")


def test_stream_mode_pools_over_calls(nets, data):
    """Two calls, 2 images then 1.  First BatchNorm layer (its input is the data itself): the second call's (mean_t, var_t) are the
    statistics of the conv output over all three images.  The reference sums the stored fp32 conv output in float64; the kernel
    folds in float64 the fp32 partial sums the convolution's workgroups leave, each over one tile of T pixels (T from the library's
    own geometry query: 256 here).  An fp32 sum of T terms carries T - 1 roundings of relative size 2^-24; roundings of a sum are
    independent in sign, so its error is of the order sqrt(T) 2^-24 of the terms' magnitude (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2's probabilistic rule), and the partials' errors do not grow when they are added in float64:
    u = sqrt(T) 2^-24 = 9.5e-7 of E|y| for the mean and of E[y^2] for the second moment.  A wrong pixel count, a missing or doubled
    call or a wrong layer moves the moments by parts in 1e-2.  Every layer: moments, acc and the counts are consistent."""
    from wtpse_hip import adapt as A, nn as E, ops
    state = A.BlendState(16, "stream", report=True)
    first = _predict(nets, data[:2].contiguous(), state)
    w_first = {m: s.w for m, s in state.slots.items()}
    second = _predict(nets, data[2:3].contiguous(), state)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in first + second)
    assert state.n_seen == 3
    bn = nets[0].inc.bn1
    nets[0].eval()
    nets[0].ensure_ready(repack=True)
    y = E._conv(nets[0].inc.conv1, data)[0].double()
    n = y.numel() // y.shape[1]
    mean, ex2, eabs = y.mean(dim=(0, 2, 3)).cpu().numpy(), (y * y).mean(dim=(0, 2, 3)).cpu().numpy(), y.abs().mean(dim=(0, 2, 3)).cpu().numpy()
    var = np.maximum(ex2 - mean * mean, 0.0)
    mom = state.slots[bn].moments.cpu().numpy()
    T = 64 * 64 // ops.lib().query("wtpse_conv_stats_blocks", 1, 64, 64)
    assert 64 <= T <= 4096
    u = np.sqrt(T) * 2.0 ** -24
    print("mean err", np.abs(mom[:, 0] - mean).max(), "var err", np.abs(mom[:, 1] - var).max())
    assert (np.abs(mom[:, 0] - mean) <= u * eabs).all()
    assert (np.abs(mom[:, 1] - var) <= u * ex2 + 2 * np.abs(mean) * u * eabs + (u * eabs) ** 2).all()
    assert state.slots[bn].pixels == n and state.slots[bn].images == 3
    for m, s in state.slots.items():
        assert s.calls == 2 and s.images == 3 and w_first[m] == 2.0 / 18.0 and s.w == 3.0 / 19.0
        assert s.count * 3 == s.pixels                                       # (the last call held one image of the three)
        acc, mom = s.acc.cpu().numpy(), s.moments.cpu().numpy()
        mt, vt = A.target_host(acc[:, 0], acc[:, 1], s.pixels)
        mb, vb = A.blend_host(m.running_mean.cpu().numpy(), m.running_var.cpu().numpy(), mt, vt, s.w)
        want = np.stack((mt, vt, mb, vb), 1)
        assert np.allclose(mom, want, rtol=1e-9, atol=1e-9 * float(np.abs(acc[:, 1] / s.pixels).max())), rel(mom, want)
    # a third call in batch mode on the same networks keeps no history
    batch = A.BlendState(16, "batch")
    _predict(nets, data[:1].contiguous(), batch)
    assert batch.n_seen == 0 and all(s.acc is None and s.moments is None and s.div is None and s.pixels == 0 for s in batch.slots.values())


@pytest.mark.parametrize("terms", [3, 1], ids=["x3", "bf16"])
def test_blended_call_under_the_other_arithmetics(nets, data, terms):
    """x2h is the default the other tests run under; under x3 and in bf16 mode no amax table exists and the path must not ask for one.
    x3 is fp32-accurate: prior 0 still equals train-mode normalisation at the logits' bar.  bf16 mode: finite, buffers untouched."""
    from wtpse_hip import adapt as A, ops
    snap = _snapshot(nets)
    was = ops.lib().query("wtpse_x3_terms", terms)
    try:
        assert ops.fwd_amax_table(torch.device(DEV, torch.cuda.current_device())) is None
        got = _predict(nets, (8.0 * data + 3.0).contiguous(), A.BlendState(0, "batch"))
        assert all(bool(torch.isfinite(t).all()) for t in got)
        if terms == 3:
            want = _predict(_clones(nets), (8.0 * data + 3.0).contiguous(), train=True)
            for g, w_ in zip(got, want):
                close(g, w_, atol=1e-4, what="x3 logits")
    finally:
        ops.lib().query("wtpse_x3_terms", was)
    for n in nets:
        n.invalidate_packed()
    _assert_unchanged(nets, snap)


def test_blend_refuses_a_tape_and_synchronised_batchnorm(nets, data):
    from wtpse_hip import adapt as A, nn as E, validate as V
    state = A.BlendState(2, "batch")
    net = nets[0]
    with V.eval_mode(nets), A.blended(nets, state):
        net.ensure_ready(repack=True)
        with pytest.raises(RuntimeError, match="bn_blend"):
            E.convd_fwd(net.inc, data, False, want_tape=True)
        with pytest.raises(RuntimeError, match="bn_blend"):
            E.upbn_fwd(net.up4.conv2, net.up4.bn2, E.Act(torch.zeros(3, 32, 32, 32, device=DEV)), False, want_tape=True)
        E.convd_fwd(net.inc, data, False, want_tape=False)                  # without a tape the same call runs
        object.__setattr__(net, "_dp", types.SimpleNamespace(bn_sync=True))
        try:
            with pytest.raises(RuntimeError, match="synchronised"):
                V.predict_pair(*nets, data)
        finally:
            object.__setattr__(net, "_dp", None)
        net.train()                                                         # train mode ignores the switch: a tape is fine
        _, tape = E.convd_fwd(net.inc, data, True, want_tape=True)
        assert tape is not None
    assert not state.slots or all(s.calls >= 1 for s in state.slots.values())
    torch.cuda.synchronize()


# ---- site mode, end to end ------------------------------------------------------------------------------------------------------------
E2E = (("eye_04.png", 300, 280), ("Patient 7 (left).png", 222, 190), ("a.png", 300, 280), ("zz-top.png", 222, 190), ("m.png", 300, 280))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Five crops at two native sizes, alternating, under names that follow no dataset prefix."""
    root = str(tmp_path_factory.mktemp("site"))
    rs = np.random.RandomState(11)
    for name, w, h in E2E:
        _sample(rs, w, h, rgb_mask=False)[0].save(os.path.join(root, name))
    return root


def test_site_statistics_end_to_end(nets, folder, tmp_path):
    from wtpse_hip import adapt as A
    from wtpse_hip.segment import Segmenter
    from wtpse_hip.test_run import CHECKPOINT_KEYS, load_checkpoint
    from wtpse_hip.validate import best_checkpoint
    N0 = 4.0
    for n in nets:
        n.train()
        n.ensure_ready(repack=True)                      # (the packed weights current, whatever arithmetic an earlier test left them in)
    snap = _snapshot(nets)
    packed = [(n._packed.clone(), n._x3.clone()) for n in nets]
    fit = A.SiteStatistics(*nets, prior=N0, batch_size=2)
    ck = fit.fit(folder, source_name="source.pth.tar")
    _assert_unchanged(nets, snap)                                            # the live networks: bitwise what they were
    for n, (p, x3) in zip(nets, packed):
        assert torch.equal(n._packed, p) and torch.equal(n._x3, x3)
    assert list(ck) == list(CHECKPOINT_KEYS) + ["site"] and ck["site"] == fit.site
    assert (fit.site["prior"], fit.site["images"], fit.site["source"]) == (N0, 5, "source.pth.tar")
    w = A.blend_weight(5, N0)
    n_bn = 0
    for key, net in zip(CHECKPOINT_KEYS, nets):
        sd, adapted = net.state_dict(), set()
        for name, m in _bn_modules(net):
            n_bn += 1
            layer = fit.site["layers"][key][name]
            if m not in fit.state.slots:
                assert layer["images"] == 0 and not any(layer["divergence"])
                continue
            s = fit.state.slots[m]
            assert s.images == 5 and s.calls == 3 and layer["images"] == 5 and s.w == w
            mom = s.moments.cpu().numpy()                                    # the pooled moments the last call emitted
            mb, vb = A.blend_host(m.running_mean.cpu().numpy(), m.running_var.cpu().numpy(), mom[:, 0], mom[:, 1], w)
            assert ulps(ck[key][name + ".running_mean"].cpu().numpy(), mb.astype(np.float32)) <= 1
            assert ulps(ck[key][name + ".running_var"].cpu().numpy(), vb.astype(np.float32)) <= 1
            assert rel(layer["divergence"], s.div.cpu().numpy()) <= 1e-9
            adapted |= {name + ".running_mean", name + ".running_var"}
        assert len(adapted) >= 2 * 20
        for k, v in sd.items():                                               # everything else equals the source bitwise
            assert k in adapted or torch.equal(ck[key][k], v), (key, k)
            assert not (k in adapted and torch.equal(ck[key][k], v)), (key, k)
    # the program: three files; the same numbers from networks loaded from the saved source checkpoint
    src = str(tmp_path / "checkpoint_1.pth.tar")
    torch.save(best_checkpoint(*nets), src)
    out = str(tmp_path / "adapted")
    assert A.main(["--images", folder, "--checkpoint", src, "--out", out, "--prior", str(N0), "--batch-size", "2"]) == 0
    assert sorted(os.listdir(out)) == ["adapted_checkpoint.pth.tar", "shift.csv", "shift.json"]
    rows, summary = A.read_shift(out)
    assert len(rows) == n_bn == sum(len(_bn_modules(n)) for n in nets)        # one row per BatchNorm module of the four networks
    assert summary["images"] == 5 and summary["prior"] == N0 and summary["source"] == "checkpoint_1.pth.tar"
    assert summary["mean_divergence"] > 0 and set(summary["networks"]) == set(CHECKPOINT_KEYS)
    assert rows == A.shift_rows(dict(fit.site, source="checkpoint_1.pth.tar"))
    saved = torch.load(os.path.join(out, "adapted_checkpoint.pth.tar"), map_location="cpu", weights_only=True)
    assert saved["site"]["images"] == 5
    for key in CHECKPOINT_KEYS:
        for k, v in ck[key].items():
            assert torch.equal(saved[key][k], v.cpu()), (key, k)
    # it loads wherever a best-Dice checkpoint does, and Segmenter runs on it
    fresh = build_nets(1)
    load_checkpoint(os.path.join(out, "adapted_checkpoint.pth.tar"), *fresh)
    for key, net in zip(CHECKPOINT_KEYS, fresh):
        for k, v in net.state_dict().items():
            assert torch.equal(v.cpu(), saved[key][k]), (key, k)
    seg_out = str(tmp_path / "segmented")
    s = Segmenter(*fresh, out_dir=seg_out, batch_size=2, overlay=False).run(folder)
    assert s["n"] == 5 and "adapt" not in s and len(os.listdir(os.path.join(seg_out, "mask"))) == 5
    # the switches on the drivers: stream over the folder, and the summary says so
    s = Segmenter(*nets, out_dir=str(tmp_path / "streamed"), batch_size=2, overlay=False, adapt="stream", prior=N0).run(folder)
    assert s["n"] == 5 and s["adapt"] == "stream" and s["prior"] == N0
    _assert_unchanged(nets, snap)
