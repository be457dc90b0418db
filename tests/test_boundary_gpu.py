"""The boundary loss on the GPU: wtpse_signed_distance against the host specification (integers and float bits exactly),
wtpse_boundary_loss against the float64 specification, TrainStep(boundary=) and TrainRun(boundary=).  Sizes of the step tests follow
tests/test_trainer_gpu.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

pytestmark = pytest.mark.gpu
B = 6
RATES = (5e-4, 4e-4, 3e-4, 2e-4)
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------- 1. the distance kernel
SHAPES = [(1, 1, 1), (3, 1, 7), (3, 7, 1), (2, 5, 64), (3, 33, 65), (6, 64, 64), (2, 100, 257), (2, 256, 256), (1, 512, 512)]
# beyond the issue's list: a row longer than one pass of the workgroup's 256 threads several times over and longer than 1024 words
# of LDS, and a column longer than the 16-bit distances of a 1024-row plane would need
EXTRA_SHAPES = [(1, 3, 1500), (2, 1300, 2)]


def _planes(h, w):
    """The planes of one shape, in the order they are batched: the planes without a contour sit among ordinary ones."""
    r = np.random.RandomState(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    corner = np.zeros((h, w))
    corner[h - 1, 0] = 1                         # the farthest pixel is (0, w - 1): the largest distance the plane can hold
    row = np.zeros((h, w))
    row[h // 3] = 1
    col = np.zeros((h, w))
    col[:, (2 * w) // 3] = 1
    d2 = (yy - 0.45 * h) ** 2 + (xx - 0.55 * w) ** 2
    rad = 0.35 * min(h, w)
    ring = (d2 <= rad * rad) & (d2 > (0.4 * rad) ** 2)      # a disc with a hole
    planes = [np.zeros((h, w)), corner, np.ones((h, w)), row, col, (yy + xx) % 2, ring, r.uniform(size=(h, w)) < 0.5,
              r.uniform(size=(h, w)) < 0.001]
    return [np.ascontiguousarray(p, dtype=np.float32) for p in planes]


_REF = {}


def _reference(h, w):
    """[(plane, phi float64, d2_out, d2_in)] of a shape, computed once.  Small planes: the all-pairs specification.  From 64 x 64 up
    that takes too long: Kervadec's scipy expression where scipy imports (tests/test_boundary_cpu.py holds it equal to the
    specification), else the specification's separable form."""
    if (h, w) not in _REF:
        from wtpse_hip import boundary as bd
        try:
            from scipy import ndimage as ndi
        except ImportError:
            ndi = None
        out = []
        for t in _planes(h, w):
            pos = t != 0
            if h * w <= 4096 or not pos.any() or pos.all():
                d2_out, d2_in = bd.squared_distances_host(t)
            elif ndi is not None:
                d2_out = np.rint(ndi.distance_transform_edt(~pos) ** 2).astype(np.int32)
                d2_in = np.rint(ndi.distance_transform_edt(pos) ** 2).astype(np.int32)
            else:
                d2_out, d2_in = bd.squared_distances_separable_host(t)
            out.append((t, bd.signed_distance_from_d2(d2_out, d2_in), d2_out, d2_in))
        _REF[(h, w)] = out
    return _REF[(h, w)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("shape", SHAPES + EXTRA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_signed_distance_exact(shape):
    from wtpse_hip import ops
    Bn, h, w = shape
    ref = _reference(h, w)
    assert not ref[0][0].any() and ref[2][0].all() and not ref[0][1].any() and not ref[2][1].any()      # empty and full: phi = 0
    for i in range(0, len(ref), Bn):
        group = [ref[j % len(ref)] for j in range(i, i + Bn)]           # the last batch is filled up from the front
        t = torch.from_numpy(np.stack([g[0] for g in group])[:, None]).to(DEV)
        phi, d2_out, d2_in = ops.signed_distance(t, want_d2=True)
        assert phi.shape == t.shape and d2_out.dtype == d2_in.dtype == torch.int32
        got_o, got_i, got_phi = d2_out.cpu().numpy()[:, 0], d2_in.cpu().numpy()[:, 0], phi.cpu().numpy()[:, 0]
        for k, (_, want_phi, want_o, want_i) in enumerate(group):
            assert np.array_equal(got_o[k], want_o), "d2_out of plane %d differs in %d pixels" % (i + k, int((got_o[k] != want_o).sum()))
            assert np.array_equal(got_i[k], want_i), "d2_in of plane %d differs in %d pixels" % (i + k, int((got_i[k] != want_i).sum()))
            same = _bits(got_phi[k]) == _bits(want_phi)
            assert same.all(), "phi of plane %d: %d pixels are not float32(float64 specification)" % (i + k, int((~same).sum()))
        # again, and without the integer maps: the same bits
        again = ops.signed_distance(t, want_d2=True)
        only = ops.signed_distance(t)
        for a, b in zip(again, (phi, d2_out, d2_in)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(only.view(torch.int32), phi.view(torch.int32))


def test_signed_distance_takes_plain_planes_and_refuses_other_sizes():
    from wtpse_hip import ops
    L = ops.lib()
    for Bn, h, w in [(1, 4097, 8), (1, 8, 4097), (0, 8, 8), (1, 0, 8), (65536, 1, 1)]:
        assert L.query("wtpse_signed_distance_ws", Bn, h, w) <= 0
    assert L.query("wtpse_signed_distance_ws", 2, 4096, 3) == 2 * 4096 * 3
    with pytest.raises(ValueError, match="unsupported size"):
        ops.signed_distance(torch.zeros(1, 1, 4097, 8, device=DEV))
    with pytest.raises(ValueError, match="unsupported size"):
        ops.signed_distance(torch.zeros(1, 1, 0, 8, device=DEV))
    with pytest.raises(ValueError):
        ops.signed_distance(torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        ops.signed_distance(torch.zeros(1, 1, 8, 8, device=DEV, dtype=torch.float64))
    # [h, w] and [B, h, w] are planes as well; nonzero = object whatever the value (NaN included)
    t = torch.zeros(5, 6, device=DEV)
    t[2, 3] = float("nan")
    phi = ops.signed_distance(t)
    assert phi.shape == (5, 6) and float(phi[2, 3]) == 0.0 and float(phi[2, 5]) == 2.0 and float(phi[0, 0]) == float(np.float32(math.sqrt(13.0)))


# ---------------------------------------------------------------------------------------------------- 2. the loss kernel
def _ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def _loss_case(shape, masked):
    from wtpse_hip import ops
    Bn, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    radii = [9, 15, 22][:Bn] if (h, w) == (64, 64) else [6, 11][:Bn]
    t = np.stack([((yy - h / 2) ** 2 + (xx - w / 2) ** 2 <= r * r) for r in radii]).astype(np.float32)[:, None]
    g = torch.Generator().manual_seed(100 * h + w + int(masked))
    x = torch.randn(t.shape, generator=g) * 3.0
    mask = (torch.rand(t.shape, generator=g) < 0.6).float() if masked else None
    phi = ops.signed_distance(torch.from_numpy(t).to(DEV))
    return x, mask, phi


@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 33, 65)], ids=lambda s: "x".join(map(str, s)))
def test_boundary_loss_value_and_gradient(shape, masked):
    from wtpse_hip import ops
    from wtpse_hip import boundary as bd
    x, mask, phi = _loss_case(shape, masked)
    n = x.numel()
    xd, md = x.to(DEV), None if mask is None else mask.to(DEV)
    phi_h = phi.cpu()
    x64, phi64 = x.double().numpy(), phi_h.double().numpy()
    m64 = None if mask is None else mask.double().numpy()
    alpha = torch.full((1,), 0.37, dtype=torch.float32, device=DEV)
    a32 = float(alpha.item())

    # ---- the value, with dx null and non-null: the same bits
    loss = ops.boundary_loss(xd, phi, None, mask=md)
    dx0 = (torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) * 1e-3).to(DEV)
    dx = dx0.clone()
    dx.wt_amax = object()                                # an amax table of the region loss's gradient would be stale now
    loss_dx = ops.boundary_loss(xd, phi, alpha, mask=md, dx=dx)
    assert dx.wt_amax is None
    assert torch.equal(loss.view(torch.int32), loss_dx.view(torch.int32)) and loss.dim() == 0
    want = bd.boundary_loss_host(x64, phi64, m64)
    z = x64 if m64 is None else x64 * m64
    M = float(np.mean(np.abs(phi64 / (1.0 + np.exp(-z)))))
    z32 = x if mask is None else x * mask
    cpu32 = float((torch.sigmoid(z32) * phi_h).mean())   # the same arithmetic in torch fp32 on the host
    bar = max(3.0 * abs(cpu32 - want), math.log2(n) * 2.0 ** -24 * M)
    err = abs(float(loss) - want)
    print("boundary_loss %s %s: L_B %.9g, |gpu - f64| / M = %.3g, |cpu fp32 - f64| / M = %.3g, bar / M = %.3g"
          % (shape, "cup" if masked else "disc", want, err / M, abs(cpu32 - want) / M, bar / M))
    assert err <= bar, (err, bar)

    # ---- the increment: d(alpha L_B)/dx added in place
    g64 = bd.boundary_grad_host(x64, phi64, a32, m64)
    s32 = torch.sigmoid(z32)
    g32 = (torch.tensor(a32) / n) * phi_h * (s32 * (1 - s32))
    if mask is not None:
        g32 = g32 * mask
    elem_bar = np.maximum(3.0 * np.abs(g32.double().numpy() - g64), 2.0 * _ulp32(g64))
    # (i) into zeros: what is stored IS the increment
    inc = torch.zeros_like(dx0)
    ops.boundary_loss(xd, phi, alpha, mask=md, dx=inc)
    e = np.abs(inc.cpu().double().numpy() - g64)
    print("  increment into zeros: max |err| / bar = %.3g, max err %.3g ulp" % (float((e / elem_bar).max()), float((e / _ulp32(g64)).max())))
    assert (e <= elem_bar).all(), int((e > elem_bar).sum())
    # (ii) into a known tensor: after - before (exact in float64) is the increment up to the rounding of the stored sum, at most
    # half an ulp of the sum, which no implementation of an in-place fp32 add can avoid
    after = dx.cpu().double().numpy()
    e = np.abs((after - dx0.cpu().double().numpy()) - g64)
    assert (e <= elem_bar + 0.5 * _ulp32(after)).all(), int((e > elem_bar + 0.5 * _ulp32(after)).sum())
    assert not torch.equal(dx, dx0)
    if mask is not None:
        off = (md == 0)
        assert bool(off.any()) and torch.equal(dx[off].view(torch.int32), dx0[off].view(torch.int32))      # exactly 0 where the mask is 0
        assert not inc[off].any()

    # ---- the weight lives on the device: 0 leaves dx alone, doubling it on the device doubles the increment
    alpha.zero_()
    dx = dx0.clone()
    ops.boundary_loss(xd, phi, alpha, mask=md, dx=dx)
    assert torch.equal(dx, dx0)
    alpha.fill_(0.25)
    one = torch.zeros_like(dx0)
    ops.boundary_loss(xd, phi, alpha, mask=md, dx=one)
    alpha.mul_(2.0)                                      # a device-side write: no host argument changes between the two calls
    two = torch.zeros_like(dx0)
    ops.boundary_loss(xd, phi, alpha, mask=md, dx=two)
    assert bool(one.any()) and torch.equal(two, 2.0 * one)
    with pytest.raises(ValueError):
        ops.boundary_loss(xd, phi, None, mask=md, dx=dx)
    with pytest.raises(ValueError):
        ops.boundary_loss(xd, phi[:1], alpha, mask=md)


# ---------------------------------------------------------------------------------------------------- 3. the step
def _setup(seed=1, noise=1234):
    import bench
    from wtpse_hip.synth import default_hparams
    dev = torch.device(DEV)
    hp = default_hparams(True)
    torch.manual_seed(0)
    nets = bench.build_nets(hp, B // 3, dev, seed=seed)
    if noise is not None:
        for n in nets:
            n.seed_noise(noise)
    return dev, hp, list(nets)


def _batch(dev, seed):
    from wtpse_hip.synth import make_batch
    return make_batch(B, 64, 64, dev, seed=seed)


def _buffers(nets):
    return [torch.cat([b.detach().reshape(-1).double() for b in n.buffers()]) for n in nets]


def _snapshot(ts, nets):
    torch.cuda.synchronize()
    opts = [ts.opt[id(n)] for n in nets]
    return dict(params=[n.flat_params().clone() for n in nets], bufs=_buffers(nets), m=[o.m.clone() for o in opts],
                v=[o.v.clone() for o in opts], t=[o.t for o in opts], ctr=[int(n._noise_ctr.item()) for n in nets])


def _assert_same(a, b, keys=("params", "bufs", "m", "v")):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), "%s of network %d differs" % (k, i)
    assert a["t"] == b["t"] and a["ctr"] == b["ctr"]


def _host_bd(logits, target, mask):
    """(L_B float64 on the device's own phi and logits, its bar as in test_boundary_loss_value_and_gradient)."""
    from wtpse_hip import boundary as bd
    x, t = logits.cpu(), target.cpu()
    m = None if mask is None else mask.cpu()
    phi64 = np.stack([bd.signed_distance_host(p[0]) for p in t.numpy()])[:, None]
    want = bd.boundary_loss_host(x.double().numpy(), phi64, None if m is None else m.double().numpy())
    z = x if m is None else x * m
    M = float(np.mean(np.abs(phi64 / (1.0 + np.exp(-z.double().numpy())))))
    cpu32 = float((torch.sigmoid(z) * torch.from_numpy(phi64).float()).mean())
    return want, max(3.0 * abs(cpu32 - want), math.log2(x.numel()) * 2.0 ** -24 * M)


def test_step_with_zero_weight_changes_nothing_and_reports_the_loss():
    """(a) alpha = 0: two steps with the term leave every network where two steps without it do, bit for bit; bd_od / bd_oc of the first
    step are the specification on that step's own logits (a twin's forward passes) and targets."""
    from wtpse_hip import ops
    from wtpse_hip.boundary import BoundaryLoss
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES, boundary=BoundaryLoss(0.0, 0.0, 1.0))
    assert ts.get_boundary_weight() == 0.0
    dev, hp, plain = _setup()
    tp = TrainStep(*plain, hp, lr=RATES)
    assert tp.get_boundary_weight() is None and tp.bd_alpha is None
    with pytest.raises(ValueError, match="boundary"):
        tp.set_boundary_weight(0.1)
    first = None
    for k in range(2):
        res = ts.step(*_batch(dev, 3 + k))
        ref = tp.step(*_batch(dev, 3 + k))
        assert list(res) == TrainStep.log_names(hp, boundary=True) and list(ref) == TrainStep.log_names(hp)
        for name, v in ref.items():
            assert torch.equal(v, res[name]), name
        first = first or {name: float(res[name]) for name in ("bd_od", "bd_oc")}
    _assert_same(_snapshot(ts, nets), _snapshot(tp, plain))
    # the first step's logits, from a third set of the same networks
    dev, hp, twin = _setup()
    TrainStep(*twin, hp, lr=RATES)                       # (puts the networks into the state a step runs them in)
    image, target_od, target_oc = _batch(dev, 3)
    out = twin[0]._forward_update(image, target_od, image, want_tape=True)[0][0]
    roi, od_pred = ops.roi(image, out)
    out_oc = twin[2]._forward_update(roi, target_oc, roi, want_tape=True)[0][0]
    for name, logits, target, mask in (("bd_od", out, target_od, None), ("bd_oc", out_oc, target_oc, od_pred)):
        want, bar = _host_bd(logits, target, mask)
        print("%s: step %.9g, specification %.9g, bar %.3g" % (name, first[name], want, bar))
        assert abs(first[name] - want) <= bar, (name, first[name], want, bar)
    assert first["bd_od"] != 0.0 and first["bd_oc"] != 0.0


_RUNS = {}


def _run(graph, weights):
    """Three steps with the boundary term and a log; weights: the weight set before each step (None: leave it).  Cached."""
    key = (graph, tuple(weights))
    if key not in _RUNS:
        from wtpse_hip.boundary import BoundaryLoss
        from wtpse_hip.step import TrainStep
        from wtpse_hip.trainer import LossLog
        dev, hp, nets = _setup()
        log = LossLog(dev, TrainStep.log_names(hp, boundary=True))
        ts = TrainStep(*nets, hp, lr=RATES, graph=graph, log=log, boundary=BoundaryLoss(0.05, 0.0, 1.0))
        assert ts.get_boundary_weight() == 0.05
        steps = []
        for k, a in enumerate(weights):
            if a is not None:
                ts.set_boundary_weight(a)
            res = ts.step(*_batch(dev, 20 + k))
            steps.append({name: float(v) for name, v in res.items()})
        sums, flag = log.read()
        _RUNS[key] = (_snapshot(ts, nets), steps, sums, flag)
        ts.close()
    return _RUNS[key]


def test_step_eager_and_plan_agree_and_the_log_sums_the_term():
    """(b) weight 0.05: eager and recorded steps agree bit for bit after three steps, and the log's bd_* sums are the steps' values."""
    se, steps_e, sums_e, flag_e = _run(False, (None, None, None))
    sp, steps_p, sums_p, flag_p = _run("plan", (None, None, None))
    _assert_same(se, sp)
    assert steps_e == steps_p and sums_e == sums_p and flag_e == flag_p == (False, 0)
    for name in ("bd_od", "bd_oc", "seg_od", "seg_oc", "dom_od"):
        total = 0.0
        for s in steps_p:
            total += s[name]
        assert sums_p[name] == total and total == total and total != 0.0, name
    # the term reaches the networks: the same steps without it end elsewhere
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    tp = TrainStep(*nets, hp, lr=RATES)
    for k in range(3):
        tp.step(*_batch(dev, 20 + k))
    s0 = _snapshot(tp, nets)
    assert not torch.equal(s0["params"][0], se["params"][0])
    if bool(tp.last_od_pred.any()):                      # (the cup call's gradient lives inside the ROI mask: an empty ROI passes none)
        assert not torch.equal(s0["params"][2], se["params"][2])


def test_weight_changes_between_replays_without_recording_again():
    """(c) set_boundary_weight between replays: the recorded step follows, and equals an eager run given the same weights."""
    schedule = (None, 0.2, 0.0)
    sp, steps_p, sums_p, _ = _run("plan", schedule)
    se, steps_e, sums_e, _ = _run(False, schedule)
    _assert_same(sp, se)
    assert steps_p == steps_e and sums_p == sums_e
    const, steps_c, _, _ = _run("plan", (None, None, None))
    # the losses are reported unweighted: call A of the step that first runs under the new weight still sees the old parameters ...
    assert steps_c[0] == steps_p[0] and all(steps_c[1][k] == steps_p[1][k] for k in ("seg_od", "dom_od", "bd_od"))
    assert steps_c[2]["seg_od"] != steps_p[2]["seg_od"]                    # ... and the changed weight shows from its Adam step on
    assert not torch.equal(const["params"][0], sp["params"][0])


def test_step_arguments():
    """(d) boundary= with dp= raises; so does a log whose names lack bd_*; so does a weight that is no weight."""
    from wtpse_hip.boundary import BoundaryLoss
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import LossLog
    dev, hp, nets = _setup()
    with pytest.raises(ValueError, match="boundary"):
        TrainStep(*nets, hp, dp=object(), boundary=BoundaryLoss())
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, TrainStep.log_names(hp)), boundary=BoundaryLoss())
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, TrainStep.log_names(hp, boundary=True)))
    ts = TrainStep(*nets, hp, boundary=BoundaryLoss(0.3, 0.0, 1.0))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ts.set_boundary_weight(bad)
    ts.set_boundary_weight(0.125)
    assert ts.get_boundary_weight() == 0.125 == float(ts.bd_alpha.item()) == ts.state_dict()["boundary_weight"]


def test_log_tests_the_boundary_scalar_for_nan():
    """The call's NaN test with the term behind its scalars (check_n | 16): a NaN boundary scalar raises the flag, in both forms, and
    a NaN in a slot the test does not cover does not; the sums take every scalar either way."""
    from wtpse_hip import ops
    dev = torch.device(DEV)
    s = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    nan = float("nan")
    step = torch.full((1,), 7, dtype=torch.int32, device=dev)
    for scalars, check_n, raised in (([1.0, nan], 17, True), ([1.0, 2.0], 17, False), ([nan, 2.0], 17, True),
                                     ([1.0, 2.0, 3.0, nan], 19, True), ([1.0, 2.0, 3.0, 4.0], 19, False), ([1.0, nan, 3.0, 4.0], 19, True),
                                     ([1.0, 2.0, 3.0, 4.0, nan], 19, False), ([1.0, nan], 1, False), ([1.0, 2.0, 3.0, nan], 3, False)):
        acc = torch.zeros(6, dtype=torch.float64, device=dev)
        flag = torch.zeros(2, dtype=torch.int32, device=dev)
        ops.loss_log([s(v) for v in scalars], acc, 0, check_n, flag, step)
        assert flag.tolist() == ([1, 7] if raised else [0, 0]), (scalars, check_n)
        got = acc.tolist()[:len(scalars)]
        assert all((a != a) if (b != b) else a == b for a, b in zip(got, scalars)), (scalars, got)


def test_step_on_frozen_batchnorm():
    """(e) freeze_bn=True with boundary=: the step runs, trains, and leaves the running statistics alone."""
    from wtpse_hip.boundary import BoundaryLoss
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES, freeze_bn=True, boundary=BoundaryLoss(0.05, 0.0, 1.0))
    bufs = _buffers(nets)
    before = [n.flat_params().clone() for n in nets]
    res = ts.step(*_batch(dev, 3))
    vals = {k: float(v) for k, v in res.items()}
    assert all(v == v for v in vals.values()) and vals["bd_od"] != 0.0 and vals["bd_oc"] != 0.0
    for a, b in zip(bufs, _buffers(nets)):
        assert torch.equal(a, b)
    assert all(not torch.equal(n.flat_params(), p0) for n, p0 in zip(nets, before))


# ---------------------------------------------------------------------------------------------------- 4. the run
def _next_batch(dev):
    def next_batch(py_rng, np_rng):
        return _batch(dev, int(np_rng.randint(1 << 20)) + py_rng.randint(0, 1000))
    return next_batch


def test_run_follows_the_schedule_and_resumes_bitwise(tmp_path):
    from wtpse_hip.boundary import BoundaryLoss
    from wtpse_hip.trainer import TrainRun
    sched = BoundaryLoss(0.01, 0.5, 1.0)
    kw = dict(iter_per_epoch=2, max_epoch=3, lr=RATES, graph="plan", seed=7)

    dev, hp, nets = _setup()
    a = TrainRun(*nets, hp, _next_batch(dev), out_dir=str(tmp_path / "a"), boundary=sched, **kw)
    assert a.log.names == a.train_step.log_names(hp, boundary=True)
    ea = []
    for epoch in range(3):
        ea.append(a.train_epoch())
        want = sched.weight_at(epoch)
        assert a.train_step.get_boundary_weight() == want == ea[-1]["boundary_weight"]
        assert float(a.train_step.bd_alpha.item()) == float(np.float32(want))
        assert ea[-1]["sums"]["bd_od"] == ea[-1]["sums"]["bd_od"] != 0.0
    assert [e["boundary_weight"] for e in ea] == [0.01, 0.51, 1.0]
    sa = _snapshot(a.train_step, nets)
    with open(tmp_path / "a" / "train_log.csv") as f:
        header = f.readline().strip().split(",")
    assert header[2:2 + len(a.log.names)] == a.log.names and "bd_od" in header and "bd_oc" in header

    dev, hp, nets1 = _setup()
    b1 = TrainRun(*nets1, hp, _next_batch(dev), boundary=sched, **kw)
    b1.train_epoch()
    b1.train_epoch()
    path = str(tmp_path / "run.pth.tar")
    b1.save(path)
    del b1
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["config"]["boundary"] == {"weight": 0.01, "ramp": 0.5, "cap": 1.0} and saved["train_step"]["boundary_weight"] == 0.51

    dev, hp, nets2 = _setup(seed=5, noise=None)
    b2 = TrainRun.load(path, *nets2, hp, _next_batch(dev), graph="plan")
    assert b2.boundary is not None and b2.boundary.config() == sched.config() and b2.epoch == 2
    assert b2.train_step.get_boundary_weight() == sched.weight_at(2)
    eb = b2.train_epoch()
    _assert_same(sa, _snapshot(b2.train_step, nets2))
    assert eb["sums"] == ea[2]["sums"] and eb["boundary_weight"] == 1.0
