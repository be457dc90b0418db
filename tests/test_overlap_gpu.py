"""The overlap loss on the GPU: wtpse_overlap_loss against the float64 specification (wtpse_hip/overlap.py), its bitwise promises,
TrainStep(overlap=) and TrainRun(overlap=).  Bars and the step tests' sizes follow tests/test_boundary_gpu.py."""
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

# (3, 33, 65): every odd plane starts 4 bytes off a 16-byte boundary and the plane ends in a ragged group; (2, 100, 257): seven
# workgroups per plane; (2, 256, 256): the training geometry, sixteen
SHAPES = [(1, 1, 1), (3, 1, 7), (2, 5, 64), (3, 33, 65), (6, 64, 64), (2, 100, 257), (2, 256, 256)]
f32 = lambda v: float(np.float32(v))           # the kernel takes its four parameters as fp32: the specification gets the same numbers
CONFIGS = {"dice": dict(fp=0.5, fn=0.5, focal=1.0, smooth=1.0), "focal_tversky": dict(fp=f32(0.3), fn=f32(0.7), focal=0.75, smooth=1.0),
           "focal2": dict(fp=f32(0.7), fn=f32(0.3), focal=2.0, smooth=f32(0.1))}


def _cfg(name):
    from wtpse_hip.overlap import OverlapLoss
    return OverlapLoss(**CONFIGS[name])


def _ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32)


_CASES = {}


def _case(shape, masked):
    """x = 3 * randn, disc-shaped targets (a radius per plane), a random 60 % mask; host tensors, made once."""
    key = (shape, masked)
    if key not in _CASES:
        Bn, h, w = shape
        yy, xx = np.mgrid[0:h, 0:w]
        t = np.stack([((yy - (h - 1) / 2) ** 2 + (xx - (w - 1) / 2) ** 2 <= ((0.15 + 0.07 * k) * min(h, w)) ** 2) for k in range(Bn)])
        t = torch.from_numpy(t.astype(np.float32)[:, None])
        g = torch.Generator().manual_seed(100 * h + w + int(masked))
        x = torch.randn(t.shape, generator=g) * 3.0
        mask = (torch.rand(t.shape, generator=g) < 0.6).float() if masked else None
        _CASES[key] = (x, t, mask)
    return _CASES[key]


def _torch_planes(x, t, m, fp, fn, focal, smooth):
    """The definition restated in torch, in the precision of its inputs (tests/test_overlap_cpu.py holds it equal to the
    specification in float64)."""
    Bn = x.shape[0]
    z = x if m is None else x * m
    mm = torch.ones_like(x) if m is None else m
    s = torch.sigmoid(z)
    tp = (mm * s * t).reshape(Bn, -1).sum(1)
    fpos = (mm * s * (1 - t)).reshape(Bn, -1).sum(1)
    fneg = (mm * (1 - s) * t).reshape(Bn, -1).sum(1)
    u = 1 - (tp + smooth) / (tp + fp * fpos + fn * fneg + smooth)
    dead = u <= 0
    safe = torch.where(dead, torch.ones_like(u), u)
    return torch.where(dead, torch.zeros_like(u), safe if focal == 1.0 else safe ** focal)


_REF = {}


def _reference(shape, masked, cfg, w32):
    """(planes64, loss64, grad64, planes32, loss32, grad32): the float64 specification and the fp32 restatement on the CPU, once."""
    key = (shape, masked, cfg, w32)
    if key not in _REF:
        from wtpse_hip import overlap as ov
        kw = CONFIGS[cfg]
        x, t, mask = _case(shape, masked)
        x64, t64 = x.double().numpy(), t.double().numpy()
        m64 = None if mask is None else mask.double().numpy()
        xr = x.clone().requires_grad_(True)
        p32 = _torch_planes(xr, t, mask, **kw)
        (torch.tensor(w32) * p32.mean()).backward()
        _REF[key] = (ov.overlap_planes_host(x64, t64, m64, **kw), ov.overlap_loss_host(x64, t64, m64, **kw),
                     ov.overlap_grad_host(x64, t64, w32, m64, **kw), p32.detach().double().numpy(), float(p32.detach().mean()),
                     xr.grad.double().numpy())
    return _REF[key]


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_overlap_loss_value_and_gradient(shape, masked):
    from wtpse_hip import ops
    x, t, mask = _case(shape, masked)
    xd, td, md = x.to(DEV), t.to(DEV), None if mask is None else mask.to(DEV)
    w_dev = torch.full((1,), 0.37, dtype=torch.float32, device=DEV)
    w32 = float(w_dev.item())
    dx0 = (torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) * 1e-3).to(DEV)
    dx0.view(-1)[0] = -0.0
    for name in CONFIGS:
        cfg = _cfg(name)
        planes64, loss64, g64, planes32, loss32, g32 = _reference(shape, masked, name, w32)

        # ---- per-plane loss and mean: max(3 x the fp32 restatement's error, 2 ulp fp32 of the specification)
        loss, planes = ops.overlap_loss(xd, td, None, cfg, mask=md, want_planes=True)
        assert loss.dim() == 0 and planes.shape == (shape[0],)
        e = np.abs(planes.cpu().double().numpy() - planes64)
        bar = np.maximum(3.0 * np.abs(planes32 - planes64), 2.0 * _ulp32(planes64))
        print("overlap_loss %s %s %s: plane losses %s, max |gpu - f64| %.3g ulp, fp32 restatement %.3g ulp"
              % (shape, "cup" if masked else "disc", name, planes64, float((e / _ulp32(planes64)).max()),
                 float((np.abs(planes32 - planes64) / _ulp32(planes64)).max())))
        assert (e <= bar).all(), (e, bar)
        e, bar = abs(float(loss) - loss64), max(3.0 * abs(loss32 - loss64), 2.0 * float(_ulp32(loss64)))
        print("  mean %.9g: |gpu - f64| %.3g ulp, fp32 restatement %.3g ulp" % (loss64, e / _ulp32(loss64), abs(loss32 - loss64) / _ulp32(loss64)))
        assert e <= bar, (e, bar)

        # ---- the increment into zeros: what is stored IS the increment
        elem_bar = np.maximum(3.0 * np.abs(g32 - g64), 2.0 * _ulp32(g64))
        inc = torch.zeros_like(dx0)
        loss_dx, planes_dx = ops.overlap_loss(xd, td, w_dev, cfg, mask=md, dx=inc, want_planes=True)
        e = np.abs(inc.cpu().double().numpy() - g64)
        print("  increment into zeros: max |err| / bar = %.3g, max err %.3g ulp" % (float((e / elem_bar).max()) if elem_bar.all() else -1.0,
                                                                                float((e / _ulp32(g64)).max())))
        assert (e <= elem_bar).all(), int((e > elem_bar).sum())
        live = bool((g64 != 0).any())                      # (a 1 x 1 plane under a mask of 0 has no gradient at all)
        assert bool(inc.any()) == live
        # the same bits with dx null and non-null, and again
        assert torch.equal(_bits(loss), _bits(loss_dx)) and torch.equal(_bits(planes), _bits(planes_dx))
        again = torch.zeros_like(dx0)
        loss2, planes2 = ops.overlap_loss(xd, td, w_dev, cfg, mask=md, dx=again, want_planes=True)
        assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(planes), _bits(planes2)) and torch.equal(_bits(inc), _bits(again))
        assert torch.equal(_bits(ops.overlap_loss(xd, td, None, cfg, mask=md)), _bits(loss))           # (without the plane array)

        # ---- into a known tensor: after - before (exact in float64) is the increment up to the ONE rounding of the stored sum
        dx = dx0.clone()
        dx.wt_amax = object()                              # an amax table of the region loss's gradient would be stale now
        ops.overlap_loss(xd, td, w_dev, cfg, mask=md, dx=dx)
        assert dx.wt_amax is None
        after = dx.cpu().double().numpy()
        e = np.abs((after - dx0.cpu().double().numpy()) - g64)
        assert (e <= elem_bar + 0.5 * _ulp32(after)).all(), int((e > elem_bar + 0.5 * _ulp32(after)).sum())
        assert torch.equal(dx, dx0) != live
        if md is not None:
            off = (md == 0)
            if bool(off.any()):                            # exactly 0 where the mask is 0
                assert torch.equal(_bits(dx[off]), _bits(dx0[off])) and not inc[off].any()
            assert bool(off.any()) or x.numel() < 8

        # ---- reversing the order of the planes reverses plane_loss bit for bit and moves the increments with it
        rev = torch.zeros_like(dx0)
        mr = None if md is None else md.flip(0).contiguous()
        _, planes_r = ops.overlap_loss(xd.flip(0).contiguous(), td.flip(0).contiguous(), w_dev, cfg, mask=mr, dx=rev, want_planes=True)
        assert torch.equal(_bits(planes_r.flip(0)), _bits(planes)), (planes_r.flip(0) - planes)
        assert torch.equal(_bits(rev.flip(0)), _bits(inc)), int((_bits(rev.flip(0)) != _bits(inc)).sum())

    # ---- the weight lives on the device: 0 leaves dx bit for bit (a -0.0 included), doubling it doubles the increment exactly
    cfg = _cfg("focal_tversky")
    w_dev.zero_()
    dx = dx0.clone()
    ops.overlap_loss(xd, td, w_dev, cfg, mask=md, dx=dx)
    assert torch.equal(_bits(dx), _bits(dx0))
    w_dev.fill_(0.25)
    one = torch.zeros_like(dx0)
    ops.overlap_loss(xd, td, w_dev, cfg, mask=md, dx=one)
    w_dev.mul_(2.0)                                        # a device-side write: no host argument changes between the two calls
    two = torch.zeros_like(dx0)
    ops.overlap_loss(xd, td, w_dev, cfg, mask=md, dx=two)
    assert bool(one.any()) == live and torch.equal(_bits(two), _bits(2.0 * one))


def test_edge_planes_among_ordinary_ones():
    """focal 0.75 (the derivative's power has exponent -0.25): an empty target with x = -1e4, a fully masked plane and an
    all-foreground target with x = +1e4 have loss 0 and an all-zero increment; nothing is NaN; the ordinary planes are untouched
    by their neighbours."""
    from wtpse_hip import ops
    from wtpse_hip import overlap as ov
    x, t, mask = (v.clone() for v in _case((3, 33, 65), True))
    x, t, mask = (torch.cat([v, v[:2]]) for v in (x, t, mask))               # planes 0, 2 ordinary; 1, 3, 4 become the edge planes
    x[1], t[1] = -1e4, 0.0
    mask[3] = 0.0
    x[4], t[4] = 1e4, 1.0
    cfg = _cfg("focal_tversky")
    w_dev = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
    inc = torch.zeros(x.shape, device=DEV)
    loss, planes = ops.overlap_loss(x.to(DEV), t.to(DEV), w_dev, cfg, mask=mask.to(DEV), dx=inc, want_planes=True)
    planes, inc = planes.cpu(), inc.cpu()
    assert not torch.isnan(planes).any() and not torch.isnan(inc).any() and not math.isnan(float(loss))
    for k in (1, 3, 4):
        assert float(planes[k]) == 0.0 and not inc[k].any(), k
    for k in (0, 2):
        assert float(planes[k]) > 0.0 and bool(inc[k].any()), k
    want = ov.overlap_planes_host(x.double().numpy(), t.double().numpy(), mask.double().numpy(), **CONFIGS["focal_tversky"])
    assert (want[[1, 3, 4]] == 0).all()
    assert (np.abs(planes.double().numpy() - want) <= 2.0 * _ulp32(want)).all()
    # the same three without a mask where they need none
    inc = torch.zeros(x.shape, device=DEV)
    _, planes = ops.overlap_loss(x.to(DEV), t.to(DEV), w_dev, cfg, dx=inc, want_planes=True)
    assert float(planes[1]) == 0.0 and float(planes[4]) == 0.0 and not inc[1].any() and not inc[4].any() and not torch.isnan(inc).any()


def test_bad_arguments():
    from wtpse_hip import ops
    cfg = _cfg("dice")
    x = torch.zeros(2, 1, 4, 4, device=DEV)
    w = torch.ones(1, device=DEV)
    with pytest.raises(ValueError, match="w_dev"):
        ops.overlap_loss(x, x, None, cfg, dx=torch.zeros_like(x))
    for bad in (dict(t=x[:1]), dict(mask=x[:1]), dict(dx=x[:1].clone())):
        kw = dict(t=x, mask=None, dx=None)
        kw.update(bad)
        with pytest.raises(ValueError, match="elements"):
            ops.overlap_loss(x, kw["t"], w, cfg, mask=kw["mask"], dx=kw["dx"])
    with pytest.raises(ValueError):
        ops.overlap_loss(x.double(), x, w, cfg)
    with pytest.raises(ValueError):
        ops.overlap_loss(x.cpu(), x, w, cfg)
    with pytest.raises(ValueError):
        ops.overlap_loss(x[:, :, :, ::2], x[:, :, :, :2].contiguous(), w, cfg)
    with pytest.raises(ValueError):
        ops.overlap_loss(torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), w, cfg)
    with pytest.raises(ValueError):
        ops.overlap_loss(torch.zeros(0, 4, device=DEV), torch.zeros(0, 4, device=DEV), w, cfg)
    assert float(ops.overlap_loss(x, x, None, cfg)) > 0.0                  # [B, 1, H, W] and [B, hw] are both planes
    assert torch.equal(ops.overlap_loss(x.view(2, 16), x.view(2, 16), None, cfg), ops.overlap_loss(x, x, None, cfg))


def test_log_tests_the_overlap_scalar_for_nan():
    """The call's NaN test with one more scalar (check_n | 32): a NaN in the covered slot raises the flag, a NaN behind it does not;
    the values in use before behave as before."""
    from wtpse_hip import ops
    dev = torch.device(DEV)
    s = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    nan = float("nan")
    step = torch.full((1,), 7, dtype=torch.int32, device=dev)
    for scalars, check_n, raised in (([1.0, 2.0, 3.0, nan], 35, True), ([1.0, 2.0, 3.0, 4.0], 35, False), ([1.0, 2.0, 3.0, 4.0, nan], 35, False),
                                     ([1.0, 2.0, nan], 49, True), ([1.0, nan, 3.0], 49, True), ([1.0, 2.0, 3.0, nan], 49, False),
                                     ([1.0, 2.0, 3.0], 49, False),
                                     ([1.0, 2.0, 3.0, 4.0, nan], 51, True), ([1.0, 2.0, 3.0, nan, 5.0], 51, True),
                                     ([1.0, 2.0, 3.0, 4.0, 5.0, nan], 51, False), ([1.0, 2.0, 3.0, 4.0, 5.0], 51, False),
                                     ([float("inf"), 2.0, 3.0, 4.0, -float("inf")], 51, True),
                                     ([1.0, 2.0, nan], 17, False), ([1.0, 2.0, 3.0, 4.0, nan], 19, False), ([1.0, nan], 17, True)):
        acc = torch.zeros(6, dtype=torch.float64, device=dev)
        flag = torch.zeros(2, dtype=torch.int32, device=dev)
        ops.loss_log([s(v) for v in scalars], acc, 0, check_n, flag, step)
        assert flag.tolist() == ([1, 7] if raised else [0, 0]), (scalars, check_n)
        got = acc.tolist()[:len(scalars)]
        assert all((a != a) if (b != b) else a == b for a, b in zip(got, scalars)), (scalars, got)


# ---------------------------------------------------------------------------------------------------- 2. the step
def _setup(seed=1, noise=1234, full=True):
    import bench
    from wtpse_hip.synth import default_hparams
    dev = torch.device(DEV)
    hp = default_hparams(full)
    torch.manual_seed(0)
    nets = bench.build_nets(hp, B // 3, dev, seed=seed)
    if noise is not None:
        for n in nets:
            if n is not None:
                n.seed_noise(noise)
    return dev, hp, list(nets)


def _batch(dev, seed):
    from wtpse_hip.synth import make_batch
    return make_batch(B, 64, 64, dev, seed=seed)


def _buffers(nets):
    return [torch.cat([b.detach().reshape(-1).double() for b in n.buffers()]) for n in nets]


def _snapshot(ts, nets):
    torch.cuda.synchronize()
    nets = [n for n in nets if n is not None]
    opts = [ts.opt[id(n)] for n in nets]
    return dict(params=[n.flat_params().clone() for n in nets], bufs=_buffers(nets), m=[o.m.clone() for o in opts],
                v=[o.v.clone() for o in opts], t=[o.t for o in opts], ctr=[int(n._noise_ctr.item()) for n in nets])


def _assert_same(a, b, keys=("params", "bufs", "m", "v")):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), "%s of network %d differs" % (k, i)
    assert a["t"] == b["t"] and a["ctr"] == b["ctr"]


STEP_CFG = dict(fp=f32(0.3), fn=f32(0.7), focal=0.75, smooth=1.0)


def _host_ov(logits, target, mask):
    """(L_ov float64 on the device's own logits, its bar as in test_overlap_loss_value_and_gradient)."""
    from wtpse_hip import overlap as ov
    x, t = logits.cpu(), target.cpu()
    m = None if mask is None else mask.cpu()
    want = ov.overlap_loss_host(x.double().numpy(), t.double().numpy(), None if m is None else m.double().numpy(), **STEP_CFG)
    cpu32 = float(_torch_planes(x, t, m, **STEP_CFG).mean())
    return want, max(3.0 * abs(cpu32 - want), 2.0 * float(_ulp32(want)))


def test_step_with_zero_weight_changes_nothing_and_reports_the_loss():
    """(a) w = 0: two steps with the term leave every network where two steps without it do, bit for bit; ov_od / ov_oc of the first
    step are the specification on that step's own logits (a twin's forward passes) and targets."""
    from wtpse_hip import ops
    from wtpse_hip.overlap import OverlapLoss
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES, overlap=OverlapLoss(0.0, **STEP_CFG))
    assert ts.get_overlap_weight() == 0.0
    dev, hp, plain = _setup()
    tp = TrainStep(*plain, hp, lr=RATES)
    assert tp.get_overlap_weight() is None and tp.ov_w is None
    with pytest.raises(ValueError, match="overlap"):
        tp.set_overlap_weight(0.1)
    first = None
    for k in range(2):
        res = ts.step(*_batch(dev, 3 + k))
        ref = tp.step(*_batch(dev, 3 + k))
        assert list(res) == TrainStep.log_names(hp, overlap=True) and list(ref) == TrainStep.log_names(hp)
        for name, v in ref.items():
            assert torch.equal(v, res[name]), name
        first = first or {name: float(res[name]) for name in ("ov_od", "ov_oc")}
    _assert_same(_snapshot(ts, nets), _snapshot(tp, plain))
    # the first step's logits, from a third set of the same networks
    dev, hp, twin = _setup()
    TrainStep(*twin, hp, lr=RATES)                       # (puts the networks into the state a step runs them in)
    image, target_od, target_oc = _batch(dev, 3)
    out = twin[0]._forward_update(image, target_od, image, want_tape=True)[0][0]
    roi, od_pred = ops.roi(image, out)
    out_oc = twin[2]._forward_update(roi, target_oc, roi, want_tape=True)[0][0]
    for name, logits, target, mask in (("ov_od", out, target_od, None), ("ov_oc", out_oc, target_oc, od_pred)):
        want, bar = _host_ov(logits, target, mask)
        print("%s: step %.9g, specification %.9g, bar %.3g" % (name, first[name], want, bar))
        assert abs(first[name] - want) <= bar, (name, first[name], want, bar)
    assert first["ov_od"] > 0.0 and first["ov_oc"] >= 0.0


_RUNS = {}


def _run(graph, weights, boundary=False):
    """Three steps with the overlap term (and the boundary term) and a log; weights: the weight set before each step (None: leave
    it).  Cached."""
    key = (graph, tuple(weights), boundary)
    if key not in _RUNS:
        from wtpse_hip.boundary import BoundaryLoss
        from wtpse_hip.overlap import OverlapLoss
        from wtpse_hip.step import TrainStep
        from wtpse_hip.trainer import LossLog
        dev, hp, nets = _setup()
        log = LossLog(dev, TrainStep.log_names(hp, boundary=boundary, overlap=True))
        ts = TrainStep(*nets, hp, lr=RATES, graph=graph, log=log, overlap=OverlapLoss(0.5, **STEP_CFG),
                       boundary=BoundaryLoss(0.05, 0.0, 1.0) if boundary else None)
        assert ts.get_overlap_weight() == 0.5
        steps = []
        for k, a in enumerate(weights):
            if a is not None:
                ts.set_overlap_weight(a)
            res = ts.step(*_batch(dev, 20 + k))
            steps.append({name: float(v) for name, v in res.items()})
        sums, flag = log.read()
        _RUNS[key] = (_snapshot(ts, nets), steps, sums, flag)
        ts.close()
    return _RUNS[key]


def test_step_eager_and_plan_agree_and_the_log_sums_the_term():
    """(b) weight 0.5: eager and recorded steps agree bit for bit after three steps, and the log's ov_* sums are the steps' values."""
    se, steps_e, sums_e, flag_e = _run(False, (None, None, None))
    sp, steps_p, sums_p, flag_p = _run("plan", (None, None, None))
    _assert_same(se, sp)
    assert steps_e == steps_p and sums_e == sums_p and flag_e == flag_p == (False, 0)
    for name in ("ov_od", "ov_oc", "seg_od", "seg_oc", "dom_od"):
        total = 0.0
        for s in steps_p:
            total += s[name]
        # (ov_oc may be 0: freshly initialised networks leave the cup call's ROI mask empty, and a fully masked plane has loss 0)
        assert sums_p[name] == total and total == total and (total != 0.0 or name == "ov_oc"), name
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
    """(c) set_overlap_weight between replays: the recorded step follows, and equals an eager run given the same weights."""
    schedule = (None, 2.0, 0.0)
    sp, steps_p, sums_p, _ = _run("plan", schedule)
    se, steps_e, sums_e, _ = _run(False, schedule)
    _assert_same(sp, se)
    assert steps_p == steps_e and sums_p == sums_e
    const, steps_c, _, _ = _run("plan", (None, None, None))
    # the losses are reported unweighted: call A of the step that first runs under the new weight still sees the old parameters ...
    assert steps_c[0] == steps_p[0] and all(steps_c[1][k] == steps_p[1][k] for k in ("seg_od", "dom_od", "ov_od"))
    assert steps_c[2]["seg_od"] != steps_p[2]["seg_od"]                    # ... and the changed weight shows from its Adam step on
    assert not torch.equal(const["params"][0], sp["params"][0])


def test_boundary_and_overlap_together():
    """Both terms: eager == plan bit for bit, ov_* directly behind bd_*, and the result differs from overlap alone."""
    from wtpse_hip.step import TrainStep
    se, steps_e, sums_e, flag_e = _run(False, (None, None, None), boundary=True)
    sp, steps_p, sums_p, flag_p = _run("plan", (None, None, None), boundary=True)
    _assert_same(se, sp)
    assert steps_e == steps_p and sums_e == sums_p and flag_e == flag_p == (False, 0)
    names = list(steps_p[0])
    assert names == TrainStep.log_names({"whitening": True}, boundary=True, overlap=True)
    assert names.index("ov_od") == names.index("bd_od") + 1 and names.index("ov_oc") == names.index("bd_oc") + 1
    alone, steps_a, _, _ = _run("plan", (None, None, None))
    assert steps_a[0]["ov_od"] == steps_p[0]["ov_od"]                      # (the first call A sees the same parameters)
    assert not torch.equal(alone["params"][0], sp["params"][0])


def test_step_arguments():
    """(d) overlap= with dp= raises; so does a log whose names lack ov_*; so does a weight that is no weight."""
    from wtpse_hip.overlap import OverlapLoss
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import LossLog
    dev, hp, nets = _setup()
    with pytest.raises(ValueError, match="overlap"):
        TrainStep(*nets, hp, dp=object(), overlap=OverlapLoss())
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, TrainStep.log_names(hp)), overlap=OverlapLoss())
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, TrainStep.log_names(hp, overlap=True)))
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, TrainStep.log_names(hp, boundary=True)), overlap=OverlapLoss())
    ts = TrainStep(*nets, hp, overlap=OverlapLoss(0.3))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ts.set_overlap_weight(bad)
    ts.set_overlap_weight(0.125)
    sd = ts.state_dict()
    assert ts.get_overlap_weight() == 0.125 == float(ts.ov_w.item()) == sd["overlap_weight"] and "boundary_weight" not in sd
    # a state from before the field loads unchanged
    ts.set_overlap_weight(0.75)
    ts.load_state_dict({k: v for k, v in sd.items() if k != "overlap_weight"})
    assert ts.get_overlap_weight() == 0.75
    ts.load_state_dict(sd)
    assert ts.get_overlap_weight() == 0.125 == float(ts.ov_w.item())


@pytest.mark.parametrize("full", [True, False], ids=["whitening", "plain"])
@pytest.mark.parametrize("boundary", [False, True], ids=["alone", "with_boundary"])
def test_nan_overlap_scalar_raises_the_flag_and_holds_adam(monkeypatch, full, boundary):
    """The overlap scalar is part of its call's NaN test in all four layouts of the call's scalars: when it alone is NaN, the log's
    flag goes up with the iteration and no Adam launch changes anything; a finite step before it trains as usual."""
    from wtpse_hip import ops
    from wtpse_hip.boundary import BoundaryLoss
    from wtpse_hip.overlap import OverlapLoss
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import LossLog
    dev, hp, nets = _setup(full=full)
    log = LossLog(dev, TrainStep.log_names(hp, boundary=boundary, overlap=True))
    ts = TrainStep(*nets, hp, lr=RATES, log=log, overlap=OverlapLoss(0.5), boundary=BoundaryLoss(0.05, 0.0, 1.0) if boundary else None)
    before = _snapshot(ts, nets)
    res = ts.step(*_batch(dev, 3))
    assert all(float(v) == float(v) for v in res.values()) and list(res) == list(log.names)
    good = _snapshot(ts, nets)
    # (the disc network: with an empty ROI mask and no whitening terms the cup network has no gradient to move by)
    assert log.read()[1] == (False, 0) and not torch.equal(before["params"][0], good["params"][0])
    real = ops.overlap_loss

    def poisoned(*a, **kw):
        loss = real(*a, **kw)
        return loss.fill_(float("nan"))
    monkeypatch.setattr(ops, "overlap_loss", poisoned)
    res = ts.step(*_batch(dev, 4))
    assert float(res["seg_od"]) == float(res["seg_od"]) and float(res["ov_od"]) != float(res["ov_od"])
    sums, flag = log.read()
    assert flag == (True, 1), flag                       # raised by call A of the second iteration
    held = _snapshot(ts, nets)
    for k in ("params", "m", "v"):
        for a, b in zip(good[k], held[k]):
            assert torch.equal(a, b), k


def test_step_on_frozen_batchnorm():
    """(e) freeze_bn=True with overlap=: the step runs, trains, and leaves the running statistics alone."""
    from wtpse_hip.overlap import OverlapLoss
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES, freeze_bn=True, overlap=OverlapLoss(0.5, **STEP_CFG))
    bufs = _buffers(nets)
    before = [n.flat_params().clone() for n in nets]
    res = ts.step(*_batch(dev, 3))
    vals = {k: float(v) for k, v in res.items()}
    assert all(v == v for v in vals.values()) and vals["ov_od"] > 0.0 and vals["ov_oc"] >= 0.0
    for a, b in zip(bufs, _buffers(nets)):
        assert torch.equal(a, b)
    assert all(not torch.equal(n.flat_params(), p0) for n, p0 in zip(nets, before))


# ---------------------------------------------------------------------------------------------------- 3. the run
def _next_batch(dev):
    def next_batch(py_rng, np_rng):
        return _batch(dev, int(np_rng.randint(1 << 20)) + py_rng.randint(0, 1000))
    return next_batch


def test_run_follows_the_schedule_and_resumes_bitwise(tmp_path):
    from wtpse_hip.overlap import OverlapLoss
    from wtpse_hip.trainer import TrainRun
    sched = OverlapLoss(0.25, ramp=0.5, cap=1.0, **STEP_CFG)
    kw = dict(iter_per_epoch=2, max_epoch=3, lr=RATES, graph="plan", seed=7)

    dev, hp, nets = _setup()
    a = TrainRun(*nets, hp, _next_batch(dev), out_dir=str(tmp_path / "a"), overlap=sched, **kw)
    assert a.log.names == a.train_step.log_names(hp, overlap=True)
    ea = []
    for epoch in range(3):
        ea.append(a.train_epoch())
        want = sched.weight_at(epoch)
        assert a.train_step.get_overlap_weight() == want == ea[-1]["overlap_weight"] and "boundary_weight" not in ea[-1]
        assert float(a.train_step.ov_w.item()) == float(np.float32(want))
        assert ea[-1]["sums"]["ov_od"] == ea[-1]["sums"]["ov_od"] != 0.0
    assert [e["overlap_weight"] for e in ea] == [0.25, 0.75, 1.0]
    sa = _snapshot(a.train_step, nets)
    with open(tmp_path / "a" / "train_log.csv") as f:
        header = f.readline().strip().split(",")
    assert header[2:2 + len(a.log.names)] == a.log.names and "ov_od" in header and "ov_oc" in header

    dev, hp, nets1 = _setup()
    b1 = TrainRun(*nets1, hp, _next_batch(dev), overlap=sched.config(), **kw)      # the dict form
    b1.train_epoch()
    b1.train_epoch()
    path = str(tmp_path / "run.pth.tar")
    b1.save(path)
    del b1
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["config"]["overlap"] == sched.config() and saved["config"]["boundary"] == {}
    assert saved["train_step"]["overlap_weight"] == 0.75

    dev, hp, nets2 = _setup(seed=5, noise=None)
    b2 = TrainRun.load(path, *nets2, hp, _next_batch(dev), graph="plan")
    assert b2.overlap is not None and b2.overlap.config() == sched.config() and b2.epoch == 2 and b2.boundary is None
    assert b2.train_step.get_overlap_weight() == sched.weight_at(2)
    eb = b2.train_epoch()
    _assert_same(sa, _snapshot(b2.train_step, nets2))
    assert eb["sums"] == ea[2]["sums"] and eb["overlap_weight"] == 1.0
