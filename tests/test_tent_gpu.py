"""Test-time entropy minimisation on the GPU (-m gpu): wtpse_entropy_loss against the float64 specification (wtpse_hip/tent.py) and
its bitwise promises, wtpse_adam_index against wtpse_adam_dev, the taped prediction path and its backward (against predict(), against
the update backward on the plain branch, against the CPU oracle in float64 with the shape prior), the affine-only switch, TentStep,
and the program end to end.  Bars: tests/test_overlap_gpu.py's for the kernel, tests/test_parity_gpu.py's assert_calibrated for the
network gradients."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

from oracle import wtpse_cpu as O
from oracle.filler import fill_state_dict
from oracle.inputs import make_inputs
from test_parity_gpu import CAL, HP, SEED_W, assert_calibrated, build_nets, oracle_grads, perturbed

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
GEOMETRIES = [(3, 32), (6, 64)]                       # (B, H) as tests/test_parity_gpu.py uses them


def _ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ==================================================================================================== kernel level
# (3,1,33,65): every odd plane starts off a 16-byte boundary, one workgroup per plane; (3,1,96,96): three workgroups per plane,
# aligned; (2,1,95,97): three workgroups, the second plane unaligned, a ragged last group
SHAPES = [(3, 1, 33, 65), (3, 1, 96, 96), (2, 1, 95, 97)]
_CASES = {}


def _case(shape, masked):
    """x = 3 randn, a random 60 % {0,1} mask; host tensors and the two host references, made once."""
    key = (shape, masked)
    if key not in _CASES:
        from wtpse_hip import tent
        g = torch.Generator().manual_seed(100 * shape[2] + shape[3] + int(masked))
        x = torch.randn(shape, generator=g) * 3.0
        mask = (torch.rand(shape, generator=g) < 0.6).float() if masked else None
        xn, mn = x.double().numpy(), None if mask is None else mask.double().numpy()
        H64 = tent.entropy_planes_host(xn, mn)[0]
        ref64 = (H64, tent.tent_loss_host(xn, mn), tent.tent_grad_host(xn, mn))
        H32, loss32, g32 = tent.entropy_fp32(xn, mn)
        _CASES[key] = (x, mask, ref64, (H32.astype(np.float64), float(loss32), g32.astype(np.float64)))
    return _CASES[key]


@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entropy_loss_value_and_gradient(shape, masked):
    """Per plane, the mean and every gradient element: max(3 x |fp32 restatement - f64|, 2 ulp fp32 of the specification)."""
    from wtpse_hip import ops
    x, mask, (H64, loss64, g64), (H32, loss32, g32) = _case(shape, masked)
    xd, md = x.to(DEV), None if mask is None else mask.to(DEV)
    loss, dx, planes, sel = ops.entropy_loss(xd, md, want_planes=True)
    assert loss.dim() == 0 and planes.shape == (shape[0],) and sel.dtype == torch.int32 and dx.shape == x.shape
    assert sel.cpu().tolist() == [1] * shape[0]
    e = np.abs(planes.cpu().double().numpy() - H64)
    bar = np.maximum(3.0 * np.abs(H32 - H64), 2.0 * _ulp32(H64))
    print("entropy_loss %s %s: plane entropies %s, max |gpu - f64| %.3g ulp, fp32 restatement %.3g ulp"
          % (shape, "cup" if masked else "disc", H64, float((e / _ulp32(H64)).max()), float((np.abs(H32 - H64) / _ulp32(H64)).max())))
    assert (e <= bar).all(), (e, bar)
    e, bar = abs(float(loss) - loss64), max(3.0 * abs(loss32 - loss64), 2.0 * float(_ulp32(loss64)))
    print("  loss %.9g: |gpu - f64| %.3g ulp, fp32 restatement %.3g ulp" % (loss64, e / _ulp32(loss64), abs(loss32 - loss64) / _ulp32(loss64)))
    assert e <= bar, (e, bar)
    elem_bar = np.maximum(3.0 * np.abs(g32 - g64), 2.0 * _ulp32(g64))
    e = np.abs(dx.cpu().double().numpy() - g64)
    print("  gradient: max err %.3g ulp, fp32 restatement %.3g ulp"
          % (float((e / _ulp32(g64)).max()), float((np.abs(g32 - g64) / _ulp32(g64)).max())))
    assert (e <= elem_bar).all(), int((e > elem_bar).sum())
    assert bool(dx.any())
    if md is not None:
        assert not dx[md == 0].any()                                        # nothing where the mask is 0
    # every element is WRITTEN: the same bits into a buffer that held something else; the value alone without a gradient
    again = ops.entropy_loss(xd, md, want_planes=True)
    assert all(_same(a, b) for a, b in zip(again, (loss, dx, planes, sel)))
    only, none = ops.entropy_loss(xd, md, want_grad=False)
    assert none is None and _same(only, loss)
    # reversing the order of the planes reverses the planes bit for bit and moves the gradients with them
    mr = None if md is None else md.flip(0).contiguous()
    _, dx_r, planes_r, _ = ops.entropy_loss(xd.flip(0).contiguous(), mr, want_planes=True)
    assert _same(planes_r.flip(0), planes) and _same(dx_r.flip(0), dx)
    # [B, 1, H, W] and [B, hw] are both planes
    assert _same(ops.entropy_loss(xd.reshape(shape[0], -1), None if md is None else md.reshape(shape[0], -1))[1].reshape(shape), dx)


def test_selection_by_the_margin():
    """Planes of Gaussian logits of scale 1, 8, 8 and 2 have entropies 0.60, 0.16, 0.16 and 0.47 nats: far from 0.4 ln 2 = 0.2773."""
    from wtpse_hip import ops, tent
    g = torch.Generator().manual_seed(9)
    x = torch.randn((4, 1, 48, 50), generator=g) * torch.tensor([1.0, 8.0, 8.0, 2.0]).reshape(4, 1, 1, 1)
    xn = x.double().numpy()
    H64, sel64, _ = tent.entropy_planes_host(xn, None, tent.EATA_MARGIN)
    assert list(sel64) == [False, True, True, False] and np.abs(H64 - tent.EATA_MARGIN).min() > 0.05
    for reweight in (False, True):
        loss, dx, planes, sel = ops.entropy_loss(x.to(DEV), None, tent.EATA_MARGIN, reweight, want_planes=True)
        assert sel.cpu().tolist() == [0, 1, 1, 0]
        for b in (0, 3):                                                    # bitwise +0.0
            assert not _bits(dx[b]).any(), b
        g64 = tent.tent_grad_host(xn, None, tent.EATA_MARGIN, reweight)
        e = np.abs(dx.cpu().double().numpy() - g64)
        assert (e <= 2.0 * _ulp32(g64)).all() and bool(dx[1].any()) and bool(dx[2].any())
        loss64 = tent.tent_loss_host(xn, None, tent.EATA_MARGIN, reweight)
        assert abs(float(loss) - loss64) <= 2.0 * float(_ulp32(loss64))
        assert (np.abs(planes.cpu().double().numpy() - H64) <= 2.0 * _ulp32(H64)).all()
    # without a margin every plane is selected
    assert ops.entropy_loss(x.to(DEV), want_planes=True)[3].cpu().tolist() == [1, 1, 1, 1]


def test_edge_planes_among_ordinary_ones():
    """An all-masked plane, a plane holding one NaN and a plane of logits +-80 between ordinary planes: the ordinary planes' entropy
    and gradient are bitwise what they are when every OTHER plane of the same batch is masked out and the plane sits in front (another
    alignment: 33 x 65 floats per plane)."""
    from wtpse_hip import ops, tent
    x, mask, _, _ = _case((3, 1, 33, 65), True)
    x, mask = torch.cat([x, x[:2] * 0.5]), torch.cat([mask, mask[:2]])       # planes 0, 2, 4 ordinary
    mask[1] = 0.0                                                            # all masked
    x[3, 0, 7, 11] = float("nan")
    sign = torch.where(torch.rand(x[0].shape, generator=torch.Generator().manual_seed(1)) < 0.5, -1.0, 1.0)
    x = torch.cat([x, 80.0 * sign[None]])                                    # plane 5: e = exp(-80) underflows in fp32, not in fp64
    mask = torch.cat([mask, torch.ones_like(mask[:1])])
    B = x.shape[0]
    loss, dx, planes, sel = ops.entropy_loss(x.to(DEV), mask.to(DEV), want_planes=True)
    dx, planes = dx.cpu(), planes.cpu()
    assert sel.cpu().tolist() == [1, 0, 1, 0, 1, 1]
    assert float(planes[1]) == 0.0 and math.isnan(float(planes[3])) and not _bits(dx[1]).any() and not _bits(dx[3]).any()
    assert torch.isfinite(dx).all() and math.isfinite(float(loss))          # the NaN plane reaches neither the loss nor dx
    assert 0.0 < float(planes[5]) < 1e-30 and bool(dx[5].any())              # 80 e^-80: finite, not flushed
    xn, mn = x.double().numpy(), mask.double().numpy()
    H64 = tent.entropy_planes_host(xn, mn)[0]
    g64 = tent.tent_grad_host(xn, mn)
    keep = [0, 2, 4, 5]
    assert (np.abs(planes.double().numpy()[keep] - H64[keep]) <= 2.0 * _ulp32(H64[keep])).all()
    assert (np.abs(dx.double().numpy()[keep] - g64[keep]) <= 2.0 * _ulp32(g64[keep])).all()
    for k in (0, 2, 4, 5):
        xa, ma = torch.zeros_like(x), torch.zeros_like(mask)
        xa[0], ma[0] = x[k], mask[k]
        _, dxa, pa, sa = ops.entropy_loss(xa.to(DEV), ma.to(DEV), want_planes=True)
        assert sa.cpu().tolist() == [1] + [0] * (B - 1)
        assert _same(pa[0].cpu(), planes[k]) and _same(dxa[0].cpu(), dx[k]), k


def test_entropy_loss_bad_arguments():
    from wtpse_hip import ops
    x = torch.zeros(2, 1, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="elements"):
        ops.entropy_loss(x, mask=x[:1])
    for bad in (x.double(), x.cpu(), x[:, :, :, ::2], torch.zeros(8, device=DEV), torch.zeros(0, 4, device=DEV)):
        with pytest.raises(ValueError):
            ops.entropy_loss(bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="margin"):
            ops.entropy_loss(x, margin=bad)
    loss, dx = ops.entropy_loss(x)
    assert abs(float(loss) - math.log(2.0)) <= 1e-7 and not dx.any()        # z = 0: ln 2, a stationary point


def test_adam_index_is_adam_dev_on_the_listed_elements():
    """5 000-element buffers, 1 000 random distinct indices (not a multiple of the workgroup), three consecutive steps with a device
    step count: bitwise wtpse_adam_dev on dense copies at the indices, p elsewhere untouched; hold = 1 changes nothing."""
    from wtpse_hip import ops
    g = torch.Generator().manual_seed(4)
    n, k = 5000, 1000
    idx = torch.randperm(n, generator=g)[:k]
    p0 = torch.randn(n, generator=g)
    lr = torch.full((1,), 1e-3, device=DEV)
    p, pd = p0.clone().to(DEV), p0.clone().to(DEV)
    idx_d = idx.to(torch.int32).to(DEV)
    m, v = torch.zeros(k, device=DEV), torch.zeros(k, device=DEV)
    md, vd = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    t, td = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    other = torch.ones(n, dtype=torch.bool)
    other[idx] = False
    for step in range(3):
        grad = (torch.randn(n, generator=g) * 10.0 ** (step - 2)).to(DEV)
        p.wt_amax = object()
        ops.adam_index(p, grad, m, v, idx_d, lr, 0.9, 0.999, 1e-8, 1, t)
        assert p.wt_amax is None                                            # an amax table of p would be stale now
        ops.counter_add(t, 1)
        ops.adam_step_dev(pd, grad, md, vd, lr, 0.9, 0.999, 1e-8, 1, td)
        ops.counter_add(td, 1)
        assert _same(p.cpu()[idx], pd.cpu()[idx]) and _same(m.cpu(), md.cpu()[idx]) and _same(v.cpu(), vd.cpu()[idx]), step
        assert _same(p.cpu()[other], p0[other]) and not _same(p.cpu()[idx], p0[idx]), step
    before = [a.clone() for a in (p, m, v)]
    ops.adam_index(p, grad, m, v, idx_d, lr, 0.9, 0.999, 1e-8, 1, t, hold=torch.ones(1, dtype=torch.int32, device=DEV))
    assert all(_same(a, b) for a, b in zip((p, m, v), before))
    ops.adam_index(p, grad, m, v, idx_d, lr, 0.9, 0.999, 1e-8, 1, t, hold=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert not _same(p, before[0])
    with pytest.raises(ValueError):
        ops.adam_index(p, grad, m, v, idx_d.long(), lr, 0.9, 0.999, 1e-8, 1, t)
    with pytest.raises(ValueError):
        ops.adam_index(p, grad, m[:-1].contiguous(), v, idx_d, lr, 0.9, 0.999, 1e-8, 1, t)


# ==================================================================================================== network level
def _nets(hp, pb=1):
    """(model, model_shape, model_oc, model_shape_oc) under `hp` with the filler's weights (test_parity_gpu.build_nets' seeds)."""
    import algorithms
    import shape_networks
    mk = lambda two_step: algorithms.WT_PSE(n_channels=3, n_classes=1, hparams=hp, device=DEV, two_step=two_step, per_domain_batch=pb,
                                            source_domain_num=3).to(DEV)
    main, main_oc = mk(False), mk(True)
    fill_state_dict(main, SEED_W)
    fill_state_dict(main_oc, SEED_W + 7)
    shapes = []
    for seed in (SEED_W + 3, SEED_W + 11):
        s = shape_networks.ShapeVariationalDist_x(dict(HP), DEV, n_classes=1, number_source_domain=3, batch_size=pb).to(DEV)
        fill_state_dict(s, seed)
        shapes.append(s.eval())
    return main, shapes[0], main_oc, shapes[1]


def _inputs(B, H, seed=600):
    img = make_inputs(seed, B, H, H)[0].to(DEV)
    return img


def _two_step_input(img):
    from wtpse_hip import ops
    logit = torch.randn(img.shape[0], 1, *img.shape[2:], generator=torch.Generator().manual_seed(3)).to(DEV)
    roi, _ = ops.roi(img.contiguous(), logit)
    return torch.stack((roi, roi), 0)


def _affines(net):
    from wtpse_hip import tent
    return [(name + "." + leaf, getattr(m, leaf)) for name, m in tent.affine_modules(net) for leaf in ("weight", "bias")]


def _affine_grads(net):
    return {k: p.grad.detach().clone() for k, p in _affines(net)}


@pytest.mark.parametrize("B,H", GEOMETRIES)
@pytest.mark.parametrize("variant", ["full", "plain", "cat_shape"])
def test_forward_predict_is_predict(variant, B, H):
    """_forward_predict, with and without the tape, returns predict()'s (logits, pre) bit for bit: train and eval mode, the one-step
    and the two-step (stacked ROI) input."""
    hp = dict(HP, cat_shape=True) if variant == "cat_shape" else dict(HP, whitening=False, shape_prior=False) if variant == "plain" else dict(HP)
    main, shape, main_oc, shape_oc = _nets(hp)
    img = _inputs(B, H)
    for net, sh, x in ((main, shape, img), (main_oc, shape_oc, _two_step_input(img))):
        for train in (True, False):
            net.train(train)
            want = net.predict(sh, x)
            for tape in (False, True):
                (out, pre), t = net._forward_predict(sh, x, want_tape=tape)
                assert (t is not None) == tape
                assert _same(out, want[0]), (variant, train, tape)
                assert (pre is None and want[1] is None) if variant == "plain" else _same(pre, want[1])
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,H", GEOMETRIES)
@pytest.mark.parametrize("train", [True, False], ids=["batch", "frozen"])
def test_plain_branch_backward_is_the_update_backward(train, B, H):
    """Without the shape prior the prediction forward IS the update forward: for the same d_out the BatchNorm weight and bias
    gradients of _backward_predict equal _backward_update's bitwise."""
    main = _nets(dict(HP, whitening=False, shape_prior=False))[0]
    img = _inputs(B, H)
    d_out = (torch.randn(B, 1, H, H, generator=torch.Generator().manual_seed(8)) * 1e-3).to(DEV)
    main.train(train)
    main.ensure_ready(repack=True)
    main.zero_grad(set_to_none=True)
    res, tape = main._forward_update(img, None, img, want_tape=True)
    main._backward_update(tape, d_out.clone())
    want = _affine_grads(main)
    main.zero_grad(set_to_none=True)
    (out, _), tape = main._forward_predict(None, img, want_tape=True)
    assert _same(out, res[0])
    main._backward_predict(tape, d_out.clone())
    got = _affine_grads(main)
    assert len(got) == 52 and all(bool(v.any()) for v in want.values())
    for k in want:
        assert _same(got[k], want[k]), k
    torch.cuda.synchronize()


class _AffinesOf:
    """What assert_calibrated reads of a module — named_parameters() with .grad — restricted to the BatchNorm affines."""

    def __init__(self, net):
        self.items = [(k, types.SimpleNamespace(grad=p.grad, numel=p.numel)) for k, p in _affines(net)]

    def named_parameters(self):
        return iter(self.items)


@pytest.mark.parametrize("B,H", GEOMETRIES)
def test_shape_prior_backward_against_the_oracle(B, H):
    """d(entropy objective) / d(every BatchNorm weight and bias) through the prediction path with the shape prior (eval mode, as the
    oracle's predict runs) against oracle.wtpse_cpu.wt_pse_predict + the entropy in torch, evaluated in float64 on the CPU.  Yardstick:
    test_parity_gpu.assert_calibrated at cal = 3 — per tensor and over all of them the HIP path is at most 3x as far from the float64
    evaluation as the oracle's own fp32 run (its bands and its perturbed-input probes as written there); the ratio is printed.
    Measured on an MI355X: both fp32 paths sit at rounding level — relative L2 distance over all 52 tensors 1.9e-7 (HIP) against 8.1e-8
    (CPU fp32) at [3-32], 1.8e-7 against 8.2e-8 at [6-64], ratios 2.4 and 2.2; every tensor is far inside its 3x + 5e-4 band.  The
    MEDIAN per-tensor ratio, the one criterion of assert_calibrated without an additive band, is 3.7 and 3.9: the plain comparison
    therefore goes on to the function's perturbed-input yardstick (inputs moved by <= 1e-5 move the oracle's own fp32 gradients by
    1e-4 .. 3e-5), where it holds with ratios below 0.01."""
    from wtpse_hip import ops
    main, shape, _, _ = build_nets(1)
    img = make_inputs(600, B, H, H)[0]
    sd_m = {k: v.detach().cpu().clone() for k, v in main.state_dict().items()}
    sd_s = {k: v.detach().cpu().clone() for k, v in shape.state_dict().items()}
    main.eval(); shape.eval()
    main.zero_grad(set_to_none=True)
    (logits, _), tape = main._forward_predict(shape, img.to(DEV), want_tape=True)
    loss, dx = ops.entropy_loss(logits)
    main._backward_predict(tape, dx)

    def objective(sd, sds, image=img):
        dt = sd["outc.0.weight"].dtype
        x, _ = O.wt_pse_predict(sd, sds, HP, image.to(dt), False)
        e = torch.exp(-x.abs())
        return (torch.log1p(e) + x.abs() * e / (1 + e)).reshape(B, -1).mean(1).mean()

    g32, g64 = oracle_grads(objective, [sd_m, sd_s], torch.float32)[0], oracle_grads(objective, [sd_m, sd_s], torch.float64)[0]
    with torch.no_grad():
        want = float(objective({k: v.double() if v.is_floating_point() else v for k, v in sd_m.items()},
                               {k: v.double() if v.is_floating_point() else v for k, v in sd_s.items()}))
    print("entropy objective: HIP %.9g, oracle fp64 %.9g" % (float(loss), want))
    assert abs(float(loss) - want) <= 1e-4
    keys = [k for k, _ in _affines(main)]
    assert len(keys) == 52 and all(k in g64 for k in keys)
    sub = lambda g: {k: g[k] for k in keys}
    probes = lambda: (sub(oracle_grads(lambda a, b: objective(a, b, q), [sd_m, sd_s], torch.float32)[0]) for q in perturbed(img, 12))
    tot_h, tot_c = assert_calibrated(_AffinesOf(main), sub(g32), sub(g64), "tent %d-%d" % (B, H), CAL, probes)
    print("BatchNorm affine gradients: HIP %.3e vs CPU-fp32 %.3e from the fp64 oracle, ratio %.2f" % (tot_h, tot_c, tot_h / max(tot_c, 1e-30)))


@pytest.mark.parametrize("train", [True, False], ids=["batch", "frozen"])
def test_affine_only_issues_no_weight_gradient(train, monkeypatch):
    """The switch on and off: the same BatchNorm gradients bit for bit; with the gradient buffer prefilled with a sentinel the switch
    leaves every convolution weight's range (the fused head's and the attention's own aside) untouched; no call whose name contains
    `wgrad` is made, and no side stream is forked."""
    from wtpse_hip import nn as E, ops
    B, H = 6, 64
    main, shape, _, _ = build_nets(1)
    img = _inputs(B, H)
    main.train(train); shape.eval()

    def run(affine_only, sentinel=None):
        main.zero_grad(set_to_none=True)
        (logits, _), tape = main._forward_predict(shape, img, want_tape=True)
        _, dx = ops.entropy_loss(logits)
        if sentinel is not None:
            main._gflat.fill_(sentinel)
        main._backward_predict(tape, dx, affine_only=affine_only)
        assert main._affine_only is False                                   # off again, whatever the call was
        torch.cuda.synchronize()
        return _affine_grads(main)

    full = run(False)
    names, L = [], ops.lib()
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    monkeypatch.setattr(E, "_side_stream", lambda *a, **k: pytest.fail("a side stream was asked for"))
    only = run(True, sentinel=123.0)
    monkeypatch.undo()
    assert names and not [n for n in names if "wgrad" in n]
    assert len(only) == 52 and all(_same(only[k], full[k]) for k in full)
    flat, n_conv = main._gflat.cpu(), 0
    for name, m in main.named_modules():
        if isinstance(m, E.ConvP) and not name.startswith(("mu.", "attention_layer", "wt_model", "prior_dist")):
            off = main.param_offset(m.weight)
            assert bool((flat[off:off + m.weight.numel()] == 123.0).all()), name
            n_conv += 1
    assert n_conv == 3 + 4 * 3 + 2 + 3 * 3 + 1                                # inc, the body, outc
    # ... and with the switch off the same launches do write them
    names2 = []
    monkeypatch.setattr(L, "call", lambda name, *a: (names2.append(name), real(name, *a))[1])
    run(False, sentinel=123.0)
    monkeypatch.undo()
    assert [n for n in names2 if "wgrad" in n]
    off = main.param_offset(main.down1.conv1.weight)
    assert not bool((main._gflat[off:off + main.down1.conv1.weight.numel()] == 123.0).any())


def _state(nets):
    return [dict(flat=n.flat_params().clone(), bufs={k: b.clone() for k, b in n.named_buffers()}) for n in nets]


def _load(dst, src):
    for a, b in zip(dst, src):
        a.load_state_dict(b.state_dict())


@pytest.fixture(scope="module")
def source():
    return build_nets(1)


@pytest.mark.parametrize("stats", ["batch", "frozen"])
def test_tent_step_moves_the_affines_alone(source, stats):
    from wtpse_hip import tent, validate as V
    B, H = 3, 32
    img = _inputs(B, H, seed=43)
    nets = build_nets(1)
    _load(nets, source)
    for n in nets:
        n.train()                                                           # the modes a step finds are the modes it leaves
    step = tent.TentStep(*nets, stats=stats)
    before = _state(nets)
    pred, pred_oc, s = step.step(img)
    torch.cuda.synchronize()
    after = _state(nets)
    assert all(n.training for n in nets) and set(s) == {"ent_od", "ent_oc", "sel_od", "sel_oc"}
    assert int(s["sel_od"]) == B and 0.0 < float(s["ent_od"]) <= math.log(2.0) and 0.0 <= float(s["ent_oc"]) <= math.log(2.0)
    # parameters: the two segmentation networks differ at the index list only (and do differ there); the shape networks not at all
    for i, opt in ((0, step.opt[0]), (2, step.opt[1])):
        idx = opt.idx.long()
        assert idx.numel() == sum(p.numel() for _, p in _affines(nets[i]))
        changed = _bits(after[i]["flat"]) != _bits(before[i]["flat"])
        listed = torch.zeros_like(changed)
        listed[idx] = True
        assert not bool((changed & ~listed).any()) and int(opt.t_dev) == 1, i
        if i == 0 or int(s["sel_oc"]) > 0:                                 # (a cup stage without a disc has no gradient: nothing moves)
            assert int(changed.sum()) > idx.numel() // 2 and bool(opt.m.any()) and bool(opt.v.any()), i
    for i in (1, 3):
        assert _same(after[i]["flat"], before[i]["flat"])
        assert all(torch.equal(after[i]["bufs"][k], v) for k, v in before[i]["bufs"].items())
    # the reference run: validate.predict_pair of the pre-step networks in the same modes
    ref = build_nets(1)
    _load(ref, source)
    for n, seg in zip(ref, (True, False, True, False)):
        n.train(seg and stats == "batch")
    want = V.predict_pair(*ref, img)
    assert _same(pred, want[0]) and _same(pred_oc, want[1])
    for i in (0, 2):
        bufs = dict(ref[i].named_buffers())
        if stats == "frozen":
            assert all(torch.equal(after[i]["bufs"][k], v) for k, v in before[i]["bufs"].items()), i
        else:                                                               # as after one plain train-mode predict() of the same inputs
            moved = [k for k, v in before[i]["bufs"].items() if not torch.equal(after[i]["bufs"][k], v)]
            assert len(moved) >= 3 * 26 - 4, len(moved)
            assert all(torch.equal(after[i]["bufs"][k], bufs[k]) for k in bufs), i
    # two runs from the same state are bitwise equal
    again = build_nets(1)
    _load(again, source)
    p2, p2_oc, s2 = tent.TentStep(*again, stats=stats).step(img)
    assert _same(p2, pred) and _same(p2_oc, pred_oc) and all(_same(s2[k].float(), s[k].float()) for k in s)
    for a, b in zip(_state(again), after):
        assert _same(a["flat"], b["flat"]) and all(torch.equal(a["bufs"][k], v) for k, v in b["bufs"].items())


def test_episodic_step_leaves_no_trace(source):
    from wtpse_hip import tent
    img = _inputs(3, 32, seed=43)
    nets = build_nets(1)
    _load(nets, source)
    step = tent.TentStep(*nets, stats="batch", episodic=True, steps=2)
    before = _state(nets)
    first = step.step(img)
    torch.cuda.synchronize()
    for a, b in zip(_state(nets), before):
        assert _same(a["flat"], b["flat"]) and all(torch.equal(a["bufs"][k], v) for k, v in b["bufs"].items())
    for opt in step.opt:
        assert not opt.m.any() and not opt.v.any() and int(opt.t_dev) == 0
    second = step.step(img)                                                 # every batch from the source: the same numbers again
    assert _same(first[0], second[0]) and _same(first[1], second[1]) and _same(first[2]["ent_oc"], second[2]["ent_oc"])
    step_k = tent.TentStep(*nets, stats="batch", episodic=False, steps=2)
    step_k.step(img)
    assert not _same(nets[0].flat_params(), before[0]["flat"]) and int(step_k.opt[0].t_dev) == 2


def test_five_steps_lower_the_entropy(source):
    """stats="frozen", one fixed batch, no margin, 5 steps at lr = 1e-3: the disc entropy of that batch afterwards is lower than
    before.  Deterministic: it holds or fails once and for all."""
    from wtpse_hip import tent
    img = _inputs(6, 64, seed=43)
    nets = build_nets(1)
    _load(nets, source)
    _, _, s = tent.TentStep(*nets, stats="frozen", steps=5, lr=1e-3).step(img)
    before = float(s["ent_od"])                                             # of the first forward: the source networks
    _, _, s = tent.TentStep(*nets, stats="frozen", steps=0).step(img)
    after = float(s["ent_od"])
    print("disc entropy of the batch: %.6f nats before, %.6f after 5 steps" % (before, after))
    assert after < before


def test_program_end_to_end(source, tmp_path):
    from PIL import Image
    from wtpse_hip import tent
    from wtpse_hip.programs import load_networks
    from wtpse_hip.synth import make_batch
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    from wtpse_hip.validate import best_checkpoint
    folder = tmp_path / "crops"
    folder.mkdir()
    img = make_batch(5, 64, 64, "cpu", seed=2)[0]
    for i in range(5):
        Image.fromarray(((img[i].permute(1, 2, 0).numpy() + 1.0) * 127.5).astype(np.uint8)).save(str(folder / ("crop_%d.png" % i)))
    src = str(tmp_path / "checkpoint_1.pth.tar")
    ck = {k: {n: v.cpu() for n, v in sd.items()} for k, sd in best_checkpoint(*source).items()}
    torch.save(ck, src)
    common = ["--images", str(folder), "--checkpoint", src, "--batch-size", "2", "--size", "64"]
    out = str(tmp_path / "tent")
    assert tent.main(common + ["--out", out, "--steps", "1", "--epochs", "2", "--margin", "0.69", "--reweight"]) == 0
    assert sorted(os.listdir(out)) == ["drift.csv", "tent.csv", "tent_checkpoint.pth.tar"]
    rows, drift = tent.read_tables(out)
    assert len(rows) == 2 * 3 and [r["images"] for r in rows] == [2, 2, 1] * 2 and [r["epoch"] for r in rows] == [0] * 3 + [1] * 3
    assert all(0.0 < r["ent_od"] <= math.log(2.0) and 0 <= r["sel_od"] <= r["images"] for r in rows)
    nets, _ = load_networks(os.path.join(out, "tent_checkpoint.pth.tar"))                  # it loads wherever a checkpoint does
    from wtpse_hip import nn as E
    n_bn = sum(1 for n in (nets[0], nets[2]) for m in n.modules() if isinstance(m, E.BNP))
    assert len(drift) == n_bn and {r["network"] for r in drift} == {"model", "model_oc"}
    moved = [r for r in drift if r["gamma_max"] > 0 or r["beta_max"] > 0]
    assert moved and all(not r["name"].startswith("prior_dist") for r in moved)
    assert all(r["gamma_max"] < 0.1 and r["beta_max"] < 0.1 for r in moved)                # six Adam steps at 1e-3
    saved = torch.load(os.path.join(out, "tent_checkpoint.pth.tar"), map_location="cpu", weights_only=True)
    assert saved["tent"]["images"] == 5 and saved["tent"]["source"] == "checkpoint_1.pth.tar" and saved["tent"]["steps"] == 1
    assert saved["tent"]["reweight"] is True and saved["tent"]["margin"] == 0.69 and "clahe" not in saved
    for key, net in zip(CHECKPOINT_KEYS, nets):
        for k, v in net.state_dict().items():
            assert torch.equal(v.cpu(), saved[key][k]), (key, k)
    assert not all(torch.equal(saved["model"][k], ck["model"][k]) for k in ck["model"])
    # --steps 0 reproduces the source's tensors bitwise, whatever the statistics mode
    out0 = str(tmp_path / "tent0")
    assert tent.main(common + ["--out", out0, "--steps", "0"]) == 0
    saved0 = torch.load(os.path.join(out0, "tent_checkpoint.pth.tar"), map_location="cpu", weights_only=True)
    for key in CHECKPOINT_KEYS:
        assert list(saved0[key]) == list(ck[key])
        for k, v in ck[key].items():
            assert saved0[key][k].dtype == v.dtype and torch.equal(saved0[key][k], v), (key, k)
    rows0, drift0 = tent.read_tables(out0)
    assert len(rows0) == 3 and all(not any(r[c] for c in tent.DRIFT_COLUMNS[3:]) for r in drift0)


def test_tent_test_run_scores_the_predictions_made_while_adapting(source, tmp_path):
    """TentTestRun with steps = 0 writes the table TestRun writes; with a step, each batch's logits are those a TentStep gives on the
    same sequence of batches, the summary names the arguments, and validate.predict_pair is what it was afterwards — also when a
    batch ends in an exception."""
    from wtpse_hip import tent, validate as V
    from wtpse_hip.test_run import TestRun, read_table
    img = _inputs(3, 64, seed=43)
    yy, xx = np.mgrid[0:64, 0:64]
    disc = torch.from_numpy(((yy - 30) ** 2 + (xx - 33) ** 2 <= 20 ** 2).astype(np.float32)).to(DEV).expand(3, 1, 64, 64).contiguous()
    cup = torch.from_numpy(((yy - 30) ** 2 + (xx - 33) ** 2 <= 9 ** 2).astype(np.float32)).to(DEV).expand(3, 1, 64, 64).contiguous()
    batches = [(img[:2].contiguous(), disc[:2], cup[:2], ["a", "b"]), (img[2:3].contiguous(), disc[2:3], cup[2:3], ["c"])]
    plain_fn = V.predict_pair
    nets = build_nets(1)
    _load(nets, source)
    outs = [str(tmp_path / n) for n in ("plain", "zero", "tent")]
    plain = TestRun(*nets, out_dir=outs[0]).run(batches)
    zero = tent.TentTestRun(*nets, out_dir=outs[1], steps=0).run(batches)
    assert V.predict_pair is plain_fn
    import json
    text = lambda obj: json.dumps(obj, sort_keys=True)                                     # (a NaN mean compares equal as text)
    assert text({k: v for k, v in zero.items() if k != "tent"}) == text(plain) and text(read_table(outs[1])[0]) == text(read_table(outs[0])[0])
    assert zero["tent"]["steps"] == 0 and text(read_table(outs[1])[1]) == text(zero)
    # one step per batch: the run's logits are the step's, batch after batch
    run = tent.TentTestRun(*nets, out_dir=outs[2], lr=1e-3, stats="batch")
    seen, inner = [], run.predict
    run.predict = lambda image, size: (seen.append([t.clone() for t in inner(image, size)]), seen[-1])[1]
    means = run.run(batches)
    assert V.predict_pair is plain_fn and means["tent"]["stats"] == "batch" and means["n"] == 3 and len(read_table(outs[2])[0]) == 3
    ref = build_nets(1)
    _load(ref, source)
    step = tent.TentStep(*ref, lr=1e-3, stats="batch")
    for (x, _, _, _), got in zip(batches, seen):
        p, p_oc, _ = step.step(x)
        assert _same(got[0], p) and _same(got[1], p_oc)
    assert _same(nets[0].flat_params(), ref[0].flat_params()) and _same(nets[2].flat_params(), ref[2].flat_params())
    assert all(n.training for n in nets)                                                  # the modes the run found
    with pytest.raises(ZeroDivisionError):
        run.predict = lambda image, size: 1 // 0
        run.run(batches)
    assert V.predict_pair is plain_fn
