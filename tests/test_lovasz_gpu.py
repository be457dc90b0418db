"""The Lovász hinge loss on the GPU: wtpse_lovasz_loss against the specification (wtpse_hip/lovasz.py) — the order of the device's
segmented sort exactly, values and increments to one fp32 ulp — its bitwise promises, TrainStep(lovasz=) and TrainRun(lovasz=).  The
step tests' sizes and helpers follow tests/test_overlap_gpu.py.

Bars.  A plane loss is a float64 sum of non-negative terms (relative error below n 2^-53) rounded once to fp32: one fp32 ulp of
float32(specification).  An increment is (w / B) (+-1) g in float64 added to the stored value and rounded once: one fp32 ulp of
float32(float64(dx_old) + specification).  The mean is wtpse_reduce_rows: a float64 sum of B fp32 values rounded to fp32, times the
fp32 1 / B: (B + 1) 2^-24 of the largest plane loss covers its three roundings for every B."""
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


_CHUNK = []


def _chunk():
    """Elements of a plane per workgroup, from the implementation: the workspace beyond the four [hw] buffers of keys and payloads
    grows by one chunk's tables at every hw that starts a new chunk."""
    if not _CHUNK:
        from wtpse_hip import lib
        q = lambda hw: lib.lib().query("wtpse_lovasz_loss_ws", 1, hw) - 16 * hw
        hw = 1
        while q(hw + 1) == q(1):
            hw += 1
            assert hw < (1 << 16)
        _CHUNK.append(hw)
    return _CHUNK[0]


# (2, 33, 65): odd planes unaligned; (2, 256, 256): the training geometry, every chunk boundary the kernels have; "chunk+1" /
# "chunk-1": one element more / less than a chunk (filled in from the implementation)
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 17, 19), (2, 33, 65), (2, 64, 64), (2, 256, 256), "chunk+1", "chunk-1"]


def _shape(s):
    return s if isinstance(s, tuple) else (2, 1, _chunk() + (1 if s == "chunk+1" else -1))


def _ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32)


_CASES = {}


def _case(shape, masked, kind="normal"):
    """x = 3 * randn ("normal") or one of eight values ("tied": nearly every key has thousands of equals), disc-shaped targets (a radius
    per plane), a random 60 % mask; host tensors, made once."""
    key = (shape, masked, kind)
    if key not in _CASES:
        Bn, h, w = shape
        yy, xx = np.mgrid[0:h, 0:w]
        t = np.stack([((yy - (h - 1) / 2) ** 2 + (xx - (w - 1) / 2) ** 2 <= ((0.15 + 0.07 * k) * max(min(h, w), 0.3 * max(h, w))) ** 2)
                      for k in range(Bn)])
        t = torch.from_numpy(t.astype(np.float32)[:, None])
        g = torch.Generator().manual_seed(100 * h + w + int(masked) + 7 * (kind == "tied"))
        if kind == "tied":
            x = (torch.randint(0, 8, t.shape, generator=g).float() - 3.5) * 0.5
        else:
            x = torch.randn(t.shape, generator=g) * 3.0
        mask = (torch.rand(t.shape, generator=g) < 0.6).float() if masked else None
        _CASES[key] = (x, t, mask)
    return _CASES[key]


_REF = {}


def _reference(shape, masked, kind, w32):
    """(ranks, planes64, grad64) of the specification, once."""
    key = (shape, masked, kind, w32)
    if key not in _REF:
        from wtpse_hip import lovasz as lv
        x, t, mask = _case(shape, masked, kind)
        m = None if mask is None else mask.numpy()
        _REF[key] = (lv.lovasz_ranks_host(x.numpy(), t.numpy(), m), lv.lovasz_planes_host(x.numpy(), t.numpy(), m),
                     lv.lovasz_grad_host(x.numpy(), t.numpy(), w32, m))
        for v in _REF[key]:
            v.setflags(write=False)
    return _REF[key]


def _to_dev(x, t, mask):
    return x.to(DEV), t.to(DEV), None if mask is None else mask.to(DEV)


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("kind", ["normal", "tied"])
@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_ranks_are_the_specifications_order(shape, masked, kind):
    """The device's order, pixel by pixel: exact integers.  "tied": eight distinct logits — sixteen distinct errors at most — so the
    places inside a run of equal keys are decided by the tie rule alone (ascending pixel index): scatter places that are not stable
    fail here."""
    from wtpse_hip import ops
    shape = _shape(shape)
    x, t, mask = _case(shape, masked, kind)
    want, _, _ = _reference(shape, masked, kind, 0.375)
    xd, td, md = _to_dev(x, t, mask)
    loss, ranks = ops.lovasz_loss(xd, td, None, mask=md, want_ranks=True)
    assert ranks.dtype == torch.int32 and ranks.shape == x.shape and loss.dim() == 0
    got = ranks.cpu().numpy()
    wrong = int((got != want).sum())
    print("ranks %s %s %s: %d pixels in the order, %d wrong" % (shape, "cup" if masked else "disc", kind, int((want >= 0).sum()), wrong))
    assert wrong == 0
    if kind == "tied" and x[0].numel() >= 15:
        assert len(np.unique(x.numpy())) <= 8 and int((want >= 0).sum()) > 2


@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_lovasz_loss_value_and_gradient(shape, masked):
    from wtpse_hip import ops
    shape = _shape(shape)
    x, t, mask = _case(shape, masked)
    xd, td, md = _to_dev(x, t, mask)
    w_dev = torch.full((1,), 0.375, dtype=torch.float32, device=DEV)
    w32 = float(w_dev.item())
    ranks64, planes64, g64 = _reference(shape, masked, "normal", w32)
    Bn = shape[0]

    # ---- per-plane loss: one fp32 ulp of float32(specification); the mean: (B + 1) 2^-24 of the largest plane loss
    loss, planes = ops.lovasz_loss(xd, td, None, mask=md, want_planes=True)
    assert loss.dim() == 0 and planes.shape == (Bn,)
    got = planes.cpu().double().numpy()
    want = planes64.astype(np.float32).astype(np.float64)
    e = np.abs(got - want)
    print("lovasz_loss %s %s: plane losses %s, max |gpu - f32(spec)| %.3g ulp" % (shape, "cup" if masked else "disc", planes64,
                                                                                 float((e / _ulp32(want)).max())))
    assert (e <= _ulp32(want)).all(), (got, want)
    e, bar = abs(float(loss) - float(got.mean())), (Bn + 1) * 2.0 ** -24 * float(got.max())
    print("  mean %.9g: |gpu - mean(planes)| %.3g, bar %.3g" % (float(loss), e, bar))
    assert e <= bar, (e, bar)

    # ---- the increment into zeros: what is stored IS the increment
    inc = torch.zeros(x.shape, device=DEV)
    loss_dx, planes_dx, ranks = ops.lovasz_loss(xd, td, w_dev, mask=md, dx=inc, want_planes=True, want_ranks=True)
    got = inc.cpu().double().numpy()
    want = g64.astype(np.float32).astype(np.float64)
    e = np.abs(got - want)
    print("  increment into zeros: max err %.3g ulp" % float((e / _ulp32(want)).max()))
    assert (e <= _ulp32(want)).all(), int((e > _ulp32(want)).sum())
    live = bool((g64 != 0).any())
    assert bool(inc.any()) == live and (got[ranks64 < 0] == 0).all()
    assert np.array_equal(ranks.cpu().numpy(), ranks64)
    # the same bits with dx null and non-null, with and without the optional outputs, and again
    assert torch.equal(_bits(loss), _bits(loss_dx)) and torch.equal(_bits(planes), _bits(planes_dx))
    again = torch.zeros_like(inc)
    loss2, planes2, ranks2 = ops.lovasz_loss(xd, td, w_dev, mask=md, dx=again, want_planes=True, want_ranks=True)
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(planes), _bits(planes2)) and torch.equal(_bits(inc), _bits(again))
    assert torch.equal(ranks, ranks2)
    assert torch.equal(_bits(ops.lovasz_loss(xd, td, None, mask=md)), _bits(loss))

    # ---- onto a known tensor: one fp32 ulp of float32(float64(dx_old) + specification); every pixel out of the order keeps its
    # bits, a stored -0.0 included
    dx0 = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) * 1e-3
    out = np.flatnonzero(ranks64.ravel() < 0)
    if out.size:
        dx0.view(-1)[int(out[0])] = -0.0
    dx0 = dx0.to(DEV)
    dx = dx0.clone()
    dx.wt_amax = object()                              # an amax table of the region loss's gradient would be stale now
    ops.lovasz_loss(xd, td, w_dev, mask=md, dx=dx)
    assert dx.wt_amax is None
    want = (dx0.cpu().double().numpy() + g64).astype(np.float32).astype(np.float64)
    e = np.abs(dx.cpu().double().numpy() - want)
    assert (e <= _ulp32(want)).all(), int((e > _ulp32(want)).sum())
    assert torch.equal(dx, dx0) != live
    off = torch.from_numpy(ranks64 < 0).to(DEV)
    assert torch.equal(_bits(dx)[off], _bits(dx0)[off])
    if md is not None:
        assert bool((off | (md != 0)).all())            # (every ignored pixel is among them)
        assert bool((md == 0).any()) or x.numel() < 8

    # ---- the weight lives on the device: 0 leaves dx bit for bit and still reports the loss; doubling it doubles the increment
    w_dev.zero_()
    dx = dx0.clone()
    loss0, planes0 = ops.lovasz_loss(xd, td, w_dev, mask=md, dx=dx, want_planes=True)
    assert torch.equal(_bits(dx), _bits(dx0)) and torch.equal(_bits(loss0), _bits(loss)) and torch.equal(_bits(planes0), _bits(planes))
    w_dev.fill_(0.25)
    one = torch.zeros_like(inc)
    ops.lovasz_loss(xd, td, w_dev, mask=md, dx=one)
    w_dev.mul_(2.0)                                    # a device-side write: no host argument changes between the two calls
    two = torch.zeros_like(inc)
    ops.lovasz_loss(xd, td, w_dev, mask=md, dx=two)
    assert bool(one.any()) == live and torch.equal(_bits(two), _bits(2.0 * one))


def _edge_case():
    """Five planes of 33 x 65 under a mask: 0 ordinary, 1 an empty mask, 2 no foreground, 3 all foreground, 4 all errors <= 0; then
    5 a single kept pixel and 6 ordinary again."""
    x, t, mask = (v.clone() for v in _case((3, 33, 65), True))
    x, t, mask = (torch.cat([v, v, v[:1]]) for v in (x, t, mask))
    mask[1] = 0.0
    t[2] = 0.0
    t[3] = 1.0
    x[4] = (2.0 * t[4] - 1.0) * (x[4].abs() + 1.0)
    mask[5] = 0.0
    mask[5].view(-1)[777] = 1.0
    return x, t, mask


def test_edge_planes_among_ordinary_ones():
    from wtpse_hip import lovasz as lv
    from wtpse_hip import ops
    x, t, mask = _edge_case()
    w_dev = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
    for m in (mask, None):
        mh = None if m is None else m.numpy()
        want_p = lv.lovasz_planes_host(x.numpy(), t.numpy(), mh)
        want_g = lv.lovasz_grad_host(x.numpy(), t.numpy(), 0.5, mh).astype(np.float32).astype(np.float64)
        want_r = lv.lovasz_ranks_host(x.numpy(), t.numpy(), mh)
        inc = torch.zeros(x.shape, device=DEV)
        loss, planes, ranks = ops.lovasz_loss(*_to_dev(x, t, None)[:2], w_dev, mask=None if m is None else m.to(DEV), dx=inc,
                                              want_planes=True, want_ranks=True)
        planes, inc = planes.cpu().double().numpy(), inc.cpu().double().numpy()
        assert not np.isnan(planes).any() and not np.isnan(inc).any() and not math.isnan(float(loss))
        assert np.array_equal(ranks.cpu().numpy(), want_r)
        want32 = want_p.astype(np.float32).astype(np.float64)
        assert (np.abs(planes - want32) <= _ulp32(want32)).all(), (planes, want_p)
        assert (np.abs(inc - want_g) <= _ulp32(want_g)).all()
        assert planes[4] == 0.0 and not inc[4].any() and want_p[4] == 0.0
        if m is not None:
            assert planes[1] == 0.0 and not inc[1].any()
            assert np.count_nonzero(inc[5]) <= 1 and planes[5] == want32[5]
        assert planes[2] > 0.0 and np.count_nonzero(inc[2]) == 1                # no foreground: the top pixel alone
        assert planes[3] > 0.0 and (inc[3] <= 0).all() and inc[3].any()         # all foreground: every live pixel is pushed up
        # the ordinary planes are untouched by their neighbours: plane 6 is plane 0 again, bit for bit
        assert planes[0] > 0.0 and planes[6] == planes[0] and np.array_equal(inc[6], inc[0]) and inc[0].any()


@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
def test_a_planes_bits_do_not_depend_on_the_batch(masked):
    """The same plane at index 0 of B = 1 and at index 2 of B = 3 (33 x 65: there it starts 8 bytes off a 16-byte boundary; and
    256 x 256): ranks, plane loss and — with w / B the same number, 0.25 / 1 = 0.75 / 3 — the increment, bit for bit."""
    from wtpse_hip import ops
    for shape in ((3, 33, 65), (3, 256, 256)):
        x, t, mask = _to_dev(*_case(shape, masked))
        pick = lambda v: None if v is None else v[2:3].contiguous()
        w1 = torch.full((1,), 0.25, dtype=torch.float32, device=DEV)
        w3 = torch.full((1,), 0.75, dtype=torch.float32, device=DEV)
        inc3, inc1 = torch.zeros(x.shape, device=DEV), torch.zeros(x[2:3].shape, device=DEV)
        _, p3, r3 = ops.lovasz_loss(x, t, w3, mask=mask, dx=inc3, want_planes=True, want_ranks=True)
        l1, p1, r1 = ops.lovasz_loss(pick(x), pick(t), w1, mask=pick(mask), dx=inc1, want_planes=True, want_ranks=True)
        assert torch.equal(r3[2:3], r1) and torch.equal(_bits(p3[2:3]), _bits(p1)) and torch.equal(_bits(inc3[2:3]), _bits(inc1))
        assert torch.equal(_bits(l1), _bits(p1[0])) and bool(inc1.any())


def test_nan_logit_inside_and_outside_the_mask():
    from wtpse_hip import ops
    x, t, mask = (v.clone() for v in _case((3, 33, 65), True))
    kept = int(torch.nonzero(mask[1].view(-1))[5])
    dropped = int(torch.nonzero(mask[1].view(-1) == 0)[5])
    w_dev = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
    xd, td, md = _to_dev(x, t, mask)
    clean = torch.zeros(x.shape, device=DEV)
    loss_c, planes_c = ops.lovasz_loss(xd, td, w_dev, mask=md, dx=clean, want_planes=True)
    for bad in (float("nan"), float("inf"), -float("inf")):
        xb = x.clone()
        xb[1].view(-1)[dropped] = bad                      # outside the mask: not seen
        inc = torch.zeros(x.shape, device=DEV)
        loss, planes = ops.lovasz_loss(xb.to(DEV), td, w_dev, mask=md, dx=inc, want_planes=True)
        assert torch.equal(_bits(loss), _bits(loss_c)) and torch.equal(_bits(planes), _bits(planes_c)) and torch.equal(_bits(inc), _bits(clean))
        xb = x.clone()
        xb[1].view(-1)[kept] = bad                         # inside: a NaN plane, a NaN mean, nothing into that plane's dx
        for m in (md, None):
            inc = torch.zeros(x.shape, device=DEV)
            loss, planes = ops.lovasz_loss(xb.to(DEV), td, w_dev, mask=m, dx=inc, want_planes=True)
            p = planes.cpu()
            assert math.isnan(float(p[1])) and math.isnan(float(loss)) and float(p[0]) == float(p[0]) and float(p[2]) == float(p[2])
            assert not inc[1].any() and bool(inc[0].any()) and bool(inc[2].any()) and not torch.isnan(inc).any()
            if m is md:
                assert torch.equal(_bits(inc[0]), _bits(clean[0])) and torch.equal(_bits(inc[2]), _bits(clean[2]))
                assert torch.equal(_bits(planes[0]), _bits(planes_c[0])) and torch.equal(_bits(planes[2]), _bits(planes_c[2]))


def test_bad_arguments():
    from wtpse_hip import ops
    x = torch.zeros(2, 1, 4, 4, device=DEV)
    w = torch.ones(1, device=DEV)
    with pytest.raises(ValueError, match="w_dev"):
        ops.lovasz_loss(x, x, None, dx=torch.zeros_like(x))
    for bad in (dict(t=x[:1]), dict(mask=x[:1]), dict(dx=x[:1].clone())):
        kw = dict(t=x, mask=None, dx=None)
        kw.update(bad)
        with pytest.raises(ValueError, match="elements"):
            ops.lovasz_loss(x, kw["t"], w, mask=kw["mask"], dx=kw["dx"])
    with pytest.raises(ValueError):
        ops.lovasz_loss(x.double(), x, w)
    with pytest.raises(ValueError):
        ops.lovasz_loss(x.cpu(), x, w)
    with pytest.raises(ValueError):
        ops.lovasz_loss(torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), w)
    with pytest.raises(ValueError):
        ops.lovasz_loss(torch.zeros(0, 4, device=DEV), torch.zeros(0, 4, device=DEV), w)
    # logits 0 against an empty target: e = 1 everywhere, J = 1 from the first place on — the loss is 1
    assert float(ops.lovasz_loss(x, x, None)) == 1.0
    assert torch.equal(ops.lovasz_loss(x.view(2, 16), x.view(2, 16), None), ops.lovasz_loss(x, x, None))


def test_log_tests_the_sixth_scalar_for_nan():
    """check_n = loss_log_code(6): a NaN in any of the six slots raises the flag, as does inf + -inf across them; finite values do
    not; the sums take all six."""
    from wtpse_hip import ops
    dev = torch.device(DEV)
    nan, inf = float("nan"), float("inf")
    step = torch.full((1,), 7, dtype=torch.int32, device=dev)
    code = ops.loss_log_code(6)
    cases = [({j: nan}, True) for j in range(6)] + [({}, False), ({0: inf, 5: -inf}, True), ({5: inf}, False), ({0: inf, 5: inf}, False)]
    for put, raised in cases:
        vals = [put.get(j, float(j + 1)) for j in range(6)]
        s = torch.tensor(vals, dtype=torch.float32, device=dev)
        acc = torch.zeros(6, dtype=torch.float64, device=dev)
        flag = torch.zeros(2, dtype=torch.int32, device=dev)
        ops.loss_log([s[j] for j in range(6)], acc, 0, code, flag, step)
        assert flag.tolist() == ([1, 7] if raised else [0, 0]), vals
        assert all((a != a) if (b != b) else a == b for a, b in zip(acc.tolist(), vals)), (vals, acc.tolist())
    # the code of five still leaves the sixth slot untested
    s = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, nan], dtype=torch.float32, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.loss_log([s[j] for j in range(6)], torch.zeros(6, dtype=torch.float64, device=dev), 0, ops.loss_log_code(5), flag, step)
    assert flag.tolist() == [0, 0]
    with pytest.raises(Exception):
        ops.loss_log([s[j] for j in range(5)], torch.zeros(6, dtype=torch.float64, device=dev), 0, code, flag, step)


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


def _host_lv(logits, target, mask):
    """(L_lv of the specification on the device's own logits, its bar: every plane within one fp32 ulp (2^-23 of it at most), then
    the mean's (B + 1) 2^-24 of the largest plane)."""
    from wtpse_hip import lovasz as lv
    planes = lv.lovasz_planes_host(logits.cpu().numpy(), target.cpu().numpy(), None if mask is None else mask.cpu().numpy())
    return float(planes.mean()), (len(planes) + 3) * 2.0 ** -24 * float(planes.max())


def test_step_with_zero_weight_changes_nothing_and_reports_the_loss():
    """w = 0: two steps with the term leave every network where two steps without it do, bit for bit; lv_od / lv_oc of the first step
    are the specification on that step's own logits (a twin's forward passes) and targets."""
    from wtpse_hip import ops
    from wtpse_hip.lovasz import LovaszLoss
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES, lovasz=LovaszLoss(0.0))
    assert ts.get_lovasz_weight() == 0.0 and ts.lovasz.config() == LovaszLoss(0.0).config() and ts.overlap is None
    dev, hp, plain = _setup()
    tp = TrainStep(*plain, hp, lr=RATES)
    assert tp.get_lovasz_weight() is None and tp.lv_w is None and tp.lovasz is None
    with pytest.raises(ValueError, match="lovasz"):
        tp.set_lovasz_weight(0.1)
    first = None
    for k in range(2):
        res = ts.step(*_batch(dev, 3 + k))
        ref = tp.step(*_batch(dev, 3 + k))
        assert list(res) == TrainStep.log_names(hp, lovasz=True) and list(ref) == TrainStep.log_names(hp)
        for name, v in ref.items():
            assert torch.equal(v, res[name]), name
        first = first or {name: float(res[name]) for name in ("lv_od", "lv_oc")}
    _assert_same(_snapshot(ts, nets), _snapshot(tp, plain))
    # the first step's logits, from a third set of the same networks
    dev, hp, twin = _setup()
    TrainStep(*twin, hp, lr=RATES)                       # (puts the networks into the state a step runs them in)
    image, target_od, target_oc = _batch(dev, 3)
    out = twin[0]._forward_update(image, target_od, image, want_tape=True)[0][0]
    roi, od_pred = ops.roi(image, out)
    out_oc = twin[2]._forward_update(roi, target_oc, roi, want_tape=True)[0][0]
    for name, logits, target, mask in (("lv_od", out, target_od, None), ("lv_oc", out_oc, target_oc, od_pred)):
        want, bar = _host_lv(logits, target, mask)
        print("%s: step %.9g, specification %.9g, bar %.3g" % (name, first[name], want, bar))
        assert abs(first[name] - want) <= bar, (name, first[name], want, bar)
    assert first["lv_od"] > 0.0 and first["lv_oc"] >= 0.0


_RUNS = {}


def _run(graph, weights, others=False):
    """Three steps with the Lovász term (others: and the boundary and overlap terms) and a log; weights: the weight set before each
    step (None: leave it).  Cached."""
    key = (graph, tuple(weights), others)
    if key not in _RUNS:
        from wtpse_hip.boundary import BoundaryLoss
        from wtpse_hip.lovasz import LovaszLoss
        from wtpse_hip.overlap import OverlapLoss
        from wtpse_hip.step import TrainStep
        from wtpse_hip.trainer import LossLog
        dev, hp, nets = _setup()
        log = LossLog(dev, TrainStep.log_names(hp, boundary=others, overlap=others, lovasz=True))
        ts = TrainStep(*nets, hp, lr=RATES, graph=graph, log=log, lovasz=LovaszLoss(0.5),
                       boundary=BoundaryLoss(0.05, 0.0, 1.0) if others else None, overlap=OverlapLoss(0.5) if others else None)
        assert ts.get_lovasz_weight() == 0.5
        steps = []
        for k, a in enumerate(weights):
            if a is not None:
                ts.set_lovasz_weight(a)
            res = ts.step(*_batch(dev, 20 + k))
            steps.append({name: float(v) for name, v in res.items()})
        sums, flag = log.read()
        _RUNS[key] = (_snapshot(ts, nets), steps, sums, flag)
        ts.close()
    return _RUNS[key]


def test_step_eager_and_plan_agree_and_the_log_sums_the_term():
    """Weight 0.5: eager and recorded steps agree bit for bit after three steps, and the log's lv_* sums are the steps' values."""
    se, steps_e, sums_e, flag_e = _run(False, (None, None, None))
    sp, steps_p, sums_p, flag_p = _run("plan", (None, None, None))
    _assert_same(se, sp)
    assert steps_e == steps_p and sums_e == sums_p and flag_e == flag_p == (False, 0)
    for name in ("lv_od", "lv_oc", "seg_od", "seg_oc", "dom_od"):
        total = 0.0
        for s in steps_p:
            total += s[name]
        # (lv_oc may be 0: freshly initialised networks leave the cup call's ROI mask empty, and a plane without a kept pixel has loss 0)
        assert sums_p[name] == total and total == total and (total != 0.0 or name == "lv_oc"), name
    # the term reaches the networks: the same steps without it end elsewhere
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    tp = TrainStep(*nets, hp, lr=RATES)
    for k in range(3):
        tp.step(*_batch(dev, 20 + k))
    s0 = _snapshot(tp, nets)
    assert not torch.equal(s0["params"][0], se["params"][0])


def test_weight_changes_between_replays_without_recording_again():
    """set_lovasz_weight between replays: the recorded step follows, and equals an eager run given the same weights."""
    schedule = (None, 2.0, 0.0)
    sp, steps_p, sums_p, _ = _run("plan", schedule)
    se, steps_e, sums_e, _ = _run(False, schedule)
    _assert_same(sp, se)
    assert steps_p == steps_e and sums_p == sums_e
    const, steps_c, _, _ = _run("plan", (None, None, None))
    # the losses are reported unweighted: call A of the step that first runs under the new weight still sees the old parameters ...
    assert steps_c[0] == steps_p[0] and all(steps_c[1][k] == steps_p[1][k] for k in ("seg_od", "dom_od", "lv_od"))
    assert steps_c[2]["seg_od"] != steps_p[2]["seg_od"]                    # ... and the changed weight shows from its Adam step on
    assert not torch.equal(const["params"][0], sp["params"][0])


def test_three_terms_with_whitening_six_scalars():
    """All three terms with whitening on — six scalars per call: eager == plan bit for bit, lv_* behind bd_*, ov_*; a NaN planted in
    the Lovász scalar alone raises the flag with the iteration and holds every Adam launch."""
    from wtpse_hip.step import TrainStep
    se, steps_e, sums_e, flag_e = _run(False, (None, None, None), others=True)
    sp, steps_p, sums_p, flag_p = _run("plan", (None, None, None), others=True)
    _assert_same(se, sp)
    assert steps_e == steps_p and sums_e == sums_p and flag_e == flag_p == (False, 0)
    names = list(steps_p[0])
    assert names == TrainStep.log_names({"whitening": True}, boundary=True, overlap=True, lovasz=True)
    assert names[:6] == ["seg_od", "ins_od", "dom_od", "bd_od", "ov_od", "lv_od"]
    alone, steps_a, _, _ = _run("plan", (None, None, None))
    assert steps_a[0]["lv_od"] == steps_p[0]["lv_od"]                      # (the first call A sees the same parameters)
    assert not torch.equal(alone["params"][0], sp["params"][0])


def test_nan_lovasz_scalar_raises_the_flag_and_holds_adam(monkeypatch):
    from wtpse_hip import ops
    from wtpse_hip.boundary import BoundaryLoss
    from wtpse_hip.lovasz import LovaszLoss
    from wtpse_hip.overlap import OverlapLoss
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import LossLog
    dev, hp, nets = _setup(full=True)
    assert hp["whitening"]
    log = LossLog(dev, TrainStep.log_names(hp, boundary=True, overlap=True, lovasz=True))
    ts = TrainStep(*nets, hp, lr=RATES, log=log, lovasz=LovaszLoss(0.5), overlap=OverlapLoss(0.5), boundary=BoundaryLoss(0.05, 0.0, 1.0))
    codes = []
    real_log = ops.loss_log

    def spy(scalars, acc, offset, check_n, flag, step_dev):
        codes.append((len(scalars), check_n))
        return real_log(scalars, acc, offset, check_n, flag, step_dev)
    monkeypatch.setattr(ops, "loss_log", spy)
    before = _snapshot(ts, nets)
    res = ts.step(*_batch(dev, 3))
    assert all(float(v) == float(v) for v in res.values()) and list(res) == list(log.names)
    assert (6, ops.loss_log_code(6)) in codes and sum(1 for c in codes if c[0] == 6) == 2      # calls A and C: six scalars, all tested
    good = _snapshot(ts, nets)
    assert log.read()[1] == (False, 0) and not torch.equal(before["params"][0], good["params"][0])
    real = ops.lovasz_loss

    def poisoned(*a, **kw):
        loss = real(*a, **kw)
        return loss.fill_(float("nan"))
    monkeypatch.setattr(ops, "lovasz_loss", poisoned)
    res = ts.step(*_batch(dev, 4))
    finite = ["seg_od", "ins_od", "dom_od", "bd_od", "ov_od"]
    assert all(float(res[n]) == float(res[n]) for n in finite) and float(res["lv_od"]) != float(res["lv_od"])
    sums, flag = log.read()
    assert flag == (True, 1), flag                       # raised by call A of the second iteration
    held = _snapshot(ts, nets)
    for k in ("params", "m", "v"):
        for a, b in zip(good[k], held[k]):
            assert torch.equal(a, b), k


def test_step_arguments():
    from wtpse_hip.lovasz import LovaszLoss
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import LossLog
    dev, hp, nets = _setup()
    with pytest.raises(ValueError, match="lovasz"):
        TrainStep(*nets, hp, dp=object(), lovasz=LovaszLoss())
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, TrainStep.log_names(hp)), lovasz=LovaszLoss())
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, TrainStep.log_names(hp, lovasz=True)))
    ts = TrainStep(*nets, hp, lovasz=LovaszLoss(0.3))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ts.set_lovasz_weight(bad)
    ts.set_lovasz_weight(0.125)
    sd = ts.state_dict()
    assert ts.get_lovasz_weight() == 0.125 == float(ts.lv_w.item()) == sd["lovasz_weight"] and "overlap_weight" not in sd
    ts.set_lovasz_weight(0.75)
    ts.load_state_dict({k: v for k, v in sd.items() if k != "lovasz_weight"})      # a state from before the field loads unchanged
    assert ts.get_lovasz_weight() == 0.75
    ts.load_state_dict(sd)
    assert ts.get_lovasz_weight() == 0.125 == float(ts.lv_w.item())


def test_step_on_frozen_batchnorm():
    """freeze_bn=True with lovasz=: the step runs, trains, and leaves the running statistics alone."""
    from wtpse_hip.lovasz import LovaszLoss
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES, freeze_bn=True, lovasz=LovaszLoss(0.5))
    bufs = _buffers(nets)
    before = [n.flat_params().clone() for n in nets]
    res = ts.step(*_batch(dev, 3))
    vals = {k: float(v) for k, v in res.items()}
    assert all(v == v for v in vals.values()) and vals["lv_od"] > 0.0 and vals["lv_oc"] >= 0.0
    for a, b in zip(bufs, _buffers(nets)):
        assert torch.equal(a, b)
    assert all(not torch.equal(n.flat_params(), p0) for n, p0 in zip(nets, before))


# ---------------------------------------------------------------------------------------------------- 3. the run
def _next_batch(dev):
    def next_batch(py_rng, np_rng):
        return _batch(dev, int(np_rng.randint(1 << 20)) + py_rng.randint(0, 1000))
    return next_batch


def test_run_follows_the_schedule_and_resumes_bitwise(tmp_path):
    from wtpse_hip.lovasz import LovaszLoss
    from wtpse_hip.trainer import TrainRun
    sched = LovaszLoss(0.25, ramp=0.5, cap=1.0)
    kw = dict(iter_per_epoch=2, max_epoch=3, lr=RATES, graph="plan", seed=7)

    dev, hp, nets = _setup()
    a = TrainRun(*nets, hp, _next_batch(dev), out_dir=str(tmp_path / "a"), lovasz=sched, **kw)
    assert a.log.names == a.train_step.log_names(hp, lovasz=True)
    ea = []
    for epoch in range(3):
        ea.append(a.train_epoch())
        want = sched.weight_at(epoch)
        assert a.train_step.get_lovasz_weight() == want == ea[-1]["lovasz_weight"] and "overlap_weight" not in ea[-1]
        assert float(a.train_step.lv_w.item()) == float(np.float32(want))
        assert ea[-1]["sums"]["lv_od"] == ea[-1]["sums"]["lv_od"] != 0.0
    assert [e["lovasz_weight"] for e in ea] == [0.25, 0.75, 1.0]
    sa = _snapshot(a.train_step, nets)
    with open(tmp_path / "a" / "train_log.csv") as f:
        header = f.readline().strip().split(",")
    assert header[2:2 + len(a.log.names)] == a.log.names and "lv_od" in header and "lv_oc" in header

    dev, hp, nets1 = _setup()
    b1 = TrainRun(*nets1, hp, _next_batch(dev), lovasz=sched.config(), **kw)       # the dict form
    b1.train_epoch()
    b1.train_epoch()
    path = str(tmp_path / "run.pth.tar")
    b1.save(path)
    del b1
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["config"]["lovasz"] == sched.config() and saved["config"]["overlap"] == {} and saved["config"]["boundary"] == {}
    assert saved["train_step"]["lovasz_weight"] == 0.75

    dev, hp, nets2 = _setup(seed=5, noise=None)
    b2 = TrainRun.load(path, *nets2, hp, _next_batch(dev), graph="plan")
    assert b2.lovasz is not None and b2.lovasz.config() == sched.config() and b2.epoch == 2 and b2.overlap is None
    assert b2.train_step.get_lovasz_weight() == sched.weight_at(2)
    eb = b2.train_epoch()
    _assert_same(sa, _snapshot(b2.train_step, nets2))
    assert eb["sums"] == ea[2]["sums"] and eb["lovasz_weight"] == 1.0
