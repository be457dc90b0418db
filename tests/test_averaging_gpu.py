"""Dense weight averaging on the GPU: wtpse_avg_step / wtpse_avg_merge against their numpy restatements (wtpse_hip/averaging.py),
TrainStep(average=), TrainRun(swad=) with resume, the BatchNorm refit of averaged_checkpoint() and the NaN hold.  Every comparison
is bit for bit unless a tolerance is stated.  Sizes follow tests/test_trainer_gpu.py: B = 6, 64 x 64, bench.build_nets."""
import os
import random
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


def _next_batch(dev):
    def next_batch(py_rng, np_rng):
        return _batch(dev, int(np_rng.randint(1 << 20)) + py_rng.randint(0, 1000))
    return next_batch


def _buffers(nets):
    return [torch.cat([b.detach().reshape(-1).double() for b in n.buffers()]) for n in nets]


def _snapshot(ts, nets):
    torch.cuda.synchronize()
    opts = [ts.opt[id(n)] for n in nets]
    return dict(params=[n.flat_params().clone() for n in nets], bufs=_buffers(nets), m=[o.m.clone() for o in opts],
                v=[o.v.clone() for o in opts], packed=[n._packed.clone() for n in nets], x3=[n._x3.clone() for n in nets],
                t=[o.t for o in opts], ctr=[int(n._noise_ctr.item()) for n in nets])


def _assert_same(a, b, keys=("params", "bufs", "m", "v")):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), "%s of network %d differs" % (k, i)
    assert a["t"] == b["t"] and a["ctr"] == b["ctr"]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(t, want, what=""):
    got = _bits(t)
    want = np.asarray(want, dtype=np.float32).view(np.uint32)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d of %d elements differ" % (what, int((got != want).sum()), got.size)


# ------------------------------------------------------------------------------------------------------------ 1. kernels
SEGMENTS = [(1, 3, 0, 1_000_003), (4, 0, 5, 255), (257, 255, 1_000_003, 0), (0, 5, 4, 3), (1_000_003, 257, 1, 4)]


@pytest.mark.parametrize("sizes", SEGMENTS)
def test_avg_step_against_spec(sizes):
    """Five consecutive calls over four segments (one of them empty, with NULL pointers) that start from garbage in `a`: every mean
    equals avg_step_spec after every call, the count ends at 5; gate = 0 and hold = 1 each leave every bit and the count alone."""
    from wtpse_hip import ops
    from wtpse_hip.averaging import avg_step_spec
    L = ops.lib()
    g = torch.Generator(device="cpu").manual_seed(sum(sizes))
    a = [torch.full((n,), float("nan"), device=DEV) if n % 2 else torch.full((n,), 1e30, device=DEV) for n in sizes]
    want = [None] * 4
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    ptr = lambda t: t.data_ptr() if t.numel() else 0

    def call(p, gate=None, hold=None):
        args = []
        for x, y in zip(a, p):
            args += [ptr(x), ptr(y), x.numel()]
        L.call("wtpse_avg_step", *args, count.data_ptr(), ops.ptr(gate), ops.ptr(hold), ops.stream_ptr())

    for k in range(1, 6):
        p_host = [(1.0 + 1e-3 * torch.randn(n, generator=g)) * (3.0 if k % 2 else -0.25) for n in sizes]
        p = [x.to(DEV) for x in p_host]
        call(p)
        want = [avg_step_spec(w, x.numpy(), k) for w, x in zip(want, p_host)]
        assert int(count.item()) == k
        for s in range(4):
            _same_bits(a[s], want[s], "call %d, segment %d (n = %d)" % (k, s, sizes[s]))
    zero, one = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    p = [torch.randn(n, device=DEV) for n in sizes]
    for kw in (dict(gate=zero), dict(hold=one), dict(gate=zero, hold=one)):
        call(p, **kw)
        assert int(count.item()) == 5
        for s in range(4):
            _same_bits(a[s], want[s], "%s, segment %d" % (sorted(kw), s))
    call(p, gate=one, hold=zero)           # an open gate and a clear flag: as without either
    assert int(count.item()) == 6
    for s in range(4):
        _same_bits(a[s], avg_step_spec(want[s], p[s].cpu().numpy(), 6), "open gate, segment %d" % s)


def test_avg_step_restart_wrapper_and_arguments():
    """Zeroing the count alone restarts a segment (k == 1 copies); the wrapper pads to four segments; misaligned bases are refused."""
    from wtpse_hip import ops
    from wtpse_hip.lib import WtpseError
    a = [torch.randn(1030, device=DEV), torch.randn(7, device=DEV)]
    p = [torch.randn(1030, device=DEV), torch.randn(7, device=DEV)]
    count = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    count.zero_()
    ops.avg_step(a, p, count)
    assert int(count.item()) == 1 and torch.equal(a[0], p[0]) and torch.equal(a[1], p[1])
    with pytest.raises(WtpseError):
        ops.avg_step([a[0][1:]], [p[0][1:]], count)
    with pytest.raises(ValueError):
        ops.avg_step(a, p[:1], count)
    assert int(count.item()) == 1


@pytest.mark.parametrize("n_acc,n_seg", [(0, 7), (3, 5), (1, 1 << 20)])
@pytest.mark.parametrize("n", [5, 1_000_003])
def test_avg_merge_against_spec(n, n_acc, n_seg):
    from wtpse_hip import ops
    from wtpse_hip.averaging import avg_merge_spec
    g = torch.Generator(device="cpu").manual_seed(n + n_seg)
    acc, seg = 1.0 + 1e-2 * torch.randn(n, generator=g), 1.0 + 1e-2 * torch.randn(n, generator=g)
    out = acc.to(DEV)
    assert ops.avg_merge(out, seg.to(DEV), n_acc, n_seg) is out
    _same_bits(out, avg_merge_spec(acc.numpy(), seg.numpy(), n_acc, n_seg), "merge (%d, %d)" % (n_acc, n_seg))


# ---------------------------------------------------------------------------------------------------------- 2. TrainStep
def test_train_step_with_average():
    """Four eager steps with average=: the means equal avg_step_spec over the parameter snapshots taken after each step; the same four
    steps in plan mode give the same bits; parameters, moments and buffers are those of a step without averaging; the recorded plans
    hold exactly one more call."""
    from wtpse_hip import ops
    from wtpse_hip.averaging import WeightAverage, avg_step_spec
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    wa = WeightAverage(nets)
    ts = TrainStep(*nets, hp, lr=RATES, average=wa)
    want = [None] * 4
    for k in range(4):
        ts.step(*_batch(dev, 50 + k))
        torch.cuda.synchronize()
        want = [avg_step_spec(w, n.flat_params().cpu().numpy(), k + 1) for w, n in zip(want, nets)]
    eager = _snapshot(ts, nets)
    assert int(wa.count.item()) == 4
    for i in range(4):
        _same_bits(wa.avg[i], want[i], "eager mean of network %d" % i)

    size = lambda step: sum(ops.lib().raw("wtpse_plan_size")(p) for _, _, p in step._graphs)
    dev, hp, nets = _setup()
    wp = WeightAverage(nets)
    tp = TrainStep(*nets, hp, lr=RATES, graph="plan", average=wp)
    for k in range(4):
        tp.step(*_batch(dev, 50 + k))
    _assert_same(eager, _snapshot(tp, nets))
    assert int(wp.count.item()) == 4
    for i in range(4):
        _same_bits(wp.avg[i], want[i], "plan-mode mean of network %d" % i)
    seg, count = wp.take()
    assert count == 4 and int(wp.count.item()) == 0 and all(torch.equal(s, a) for s, a in zip(seg, wp.avg))
    with_average = size(tp)

    dev, hp, nets = _setup()
    plain = TrainStep(*nets, hp, lr=RATES, graph="plan")
    for k in range(4):
        plain.step(*_batch(dev, 50 + k))
    _assert_same(eager, _snapshot(plain, nets))              # averaging observes and never perturbs
    assert size(plain) > 1000 and with_average == size(plain) + 1

    with pytest.raises(ValueError, match="order"):
        TrainStep(*nets, hp, average=WeightAverage(nets[::-1]))
    with pytest.raises(ValueError, match="data-parallel"):
        TrainStep(*nets, hp, average=WeightAverage(nets), dp=object())


def test_segment_length_limit():
    from wtpse_hip.averaging import MAX_SEGMENT, WeightAverage
    dev, hp, nets = _setup()
    wa = WeightAverage(nets[:1])
    wa._issued = MAX_SEGMENT
    with pytest.raises(ValueError, match="2\\^24"):
        wa.update()
    assert int(wa.count.item()) == 0


# ----------------------------------------------------------------------------------------------------------- 3. TrainRun
LOSSES = [1.0, 0.5, 0.6, 2.0]          # Ns = Ne = 2: no start at 0 (1.0 > 0.5), start 1 (decided at 2), T = 0.825; the run ends with the valley open


def _scripted(run):
    return LOSSES[len(run.swad.losses)]


def _ckpt_params(ckpt_net, net):
    return torch.cat([ckpt_net[name].reshape(-1) for name, _ in net.named_parameters()])


def test_train_run_swad_and_resume(tmp_path):
    """Two epochs of four iterations, an evaluation every two: the averaged parameters equal the brute-force fold over an eager twin
    run's snapshots; a run saved after epoch 1 and continued in fresh networks writes the same swad_checkpoint, bit for bit."""
    from wtpse_hip.averaging import LossValley, avg_merge_spec, avg_step_spec
    from wtpse_hip.trainer import TrainRun
    kw = dict(iter_per_epoch=4, max_epoch=2, lr=RATES, seed=3)
    swad = lambda: dict(swad=LossValley(2, 2, 1.5), swad_every=2, swad_loss=_scripted)

    # the eager twin, without averaging: the parameters after every iteration
    dev, hp, nets = _setup()
    twin = TrainRun(*nets, hp, _next_batch(dev), graph=False, **kw)
    snaps = []
    for _ in range(8):
        twin.train_step.step(*twin.next_batch(twin.py_rng, twin.np_rng))
        torch.cuda.synchronize()
        snaps.append([n.flat_params().cpu().numpy() for n in nets])
    segments = []
    for e in range(4):
        seg = [None] * 4
        for k in (1, 2):
            seg = [avg_step_spec(s, p, k) for s, p in zip(seg, snaps[2 * e + k - 1])]
        segments.append(seg)
    want, total = [None] * 4, 0
    for e in (1, 2, 3):                      # start 1, the valley still open at the end
        want = [avg_merge_spec(w, s, total, 2) for w, s in zip(want, segments[e])]
        total += 2

    dev, hp, nets = _setup()
    out_a = str(tmp_path / "a")
    a = TrainRun(*nets, hp, _next_batch(dev), out_dir=out_a, **kw, **swad())
    a.train()
    tensors, info = a.swad.result()
    assert (info["converged"], info["start"], info["end"], info["iterates"], info["threshold"]) == \
        (True, 1, None, 6, 1.5 * float(np.mean(np.array(LOSSES[1:3], dtype=np.float64))))
    assert info["losses"] == LOSSES and info["iterations"] == [2, 4, 6, 8]
    for i in range(4):
        _same_bits(tensors[i], want[i], "averaged parameters of network %d" % i)
    # the live run still holds the LAST iterate, not the average
    for i, n in enumerate(nets):
        _same_bits(n.flat_params(), snaps[-1][i], "live parameters of network %d" % i)
    file_a = torch.load(os.path.join(out_a, "swad_checkpoint.pth.tar"), map_location="cpu", weights_only=True)
    assert file_a["swad"] == info
    for i, (key, n) in enumerate(zip(("model", "model_shape", "model_oc", "model_oc_shape"), nets)):
        _same_bits(_ckpt_params(file_a[key], n), want[i], "swad_checkpoint, %s" % key)
    with open(os.path.join(out_a, "swad.csv")) as f:
        rows = [r.strip().split(",") for r in f]
    assert rows[0] == ["evaluation", "iteration", "loss", "status"]
    assert [r[3] for r in rows[1:]] == ["outside", "merged", "merged", "held"] and [r[1] for r in rows[1:]] == ["2", "4", "6", "8"]

    # the same run, interrupted after epoch 1
    dev, hp, nets1 = _setup()
    b1 = TrainRun(*nets1, hp, _next_batch(dev), **kw, **swad())
    b1.train_epoch()
    path = str(tmp_path / "run.pth.tar")
    b1.save(path)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["config"]["swad"] == {"n_converge": 2, "n_tolerance": 2, "tolerance_ratio": 1.5} and saved["config"]["swad_every"] == 2
    assert saved["swad_state"]["valley"]["losses"] == LOSSES[:2] and saved["swad_state"]["valley"]["held_index"] == [1]
    del b1
    dev, hp, nets2 = _setup(seed=5, noise=None)
    out_b = str(tmp_path / "b")
    b2 = TrainRun.load(path, *nets2, hp, _next_batch(dev), swad_loss=_scripted, out_dir=out_b)
    assert b2.swad is not None and b2.swad_every == 2 and b2.swad.losses == LOSSES[:2] and b2.swad.held == 1
    b2.train()
    file_b = torch.load(os.path.join(out_b, "swad_checkpoint.pth.tar"), map_location="cpu", weights_only=True)
    assert file_b["swad"] == file_a["swad"]
    for key in ("model", "model_shape", "model_oc", "model_oc_shape"):
        assert list(file_a[key]) == list(file_b[key])
        for name, v in file_a[key].items():               # parameters AND BatchNorm buffers
            assert torch.equal(v, file_b[key][name]), (key, name)
        assert any(name.endswith("running_var") for name in file_a[key])

    # swad state into a run without swad: refused, as a feed's state is; a checkpoint from before the field: swad off
    with pytest.raises(ValueError, match="swad"):
        TrainRun.load(path, *nets2, hp, _next_batch(dev), swad=None)
    old = dict(saved)
    del old["swad_state"]
    old["config"] = {k: v for k, v in saved["config"].items() if not k.startswith("swad")}
    old_path = str(tmp_path / "old.pth.tar")
    torch.save(old, old_path)
    r = TrainRun.load(old_path, *nets2, hp, _next_batch(dev))
    assert r.swad is None and r.average is None and r.train_step.average is None
    with pytest.raises(ValueError, match="swad_every"):
        TrainRun(*nets2, hp, _next_batch(dev), swad=LossValley(), swad_loss=_scripted, **kw)
    with pytest.raises(ValueError, match="swad_batches"):
        TrainRun(*nets2, hp, _next_batch(dev), swad=LossValley(), swad_every=2, **kw)


class _CountingFeed:
    """A feed with state of its own: the number of batches it has handed out decides the next one."""

    def __init__(self, dev):
        self.dev, self.calls = dev, 0

    def __call__(self, py_rng, np_rng):
        self.calls += 1
        return _batch(self.dev, 1000 * self.calls + int(np_rng.randint(1 << 10)) + py_rng.randint(0, 100))

    def state(self):
        return {"calls": self.calls}

    def load_state(self, state):
        self.calls = int(state["calls"])


def _bn_layers(net):
    from wtpse_hip.nn import BNP
    return [(name, m) for name, m in net.named_modules() if isinstance(m, BNP)]


def test_averaged_checkpoint_refits_batchnorm_and_restores_the_run():
    """averaged_checkpoint(bn_batches=3): every BatchNorm has seen three batches; the running statistics of an early and a deep
    BatchNorm are the mean of the three per-batch statistics (each from a reset layer with momentum 1) within 1e-6 max|statistic| —
    three fp32 roundings plus the rounded 1/3 bound the error near 2e-7 max; the live run is bit-identical before and after; the dict
    loads through test_run's filtered load and predicts finite logits.  The default swad loss drives the evaluations."""
    from wtpse_hip.averaging import LossValley
    from wtpse_hip.test_run import load_checkpoint
    from wtpse_hip.trainer import TrainRun
    from wtpse_hip.validate import predict_pair
    dev, hp, nets = _setup()
    feed = _CountingFeed(dev)
    held_out = [_batch(dev, 90), _batch(dev, 91)]
    run = TrainRun(*nets, hp, feed, iter_per_epoch=2, max_epoch=1, lr=RATES, seed=3, swad=LossValley(1, 1, 1e9), swad_every=1,
                   swad_batches=lambda: iter(held_out))
    run.train_epoch()
    assert len(run.swad.losses) == 2 and all(0 < l < 100 for l in run.swad.losses) and run.swad.start == 0 and not run.swad.closed
    assert all(n.training for n in nets)                       # an evaluation leaves the networks in training mode
    before = _snapshot(run.train_step, nets)
    host = (run.py_rng.getstate(), run.np_rng.get_state()[1].copy(), run.np_rng.get_state()[2], feed.state())
    start_ctr = [n._noise_ctr.clone() for n in nets]

    d = run.averaged_checkpoint(bn_batches=3)

    after = _snapshot(run.train_step, nets)
    _assert_same(before, after, keys=("params", "bufs", "m", "v", "packed", "x3"))
    assert run.py_rng.getstate() == host[0] and np.array_equal(run.np_rng.get_state()[1], host[1]) and run.np_rng.get_state()[2] == host[2]
    assert feed.state() == host[3] and all(n.training for n in nets) and all(n.bn_momentum == 0.1 for n in nets)
    assert d["swad"]["iterates"] == 2 and d["swad"]["converged"]
    keys = ("model", "model_shape", "model_oc", "model_oc_shape")
    tracked = [int(v) for key in keys for name, v in d[key].items() if name.endswith("num_batches_tracked")]
    assert len(tracked) > 40 and set(tracked) == {3}
    averaged, _ = run.swad.result()
    for i, (key, n) in enumerate(zip(keys, nets)):
        assert torch.equal(_ckpt_params(d[key], n), averaged[i])

    # the three per-batch statistics, from fresh networks that carry the averaged weights and the run's Philox positions
    _, _, fresh = _setup(seed=8)
    load_checkpoint(d, *fresh)
    probe = TrainRun(*fresh, hp, feed, iter_per_epoch=1, max_epoch=1, graph=False)
    picks = []
    for i in (0, 1, 2):
        layers = _bn_layers(fresh[i])
        picks += [(i, layers[0][0], layers[0][1]), (i, layers[len(layers) // 2][0], layers[len(layers) // 2][1])]
    for n, ctr in zip(fresh, start_ctr):
        n.train(True)
        n._noise_ctr.copy_(ctr)
        object.__setattr__(n, "bn_momentum", 1.0)
    py_rng, np_rng = random.Random(3 + 1), np.random.RandomState(3 + 1)
    calls = feed.calls
    stats = []
    for k in range(3):
        for n in fresh:
            for _, m in _bn_layers(n):
                m.running_mean.zero_(); m.running_var.fill_(1.0); m.num_batches_tracked.zero_()
        probe._forward_only(*feed(py_rng, np_rng))
        stats.append([(m.running_mean.double().clone(), m.running_var.double().clone()) for _, _, m in picks])
    feed.calls = calls
    for j, (i, name, _) in enumerate(picks):
        for s, what in ((0, "running_mean"), (1, "running_var")):
            want = (stats[0][j][s] + stats[1][j][s] + stats[2][j][s]) / 3.0
            got = d[keys[i]][name + "." + what].double().to(want.device)
            err, tol = float((got - want).abs().max()), 1e-6 * float(want.abs().max())
            print("%s %s.%s: max error %.3e (tolerance %.3e)" % (keys[i], name, what, err, tol))
            assert err <= tol, (keys[i], name, what, err, tol)
            assert float(want.abs().max()) > 0

    for n in fresh:
        object.__setattr__(n, "bn_momentum", 0.1)
    load_checkpoint(d, *fresh)
    for n in fresh:
        n.eval()
    image = _batch(dev, 95)[0]
    pred, pred_oc = predict_pair(*fresh, image)
    assert bool(torch.isfinite(pred).all()) and bool(torch.isfinite(pred_oc).all())


# ---------------------------------------------------------------------------------------------------------------- 4. NaN
def _poisoned(dev, k):
    image, od, oc = _batch(dev, 60 + k)
    if k == 2:
        od = od.clone()
        od[0, 0, 0, 0] = float("nan")
    return image, od, oc


@pytest.mark.parametrize("graph", [False, "plan"])
def test_nan_holds_the_average(graph, tmp_path):
    """With the loss log's flag raised (the third of five batches is poisoned) further steps change neither means nor count, and
    train() writes no swad_checkpoint."""
    from wtpse_hip.averaging import LossValley, WeightAverage
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import LossLog, TrainRun
    dev, hp, nets = _setup()
    wa = WeightAverage(nets)
    log = LossLog(dev, TrainStep.log_names(hp))
    ts = TrainStep(*nets, hp, lr=RATES, graph=graph, log=log, average=wa)
    for k in range(2):
        ts.step(*_poisoned(dev, k))
    torch.cuda.synchronize()
    want = [a.clone() for a in wa.avg]
    assert int(wa.count.item()) == 2
    for k in range(2, 5):
        ts.step(*_poisoned(dev, k))
    assert log.read()[1] == (True, 2)
    assert int(wa.count.item()) == 2
    for i in range(4):
        assert torch.equal(wa.avg[i].view(torch.int32), want[i].view(torch.int32)), "mean of network %d moved after the NaN" % i

    dev, hp, nets = _setup()
    it = iter(range(5))
    out = tmp_path / "run"
    run = TrainRun(*nets, hp, lambda py, nr: _poisoned(dev, next(it)), iter_per_epoch=5, max_epoch=1, lr=RATES, graph=graph,
                   out_dir=str(out), swad=LossValley(1, 1, 1.5), swad_every=2, swad_loss=lambda r: 1.0)
    with pytest.raises(ValueError, match=r"loss is nan while training.*iteration 2\b"):
        run.train()
    assert len(run.swad.losses) == 1                           # the evaluation at iteration 2 ran, the one at 4 found the flag
    assert os.listdir(out) == []
    with pytest.raises(ValueError, match="loss is nan while training"):
        run.write_swad()
    assert os.listdir(out) == []
