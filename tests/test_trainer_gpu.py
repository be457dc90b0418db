"""The training-run driver on the GPU (wtpse_hip/trainer.py, the device-resident learning rate / hold flag / loss log of
wtpse_hip/step.py, wtpse_adam_dev and wtpse_loss_log).  Every comparison is bit for bit: the design makes the bits equal, no
tolerance is involved.  Sizes follow tests/test_determinism_gpu.py."""
import csv
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

pytestmark = pytest.mark.gpu
B = 6
RATES = (5e-4, 4e-4, 3e-4, 2e-4)          # (od, od_shape, oc, oc_shape): four different ones, as train.py:120-138 allows


def _setup(seed=1, noise=1234):
    import bench
    from wtpse_hip.synth import default_hparams
    dev = torch.device("cuda:0")
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
    """Everything a step moves: parameters, BatchNorm buffers, Adam moments, step counts, Philox positions."""
    torch.cuda.synchronize()
    opts = [ts.opt[id(n)] for n in nets]
    return dict(params=[n.flat_params().clone() for n in nets], bufs=_buffers(nets), m=[o.m.clone() for o in opts],
                v=[o.v.clone() for o in opts], t=[o.t for o in opts], ctr=[int(n._noise_ctr.item()) for n in nets])


def _assert_same(a, b, keys=("params", "bufs", "m", "v")):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), "%s of network %d differs" % (k, i)
    assert a["t"] == b["t"] and a["ctr"] == b["ctr"]


# ---------------------------------------------------------------------------------------------------------------- 1. Adam
@pytest.mark.parametrize("n", [1, 3, 255, 257, 1_000_003])
def test_adam_dev_bitwise_and_hold(n):
    """wtpse_adam_dev against wtpse_adam on the same operands: three consecutive steps with a device step count, for three rates;
    p, m, v bit-equal after every step.  hold = 1: the launch changes nothing; hold = 0: as without a flag."""
    from wtpse_hip import ops
    dev = torch.device("cuda:0")
    L = ops.lib()
    gen = torch.Generator().manual_seed(n)
    for lr in (5e-4, 5e-7, 1.0 / 3.0):
        lr_dev = torch.full((1,), lr, dtype=torch.float32, device=dev)
        lr_host = float(lr_dev.item())                   # (double)*lr_dev
        p0 = torch.randn(n, generator=gen).to(dev)
        ref = [p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
        got = [t.clone() for t in ref]
        flagged = [t.clone() for t in ref]
        t_ref, t_got, t_flag = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
        hold0 = torch.zeros(1, dtype=torch.int32, device=dev)
        hold1 = torch.ones(1, dtype=torch.int32, device=dev)
        for step in range(3):
            g = (torch.randn(n, generator=gen) * 0.1).to(dev)
            L.call("wtpse_adam", ref[0].data_ptr(), g.data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), n, lr_host, 0.9, 0.99, 1e-8, 1,
                   t_ref.data_ptr(), ops.stream_ptr())
            ops.counter_add(t_ref, 1)
            ops.adam_step_dev(got[0], g, got[1], got[2], lr_dev, 0.9, 0.99, 1e-8, 1, t_got, None)
            ops.counter_add(t_got, 1)
            for a, b, what in zip(ref, got, "pmv"):
                assert torch.equal(a, b), "n=%d lr=%g step %d: %s differs in %d elements" % (n, lr, step, what, int((a != b).sum()))
            # held: nothing moves
            before = [t.clone() for t in flagged]
            ops.adam_step_dev(flagged[0], g, flagged[1], flagged[2], lr_dev, 0.9, 0.99, 1e-8, 1, t_flag, hold1)
            for a, b, what in zip(before, flagged, "pmv"):
                assert torch.equal(a, b), "hold = 1 changed %s" % what
            # hold = 0: the same step as without a flag
            ops.adam_step_dev(flagged[0], g, flagged[1], flagged[2], lr_dev, 0.9, 0.99, 1e-8, 1, t_flag, hold0)
            ops.counter_add(t_flag, 1)
            for a, b, what in zip(ref, flagged, "pmv"):
                assert torch.equal(a, b), "hold = 0: %s differs" % what
        assert int(t_ref.item()) == int(t_got.item()) == 3
        assert not torch.equal(ref[0], p0)


def test_loss_log_kernel():
    """wtpse_loss_log alone: double sums of fp32 scalars in call order, null trailing scalars, the fp32 NaN test in the
    reference's order ((s0 + s1) + s2; inf + -inf counts), the sticky flag with the step count of its first raise."""
    from wtpse_hip import ops
    dev = torch.device("cuda:0")
    acc = torch.zeros(8, dtype=torch.float64, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    vals = [[0.1, 0.2, 0.3, 1e-8, 5.0, 7.0], [1e10, 3.0, -2.0, 4.0, 0.25, 0.5], [1 / 3, 2 / 3, 1e-20, 9.0, 8.0, 1.5]]
    want = [0.0] * 6
    for row in vals:
        s = torch.tensor(row, dtype=torch.float32, device=dev)
        ops.loss_log([s[j] for j in range(6)], acc, 1, 3, flag, t_dev)
        ops.counter_add(t_dev, 1)
        for j in range(6):
            want[j] += float(s[j])                       # the reference: running += loss.item()
    assert acc.tolist() == [0.0] + want + [0.0]
    assert flag.tolist() == [0, 0]
    # trailing scalars missing, no test
    s = torch.tensor([2.0, float("nan")], dtype=torch.float32, device=dev)
    ops.loss_log([s[0], s[1]], acc, 6, 0, flag, t_dev)
    got = acc.tolist()
    assert got[6] == want[5] + 2.0 and got[7] != got[7] and flag.tolist() == [0, 0]
    # check_n = 1 looks at s0 only
    ops.loss_log([s[0], s[1]], acc, 6, 1, flag, t_dev)
    assert flag.tolist() == [0, 0]
    # inf + -inf is a NaN of the sum; the flag names the step count and is sticky
    s = torch.tensor([float("inf"), float("-inf"), 1.0], dtype=torch.float32, device=dev)
    ops.loss_log([s[0], s[1], s[2]], acc, 0, 3, flag, t_dev)
    assert flag.tolist() == [1, 3]
    ops.counter_add(t_dev, 1)
    ops.loss_log([s[0], s[1], s[2]], acc, 0, 3, flag, t_dev)
    assert flag.tolist() == [1, 3]


def test_loss_log_codes_are_counts():
    """Every accepted check_n NaN-tests the fp32 sum of the first k scalars and nothing else (the table of include/wtpse_hip.h), with
    six scalars given: a NaN in slot j raises the flag exactly when j < k; +inf in slot 0 with -inf in slot k - 1 raises (k >= 2),
    with the -inf in slot k it does not (1 <= k <= 5; k = 0 has no such pair, and its six NaN cases show that no slot is tested);
    the sums take all six values in every case; the two names of k = 3 and of k = 4 give the same flag and sums."""
    from wtpse_hip import ops
    dev = torch.device("cuda:0")
    nan, inf = float("nan"), float("inf")
    step = torch.full((1,), 7, dtype=torch.int32, device=dev)
    got = {}
    for code, k in {0: 0, 1: 1, 17: 2, 3: 3, 49: 3, 19: 4, 35: 4, 51: 5}.items():
        cases = [({j: nan}, j < k) for j in range(6)]
        if k >= 2:
            cases.append(({0: inf, k - 1: -inf}, True))
        if k >= 1:
            cases.append(({0: inf, k: -inf}, False))
        for put, raised in cases:
            vals = [put.get(j, float(j + 1)) for j in range(6)]
            s = torch.tensor(vals, dtype=torch.float32, device=dev)
            acc = torch.zeros(6, dtype=torch.float64, device=dev)
            flag = torch.zeros(2, dtype=torch.int32, device=dev)
            ops.loss_log([s[j] for j in range(6)], acc, 0, code, flag, step)
            print("check_n %d (k = %d), %s: flag %s" % (code, k, vals, flag.tolist()))
            assert flag.tolist() == ([1, 7] if raised else [0, 0]), (code, vals)
            assert all((a != a) if (b != b) else a == b for a, b in zip(acc.tolist(), vals)), (code, vals, acc.tolist())
            got[code, repr(vals)] =(flag.tolist(), [repr(a) for a in acc.tolist()])
    for a, b in ((3, 49), (19, 35)):
        mine = {case: r for (code, case), r in got.items() if code == a}
        assert mine and mine == {case: r for (code, case), r in got.items() if code == b}, (a, b)


# ------------------------------------------------------------------------------------------- 2. schedule under replay
def _scheduled_run(graph, change=True):
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import reference_lr
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES, graph=graph)
    losses = []
    for k in range(6):
        if change and k == 2:
            ts.set_lr(*[r * 0.5 for r in RATES])
        if change and k == 4:
            ts.set_lr(*[reference_lr(120, 200, r) for r in RATES])
        res = ts.step(*_batch(dev, 10 + k))
        losses.append({k2: float(v) for k2, v in res.items()})
    snap = _snapshot(ts, nets)
    assert (ts._graphs is not None) == bool(graph)
    if change:
        assert ts.get_lr() == dict(zip(("od", "od_shape", "oc", "oc_shape"), (reference_lr(120, 200, r) for r in RATES)))
    return snap, losses


@pytest.mark.parametrize("mode", ["plan", True])
def test_lr_schedule_under_replay(mode):
    """Six steps with the four rates changed before steps 2 and 4: eager against the recorded modes.  A recorded step that took the
    rate by value would keep the first one."""
    se, le = _scheduled_run(False)
    sg, lg = _scheduled_run(mode)
    assert se["t"] == [6, 6, 6, 6]
    assert all(v == v for d in le for v in d.values()), le
    assert le == lg
    _assert_same(se, sg)
    # ... and the changes are not a no-op: the same six steps at the first rates end elsewhere
    s0, _ = _scheduled_run(False, change=False)
    assert all(not torch.equal(x, y) for x, y in zip(s0["params"], se["params"]))


def test_four_rates_reach_their_networks():
    """lr as a 4-tuple: one step from zero moments moves every parameter with a non-zero gradient by its network's rate
    (Adam's first step is lr * g / (|g| + eps)), so the largest move of each network is its own rate."""
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    before = [n.flat_params().clone() for n in nets]
    ts = TrainStep(*nets, hp, lr=RATES)
    ts.step(*_batch(dev, 3))
    torch.cuda.synchronize()
    for n, p0, r in zip(nets, before, RATES):
        move = float((n.flat_params() - p0).abs().max())
        # the difference of two fp32 parameters of magnitude < 4 is exact to half an ulp of 4 (2.4e-7); the rates differ by 1e-4
        assert abs(move - r) < 2.5e-7 + 1e-5 * r, (move, r)
    with pytest.raises(ValueError, match="four"):
        TrainStep(*nets, hp, lr=(1e-3, 1e-3))


# ---------------------------------------------------------------------------------------------------------- 3. resume
def _next_batch(dev):
    def next_batch(py_rng, np_rng):
        # both host generators decide the batch, so both have to survive a checkpoint
        return _batch(dev, int(np_rng.randint(1 << 20)) + py_rng.randint(0, 1000))
    return next_batch


def _rows(out_dir):
    with open(os.path.join(out_dir, "train_log.csv"), newline="") as f:
        return [r[:-1] for r in csv.reader(f)]          # elapsed seconds aside


@pytest.mark.parametrize("graph", [False, "plan"])
def test_resume_continues_bitwise(graph, tmp_path):
    """Two epochs of three iterations run through, against: one epoch, save, NEW networks and a new TrainRun from load, one more
    epoch (the rates changed after the first epoch, so they have to travel with the optimiser state)."""
    from wtpse_hip.trainer import TrainRun, reference_lr
    new_rates = [reference_lr(0, 2, r) * 100 for r in RATES]
    kw = dict(iter_per_epoch=3, max_epoch=2, lr=RATES, graph=graph, seed=7)

    dev, hp, nets = _setup()
    a = TrainRun(*nets, hp, _next_batch(dev), out_dir=str(tmp_path / "a"), **kw)
    a.train_epoch()
    a.train_step.set_lr(*new_rates)
    ea = a.train_epoch()
    sa = _snapshot(a.train_step, nets)

    dev, hp, nets1 = _setup()
    b1 = TrainRun(*nets1, hp, _next_batch(dev), out_dir=str(tmp_path / "b"), **kw)
    e0 = b1.train_epoch()
    b1.train_step.set_lr(*new_rates)
    path = str(tmp_path / "b" / "run.pth.tar")
    b1.save(path)
    assert sorted(os.listdir(tmp_path / "b")) == ["run.pth.tar", "train_log.csv"]
    del b1

    dev, hp, nets2 = _setup(seed=5, noise=None)         # other weights, default Philox seed: everything comes from the file
    assert not torch.equal(nets2[0].flat_params(), nets1[0].flat_params())
    b2 = TrainRun.load(path, *nets2, hp, _next_batch(dev), out_dir=str(tmp_path / "b"), graph=graph)
    assert (b2.epoch, b2.iteration, b2.max_epoch, b2.iter_per_epoch, b2.seed) == (1, 3, 2, 3, 7)
    assert b2.last["sums"] == e0["sums"]
    assert [b2.train_step.get_lr()[k] for k in ("od", "od_shape", "oc", "oc_shape")] == new_rates
    eb = b2.train_epoch()
    sb = _snapshot(b2.train_step, nets2)

    _assert_same(sa, sb)
    assert sa["t"] == [6, 6, 6, 6]
    assert ea["sums"] == eb["sums"] and ea["means"] == eb["means"] and ea["lr"] == eb["lr"] and ea["epoch"] == eb["epoch"] == 1
    assert all(v == v for v in ea["sums"].values())
    ra, rb = _rows(str(tmp_path / "a")), _rows(str(tmp_path / "b"))
    assert len(ra) == 3 and ra == rb                      # header + one line per epoch
    # the checkpoint is plain data, and the best-Dice checkpoint's reader finds its four networks in it
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert {"model", "model_shape", "model_oc", "model_oc_shape", "train_step", "epoch", "iteration", "py_rng", "np_rng"} <= set(d)


def test_load_state_into_recorded_step():
    """load_state_dict into a TrainStep that has already replayed its plan, then one more step == the same done eagerly: the state
    is copied into the buffers the recording reads.  A different Philox seed is refused (it is frozen into the recording)."""
    from wtpse_hip.step import TrainStep
    dev, hp, nets = _setup()
    eager = TrainStep(*nets, hp, lr=RATES)
    eager.step(*_batch(dev, 40))
    eager.set_lr(*[r * 0.25 for r in RATES])
    torch.cuda.synchronize()
    state = eager.state_dict()
    weights = [{k: v.clone() for k, v in n.state_dict().items()} for n in nets]
    eager.step(*_batch(dev, 41))
    want = _snapshot(eager, nets)

    dev, hp, nets2 = _setup(seed=5)
    rec = TrainStep(*nets2, hp, lr=1e-3, graph="plan")
    rec.step(*_batch(dev, 99))                           # records, then replays the plan once
    rec.step(*_batch(dev, 98))
    torch.cuda.synchronize()
    ptrs = [(o.m.data_ptr(), o.v.data_ptr(), o.t_dev.data_ptr(), o.lr_dev.data_ptr()) for o in rec.opt.values()]
    for n, w in zip(nets2, weights):
        n.load_state_dict(w)
    rec.load_state_dict(state)
    assert ptrs == [(o.m.data_ptr(), o.v.data_ptr(), o.t_dev.data_ptr(), o.lr_dev.data_ptr()) for o in rec.opt.values()]
    graphs = rec._graphs
    rec.step(*_batch(dev, 41))
    assert rec._graphs is graphs                         # the same recording
    got = _snapshot(rec, nets2)
    _assert_same(want, got)
    assert want["t"] == [2, 2, 2, 2]

    other = dict(state, noise={k: dict(v, seed=v["seed"] + 1) for k, v in state["noise"].items()})
    with pytest.raises(ValueError, match="seed"):
        rec.load_state_dict(other)
    fresh = TrainStep(*_setup(seed=6)[2], hp)            # no recording yet: the seed is simply taken over
    fresh.load_state_dict(other)
    assert all(n._noise_seed == 1235 for n in fresh.nets)


def _fundus_feed(root, dev, record):
    """FundusBatches over the synthetic PNG tree (three source domains with pools of 3, 4 and 3 samples), recording what it hands out."""
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.trainer import FundusBatches

    class Recorded(FundusBatches):
        def __call__(self, py_rng, np_rng):
            batch = super().__call__(py_rng, np_rng)
            record.append((list(self.order), [t.clone() for t in batch]))
            return batch

    return Recorded([FundusTree(root, "train", (i,), size=64) for i in (1, 2, 3)], B, dev, size=64)


@pytest.mark.parametrize("graph", [False, "plan"])
def test_resume_on_the_dataset_feed(graph, tmp_path):
    """The resume comparison on the feed a real run uses: FundusBatches on a seeded synthetic PNG tree.  The feed shuffles its domain
    list cumulatively (Trainer.py:769), so the order it has reached is run state: a NEW feed, built in construction order, must
    continue with the batches the uninterrupted run draws — same domain order, same samples, same crops — and end on the same bits."""
    from oracle.fundus_tree import make_tree
    from wtpse_hip.trainer import TrainRun
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    kw = dict(iter_per_epoch=3, max_epoch=2, lr=RATES, graph=graph, seed=3)

    dev, hp, nets = _setup()
    seen_a = []
    a = TrainRun(*nets, hp, _fundus_feed(root, dev, seen_a), **kw)
    a.train_epoch()
    ea = a.train_epoch()
    sa = _snapshot(a.train_step, nets)

    dev, hp, nets1 = _setup()
    seen_b = []
    b1 = TrainRun(*nets1, hp, _fundus_feed(root, dev, seen_b), **kw)
    b1.train_epoch()
    path = str(tmp_path / "run.pth.tar")
    b1.save(path)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    # the case is a real one: the order the first epoch left is not the order a new feed starts from
    assert saved["feed"] == {"order": seen_b[-1][0]} and saved["feed"]["order"] != [0, 1, 2]
    del b1

    dev, hp, nets2 = _setup(seed=5, noise=None)
    feed = _fundus_feed(root, dev, seen_b)
    assert feed.order == [0, 1, 2]
    b2 = TrainRun.load(path, *nets2, hp, feed)
    assert feed.order == saved["feed"]["order"] and b2.graph == graph
    eb = b2.train_epoch()
    sb = _snapshot(b2.train_step, nets2)

    assert len(seen_a) == len(seen_b) == 6
    for k, ((oa, ba), (ob, bb)) in enumerate(zip(seen_a, seen_b)):
        assert oa == ob, "iteration %d: domain order %s against %s" % (k, oa, ob)
        for x, y, what in zip(ba, bb, ("image", "target_od", "target_oc")):
            assert torch.equal(x, y), "iteration %d: %s differs" % (k, what)
    assert len({tuple(o) for o, _ in seen_a}) > 1         # the order does move between iterations
    _assert_same(sa, sb)
    assert ea["sums"] == eb["sums"] and all(v == v for v in ea["sums"].values())
    # a feed that cannot take the saved state is refused, not silently restarted
    with pytest.raises(ValueError, match="feed"):
        TrainRun.load(path, *nets2, hp, _next_batch(dev))
    with pytest.raises(ValueError, match="permutation"):
        feed.load_state({"order": [0, 0, 1]})


# -------------------------------------------------------------------------------------------------------- 4. loss log
def test_loss_log_equals_item_sums():
    """An eager run that reads every returned scalar with float() and adds it to a Python float per name, in order — what the
    reference's running sums do — against the LossLog of an identical run in plan mode: the doubles are ==."""
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import LossLog
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES)
    sums = {}
    for k in range(4):
        res = ts.step(*_batch(dev, 50 + k))
        for name, v in res.items():
            sums[name] = sums.get(name, 0.0) + float(v)
    plain = _snapshot(ts, nets)

    dev, hp, nets = _setup()
    log = LossLog(dev, TrainStep.log_names(hp))
    ts = TrainStep(*nets, hp, lr=RATES, graph="plan", log=log)
    for k in range(4):
        ts.step(*_batch(dev, 50 + k))
    got, (nan, _) = log.read()
    assert not nan
    assert set(got) == set(sums) and len(got) == 14
    for name in got:
        assert got[name] == sums[name], (name, got[name], sums[name])
    _assert_same(plain, _snapshot(ts, nets))             # logging moves nothing else
    log.reset()
    assert log.read() == ({k: 0.0 for k in got}, (False, 0))
    with pytest.raises(ValueError, match="log_names"):
        TrainStep(*nets, hp, log=LossLog(dev, ["seg_od"]))


# ------------------------------------------------------------------------------------------------------------- 5. NaN
def _poisoned(dev, k):
    image, od, oc = _batch(dev, 60 + k)
    if k == 2:
        od = od.clone()
        od[0, 0, 0, 0] = float("nan")       # BCE's t * log(p) + (1 - t) * log(1 - p) carries a NaN target into the loss by arithmetic
    return image, od, oc


@pytest.mark.parametrize("graph", [False, "plan"])
def test_nan_stops_the_run(graph, tmp_path):
    """Five iterations with the third batch poisoned so that seg_od is NaN.  After the five, the parameters and Adam moments of all
    four networks are what they were after the first two iterations, train_epoch() raises the reference's ValueError naming
    iteration 2, and nothing was written."""
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import TrainRun
    # precondition, eagerly: the poison reaches the loss
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES)
    seg = [float(ts.step(*_poisoned(dev, k))["seg_od"]) for k in range(3)]
    assert seg[0] == seg[0] and seg[1] == seg[1] and seg[2] != seg[2], seg
    # the state after the first two iterations, from a run of those two alone
    dev, hp, nets = _setup()
    it = iter(range(5))
    two = TrainRun(*nets, hp, lambda py, nr: _poisoned(dev, next(it)), iter_per_epoch=2, max_epoch=1, lr=RATES, graph=graph)
    two.train_epoch()
    want = _snapshot(two.train_step, nets)
    # the run
    dev, hp, nets = _setup()
    it = iter(range(5))
    out = tmp_path / "run"
    run = TrainRun(*nets, hp, lambda py, nr: _poisoned(dev, next(it)), iter_per_epoch=5, max_epoch=1, lr=RATES, graph=graph,
                   out_dir=str(out), checkpoint_every=1)
    with pytest.raises(ValueError, match=r"loss is nan while training.*iteration 2\b"):
        run.train_epoch()
    got = _snapshot(run.train_step, nets)
    for k in ("params", "m", "v"):
        for i, (x, y) in enumerate(zip(want[k], got[k])):
            assert torch.equal(x, y), "%s of network %d moved after the NaN" % (k, i)
    assert got["t"] == [5, 5, 5, 5]                       # the step counters are not held
    assert os.listdir(out) == []
    with pytest.raises(ValueError, match="loss is nan while training"):
        run.save(str(out / "ckpt.pth.tar"))
    assert os.listdir(out) == []


# ------------------------------------------------------------------------------------------------------------- 6. run
def _load_filtered(net, pretrained_dict):
    """test_visulization.py:132-140, as tests/test_checkpoint_gpu.py restates it."""
    model_dict = net.state_dict()
    pretrained_dict = {k: v for k, v in pretrained_dict.items() if k in model_dict}
    model_dict.update(pretrained_dict)
    net.load_state_dict(model_dict)


def test_train_run_order_and_checkpoints(tmp_path):
    """TrainRun.train() over 5 epochs x 2 iterations with validation every epoch: the Validator runs for epochs 3 and 4 only
    (Trainer.py:1048: epoch > 2), stop_epoch ends the loop before that epoch's validation, the six returned values come in the
    reference's order, and both kinds of checkpoint load through the filtered-load sequence of test_visulization.py:132-193."""
    from wtpse_hip.trainer import TrainRun, reference_lr
    from wtpse_hip.validate import Validator

    class Recording(Validator):
        def __call__(self, epoch, *a):
            r = super().__call__(epoch, *a)
            calls.append((epoch, r[0], dict(self.last)))
            return r

    def run(stop_epoch, out):
        dev, hp, nets = _setup()
        val = [_batch(dev, 90), _batch(dev, 91)]
        os.makedirs(out, exist_ok=True)
        r = TrainRun(*nets, hp, _next_batch(dev), iter_per_epoch=2, max_epoch=5, lr=RATES, stop_epoch=stop_epoch, val_batches=val,
                     validator=Recording(out_dir=out, metrics="device"), interval_validate=1, lr_schedule="reference", out_dir=out,
                     seed=3, checkpoint_every=2)
        return r, r.train(), nets

    calls = []
    r, best, nets = run(-1, str(tmp_path / "full"))
    assert [c[0] for c in calls] == [3, 4]
    assert calls[0][1] == 1                               # the first validation is always a new best (Dice > 0)
    m = [c[2] for c in calls if c[1] == 1][-1]
    assert best == [m["cup_dice"], m["cup_hd"], m["cup_asd"], m["disc_dice"], m["disc_hd"], m["disc_asd"]]
    assert r.epoch == 5 and r.iteration == 10
    # the schedule: after epoch e the rates are reference_lr(e, ...) of the SEGMENTATION networks' base rates, for the shape nets too
    od, oc = reference_lr(4, 5, RATES[0]), reference_lr(4, 5, RATES[2])
    assert r.train_step.get_lr() == {"od": od, "od_shape": od, "oc": oc, "oc_shape": oc}
    rows = _rows(str(tmp_path / "full"))
    assert [row[0] for row in rows[1:]] == ["0", "1", "2", "3", "4"] and [row[1] for row in rows[1:]] == ["2", "4", "6", "8", "10"]
    assert float(rows[1][rows[0].index("lr_od")]) == RATES[0] and float(rows[2][rows[0].index("lr_od_shape")]) == reference_lr(0, 5, RATES[0])
    # checkpoints: the best one (Trainer.py:282-288) and the run's own, both through the filtered load
    files = sorted(os.listdir(tmp_path / "full"))
    assert "run_checkpoint.pth.tar" in files and "checkpoint_%d.pth.tar" % r.validator.best_epoch in files
    for name in ("checkpoint_%d.pth.tar" % r.validator.best_epoch, "run_checkpoint.pth.tar"):
        ckpt = torch.load(str(tmp_path / "full" / name), map_location="cpu", weights_only=True)
        _, _, fresh = _setup(seed=8)
        for n, key in zip(fresh, ("model", "model_shape", "model_oc", "model_oc_shape")):
            _load_filtered(n, ckpt[key])
            for k, v in n.state_dict().items():
                assert torch.equal(v.cpu(), ckpt[key][k]), (name, key, k)
    run_ckpt = torch.load(str(tmp_path / "full" / "run_checkpoint.pth.tar"), map_location="cpu", weights_only=True)
    assert run_ckpt["epoch"] == 4 and run_ckpt["iteration"] == 8         # written after epochs 1 and 3 (checkpoint_every = 2)

    # a run continued from that checkpoint (written after epoch 3, whose validation was the first best) knows the six best values,
    # so it returns them when it finds no new best; and the log's line of epoch 4, which the checkpoint has not seen, is dropped
    dev, hp, fresh = _setup(seed=8, noise=None)
    first = calls[0][2]
    r2 = TrainRun.load(str(tmp_path / "full" / "run_checkpoint.pth.tar"), *fresh, hp, _next_batch(dev), val_batches=[_batch(dev, 90)],
                       validator=Recording(metrics="device"), out_dir=str(tmp_path / "full"))
    assert r2.best == [first[k] for k in ("cup_dice", "cup_hd", "cup_asd", "disc_dice", "disc_hd", "disc_asd")]
    assert (r2.epoch, r2.iteration, r2.validator.best_epoch, r2.graph, r2.lr_schedule) == (4, 8, 4, "plan", "reference")
    assert [row[0] for row in _rows(str(tmp_path / "full"))[1:]] == ["0", "1", "2", "3"]

    calls.clear()
    r, best, _ = run(4, str(tmp_path / "stopped"))
    assert [c[0] for c in calls] == [3]                   # epoch 4 is trained, then the loop ends before its validation
    assert r.epoch == 5


# --------------------------------------------------------------------------------------------------------- 7. interop
def test_optimizer_state_interop_with_torch_adam():
    """Two iterations of calls A and B through the drop-in path with torch.optim.Adam (update() -> torch loss glue -> backward()
    -> optim.step(), as tests/test_parity_gpu.py::test_iterations_dropin_vs_golden drives it); optim.state_dict() ->
    FlatAdam.load_state_dict: m / v are the flattened exp_avg / exp_avg_sq, t == 2, the rate travels; and back."""
    from wtpse_hip.step import FlatAdam
    dev, hp, nets = _setup()
    model, shape = nets[0], nets[1]
    opts = [torch.optim.Adam(n.parameters(), lr=r, betas=(0.9, 0.99)) for n, r in zip((model, shape), RATES)]
    bce = torch.nn.BCELoss()
    for n in nets:
        n.train()
    for k in range(2):
        image, od, _ = _batch(dev, 70 + k)
        opts[0].zero_grad(); model.zero_grad()
        output, _, _, ins, dom = model.update(image, od, two_stage_inputs=image, sp_mask=od, two_step=True)
        (bce(torch.sigmoid(output), od) + ins + dom).backward()
        opts[0].step()
        opts[1].zero_grad(); shape.zero_grad()
        kd, ins_t, _, _, dom_s = shape.update(model, image, od, two_stage_inputs=image, two_step=True)
        (kd + ins_t + dom_s).backward()
        opts[1].step()
    torch.cuda.synchronize()
    for net, opt, rate in zip((model, shape), opts, RATES):
        params = list(net.parameters())
        # (torch keeps no state for a parameter that never had a gradient: zero moments on the flat side)
        zeros = lambda p, k: opt.state[p][k].reshape(-1) if p in opt.state else torch.zeros(p.numel(), device=dev)
        fa = FlatAdam(net, lr=1.0)
        fa.load_state_dict(opt.state_dict())
        assert fa.t == 2 and fa.lr == rate and float(fa.lr_dev.item()) == float(torch.tensor(rate, dtype=torch.float32))
        assert torch.equal(fa.m, torch.cat([zeros(p, "exp_avg") for p in params]))
        assert torch.equal(fa.v, torch.cat([zeros(p, "exp_avg_sq") for p in params]))
        assert bool(fa.m.any()) and bool(fa.v.any())
        # and back: a fresh torch.optim.Adam takes FlatAdam's state
        back = torch.optim.Adam(params, lr=9.0)
        back.load_state_dict(fa.state_dict())
        assert back.param_groups[0]["lr"] == rate and tuple(back.param_groups[0]["betas"]) == (0.9, 0.99)
        for p in params:
            assert float(back.state[p]["step"]) == 2.0
            assert torch.equal(back.state[p]["exp_avg"].reshape(-1), zeros(p, "exp_avg"))
            assert torch.equal(back.state[p]["exp_avg_sq"].reshape(-1), zeros(p, "exp_avg_sq"))
