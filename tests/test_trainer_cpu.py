"""Host-side parts of the training-run driver (wtpse_hip/trainer.py, the optimiser-state conversion of wtpse_hip/step.py) and the
boundary of its two entry points: nothing here needs a GPU."""
import io
import os
import random
from bisect import bisect_right

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_lr_restated():
    """Trainer.lr_update (Trainer.py:989-1004, constants of :1016-1021) for every epoch of a 200-epoch run, against an independent
    restatement and three hand values."""
    from wtpse_hip.trainer import reference_lr
    M = 200
    for base in (5e-4, 1e-3):
        for e in range(M):
            alpha = e / (2 * M)
            wf = 0.001 * (1 - alpha) + alpha
            want = base * wf * 0.5 ** bisect_right((100, 150), e)
            assert reference_lr(e, M, base) == pytest.approx(want, rel=1e-12), e
    assert reference_lr(0, M, 5e-4) == pytest.approx(5e-7, rel=1e-12)
    assert reference_lr(100, M, 5e-4) == pytest.approx(6.26875e-5, rel=1e-12)
    assert reference_lr(150, M, 5e-4) == pytest.approx(4.6953125e-5, rel=1e-12)
    # the warm-up never completes: the factor at the last epoch is still about one half
    assert reference_lr(M - 1, M, 1.0, steps=()) < 0.51


def test_adam_state_in_torch_layout():
    """What FlatAdam.state_dict() is made of (step.adam_state_to_torch) is accepted by torch.optim.Adam over parameters of the same
    shapes; exp_avg / exp_avg_sq are the matching slices of the flat m / v; and the way back fills the flat buffers in place."""
    from wtpse_hip.step import adam_state_to_torch, adam_state_from_torch
    shapes = [(4, 3, 3, 3), (4,), (2, 4), (1,)]
    n = sum(int(np.prod(s)) for s in shapes)
    g = torch.Generator().manual_seed(3)
    m, v = torch.randn(n, generator=g), torch.rand(n, generator=g)
    sd = adam_state_to_torch(m, v, 7, shapes, 2.5e-4, (0.9, 0.99), 1e-8)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    opt = torch.optim.Adam(params, lr=1.0, betas=(0.5, 0.5))
    opt.load_state_dict(sd)
    grp = opt.param_groups[0]
    assert grp["lr"] == 2.5e-4 and tuple(grp["betas"]) == (0.9, 0.99) and grp["eps"] == 1e-8
    assert grp["weight_decay"] == 0 and grp["amsgrad"] is False
    off = 0
    for p, s in zip(params, shapes):
        k = int(np.prod(s))
        st = opt.state[p]
        assert float(st["step"]) == 7.0
        assert torch.equal(st["exp_avg"], m[off:off + k].view(s)) and torch.equal(st["exp_avg_sq"], v[off:off + k].view(s))
        off += k
    # torch's optimiser takes a step from that state without complaint
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    assert float(opt.state[params[0]]["step"]) == 8.0
    # and back, into existing buffers
    m2, v2 = torch.zeros(n), torch.zeros(n)
    pm, pv = m2.data_ptr(), v2.data_ptr()
    opt2 = torch.optim.Adam(params, lr=1.0)
    opt2.load_state_dict(adam_state_to_torch(m, v, 7, shapes, 2.5e-4, (0.9, 0.99), 1e-8))      # (opt.step() moved sd's tensors)
    t, grp = adam_state_from_torch(opt2.state_dict(), shapes, m2, v2)
    assert t == 7 and grp["lr"] == 2.5e-4
    assert torch.equal(m2, m) and torch.equal(v2, v) and (m2.data_ptr(), v2.data_ptr()) == (pm, pv)
    # an optimiser that has not stepped: empty state = step 0, zero moments
    t, _ = adam_state_from_torch(torch.optim.Adam(params, lr=1.0).state_dict(), shapes, m2, v2)
    assert t == 0 and not m2.any() and not v2.any()


def test_adam_state_refusals():
    from wtpse_hip.step import adam_state_to_torch, adam_state_from_torch
    shapes = [(3,), (2, 2)]
    m, v = torch.zeros(7), torch.zeros(7)
    sd = adam_state_to_torch(m, v, 3, shapes, 1e-3, (0.9, 0.99), 1e-8)
    sd["state"][1]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match="step counts differ"):
        adam_state_from_torch(sd, shapes, m, v)
    sd = adam_state_to_torch(m, v, 3, shapes, 1e-3, (0.9, 0.99), 1e-8)
    sd["param_groups"][0]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="weight_decay"):
        adam_state_from_torch(sd, shapes, m, v)
    sd = adam_state_to_torch(m, v, 3, shapes, 1e-3, (0.9, 0.99), 1e-8)
    with pytest.raises(ValueError, match="shape"):
        adam_state_from_torch(sd, [(3,), (4,)], m, v)
    # a parameter torch.optim.Adam never saw a gradient for has no entry: zero moments, the others' step count
    sd = adam_state_to_torch(torch.arange(7.), torch.arange(7.) + 1, 3, shapes, 1e-3, (0.9, 0.99), 1e-8)
    del sd["state"][0]
    m, v = torch.full((7,), 9.0), torch.full((7,), 9.0)
    t, _ = adam_state_from_torch(sd, shapes, m, v)
    assert t == 3 and m.tolist() == [0, 0, 0, 3, 4, 5, 6] and v.tolist() == [0, 0, 0, 4, 5, 6, 7]


def test_entry_points_declared_exported_recordable():
    """The header declares wtpse_adam_dev and wtpse_loss_log (and still wtpse_adam, with its signature), the built library exports
    them, and both can be recorded into a launch plan (wtpse_plan_fn_name lists them)."""
    import ctypes
    from wtpse_hip import build
    from wtpse_hip.lib import LIB_PATH
    protos = build.parse_prototypes()
    assert protos["wtpse_adam"] == ["float*", "const float*", "float*", "float*", "long long", "double", "double", "double", "double",
                                    "int", "const int*", "void*"]
    assert protos["wtpse_adam_dev"] == ["float*", "const float*", "float*", "float*", "long long", "const float*", "double", "double",
                                        "double", "int", "const int*", "const int*", "void*"]
    assert protos["wtpse_loss_log"] == ["const float*"] * 6 + ["double*", "int", "int*", "const int*", "void*"]
    build.build()
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("wtpse_adam", "wtpse_adam_dev", "wtpse_loss_log"):
        assert hasattr(dll, name), name
    dll.wtpse_plan_fn_name.restype = ctypes.c_char_p
    names = {dll.wtpse_plan_fn_name(i).decode() for i in range(dll.wtpse_plan_fn_count())}
    assert {"wtpse_adam", "wtpse_adam_dev", "wtpse_loss_log"} <= names


def test_loss_log_argument_checks():
    """The launchers refuse what the header rules out before anything is launched (status -1).  Every non-null pointer below is real
    memory of the right size — device memory where there is a GPU — so that a missing check shows as a wrong status, never as a
    launch on an address nobody owns."""
    import ctypes
    from wtpse_hip import build
    from wtpse_hip.lib import LIB_PATH
    build.build()
    gpu = torch.cuda.is_available()
    if gpu:
        torch.cuda.init()
    dll = ctypes.CDLL(LIB_PATH)
    keep = []

    def mem(n, dtype):
        t = torch.zeros(n, dtype=dtype, device="cuda" if gpu else "cpu")
        keep.append(t)
        return t.data_ptr()

    fn = dll.wtpse_loss_log
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    s, acc, flag, t = mem(1, torch.float32), mem(6, torch.float64), mem(2, torch.int32), mem(1, torch.int32)
    assert fn(None, None, None, None, None, None, acc, 0, flag, t, None) == -1       # s0 missing
    assert fn(s, None, None, None, None, None, None, 0, flag, t, None) == -1         # acc missing
    assert fn(s, None, None, None, None, None, acc, 0, None, t, None) == -1          # flag missing
    assert fn(s, s, s, None, None, None, acc, 2, flag, t, None) == -1                # check_n not in {0, 1, 3}
    assert fn(s, s, None, None, None, None, acc, 3, flag, t, None) == -1             # a tested scalar missing
    ad = dll.wtpse_adam_dev
    ad.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    ad.restype = ctypes.c_int
    p, g, m, v, lr = (mem(8, torch.float32) for _ in range(5))
    assert ad(p, g, m, v, 8, None, 0.9, 0.99, 1e-8, 1, None, None, None) == -1       # lr_dev missing
    assert ad(p, g, m, v, 0, lr, 0.9, 0.99, 1e-8, 1, None, None, None) == -1         # n == 0
    assert ad(p, g, m, v, 8, lr, 0.9, 0.99, 1e-8, 0, None, None, None) == -1         # step < 1


LOSS_LOG_COUNTS = {0: 0, 1: 1, 17: 2, 3: 3, 49: 3, 19: 4, 35: 4, 51: 5}      # check_n -> tested scalars (include/wtpse_hip.h)


def test_loss_log_codes_are_counts():
    """wtpse_loss_log's check_n is a historical name for a count k: for every accepted code each of s0 .. s(k-1) is required, every
    other integer from -1 to 64 is refused with all six scalars given, and ops names the code of every count.  As above: real memory
    behind every non-null pointer, status -1 expected, nothing launched."""
    import ctypes
    from wtpse_hip import build, ops
    from wtpse_hip.lib import LIB_PATH
    build.build()
    gpu = torch.cuda.is_available()
    if gpu:
        torch.cuda.init()
    dll = ctypes.CDLL(LIB_PATH)
    keep = []

    def mem(n, dtype):
        t = torch.zeros(n, dtype=dtype, device="cuda" if gpu else "cpu")
        keep.append(t)
        return t.data_ptr()

    fn = dll.wtpse_loss_log
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    s = [mem(1, torch.float32) for _ in range(6)]
    acc, flag, t = mem(6, torch.float64), mem(2, torch.int32), mem(1, torch.int32)
    for code, k in LOSS_LOG_COUNTS.items():
        for j in range(k):
            args = list(s)
            args[j] = None
            assert fn(*args, acc, code, flag, t, None) == -1, (code, j)
    for code in range(-1, 65):
        if code not in LOSS_LOG_COUNTS:
            assert fn(*s, acc, code, flag, t, None) == -1, code
    assert tuple(ops.loss_log_code(k) for k in range(6)) == (0, 1, 17, 3, 19, 51)
    assert [LOSS_LOG_COUNTS[ops.loss_log_code(k)] for k in range(6)] == list(range(6))


def test_run_state_round_trips_weights_only():
    """A saved-state dict as TrainRun.state() builds it — tensors, numbers, strings, lists, dicts — through torch.save and
    torch.load(weights_only=True), the two host generators included: they continue their streams where they were."""
    from wtpse_hip import trainer
    from wtpse_hip.step import adam_state_to_torch
    py, nr = random.Random(5), np.random.RandomState(5)
    py.random(); py.gauss(0, 1); nr.choice(9, 1); nr.standard_normal()
    shapes = [(2, 3), (3,)]
    opt = adam_state_to_torch(torch.arange(9.), torch.ones(9), 4, shapes, 1e-3, (0.9, 0.99), 1e-8)
    d = {"model": {"w": torch.ones(2, 3), "bn.num_batches_tracked": torch.tensor(4)},
         "train_step": {"optim": {"od": opt}, "noise": {"od": {"seed": 1234, "ctr": 1 << 40}}},
         "epoch": 3, "iteration": 12, "best_mean_dice": 0.5, "best_epoch": 2,
         "config": {"lr": [1e-3] * 4, "lr_schedule": "", "seed": 5},
         "py_rng": trainer._py_state_to_lists(py.getstate()), "np_rng": trainer._np_state_to_lists(nr.get_state()),
         "loss_sums": {"seg_od": 0.1 + 0.2}, "loss_names": ["seg_od"]}
    buf = io.BytesIO()
    torch.save(d, buf)
    buf.seek(0)
    r = torch.load(buf, map_location="cpu", weights_only=True)
    assert r["epoch"] == 3 and r["iteration"] == 12 and r["loss_sums"] == {"seg_od": 0.1 + 0.2}
    assert r["train_step"]["noise"]["od"] == {"seed": 1234, "ctr": 1 << 40}
    assert torch.equal(r["train_step"]["optim"]["od"]["state"][0]["exp_avg"], torch.arange(6.).view(2, 3))
    py2, nr2 = random.Random(0), np.random.RandomState(0)
    py2.setstate(trainer._py_state_from_lists(r["py_rng"]))
    nr2.set_state(trainer._np_state_from_lists(r["np_rng"]))
    assert [py2.random(), py2.gauss(0, 1), py2.randint(0, 99)] == [py.random(), py.gauss(0, 1), py.randint(0, 99)]
    assert np.array_equal(nr2.choice(1000, 8), nr.choice(1000, 8)) and nr2.standard_normal() == nr.standard_normal()
