"""The Lovász hinge loss without a GPU (wtpse_hip/lovasz.py: the host specification of csrc/lovasz.hip, the weight schedule; the names
a step logs; the sixth scalar of the loss log; the C-ABI surface).  Value and gradient are compared with torch float64 autograd of the
published flat Lovász hinge, restated here."""
import ctypes
import inspect
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

from wtpse_hip import lovasz as lv


# ---- Berman's lovasz_losses.py, the binary flat form, in torch (float64 when its inputs are); a stable sort fixes the tie rule
def _lovasz_grad(gt_sorted):
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if len(gt_sorted) > 1:
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
    return jaccard


def _lovasz_hinge_flat(logits, labels):
    if len(labels) == 0:
        return logits.sum() * 0.0
    signs = 2.0 * labels - 1.0
    errors = 1.0 - logits * signs
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
    grad = _lovasz_grad(labels[perm])
    return torch.dot(torch.relu(errors_sorted), grad)


def _published(x, t, mask, w):
    """-> (planes, gradient of w * mean(planes)) by autograd, one image at a time with the ignored pixels taken out."""
    B = x.shape[0]
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t, dtype=torch.float64)
    planes = []
    for b in range(B):
        keep = torch.ones(xt[b].numel(), dtype=torch.bool) if mask is None else torch.tensor(mask[b].reshape(-1) != 0)
        planes.append(_lovasz_hinge_flat(xt[b].reshape(-1)[keep], tt[b].reshape(-1)[keep]))
    planes = torch.stack(planes)
    (w * planes.mean()).backward()
    return planes.detach().numpy(), xt.grad.numpy()


def _case(n, masked, seed):
    """B = 4 planes of n pixels: logits are multiples of 1/8 in [-3, 3] (fp32 and float64 errors coincide, and nearly every error
    is tied with others), targets a random half."""
    r = np.random.RandomState(seed)
    x = (r.randint(-24, 25, size=(4, 1, 1, n)) / 8.0).astype(np.float32)
    t = (r.uniform(size=x.shape) < 0.4).astype(np.float32)
    mask = (r.uniform(size=x.shape) < 0.6).astype(np.float32) if masked else None
    return x, t, mask


@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("n", [1, 7, 300, 4096])
def test_specification_equals_the_published_loss(n, masked):
    x, t, mask = _case(n, masked, seed=n + int(masked))
    w = 0.5                                                 # w / B is a power of two: the gradient's factors commute exactly
    want_planes, want_grad = _published(x, t, mask, w)
    planes = lv.lovasz_planes_host(x, t, mask)
    grad = lv.lovasz_grad_host(x, t, w, mask)
    assert planes.dtype == np.float64 and grad.dtype == np.float64 and grad.shape == x.shape
    scale = max(np.abs(want_planes).max(), 1e-300)
    assert np.abs(planes - want_planes).max() <= 1e-12 * scale, (planes, want_planes)
    assert abs(lv.lovasz_loss_host(x, t, mask) - want_planes.mean()) <= 1e-12 * scale
    assert np.array_equal(grad, want_grad), int((grad != want_grad).sum())
    if n >= 300:
        assert grad.any() and (planes > 0).all()
        e = 1.0 - x.astype(np.float64) * np.where(t > 0, 1.0, -1.0)
        assert len(np.unique(e)) < n // 4                   # heavy ties
    if masked:
        assert not grad[mask == 0].any()
    # ranks: a permutation of 0 .. k-1 over the kept pixels with e > 0 of every plane, -1 elsewhere, ties in pixel order
    ranks = lv.lovasz_ranks_host(x, t, mask)
    assert ranks.dtype == np.int32 and ranks.shape == x.shape
    e32 = np.float32(1) - x * np.where(t > 0, np.float32(1), np.float32(-1))
    live = (e32 > 0) & (True if mask is None else mask != 0)
    assert ((ranks >= 0) == live).all()
    for b in range(x.shape[0]):
        rb, eb = ranks[b].ravel(), e32[b].ravel()
        idx = np.flatnonzero(rb >= 0)
        assert sorted(rb[idx]) == list(range(idx.size))
        order = idx[np.argsort(rb[idx])]
        assert all(eb[i] > eb[j] or (eb[i] == eb[j] and i < j) for i, j in zip(order[:-1], order[1:]))
        assert (grad[b].ravel()[rb < 0] == 0).all()


def test_worked_example():
    x = np.array([[0.5, -1.0, 2.0, 0.25]], dtype=np.float32)
    t = np.array([[1, 0, 1, 0]], dtype=np.float32)
    assert lv.lovasz_ranks_host(x, t).tolist() == [[1, -1, -1, 0]]          # e = [0.5, 0, -1, 1.25]: pixels 3, 0 (then 1, 2)
    want = float(Fraction(5, 4) / 3 + Fraction(1, 2) / 3)
    assert abs(lv.lovasz_planes_host(x, t)[0] - want) <= 2e-16 and abs(want - 0.58333333333333337) < 1e-15
    assert lv.lovasz_loss_host(x, t) == lv.lovasz_planes_host(x, t)[0]
    g = lv.lovasz_grad_host(x, t, 1.0)
    assert np.abs(g - np.array([[-1 / 3, 0, 0, 1 / 3]])).max() <= 1.2e-16 and g[0, 1] == 0.0 and g[0, 2] == 0.0
    assert g[0, 3] == 1.0 - 2.0 / 3.0                                       # J_1 itself, on pixel 3 (background: +)
    # g itself, to the stated fractions: J = [1/3, 2/3, 3/4, 1]
    idx, gg = lv._sorted_plane(np.float32(1) - x[0] * np.array([1, -1, 1, -1], dtype=np.float32), t[0] > 0, np.ones(4, dtype=bool))
    assert idx.tolist() == [3, 0, 1, 2]
    assert np.abs(gg - np.array([1 / 3, 1 / 3, 1 / 12, 1 / 4])).max() <= 1.2e-16


def test_edge_planes():
    r = np.random.RandomState(3)
    x = r.normal(scale=2.0, size=(1, 1, 5, 7)).astype(np.float32)
    t = (r.uniform(size=x.shape) < 0.5).astype(np.float32)
    # an empty mask: 0 and a zero gradient
    zero = np.zeros_like(x)
    assert lv.lovasz_planes_host(x, t, zero)[0] == 0.0 and not lv.lovasz_grad_host(x, t, 1.0, zero).any()
    assert (lv.lovasz_ranks_host(x, t, zero) == -1).all()
    # no foreground: J = 1 from the first place on — L = max(e, 0) of the top pixel, the gradient sits on that pixel alone
    e = np.float32(1) + x                                   # sign = -1 everywhere
    top = int(np.argmax(e.ravel()))
    assert e.ravel()[top] > 0
    assert lv.lovasz_planes_host(x, zero)[0] == float(e.ravel()[top])
    g = lv.lovasz_grad_host(x, zero, 0.75)
    assert g.ravel()[top] == 0.75 and np.count_nonzero(g) == 1
    assert lv.lovasz_planes_host(-np.abs(x) - 1, zero)[0] == 0.0             # ... and 0 when even the top error is <= 0
    # all foreground: J_r = r / n, every g = 1 / n up to rounding: the mean of the positive errors
    one = np.ones_like(x)
    e = (np.float32(1) - x).astype(np.float64).ravel()
    want = np.maximum(e, 0).sum() / e.size
    assert abs(lv.lovasz_planes_host(x, one)[0] - want) <= 1e-14 * want
    g = lv.lovasz_grad_host(x, one, 1.0).ravel()
    assert (g[e > 0] < 0).all() and np.abs(g[e > 0] + 1.0 / e.size).max() <= 1e-15 and not g[e <= 0].any()
    # all errors <= 0 (every pixel right by a margin of at least 1): 0, no gradient, no rank
    sure = np.where(t > 0, np.float32(1), np.float32(-1)) * (np.abs(x) + np.float32(1))
    assert lv.lovasz_planes_host(sure, t)[0] == 0.0 and not lv.lovasz_grad_host(sure, t, 1.0).any()
    assert (lv.lovasz_ranks_host(sure, t) == -1).all()
    # a single kept pixel
    m = zero.copy()
    m.ravel()[4] = 1
    ek = float(np.float32(1) - x.ravel()[4] * (1 if t.ravel()[4] > 0 else -1))
    assert lv.lovasz_planes_host(x, t, m)[0] == max(ek, 0.0)
    # a non-finite kept logit: a NaN plane and no gradient; outside the mask it is not seen
    for bad in (np.nan, np.inf, -np.inf):
        xb = np.concatenate([x, x])
        xb[1].ravel()[4] = bad
        tb, keep, drop = np.concatenate([t, t]), np.concatenate([m, m]), np.concatenate([1 - m, 1 - m])
        for mask in (None, keep):
            planes = lv.lovasz_planes_host(xb, tb, mask)
            assert math.isnan(planes[1]) and planes[0] == lv.lovasz_planes_host(x, t, None if mask is None else m)[0]
            assert math.isnan(lv.lovasz_loss_host(xb, tb, mask))
            g = lv.lovasz_grad_host(xb, tb, 1.0, mask)
            assert not g[1].any() and np.isfinite(g).all()
            assert np.array_equal(g[0], lv.lovasz_grad_host(x, t, 1.0, None if mask is None else m)[0] / 2)
        planes = lv.lovasz_planes_host(xb, tb, drop)
        assert planes[1] == planes[0] and np.isfinite(planes).all()
    with pytest.raises(ValueError):
        lv.lovasz_loss_host(x, np.concatenate([t, t]))
    with pytest.raises(ValueError):
        lv.lovasz_loss_host(x.ravel(), t.ravel())


def test_validation_and_weight_schedule():
    o = lv.LovaszLoss()
    assert o.config() == {"weight": 1.0, "ramp": 0.0, "cap": None}
    assert o.weight_at(0) == 1.0 == o.weight_at(100)
    o = lv.LovaszLoss(0.1, ramp=0.25)
    assert [o.weight_at(e) for e in range(3)] == [0.1, 0.35, 0.6] and o.weight_at(10 ** 6) == 0.1 + 0.25 * 10 ** 6      # no cap
    o = lv.LovaszLoss(0.1, ramp=0.25, cap=0.5)
    assert [o.weight_at(e) for e in range(4)] == [0.1, 0.35, 0.5, 0.5]
    assert lv.LovaszLoss(2.0, cap=1.0).weight_at(0) == 1.0 and lv.LovaszLoss(0.0).weight_at(5) == 0.0
    assert lv.LovaszLoss(**o.config()).config() == o.config()
    assert eval(repr(o), {"LovaszLoss": lv.LovaszLoss}).config() == o.config()
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "1", True):
        for k in ("weight", "ramp", "cap"):
            with pytest.raises(ValueError, match=k):
                lv.LovaszLoss(**{k: bad})
    with pytest.raises(ValueError, match="weight"):
        lv.LovaszLoss(weight=None)


def test_log_names_with_and_without_the_term():
    from wtpse_hip.step import TERMS, TrainStep
    assert [(key, tag) for key, tag, _, _ in TERMS][:3] == [("boundary", "bd"), ("overlap", "ov"), ("lovasz", "lv")]
    assert TERMS[2][2] is lv.LovaszLoss
    full, plain = {"whitening": True}, {"whitening": False}
    old_full = ["seg_od", "ins_od", "dom_od", "kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od",
                "seg_oc", "ins_oc", "dom_oc", "kd_oc", "ins_shape_oc", "dom_shape_oc"]
    # without the term the names are exactly as before
    assert TrainStep.log_names(full) == TrainStep.log_names(full, False, False) == TrainStep.log_names(full, lovasz=False) == old_full
    assert TrainStep.log_names(plain) == TrainStep.log_names(plain, lovasz=False) == ["seg_od", "seg_oc"]
    assert TrainStep.log_names(plain, boundary=True, overlap=True) == ["seg_od", "bd_od", "ov_od", "seg_oc", "bd_oc", "ov_oc"]
    # alone: where bd_* / ov_* would go
    assert TrainStep.log_names(plain, lovasz=True) == ["seg_od", "lv_od", "seg_oc", "lv_oc"]
    assert TrainStep.log_names(full, lovasz=True) == [n.replace("ov_", "lv_") for n in TrainStep.log_names(full, overlap=True)]
    # with the others: behind them, in the table's order
    assert TrainStep.log_names(plain, boundary=True, lovasz=True) == ["seg_od", "bd_od", "lv_od", "seg_oc", "bd_oc", "lv_oc"]
    assert TrainStep.log_names(plain, overlap=True, lovasz=True) == ["seg_od", "ov_od", "lv_od", "seg_oc", "ov_oc", "lv_oc"]
    assert TrainStep.log_names(plain, True, True, True) == ["seg_od", "bd_od", "ov_od", "lv_od", "seg_oc", "bd_oc", "ov_oc", "lv_oc"]
    every = TrainStep.log_names(full, boundary=True, overlap=True, lovasz=True)
    assert every == ["seg_od", "ins_od", "dom_od", "bd_od", "ov_od", "lv_od", "kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od",
                     "seg_oc", "ins_oc", "dom_oc", "bd_oc", "ov_oc", "lv_oc", "kd_oc", "ins_shape_oc", "dom_shape_oc"]
    assert [n for n in every if n[:3] not in ("bd_", "ov_", "lv_")] == old_full
    # each call's scalars are one run of six slots: one wtpse_loss_log launch per call
    assert every.index("lv_od") - every.index("seg_od") == every.index("lv_oc") - every.index("seg_oc") == 5


def test_arguments_of_step_and_run():
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import TrainRun
    assert inspect.signature(TrainStep.__init__).parameters["lovasz"].default is None
    assert inspect.signature(TrainRun.__init__).parameters["lovasz"].default is None
    assert inspect.signature(TrainStep.log_names).parameters["lovasz"].default is False
    for name in ("lovasz", "lv_w", "set_lovasz_weight", "get_lovasz_weight"):
        assert hasattr(TrainStep, name), name
    with pytest.raises(ValueError, match="lovasz"):
        TrainStep(None, None, None, None, {"whitening": True}, dp=object(), lovasz=lv.LovaszLoss())
    run = TrainRun.__new__(TrainRun)
    run.base_lr, run.iter_per_epoch, run.max_epoch, run.stop_epoch = (1e-3,) * 4, 3, 2, -1
    run.interval_validate, run.lr_schedule, run.seed, run.checkpoint_every = 10, None, 5, 0
    run.graph, run.betas, run.freeze_bn = "plan", (0.9, 0.99), False
    assert run.config()["lovasz"] == {}                                       # off unless the constructor switches it on
    run.lovasz = lv.LovaszLoss(0.5, ramp=0.1, cap=2.0)
    cfg = run.config()
    assert cfg["lovasz"] == {"weight": 0.5, "ramp": 0.1, "cap": 2.0} and cfg["overlap"] == {} and cfg["boundary"] == {}
    kw = TrainRun.config_kwargs(cfg)
    assert kw["lovasz"] == cfg["lovasz"] and set(kw) <= set(inspect.signature(TrainRun.__init__).parameters)
    old = {k: v for k, v in cfg.items() if k != "lovasz"}                      # a checkpoint from before the field
    assert TrainRun.config_kwargs(old)["lovasz"] == {}


def _memory():
    """mem(n, dtype) -> the address of n zeroed elements that live as long as the returned list does: device memory where there is a
    device, host memory otherwise (nothing below is ever launched)."""
    gpu = torch.cuda.is_available()
    if gpu:
        torch.cuda.init()
    keep = []

    def mem(n, dtype):
        t = torch.zeros(n, dtype=dtype, device="cuda" if gpu else "cpu")
        keep.append(t)
        return t.data_ptr()
    return mem, keep


def test_loss_log_tests_six_scalars():
    """ops.loss_log_code(6): one new check_n outside -1 .. 64 (every unlisted value of that range stays refused: tests/test_trainer_cpu.py);
    every one of s0 .. s5 is required — status -1 before anything is launched; with all six the arguments pass (the status is then the
    launch's: 0 with a device, the runtime's error without one)."""
    from wtpse_hip import build, ops
    from wtpse_hip.lib import LIB_PATH
    build.build()
    code = ops.loss_log_code(6)
    assert isinstance(code, int) and not -1 <= code <= 64
    assert tuple(ops.loss_log_code(k) for k in range(6)) == (0, 1, 17, 3, 19, 51)         # codes 0 .. 5 are unchanged
    with pytest.raises(ValueError):
        ops.loss_log_code(-1)
    mem, keep = _memory()
    dll = ctypes.CDLL(LIB_PATH)
    fn = dll.wtpse_loss_log
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    s = [mem(1, torch.float32) for _ in range(6)]
    acc, flag, t = mem(6, torch.float64), mem(2, torch.int32), mem(1, torch.int32)
    for j in range(6):
        args = list(s)
        args[j] = None
        assert fn(*args, acc, code, flag, t, None) == -1, j
    assert fn(*s, None, code, flag, t, None) == -1 and fn(*s, acc, code, None, t, None) == -1
    assert fn(*s, acc, code, flag, t, None) != -1
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def test_header_declares_and_library_binds_the_new_entries():
    from wtpse_hip import build, lib
    protos = build.parse_prototypes()
    bound = lib.parse_header()
    assert protos["wtpse_lovasz_loss_ws"] == ["int", "int"]
    assert protos["wtpse_lovasz_loss"] == ["const float*"] * 4 + ["int", "int", "void*", "float*", "int*", "float*", "float*", "void*"]
    assert len(bound["wtpse_lovasz_loss"]) == 12
    build.build()
    dll = ctypes.CDLL(lib.LIB_PATH)
    dll.wtpse_plan_fn_name.restype = ctypes.c_char_p
    recordable = {dll.wtpse_plan_fn_name(i).decode() for i in range(dll.wtpse_plan_fn_count())}
    assert dll.wtpse_lovasz_loss is not None and "wtpse_lovasz_loss" in recordable
    # the sizing helper is host-only: bytes, per plane a function of hw alone, the limits of the overlap entry point
    L = lib.lib()
    q = lambda B, hw: L.query("wtpse_lovasz_loss_ws", B, hw)
    assert q(1, 1) > 16 and q(1, 1) % 4 == 0
    for hw in (1, 2047, 2048, 2049, 256 * 256):
        assert q(32, hw) == 32 * q(1, hw) and q(3, hw) == 3 * q(1, hw), hw
        assert q(1, hw) >= 16 * hw                                             # two buffers each of keys and payloads
    assert q(1, 2049) - q(1, 2048) > q(1, 2048) - q(1, 2047) == 16            # one chunk more from 2049 on
    for B, hw in [(0, 4), (1, 0), (-1, 4), (1, -4), (65536, 1), (4096, 1 << 20), (1, (1 << 30) + 1), (1, 1 << 30), (2, 1 << 27)]:
        assert q(B, hw) == -1, (B, hw)
    assert q(1, 1 << 26) > 0
    # arguments are checked before anything is launched
    mem, keep = _memory()
    p, pi = mem(64, torch.float64), mem(64, torch.int32)
    ws = mem(q(1, 1) // 8 + 1, torch.float64)
    fn = L.raw("wtpse_lovasz_loss")
    ok = dict(x=p, mask=None, t=p, w=p, B=1, hw=1, ws=ws, planes=None, ranks=None, loss=p, dx=None)
    for change in (dict(x=None), dict(t=None), dict(ws=None), dict(loss=None), dict(dx=p, w=None), dict(dx=p, w=None, ranks=pi, planes=p),
                   dict(B=0), dict(hw=0), dict(B=-1), dict(hw=-1), dict(B=65536), dict(hw=(1 << 30) + 1), dict(B=4096, hw=1 << 20),
                   dict(ws=ws + 4)):
        a = dict(ok, **change)
        assert fn(a["x"], a["mask"], a["t"], a["w"], a["B"], a["hw"], a["ws"], a["planes"], a["ranks"], a["loss"], a["dx"], None) == -1, change
