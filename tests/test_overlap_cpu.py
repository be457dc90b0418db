"""The overlap loss without a GPU (wtpse_hip/overlap.py: the host specification of csrc/overlap.hip, the weight schedule; the names a
step logs; the C-ABI surface).  The gradient is compared with torch float64 autograd of a direct restatement of the definition."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

from wtpse_hip import overlap as ov

CONFIGS = {"dice": dict(fp=0.5, fn=0.5, focal=1.0, smooth=1.0), "tversky": dict(fp=0.3, fn=0.7, focal=1.0, smooth=1.0),
           "focal075": dict(fp=0.3, fn=0.7, focal=0.75, smooth=1.0), "focal2": dict(fp=0.5, fn=0.5, focal=2.0, smooth=0.5)}
NEW_ENTRIES = ("wtpse_overlap_loss",)


def _case(masked, seed=0):
    """x, t, mask [5, 1, 9, 11]: two ordinary planes, an all-background plane, an all-foreground plane and — masked — a plane with
    m = 0 everywhere."""
    r = np.random.RandomState(seed)
    x = r.normal(scale=3.0, size=(5, 1, 9, 11))
    t = np.zeros_like(x)
    t[0, 0, 2:7, 3:9] = 1
    t[1, 0, 4:6, 1:4] = 1
    t[3] = 1
    t[4, 0, 1:8, 2:10] = 1
    mask = None
    if masked:
        mask = (r.uniform(size=x.shape) < 0.6).astype(np.float64)
        mask[4] = 0
    return x, t, mask


def _torch_planes(x, t, m, fp, fn, focal, smooth):
    """The definition, written out once more in torch (float64 when its inputs are): [B] plane losses.  The plane with
    1 - TI == 0 is cut out before the power (torch.where with a safe base: no NaN gradient through the unused branch)."""
    B = x.shape[0]
    z = x if m is None else x * m
    mm = torch.ones_like(x) if m is None else m
    s = torch.sigmoid(z)
    tp = (mm * s * t).reshape(B, -1).sum(1)
    fpos = (mm * s * (1 - t)).reshape(B, -1).sum(1)
    fneg = (mm * (1 - s) * t).reshape(B, -1).sum(1)
    u = 1 - (tp + smooth) / (tp + fp * fpos + fn * fneg + smooth)
    dead = u <= 0
    safe = torch.where(dead, torch.ones_like(u), u)
    return torch.where(dead, torch.zeros_like(u), safe if focal == 1.0 else safe ** focal)


@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_gradient_equals_float64_autograd(cfg, masked):
    kw = CONFIGS[cfg]
    x, t, mask = _case(masked)
    w = 0.37
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    mt = None if mask is None else torch.tensor(mask)
    planes = _torch_planes(xt, torch.tensor(t), mt, **kw)
    (w * planes.mean()).backward()
    want = xt.grad.numpy()
    got = ov.overlap_grad_host(x, t, w, mask, **kw)
    assert got.shape == x.shape and got.dtype == np.float64
    scale = np.abs(want).max()
    assert scale > 0 and np.abs(got - want).max() <= 1e-12 * scale, np.abs(got - want).max() / scale
    assert np.abs(ov.overlap_planes_host(x, t, mask, **kw) - planes.detach().numpy()).max() <= 1e-12
    assert abs(ov.overlap_loss_host(x, t, mask, **kw) - float(planes.detach().mean())) <= 1e-12
    assert got[2].any() and got[3].any()                   # empty and full targets, ordinary logits: a gradient all the same
    if masked:
        assert not got[4].any() and (got[mask == 0] == 0).all()
        assert ov.overlap_planes_host(x, t, mask, **kw)[4] == 0.0


def test_dice_closed_form():
    x, t, mask = _case(True)
    m = mask.reshape(5, -1)
    s = 1.0 / (1.0 + np.exp(-(x.reshape(5, -1) * m)))
    tt = t.reshape(5, -1)
    for eps in (1.0, 0.25):
        want = 1.0 - (2.0 * (m * s * tt).sum(1) + 2.0 * eps) / ((m * s).sum(1) + (m * tt).sum(1) + 2.0 * eps)
        got = ov.overlap_planes_host(x, t, mask, smooth=eps)
        assert np.abs(got - want).max() <= 1e-13
    # unmasked, against the textbook form on one plane
    s = 1.0 / (1.0 + np.exp(-x[0].ravel()))
    want = 1.0 - (2.0 * (s * t[0].ravel()).sum() + 2.0) / (s.sum() + t[0].sum() + 2.0)
    assert abs(ov.overlap_planes_host(x[:1], t[:1])[0] - want) <= 1e-13


def test_deliberate_definitions():
    # 1. the sums carry m: what the network does outside the mask changes nothing, and those pixels add nothing to FP
    x, t, mask = _case(True)
    x2 = x.copy()
    x2[mask == 0] = 50.0
    t2 = t.copy()
    t2[mask == 0] = 1 - t2[mask == 0]                      # nor do target pixels outside the mask count (FN)
    for kw in CONFIGS.values():
        a = ov.overlap_planes_host(x, t, mask, **kw)
        assert np.array_equal(a, ov.overlap_planes_host(x2, t2, mask, **kw))
        assert np.array_equal(ov.overlap_grad_host(x, t, 1.0, mask, **kw), ov.overlap_grad_host(x2, t2, 1.0, mask, **kw))
    # 2. 1 - TI == 0 exactly: loss 0, gradient exactly 0, no NaN — with focal 0.75 the derivative's power has exponent -0.25
    kw = CONFIGS["focal075"]
    with np.errstate(divide="raise", invalid="raise"):      # (no inf * 0, no 0 / 0 on the way)
        x = np.full((3, 1, 4, 5), -1e4)
        t = np.zeros_like(x)
        x[1] = np.random.RandomState(1).normal(size=(1, 4, 5))
        x[2], t[2] = 1e4, 1.0                              # all foreground, s = 1
        planes = ov.overlap_planes_host(x, t, None, **kw)
        g = ov.overlap_grad_host(x, t, 2.0, None, **kw)
    assert planes[0] == 0.0 and planes[2] == 0.0 and planes[1] > 0.0
    assert not g[0].any() and not g[2].any() and g[1].any() and np.isfinite(g).all()
    assert not np.signbit(planes).any()
    # a NaN logit is not swallowed by the rule
    x[0, 0, 0, 0] = np.nan
    assert math.isnan(ov.overlap_planes_host(x, t, None, **kw)[0]) and math.isnan(ov.overlap_loss_host(x, t, None, **kw))


def test_validation_and_weight_schedule():
    o = ov.OverlapLoss()
    assert o.config() == {"weight": 1.0, "fp": 0.5, "fn": 0.5, "focal": 1.0, "smooth": 1.0, "ramp": 0.0, "cap": None}
    assert o.weight_at(0) == 1.0 == o.weight_at(100)
    o = ov.OverlapLoss(0.1, ramp=0.25)
    assert [o.weight_at(e) for e in range(3)] == [0.1, 0.35, 0.6] and o.weight_at(10 ** 6) == 0.1 + 0.25 * 10 ** 6      # no cap
    o = ov.OverlapLoss(0.1, 0.3, 0.7, 0.75, 0.5, ramp=0.25, cap=0.5)
    assert [o.weight_at(e) for e in range(4)] == [0.1, 0.35, 0.5, 0.5]
    assert ov.OverlapLoss(2.0, cap=1.0).weight_at(0) == 1.0 and ov.OverlapLoss(0.0).weight_at(5) == 0.0
    assert ov.OverlapLoss(**o.config()).config() == o.config()
    assert eval(repr(o), {"OverlapLoss": ov.OverlapLoss}).config() == o.config()
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "1", True):
        for k in ("weight", "fp", "fn", "focal", "smooth", "ramp", "cap"):
            with pytest.raises(ValueError, match=k):
                ov.OverlapLoss(**{k: bad})
    with pytest.raises(ValueError, match="weight"):
        ov.OverlapLoss(weight=None)
    for k in ("focal", "smooth"):
        with pytest.raises(ValueError, match=k):
            ov.OverlapLoss(**{k: 0})
    with pytest.raises(ValueError, match="fp"):
        ov.OverlapLoss(fp=0, fn=0)
    assert ov.OverlapLoss(fp=0, fn=1).fp == 0.0 and ov.OverlapLoss(fp=1, fn=0).fn == 0.0
    # the host functions refuse the same parameters
    x, t, _ = _case(False)
    for kw in (dict(fp=-1.0), dict(fp=0.0, fn=0.0), dict(focal=0.0), dict(smooth=0.0), dict(smooth=float("nan"))):
        with pytest.raises(ValueError):
            ov.overlap_loss_host(x, t, **kw)
    with pytest.raises(ValueError):
        ov.overlap_loss_host(x, t[:2])


def test_log_names_with_and_without_the_terms():
    from wtpse_hip.step import TrainStep
    full, plain = {"whitening": True}, {"whitening": False}
    old_full = ["seg_od", "ins_od", "dom_od", "kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od",
                "seg_oc", "ins_oc", "dom_oc", "kd_oc", "ins_shape_oc", "dom_shape_oc"]
    bd_full = ["seg_od", "ins_od", "dom_od", "bd_od", "kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od",
               "seg_oc", "ins_oc", "dom_oc", "bd_oc", "kd_oc", "ins_shape_oc", "dom_shape_oc"]
    # the existing outputs are unchanged
    assert TrainStep.log_names(full) == TrainStep.log_names(full, False, False) == TrainStep.log_names(full, overlap=False) == old_full
    assert TrainStep.log_names(plain) == TrainStep.log_names(plain, overlap=False) == ["seg_od", "seg_oc"]
    assert TrainStep.log_names(full, boundary=True) == TrainStep.log_names(full, True, False) == bd_full
    assert TrainStep.log_names(plain, boundary=True) == ["seg_od", "bd_od", "seg_oc", "bd_oc"]
    # overlap alone: where bd_* would go
    assert TrainStep.log_names(plain, overlap=True) == ["seg_od", "ov_od", "seg_oc", "ov_oc"]
    assert TrainStep.log_names(full, overlap=True) == [n.replace("bd_", "ov_") for n in bd_full]
    # both: directly behind bd_*
    assert TrainStep.log_names(plain, boundary=True, overlap=True) == ["seg_od", "bd_od", "ov_od", "seg_oc", "bd_oc", "ov_oc"]
    both = TrainStep.log_names(full, boundary=True, overlap=True)
    assert both == ["seg_od", "ins_od", "dom_od", "bd_od", "ov_od", "kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od",
                    "seg_oc", "ins_oc", "dom_oc", "bd_oc", "ov_oc", "kd_oc", "ins_shape_oc", "dom_shape_oc"]
    assert [n for n in both if n[:3] not in ("bd_", "ov_")] == old_full
    # each call's scalars stay one run of at most six slots: one wtpse_loss_log launch per call
    assert both.index("ov_od") - both.index("seg_od") == both.index("ov_oc") - both.index("seg_oc") == 4


def test_arguments_of_step_and_run():
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import TrainRun
    assert inspect.signature(TrainStep.__init__).parameters["overlap"].default is None
    assert inspect.signature(TrainRun.__init__).parameters["overlap"].default is None
    with pytest.raises(ValueError, match="overlap"):
        TrainStep(None, None, None, None, {"whitening": True}, dp=object(), overlap=ov.OverlapLoss())
    run = TrainRun.__new__(TrainRun)
    run.base_lr, run.iter_per_epoch, run.max_epoch, run.stop_epoch = (1e-3,) * 4, 3, 2, -1
    run.interval_validate, run.lr_schedule, run.seed, run.checkpoint_every = 10, None, 5, 0
    run.graph, run.betas, run.freeze_bn = "plan", (0.9, 0.99), False
    assert run.config()["overlap"] == {}                                      # off unless the constructor switches it on
    run.overlap = ov.OverlapLoss(0.5, 0.3, 0.7, 0.75, 1.0, ramp=0.1, cap=2.0)
    cfg = run.config()
    assert cfg["overlap"] == {"weight": 0.5, "fp": 0.3, "fn": 0.7, "focal": 0.75, "smooth": 1.0, "ramp": 0.1, "cap": 2.0}
    kw = TrainRun.config_kwargs(cfg)
    assert kw["overlap"] == cfg["overlap"] and set(kw) <= set(inspect.signature(TrainRun.__init__).parameters)
    old = {k: v for k, v in cfg.items() if k != "overlap"}                     # a checkpoint from before the field
    assert TrainRun.config_kwargs(old)["overlap"] == {}


def test_header_declares_and_library_binds_the_new_entries():
    from wtpse_hip import build, lib
    protos = build.parse_prototypes()
    bound = lib.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos and protos[name][-1] == "void*", name            # (stream last: the entry gets a plan thunk)
        assert len(bound[name]) == len(protos[name])
    assert protos["wtpse_overlap_loss_ws"] == ["int", "int"]
    assert protos["wtpse_overlap_loss"] == ["const float*"] * 4 + ["int", "int"] + ["float"] * 4 + ["void*"] + ["float*"] * 3 + ["void*"]
    build.build()
    dll = ctypes.CDLL(lib.LIB_PATH)
    dll.wtpse_plan_fn_name.restype = ctypes.c_char_p
    recordable = {dll.wtpse_plan_fn_name(i).decode() for i in range(dll.wtpse_plan_fn_count())}
    for name in NEW_ENTRIES:
        assert getattr(dll, name) is not None and name in recordable, name
    # the sizing helper is host-only: bytes, and a function of hw alone per plane
    L = lib.lib()
    q = lambda B, hw: L.query("wtpse_overlap_loss_ws", B, hw)
    assert q(1, 1) == 3 * 8 + 4 and q(32, 256 * 256) == 32 * q(1, 256 * 256) and q(1, 256 * 256) > q(1, 64 * 64) == q(1, 1)
    for B, hw in [(0, 4), (1, 0), (-1, 4), (1, -4), (65536, 1), (4096, 1 << 20), (1, (1 << 30) + 1)]:
        assert q(B, hw) == -1, (B, hw)
    # arguments are checked before anything is launched
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    fn = L.raw("wtpse_overlap_loss")
    ok = dict(x=p, mask=None, t=p, w=p, B=1, hw=1, fp=0.5, fn=0.5, focal=1.0, smooth=1.0, ws=p, planes=None, loss=p, dx=None)
    for change in (dict(x=None), dict(t=None), dict(ws=None), dict(loss=None), dict(dx=p, w=None), dict(B=0), dict(hw=0), dict(B=65536),
                   dict(fp=-0.5), dict(fp=0.0, fn=0.0), dict(focal=0.0), dict(smooth=0.0), dict(smooth=float("nan")),
                   dict(focal=float("inf")), dict(fn=float("nan")), dict(ws=p + 4)):
        a = dict(ok, **change)
        assert fn(a["x"], a["mask"], a["t"], a["w"], a["B"], a["hw"], a["fp"], a["fn"], a["focal"], a["smooth"], a["ws"], a["planes"],
                  a["loss"], a["dx"], None) == -1, change
    # the log's NaN test with one more scalar: 35, 49, 51 are new; every value refused before is still refused
    log = L.raw("wtpse_loss_log")
    acc = (ctypes.c_double * 6)()
    a = ctypes.addressof(acc)
    assert log(p, p, p, None, None, None, a, 35, p, None, None) == -1                       # s3 missing
    assert log(p, None, None, None, None, None, a, 49, p, None, None) == -1                 # s1, s2 missing
    assert log(p, p, None, None, None, None, a, 49, p, None, None) == -1                    # s2 missing
    assert log(p, p, p, p, None, None, a, 51, p, None, None) == -1                          # s4 missing
    for bad in (2, 4, 16, 18, 20, 32, 33, 34, 36, 48, 50, 52, 64, 67, -1):
        assert log(p, p, p, p, p, p, a, bad, p, None, None) == -1, bad
