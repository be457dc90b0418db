"""The boundary loss without a GPU (wtpse_hip/boundary.py: the host specification of csrc/boundary.hip, the weight schedule; the
names a step logs; the C-ABI surface).  The specification is compared with Kervadec's scipy expression where scipy imports, and
with hand-checked planes everywhere."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

from wtpse_hip import boundary as bd

SHAPES = [(1, 1), (1, 7), (7, 1), (5, 64), (33, 65), (64, 64), (40, 130)]
DENSITIES = [0.05, 0.5, 0.95]
NEW_ENTRIES = ("wtpse_signed_distance", "wtpse_boundary_loss")


def _planes():
    r = np.random.RandomState(11)
    for h, w in SHAPES:
        for p in DENSITIES:
            yield (r.uniform(size=(h, w)) < p).astype(np.float32)


def test_host_spec_equals_the_scipy_expression():
    """one_hot2dist: edt(neg) * neg - (edt(pos) - 1) * pos, difference 0 (a plane without a contour aside: zero by definition)."""
    ndi = pytest.importorskip("scipy.ndimage")
    seen = 0
    for t in _planes():
        pos = t != 0
        phi = bd.signed_distance_host(t)
        if not pos.any() or pos.all():
            assert not phi.any()
            continue
        neg = ~pos
        want = ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos) - 1) * pos
        assert np.array_equal(phi, want), t.shape          # (-0.0 == 0.0: the inside pixels next to the background)
        d2_out, d2_in = bd.squared_distances_host(t)
        assert np.array_equal(d2_out, np.rint(ndi.distance_transform_edt(neg) ** 2)) and np.array_equal(d2_in, np.rint(ndi.distance_transform_edt(pos) ** 2))
        seen += 1
    assert seen >= 15


def test_separable_form_gives_the_same_integers():
    for t in _planes():
        a, b = bd.squared_distances_host(t, chunk=1 << 12), bd.squared_distances_separable_host(t)
        assert a[0].dtype == b[0].dtype == np.int32
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), t.shape


def test_hand_checked_planes():
    t = np.zeros((3, 3))
    t[1, 1] = 1
    s2 = np.sqrt(2.0)
    assert np.array_equal(bd.signed_distance_host(t), np.array([[s2, 1, s2], [1, 0, 1], [s2, 1, s2]]))
    d2_out, d2_in = bd.squared_distances_host(t)
    assert d2_out.tolist() == [[2, 1, 2], [1, 0, 1], [2, 1, 2]] and d2_in.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    t = np.zeros((4, 4))
    t[1:3, 1:3] = 5.0                                      # nonzero = object, whatever the value
    want = np.array([[s2, 1, 1, s2], [1, 0, 0, 1], [1, 0, 0, 1], [s2, 1, 1, s2]])
    assert np.array_equal(bd.signed_distance_host(t), want)
    # a 3 x 3 block in 5 x 5: the centre lies 2 from the background, phi = 1 - 2
    t = np.zeros((5, 5))
    t[1:4, 1:4] = 1
    assert bd.signed_distance_host(t)[2, 2] == -1.0 and bd.signed_distance_host(t)[0, 0] == s2


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (16, 16)])
def test_planes_without_a_contour_are_zero(shape):
    for t in (np.zeros(shape), np.ones(shape)):
        phi = bd.signed_distance_host(t)
        assert phi.shape == shape and phi.dtype == np.float64 and not phi.any()
        d2_out, d2_in = bd.squared_distances_host(t)
        empty, own = (d2_out, d2_in) if not t.any() else (d2_in, d2_out)
        assert (empty == -1).all() and (own == 0).all()
    with pytest.raises(ValueError):
        bd.signed_distance_host(np.zeros((2, 3, 4)))


@pytest.mark.parametrize("masked", [False, True])
def test_gradient_against_central_differences(masked):
    r = np.random.RandomState(3)
    t = np.zeros((9, 11))
    t[2:7, 3:9] = 1
    phi = np.stack([bd.signed_distance_host(t), bd.signed_distance_host(1 - t)])
    x = r.normal(scale=3.0, size=phi.shape)
    mask = (r.uniform(size=phi.shape) < 0.7).astype(np.float64) if masked else None
    alpha = 0.37
    g = bd.boundary_grad_host(x, phi, alpha, mask)
    assert g.shape == x.shape
    eps = 1e-5
    points = [(0, 0, 0), (0, 4, 5), (1, 8, 10), (1, 3, 3), (0, 2, 3)]
    if masked:
        points += [tuple(i) for i in np.argwhere(mask == 0)[:2]]
    for idx in points:
        xp, xm = x.copy(), x.copy()
        xp[idx] += eps
        xm[idx] -= eps
        fd = alpha * (bd.boundary_loss_host(xp, phi, mask) - bd.boundary_loss_host(xm, phi, mask)) / (2 * eps)
        # central difference: truncation eps^2 |f'''| / 6 and rounding ~1e-16 |L| / eps, both far below 1e-9 here
        assert abs(fd - g[idx]) < 1e-9, (idx, fd, g[idx])
    if masked:
        assert (g[mask == 0] == 0).all()
    # the loss itself, written out
    z = x if mask is None else x * mask
    assert abs(bd.boundary_loss_host(x, phi, mask) - float(np.mean(phi / (1 + np.exp(-z))))) < 1e-13


def test_weight_schedule_and_argument_errors():
    b = bd.BoundaryLoss()
    assert (b.weight, b.ramp, b.cap) == (0.01, 0.01, 1.0)
    assert b.weight_at(0) == 0.01 and b.weight_at(5) == 0.01 + 0.01 * 5 and b.weight_at(99) == 1.0 and b.weight_at(10 ** 6) == 1.0
    b = bd.BoundaryLoss(0.01, 0.5, 1.0)
    assert [b.weight_at(e) for e in range(4)] == [0.01, 0.51, 1.0, 1.0]
    assert bd.BoundaryLoss(0.0, 0.0, 0.0).weight_at(7) == 0.0 and bd.BoundaryLoss(2.0, 0.0, 1.0).weight_at(0) == 1.0
    assert bd.BoundaryLoss(**b.config()).config() == b.config() == {"weight": 0.01, "ramp": 0.5, "cap": 1.0}
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "1", None):
        for k in ("weight", "ramp", "cap"):
            with pytest.raises(ValueError, match=k):
                bd.BoundaryLoss(**{k: bad})


def test_log_names_with_and_without_the_term():
    from wtpse_hip.step import TrainStep
    full, plain = {"whitening": True}, {"whitening": False}
    old_full = ["seg_od", "ins_od", "dom_od", "kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od",
                "seg_oc", "ins_oc", "dom_oc", "kd_oc", "ins_shape_oc", "dom_shape_oc"]
    assert TrainStep.log_names(full) == TrainStep.log_names(full, boundary=False) == old_full
    assert TrainStep.log_names(plain) == TrainStep.log_names(plain, False) == ["seg_od", "seg_oc"]
    assert TrainStep.log_names(plain, boundary=True) == ["seg_od", "bd_od", "seg_oc", "bd_oc"]
    got = TrainStep.log_names(full, boundary=True)
    assert got == ["seg_od", "ins_od", "dom_od", "bd_od", "kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od",
                   "seg_oc", "ins_oc", "dom_oc", "bd_oc", "kd_oc", "ins_shape_oc", "dom_shape_oc"]
    # each call's scalars stay one run of at most six slots: one wtpse_loss_log launch per call
    assert got.index("bd_od") - got.index("seg_od") == got.index("bd_oc") - got.index("seg_oc") == 3
    assert [n for n in got if not n.startswith("bd_")] == old_full


def test_arguments_of_step_and_run():
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import TrainRun
    assert inspect.signature(TrainStep.__init__).parameters["boundary"].default is None
    assert inspect.signature(TrainRun.__init__).parameters["boundary"].default is None
    with pytest.raises(ValueError, match="boundary"):
        TrainStep(None, None, None, None, {"whitening": True}, dp=object(), boundary=bd.BoundaryLoss())
    run = TrainRun.__new__(TrainRun)
    run.base_lr, run.iter_per_epoch, run.max_epoch, run.stop_epoch = (1e-3,) * 4, 3, 2, -1
    run.interval_validate, run.lr_schedule, run.seed, run.checkpoint_every = 10, None, 5, 0
    run.graph, run.betas, run.freeze_bn = "plan", (0.9, 0.99), False
    assert run.config()["boundary"] == {}                                     # off unless the constructor switches it on
    run.boundary = bd.BoundaryLoss(0.02, 0.1, 0.5)
    cfg = run.config()
    assert cfg["boundary"] == {"weight": 0.02, "ramp": 0.1, "cap": 0.5}        # the run's metadata names the schedule
    kw = TrainRun.config_kwargs(cfg)
    assert kw["boundary"] == cfg["boundary"] and set(kw) <= set(inspect.signature(TrainRun.__init__).parameters)
    old = {k: v for k, v in cfg.items() if k != "boundary"}                    # a checkpoint from before the field
    assert TrainRun.config_kwargs(old)["boundary"] == {}


def test_header_declares_and_library_binds_the_new_entries():
    from wtpse_hip import build, lib
    protos = build.parse_prototypes()
    bound = lib.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos and protos[name][-1] == "void*", name            # (stream last: the entry gets a plan thunk)
        assert len(bound[name]) == len(protos[name])
    assert protos["wtpse_signed_distance_ws"] == ["int", "int", "int"]
    assert protos["wtpse_signed_distance"] == ["const float*", "float*", "int*", "int*", "void*", "int", "int", "int", "void*"]
    assert protos["wtpse_boundary_loss"] == ["const float*"] * 4 + ["long long", "float*", "float*", "float*", "void*"]
    build.build()
    dll = ctypes.CDLL(lib.LIB_PATH)
    dll.wtpse_plan_fn_name.restype = ctypes.c_char_p
    recordable = {dll.wtpse_plan_fn_name(i).decode() for i in range(dll.wtpse_plan_fn_count())}
    for name in NEW_ENTRIES:
        assert getattr(dll, name) is not None and name in recordable, name
    # the sizing helper is host-only: one word per pixel, <= 0 for what the kernels do not take
    L = lib.lib()
    assert L.query("wtpse_signed_distance_ws", 32, 256, 256) == 32 * 256 * 256
    assert L.query("wtpse_signed_distance_ws", 1, 1, 1) == 1 and L.query("wtpse_signed_distance_ws", 1, 1024, 1024) == 1 << 20
    for B, h, w in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 4097, 4), (1, 4, 4097), (65536, 1, 1), (4096, 1024, 1024)]:
        assert L.query("wtpse_signed_distance_ws", B, h, w) <= 0, (B, h, w)
    # arguments are checked before anything is launched
    one = (ctypes.c_float * 4)()
    p = ctypes.addressof(one)
    assert L.raw("wtpse_signed_distance")(None, p, None, None, p, 1, 1, 1, None) == -1
    assert L.raw("wtpse_signed_distance")(p, p, None, None, None, 1, 1, 1, None) == -1
    assert L.raw("wtpse_signed_distance")(p, p, None, None, p, 1, 4097, 1, None) == -1
    assert L.raw("wtpse_boundary_loss")(p, None, None, p, 4, p, p, None, None) == -1        # phi missing
    assert L.raw("wtpse_boundary_loss")(p, None, p, p, 0, p, p, None, None) == -1           # n == 0
    assert L.raw("wtpse_boundary_loss")(p, None, p, None, 4, p, p, p, None) == -1           # dx without the weight
    # the log's NaN test with the boundary scalar: 16 | 1 and 16 | 3, nothing else new
    fn = L.raw("wtpse_loss_log")
    acc = (ctypes.c_double * 6)()
    a = ctypes.addressof(acc)
    assert fn(p, None, None, None, None, None, a, 17, p, None, None) == -1                  # s1 missing
    assert fn(p, p, p, None, None, None, a, 19, p, None, None) == -1                        # s3 missing
    for bad in (2, 4, 16, 18, 20, 33):
        assert fn(p, p, p, p, None, None, a, bad, p, None, None) == -1
