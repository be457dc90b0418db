"""The fused 1x1 heads (csrc/head.hip) on operands they must get exactly right (tests/exact_head_cases.py; proved on the host by
test_exact_head_cpu.py): forward with and without tape, backward with and without accumulate, the two- and the three-layer head, in the
x2h arithmetic (mode 2: head_*_h_k, with the amax tables the step passes and without x_amax) and on the fp32-input MFMA (any other
mode: head_*_k), compared BIT FOR BIT with the fp64 chain — no tolerance.  Outputs an entry point overwrites start as a sentinel NaN,
and so does the slab workspace: a block, image, row, slab or cross product that is dropped, doubled or misplaced, a ReLU mask taken
from other bits than the forward's, or a wrong power of two on the way back changes bits somewhere and fails the call."""
import pytest
import torch

import exact_cases as E
import exact_head_cases as HC
from dispatch_cases import NAN_BITS
from test_kernels_gpu import ops, DEV
from test_exact_conv_gpu import _DEV, dev, differs, finish, sentinel, x3_terms

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_device_copies():
    _DEV.clear()
    yield
    _DEV.clear()
    HC.clear_caches()


def amax_tables(p):
    """x_amax / dy_amax as the training step passes them: the input's own table for a raw input, its bound behind a prologue."""
    o = ops()
    xam = o.amax_of(dev(p["x"]))
    if p["pro"] is not None:
        xam = o.act_bound(dev(p["pro"]), xam)
    return xam, o.amax_of(dev(p["o"]["dy"]))


def head_args(p):
    o, v = p["o"], p["v"]
    return [dev(p["x"]), dev(p["pro"]), int(bool(v.pro))] + [dev(o[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]


def run_forward(p, tape, x_amax):
    """wtpse_head_fwd as ops.head_fwd calls it, on sentinel outputs.  -> {y, h2, h1} (what the call writes)"""
    o = ops()
    B, H, W = p["shape"]
    P, nc = H * W, p["v"].nc
    x, pro, relu, w1, b1, w2, b2, w3, b3 = head_args(p)
    y = sentinel(B, nc, P) if nc else None
    h2 = sentinel(B, 8, P) if (tape or not nc) else None
    h1 = sentinel(B, 32, P) if tape else None
    ptr = o.ptr
    o.lib().call("wtpse_head_fwd", ptr(x), ptr(pro), relu, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), nc, ptr(h1), ptr(h2), ptr(y),
                 ptr(x_amax), B, P, o.stream_ptr())
    return {k: t for k, t in (("y", y), ("h2", h2), ("h1", h1)) if t is not None}


def run_backward(p, mode, x_amax, dy_amax):
    """wtpse_head_bwd as ops.head_bwd calls it: the slab workspace is ops.workspace's, filled with the sentinel; dx and (without
    accumulate) dparams start as the sentinel; the tapes are the reference's — mode 2 gets no h1.  -> (dx, dparams)"""
    o = ops()
    B, H, W = p["shape"]
    P, v, r = H * W, p["v"], p["r"]
    x, pro, relu, w1, b1, w2, b2, w3, b3 = head_args(p)
    ns = HC.head_ns(v.nc)
    slab = o.workspace("head_slab", o.lib().query("wtpse_head_slabs", B, P) * ns, DEV)
    slab.view(torch.int32).fill_(NAN_BITS)
    dparams = dev(p["base"]).clone() if v.acc else sentinel(ns)
    dx = sentinel(B, 32, P)
    h1 = dev(r["h1"]) if mode != 2 else None
    h2 = dev(r["h2"]) if v.nc else None
    ptr = o.ptr
    o.lib().call("wtpse_head_bwd", ptr(dev(p["o"]["dy"])), ptr(x), ptr(pro), relu, ptr(h1), ptr(h2), ptr(w1), ptr(b1), ptr(w2), ptr(w3), v.nc,
                 ptr(dx), ptr(slab), ptr(dparams), int(v.acc), ptr(x_amax), ptr(dy_amax), B, P, o.stream_ptr())
    return dx, dparams


def differs32(got, ref32, what):
    """dparams: the fold rounds the exact sum once — the reference is float32(exact sum) [+ base, in fp32], compared as fp32 bits."""
    if torch.equal(got, dev(ref32)):
        return None
    return E.first_difference(got, ref32.double(), what)


def settings_of(name, p):
    """(mode, with tables) a problem runs in: the fp32-input kernels (mode 3; mode 1 in one small case), x2h with the amax tables and —
    where the host proof admits it — with x_amax = None."""
    runs = [(3, False), (2, True)] + ([(2, False)] if p["notable"] else [])
    return runs + ([(1, False)] if name == HC.MODE1_CASE else [])


def check_problem(name, p, failures):
    v, r, check = p["v"], p["r"], p["check"]
    for mode, tables in settings_of(name, p):
        tag = "%s %s class %s %s mode %d%s" % (name, p["shape"], p["cls"], HC.hvid(v), mode, " amax" if tables else "")
        with x3_terms(mode):
            xam, dam = amax_tables(p) if mode == 2 else (None, None)
            if not tables:
                xam = None
            for tape in (True, False):
                got = run_forward(p, tape, xam)
                for k, t in got.items():
                    if check[k]:
                        f = differs(t, r[k], "%s forward %s: %s (image, channel, pixel)" % (tag, "with tape" if tape else "without tape", k))
                        if f:
                            failures.append(f)
            dx, dparams = run_backward(p, mode, xam, dam)
        f = differs(dx, r["dx"], tag + " backward: dx (image, channel, pixel)")
        if f:
            failures.append(f)
        for k, off, shape in HC.sections(v.nc):
            if check[k]:
                n = 1
                for s in shape:
                    n *= s
                f = differs32(dparams[off:off + n].view(shape), p["dparams"][off:off + n].view(shape).contiguous(),
                              "%s backward%s: %s %s" % (tag, " accumulate" if v.acc else "", k, shape))
                if f:
                    failures.append(f)


@pytest.mark.parametrize("cls", HC.SETTINGS)
@pytest.mark.parametrize("name", list(HC.HEAD_CASES))
def test_head(name, cls):
    """Every variant of one case in one operand setting, in every arithmetic; the failures of all calls in one message."""
    failures = []
    for v in HC.HEAD_CASES[name][2]:
        if (name, cls, HC.hvid(v)) in HC.CLASS_I_ONLY:
            continue
        p = HC.head_problem(name, cls, v)
        assert p["d"] is not None, (name, cls, HC.hvid(v))
        check_problem(name, p, failures)
    finish(failures)


def test_head_through_the_wrappers():
    """ops.head_fwd / ops.head_bwd themselves (their own output buffers, tape choices and amax_of) on a class-I and a class-T problem:
    mode 2 as the step calls them — no h1 tape, scales from the tables — and mode 3 with the tape."""
    o = ops()
    failures = []
    for name, cls, v in (("b33", "I", HC.HEAD_CASES["b33"][2][1]), ("b5", "TX", HC.HEAD_CASES["b5"][2][0])):
        p = HC.head_problem(name, cls, v)
        B, H, W = p["shape"]
        r, nc = p["r"], v.nc
        x, pro, relu, w1, b1, w2, b2, w3, b3 = head_args(p)
        x4, dy4 = x.view(B, 32, H, W), dev(p["o"]["dy"]).view(B, -1, H, W)
        ns = HC.head_ns(nc)
        for mode in (2, 3):
            tag = "ops %s class %s %s mode %d" % (name, cls, HC.hvid(v), mode)
            with x3_terms(mode):
                xam = amax_tables(p)[0] if mode == 2 else None
                out, h1, h2 = o.head_fwd(x4, pro, relu, w1, b1, w2, b2, w3, b3, True, x_amax=xam, want_h1=mode != 2)
                assert (h1 is None) == (mode == 2), tag
                dparams = sentinel(ns)
                dx = o.head_bwd(dy4, x4, pro, relu, h1, h2, w1, w2, w3, dparams, b1=b1, x_amax=xam)
            got = {"y" if nc else "h2": out, "h2": h2, "dx": dx}
            if h1 is not None:
                got["h1"] = h1
            for k, t in got.items():
                f = differs(t.view(B, -1, H * W), r[k], "%s: %s" % (tag, k))
                if f:
                    failures.append(f)
            assert all(p["check"].values()), tag
            f = differs32(dparams, p["dparams"], tag + ": dparams")
            if f:
                failures.append(f)
    finish(failures)
