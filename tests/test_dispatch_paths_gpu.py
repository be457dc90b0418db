"""Every dispatch branch of the bandwidth-bound step kernels (-m gpu): csrc/pointwise.hip, csrc/bn.hip, csrc/wt_loss.hip.

The cases, their seeded inputs, their fp64 / stock-PyTorch references and the branch each one is there for live in
dispatch_cases.py; test_dispatch_paths_cpu.py proves on the host that each case takes that branch.  Here every case
  * repeats the branch assertion (predicate restatement and, where there is one, the library's host query) before it launches,
  * writes every output into a buffer with 64 floats of a fixed NaN pattern on either side and pre-filled with the same pattern: an
    overrun breaks a guard, and an element no kernel wrote is still that NaN — the close() of this file asserts that a result is
    finite before it compares it (test_kernels_gpu.close alone lets a NaN through: NaN > tol is False), torch.equal and the amax
    equalities fail on it by themselves; neither needs a fault to show,
  * runs the misaligned form of an operand — the same data 4 bytes off a 16-byte boundary, in bounds — next to the aligned one,
  * compares (a) the vector kernel with the scalar kernel, bitwise where the source promises the same expression tree, and
    (b) the result with a plain fp64 reference at the tolerance of the existing test of the same entry point (quoted at each use).
Launches go through ops.lib().call() with data_ptr() arithmetic wherever the ops wrapper would allocate the output itself."""
import pytest
import torch
import torch.nn.functional as F

import dispatch_cases as D
from test_conv_x3_gpu import amax_value
from test_kernels_gpu import DEV, ops
from test_kernels_gpu import close as _close

pytestmark = pytest.mark.gpu

GUARD = D.GUARD


def L():
    return ops().lib()


def S():
    return ops().stream_ptr()


def P(t):
    return 0 if t is None else t.data_ptr()


def out(shape, off=0, init=None, dtype=torch.float32):
    """A tensor of `shape` inside a larger buffer: GUARD words of the NaN pattern in front and behind, the tensor itself filled
    with the pattern (or `init`); off = 1 puts it 4 bytes past a 16-byte boundary."""
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    raw = torch.full((GUARD + off + n + GUARD + 3,), D.NAN_BITS, dtype=torch.int32, device=DEV)
    v = raw[GUARD + off: GUARD + off + n]
    v = (v.view(torch.float32) if dtype == torch.float32 else v).view(shape)
    assert raw.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * off
    if init is not None:
        v.copy_(init.to(DEV).reshape(shape))
    v.raw, v.lo = raw, GUARD + off
    return v


def dev(t, off=0):
    return out(t.shape, off, init=t.contiguous())


def table():
    """A zeroed amax table between guards."""
    return out((ops().AMAX_WORDS,), init=torch.zeros(ops().AMAX_WORDS, dtype=torch.int32), dtype=torch.int32)


def guards_ok(*tensors):
    for t in tensors:
        if t is None:
            continue
        hi = t.lo + t.numel()
        assert bool((t.raw[:t.lo] == D.NAN_BITS).all()), "front guard overwritten"
        assert bool((t.raw[hi:] == D.NAN_BITS).all()), "rear guard overwritten"


def close(a, b, rtol=1e-4, atol=1e-5, what=""):
    """test_kernels_gpu.close behind a finiteness check: an unwritten element (the NaN pre-fill) or a computed NaN must not pass."""
    bad = ~torch.isfinite(a.detach())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements are not finite (unwritten or NaN)"
    _close(a, b, rtol=rtol, atol=atol, what=what)


def subset(branch, expect, what):
    for k, v in expect.items():
        assert branch[k] == v, (what, k, branch)


def pros(C):
    return (None, D.make_pro(C, 7))


# =============================================================================================== pooling
def run_pool_fwd(x, pro, relu, offs=(0, 0)):
    B, C, H, W = x.shape
    xd, o = dev(x, offs[0]), out((B, C, H // 2, W // 2), offs[1])
    pd = None if pro is None else dev(pro)
    L().call("wtpse_maxpool2_fwd", P(xd), P(pd), int(relu), P(o), B, C, H, W, S())
    guards_ok(o, xd)
    return o


@pytest.mark.parametrize("name", list(D.POOL_FWD_CASES))
def test_maxpool_forward_paths(name):
    """Vector (one plane per blockIdx.y, looped past 32768 planes) against the flat scalar kernel: "Same expression trees, bitwise
    equal" (pointwise.hip); both against fp64 max_pool2d at test_pool_and_upsample's close() defaults."""
    shape, branch, trips = D.POOL_FWD_CASES[name]
    B, C, H, W = shape
    assert D.pool_fwd_branch(H, W) == branch and D.plane_trips(B * C) == trips
    x = D.pool_input(name, shape)
    for pro in pros(C):
        for relu in (0, 1):
            ref = F.max_pool2d(D.act64(x, pro, relu), 2)
            a = run_pool_fwd(x, pro, relu)
            close(a, ref, what=f"pool fwd {name} pro={pro is not None} relu={relu}")
            forms = [(1, 0)] + ([(0, 1), (1, 1)] if name == "align" else [])
            for offs in forms:                        # a misaligned x or out: the scalar kernel
                assert D.pool_fwd_branch(H, W, False) == "scalar"
                assert torch.equal(run_pool_fwd(x, pro, relu, offs), a), (name, offs, relu)


def run_pool_bwd(x, pro, relu, dp, base, acc, offs=(0, 0, 0)):
    B, C, H, W = x.shape
    xd, dd = dev(x, offs[0]), dev(dp, offs[1])
    dx = out(x.shape, offs[2], init=base if acc & 1 else None)
    pd = None if pro is None else dev(pro)
    L().call("wtpse_maxpool2_bwd", P(xd), P(pd), int(relu), P(dd), P(dx), int(acc), B, C, H, W, S())
    guards_ok(dx, xd, dd)
    return dx


@pytest.mark.parametrize("name", list(D.POOL_BWD_CASES))
def test_maxpool_backward_paths(name):
    """accumulate 0..3 (bit 0: add to dx, bit 1: times [act(x) > 0]), with and without the scale/shift table and the ReLU on load;
    vector against scalar bitwise, both against fp64 autograd at test_pool_and_upsample's close() defaults.  "ties": all-equal and
    all-negative-under-ReLU windows, where the first element wins as in ATen."""
    shape, branch, trips = D.POOL_BWD_CASES[name]
    B, C, H, W = shape
    assert D.pool_bwd_branch(H, W) == branch and D.plane_trips(B * C) == trips
    assert L().query("wtpse_maxpool2_bwd_stats_blocks", B, H, W) == D.pool_stats_blocks(B, H, W)
    x = D.pool_input(name, shape)
    dp, base = D.rnd(B, C, H // 2, W // 2, seed=32), D.rnd(*shape, seed=33)
    for pro in pros(C):
        for relu in (0, 1):
            for acc in (0, 1, 2, 3):
                what = f"pool bwd {name} pro={pro is not None} relu={relu} acc={acc}"
                _, ref = D.pool_ref(x, pro, relu, dp, base, acc)
                a = run_pool_bwd(x, pro, relu, dp, base, acc)
                close(a, ref, what=what)
                forms = [(1, 0, 0)] + ([(0, 1, 0), (0, 0, 1)] if name == "align" else [])
                for offs in forms:
                    assert torch.equal(run_pool_bwd(x, pro, relu, dp, base, acc, offs), a), (what, offs)


# =============================================================================================== bilinear x2
def run_up_fwd(x, pro, relu, offs=(0, 0)):
    B, C, H, W = x.shape
    xd, o = dev(x, offs[0]), out((B, C, 2 * H, 2 * W), offs[1])
    pd = None if pro is None else dev(pro)
    L().call("wtpse_upsample2x_fwd", P(xd), P(pd), int(relu), P(o), B, C, H, W, S())
    guards_ok(o, xd)
    return o


@pytest.mark.parametrize("name", list(D.UP_FWD_CASES))
def test_upsample_forward_paths(name):
    """upsample2x_fwd4_v_k (even W, aligned out) against upsample2x_fwd_k: "Per output bitwise the expression tree of the scalar
    kernel / ATen"; both against fp64 F.interpolate at test_pool_and_upsample's close() defaults."""
    shape, branch, trips = D.UP_FWD_CASES[name]
    B, C, H, W = shape
    assert D.up_fwd_branch(H, W) == branch and D.plane_trips(B * C) == trips
    assert L().query("wtpse_upsample2x_stats_blocks", B, H, W) == D.up_stats_blocks(B, H, W)
    x = D.rnd(*shape, seed=34)
    for pro in pros(C):
        for relu in (0, 1):
            a = run_up_fwd(x, pro, relu)
            close(a, D.up_ref(x, pro, relu), what=f"up fwd {name} pro={pro is not None} relu={relu}")
            assert torch.equal(run_up_fwd(x, pro, relu, (0, 1)), a), (name, "out misaligned: scalar kernel")
            if name == "align":                       # x is read with scalar loads: its alignment does not change the path
                assert torch.equal(run_up_fwd(x, pro, relu, (1, 0)), a)
                assert torch.equal(run_up_fwd(x, pro, relu, (1, 1)), a)


def run_up_bwd(du, base, acc, offs=(0, 0)):
    B, C, Ho, Wo = du.shape
    dd = dev(du, offs[0])
    dx = out((B, C, Ho // 2, Wo // 2), offs[1], init=base if acc else None)
    tab = table()
    L().call("wtpse_upsample2x_bwd", P(dd), P(dx), int(acc), B, C, Ho // 2, Wo // 2, P(tab), S())
    guards_ok(dx, dd, tab)
    assert amax_value(tab) == float(dx.abs().max()), "amax table of dx"
    return dx


@pytest.mark.parametrize("name", list(D.UP_BWD_CASES))
def test_upsample_backward_paths(name):
    """upsample2x_bwd_v_k against upsample2x_bwd_k ("per output the same loops and summation order as the scalar kernel"), fp64
    autograd at test_pool_and_upsample's "up bwd" tolerance (rtol 1e-4, atol 1e-5), and the amax table both paths leave behind
    (published in-kernel on the vector path, by a second pass on the scalar path) against abs().max() of what was stored."""
    shape, branch, trips = D.UP_BWD_CASES[name]
    B, C, H, W = shape
    assert D.up_bwd_branch(H, W) == branch and D.plane_trips(B * C) == trips
    du, base = D.rnd(B, C, 2 * H, 2 * W, seed=35), D.rnd(*shape, seed=36)
    for acc in (0, 1):
        a = run_up_bwd(du, base, acc)
        close(a, D.up_bwd_ref(du, base if acc else None), rtol=1e-4, atol=1e-5, what=f"up bwd {name} acc={acc}")
        forms = [(1, 0)] + ([(0, 1)] if name == "align" else [])
        for offs in forms:
            assert torch.equal(run_up_bwd(du, base, acc, offs), a), (name, acc, offs)


@pytest.mark.parametrize("name", list(D.UP_BWD_BN_CASES))
def test_upsample_backward_with_batchnorm_apply_on_load(name):
    """wtpse_upsample2x_bwd_bn against wtpse_bn_bwd_apply_coef followed by wtpse_upsample2x_bwd: "bn_bwd_apply_k's expression, bn.hip:
    the same bits"; the amax tables agree and equal abs().max() of dx."""
    B, C, H, W = D.UP_BWD_BN_CASES[name]
    assert D.up_bwd_branch(H, W) == "vec"
    g, y = D.rnd(B, C, 2 * H, 2 * W, seed=37), D.rnd(B, C, 2 * H, 2 * W, seed=38)
    coef = torch.stack([D.rnd(C, seed=39) * 0.3 + 1, D.rnd(C, seed=40) * 0.2, D.rnd(C, seed=41) * 0.1], 1).contiguous()
    gd, yd, cd = dev(g), dev(y), dev(coef)
    dout, t0 = out(g.shape), table()
    L().call("wtpse_bn_bwd_apply_coef", P(gd), P(yd), P(cd), P(dout), B, C, 4 * H * W, P(t0), S())
    dx1, t1 = out((B, C, H, W)), table()
    L().call("wtpse_upsample2x_bwd", P(dout), P(dx1), 0, B, C, H, W, P(t1), S())
    dx2, t2 = out((B, C, H, W)), table()
    L().call("wtpse_upsample2x_bwd_bn", P(gd), P(yd), P(cd), P(dx2), B, C, H, W, P(t2), S())
    guards_ok(dout, dx1, dx2, t0, t1, t2)
    assert torch.equal(dx1, dx2)
    assert amax_value(t1) == amax_value(t2) == float(dx2.abs().max())
    assert amax_value(t0) == float(dout.abs().max())
    k = coef.double().view(1, C, 3, 1, 1)
    close(dx2, D.up_bwd_ref(k[:, :, 0] * g.double() + k[:, :, 1] * y.double() + k[:, :, 2]), rtol=1e-4, atol=1e-5, what="up bwd bn")


# =============================================================================================== amax / relu_mask / axpy
@pytest.mark.parametrize("n", D.AMAX_SIZES)
def test_amax_table_of_a_tensor(n):
    """wtpse_amax: 16-byte body, scalar tail and the misaligned form against abs().max(), with the maximum where each can lose it."""
    assert D.amax_branch(n) == ("body" if n % 4 == 0 else "body+tail")
    base = (D.rnd(n, seed=71) * 0.5).clamp(-4, 4)
    variants = {}
    v = base.clone(); v[-1] = 9.5; variants["max last"] = v
    v = base.clone(); v[0] = -9.5; variants["max first"] = v
    variants["negative zeros"] = torch.full((n,), -0.0)
    v = base.clone(); v[n // 2] = float("-inf"); variants["inf"] = v
    v = base.clone(); v[0] = float("inf"); v[-1] = float("nan"); variants["nan"] = v
    for what, x in variants.items():
        for off in (0, 1):
            xd = dev(x, off)
            tab = out((ops().AMAX_WORDS,), init=torch.full((ops().AMAX_WORDS,), 0x7F7FFFFF, dtype=torch.int32), dtype=torch.int32)
            L().call("wtpse_amax", P(xd), n, P(tab), S())      # (zeroes the table itself)
            guards_ok(tab, xd)
            bits = int(tab[::16].max())
            if what == "nan":      # a NaN's bit pattern sorts above inf (wtpse_hip.h)
                assert bits == 0x7FC00000 and bits > 0x7F800000, (what, n, off, hex(bits))
            else:
                assert amax_value(tab) == float(x.abs().max()), (what, n, off)
                assert bits == int(x.abs().max().view(torch.int32)), (what, n, off)


@pytest.mark.parametrize("n", D.FLAT_SIZES)
def test_relu_mask_and_axpy_forms(n):
    """16 bytes per lane (n % 4 == 0, aligned) against the scalar forms, each pointer misaligned in turn: bitwise equal."""
    dz, ref, base = D.rnd(n, seed=72), D.rnd(n, seed=73), D.rnd(n, seed=74)
    ref[::3] = 0.0                                        # exactly zero counts as "not positive"
    for acc in (0, 1):
        want = torch.where(ref > 0, dz, torch.zeros_like(dz))
        want = base + want if acc else want
        outs = []
        for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            assert D.flat_branch(n, offs == (0, 0, 0)) == ("vec" if n % 4 == 0 and offs == (0, 0, 0) else "scalar")
            a, b = dev(dz, offs[0]), dev(ref, offs[1])
            o = out((n,), offs[2], init=base if acc else None)
            L().call("wtpse_relu_mask", P(a), P(b), P(o), acc, n, S())
            guards_ok(o, a, b)
            outs.append(o)
        assert all(torch.equal(o.cpu(), want) for o in outs), (n, acc)
    outs = []
    for offs in ((0, 0), (1, 0), (0, 1)):
        d, s = dev(base, offs[0]), dev(dz, offs[1])
        L().call("wtpse_axpy", P(d), P(s), 0.37, n, S())
        guards_ok(d, s)
        outs.append(d)
    assert all(torch.equal(o, outs[0]) for o in outs[1:]), n
    close(outs[0], base.double() + float(torch.tensor(0.37, dtype=torch.float32)) * dz.double(), what="axpy")   # test_pool_and_upsample


# =============================================================================================== losses
@pytest.mark.parametrize("n", list(D.LOSS_SIZES))
def test_loss_kernels_over_the_reduction_grids(n):
    """One workgroup, two, and the 1024-workgroup cap with a grid-stride second trip, against fp64 at test_losses_roi_adam's
    tolerances (quoted per call); device-scalar upstream gradient g = 2 and host weight w = 0.25 in the backward calls."""
    nb = D.LOSS_SIZES[n]
    assert L().query("wtpse_reduce_blocks", n) == nb == D.reduce_blocks(n)
    x, t, m, a, b = D.loss_inputs(n)
    r1, r = D.loss_refs(x, t, m, a, b), D.loss_refs(x, t, m, a, b, g=2.0, w=0.25)
    xd, td, md, ad, bd = dev(x), dev(t), dev(m), dev(a), dev(b)
    g2 = torch.tensor(2.0, device=DEV)

    def fwd(entry, *operands):
        part, loss = out((nb,)), out((1,))
        L().call(entry, *[P(o) for o in operands], n, P(part), P(loss), S())
        guards_ok(part, loss)
        return loss[0]

    close(fwd("wtpse_bce_sigmoid_fwd", xd, td), r1["bce"], rtol=1e-5, atol=1e-6, what="bce")
    close(fwd("wtpse_mse_fwd", ad, bd), r1["mse"], rtol=1e-5, what="mse")
    part, sums, pw = out((2 * nb,)), out((2,)), out((1,))
    L().call("wtpse_pos_weight", P(md), P(td), n, P(part), P(sums), P(pw), S())
    guards_ok(part, sums, pw)
    close(sums, r1["sums"], rtol=1e-6, what="pos_weight sums")
    close(pw[0], r1["pw"], rtol=1e-6, what="pos_weight")
    part, loss = out((nb,)), out((1,))
    L().call("wtpse_bce_logits_pw_fwd", P(xd), P(md), P(td), P(pw), n, P(part), P(loss), S())
    guards_ok(part, loss)
    close(loss[0], r1["bpw"], rtol=1e-5, atol=1e-6, what="bce pw")
    for gd, w, rr in ((None, 1.0, r1), (g2, 0.25, r)):
        dx = out((n,))
        L().call("wtpse_bce_sigmoid_bwd", P(xd), P(td), P(gd), w, n, P(dx), S())
        close(dx, rr["dbce"], rtol=1e-4, atol=1e-8, what="dbce")
        dx2 = out((n,))
        L().call("wtpse_bce_logits_pw_bwd", P(xd), P(md), P(td), P(pw), P(gd), w, n, P(dx2), S())
        close(dx2, rr["dbpw"], rtol=1e-4, atol=1e-8, what="dbce pw")
        da = out((n,))
        L().call("wtpse_mse_bwd", P(ad), P(bd), P(gd), w, n, P(da), S())
        close(da, rr["dmse"], rtol=1e-5, atol=1e-9, what="dmse")
        guards_ok(dx, dx2, da)


def test_bce_of_saturated_logits():
    """bce_sigmoid_* at logits of +-0..8 and +-20, +-40, +-90 with both targets against stock fp32 PyTorch on the host,
    F.binary_cross_entropy(torch.sigmoid(x), t): where the sigmoid saturates and the -100 clamp are properties of fp32, and the
    reference program computes exactly this.  9 < |x| < 18 is kept out: there 1 - sigmoid(x) has only a few bits and one ulp of
    difference in the sigmoid moves the element's loss by percents (the formula, not an implementation).
    Gradients: exactly 0 wherever the fp32 sigmoid is exactly 0 or 1 (x >= 20, x = -90), as in stock PyTorch.  At x = -20 and -40
    the sigmoid is a small normal number, s (1 - s) = s does not vanish and the gradient (s - t) / n is the true one: it is held
    against stock fp32 autograd like the rest, not against 0."""
    x, t = D.saturated_inputs()
    n = x.numel()
    xr = x.clone().requires_grad_(True)
    ref = F.binary_cross_entropy(torch.sigmoid(xr), t)
    ref.backward()
    xd, td = dev(x), dev(t)
    part, loss, dx = out((1,)), out((1,)), out((n,))
    L().call("wtpse_bce_sigmoid_fwd", P(xd), P(td), n, P(part), P(loss), S())
    L().call("wtpse_bce_sigmoid_bwd", P(xd), P(td), 0, 1.0, n, P(dx), S())
    guards_ok(part, loss, dx)
    close(loss[0], ref.detach(), rtol=1e-5, atol=1e-6, what="bce, saturated")          # test_losses_roi_adam "bce"
    close(dx, xr.grad, rtol=1e-4, atol=1e-8, what="dbce, saturated")                   # test_losses_roi_adam "dbce"
    s = torch.sigmoid(x)
    flat = (s == 0) | (s == 1)
    assert bool(flat[(x >= 20) | (x == -90)].all())
    assert bool((dx.cpu()[flat] == 0).all()) and bool((xr.grad[flat] == 0).all())


@pytest.mark.parametrize("mask", ["none", "no_positive", "one", "all", "half"])
def test_bce_with_logits_of_saturated_logits(mask):
    """bce_logits_pw_* at the same logits plus +-1e4 against fp64, with a zero mask (0 / 0 -> pos_weight 1; every effective logit
    is x * m = 0), a ones mask and no positive target (n / 0 = inf -> 1, the saturated logits live), and one, all and half of the
    targets positive; tolerances of test_losses_roi_adam "bce pw" / "dbce pw"."""
    x, t = D.saturated_inputs()
    big = torch.tensor([1e4, -1e4, 1e4, -1e4])
    x, t = torch.cat([x, big]), torch.cat([t, torch.tensor([0.0, 0.0, 1.0, 1.0])])
    n = x.numel()
    m = torch.ones(n)
    if mask == "none":
        m = torch.zeros(n)
    elif mask == "no_positive":
        t = torch.zeros(n)
    elif mask == "one":
        t = torch.zeros(n); t[5] = 1.0
    elif mask == "all":
        t = torch.ones(n)
    r = D.loss_refs(x, t, m, x, x)
    assert float(r["pw"]) == {"none": 1.0, "no_positive": 1.0, "one": float(n), "all": 1.0, "half": 2.0}[mask]
    xd, td, md = dev(x), dev(t), dev(m)
    part, sums, pw, loss, dx = out((2,)), out((2,)), out((1,)), out((1,)), out((n,))
    L().call("wtpse_pos_weight", P(md), P(td), n, P(part), P(sums), P(pw), S())
    assert float(pw[0]) == float(r["pw"])
    L().call("wtpse_bce_logits_pw_fwd", P(xd), P(md), P(td), P(pw), n, P(part), P(loss), S())
    L().call("wtpse_bce_logits_pw_bwd", P(xd), P(md), P(td), P(pw), 0, 1.0, n, P(dx), S())
    guards_ok(part, sums, pw, loss, dx)
    close(loss[0], r["bpw"], rtol=1e-5, atol=1e-6, what="bce pw, saturated")
    close(dx, r["dbpw"], rtol=1e-4, atol=1e-8, what="dbce pw, saturated")


# =============================================================================================== Adam
@pytest.mark.parametrize("n", D.ADAM_SIZES)
def test_adam_forms(n):
    """The fp64 Adam recurrence at test_losses_roi_adam's "adam" tolerance (rtol 1e-6, atol 1e-7) for step 1 and step 100000 (both
    bias corrections ~ 1), by value and through the device counter; wtpse_adam_dev with the same float lr gives the same bits
    ("the element-wise part is the same code for both entry points"); hold = 1 changes nothing."""
    lr, b1, b2, eps = 5e-4, 0.9, 0.99, 1e-8
    p0, g = D.rnd(n, seed=68), D.rnd(n, seed=69)
    m0, v0 = D.rnd(n, seed=70) * 0.1, D.rnd(n, seed=71).abs() * 0.01
    g[0] = m0[0] = v0[0] = 0.0                       # zero gradient on zero state: the denominator is eps, the step 0
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=DEV)

    def run(entry, step, step_dev=None, hold=None):
        p, m, v, gd = dev(p0), dev(m0), dev(v0), dev(g)
        if entry == "wtpse_adam":
            L().call(entry, P(p), P(gd), P(m), P(v), n, lr, b1, b2, eps, step, P(step_dev), S())
        else:
            L().call(entry, P(p), P(gd), P(m), P(v), n, P(lr_dev), b1, b2, eps, step, P(step_dev), P(hold), S())
        guards_ok(p, m, v, gd)
        return p, m, v

    for step in (1, 100000):
        want = D.adam_ref(p0, g, m0, v0, lr, b1, b2, eps, step)
        by_value = run("wtpse_adam", step)
        counter = torch.tensor([step - 1], dtype=torch.int32, device=DEV)
        by_counter = run("wtpse_adam", 1, counter)
        for got in (by_value, by_counter):
            for a, w, what in zip(got, want, ("p", "m", "v")):
                close(a, w, rtol=1e-6, atol=1e-7, what=f"adam {what} n={n} step={step}")
        assert float(by_value[0][0]) == float(p0[0])
        for a, b in zip(run("wtpse_adam_dev", step), by_value):
            assert torch.equal(a, b), (n, step, "adam_dev by value")
        for a, b in zip(run("wtpse_adam_dev", 1, counter), by_counter):
            assert torch.equal(a, b), (n, step, "adam_dev through the counter")
        held = run("wtpse_adam_dev", step, None, torch.ones(1, dtype=torch.int32, device=DEV))
        for a, b in zip(held, (p0, m0, v0)):
            assert torch.equal(a.cpu(), b), (n, step, "hold")
        free = run("wtpse_adam_dev", step, None, torch.zeros(1, dtype=torch.int32, device=DEV))
        assert torch.equal(free[0], by_value[0])


# =============================================================================================== attention fusion backward
@pytest.mark.parametrize("name", list(D.ATTN_CASES))
def test_attn_fuse_backward_folds(name):
    """The (dw, db) partials folded by reduce_rows_k (1023 rows) and reduce_rows_tall_k (1024 rows: the boundary; 1025 with a ragged
    last workgroup), accumulating into d_wb and not; tolerances of test_attention_fuse_and_sampling."""
    B, CE, HW, rows, kernel = D.ATTN_CASES[name]
    assert D.ceil_div(B * HW, 256) == rows and D.reduce_rows_branch(rows, 2) == kernel
    r = D.attn_ref(B, CE, HW)
    zd, ed, dd, ad, wbd = dev(r["z"]), dev(r["emb"]), dev(r["dfuse"]), dev(r["att"]), dev(r["wb"])
    prior = torch.tensor([0.5, -1.5])
    for acc in (0, 1):
        demb, dz, part, dwb = out(r["emb"].shape), out(r["z"].shape), out((2 * rows,)), out((2,), init=prior if acc else None)
        L().call("wtpse_attn_fuse_bwd", P(dd), P(zd), P(ed), P(ad), P(wbd), 0.3, P(demb), P(dz), P(part), P(dwb), acc, B, CE, HW, S())
        guards_ok(demb, dz, part, dwb)
        close(demb, r["demb"], what="demb")
        close(dz, r["dz"], what="dz")
        want = r["dwb"] + (prior.double() if acc else 0)
        close(dwb, want, rtol=1e-4, atol=1e-4 * max(1.0, float(r["dwb"].abs().max())), what=f"dwb {name} acc={acc}")


def test_randn_partial_last_block():
    """n % 4 != 0: the last Philox block is cut; the stream is the prefix of the n = 1004 stream at the same (seed, offset)."""
    full = out((1004,))
    L().call("wtpse_randn", P(full), 1004, 7, 4096, 0, S())
    for n in D.RANDN_SIZES:
        o = out((n,))
        L().call("wtpse_randn", P(o), n, 7, 4096, 0, S())
        guards_ok(o, full)
        assert torch.equal(o, full[:n]) and bool(torch.isfinite(o).all()), n


# =============================================================================================== BatchNorm backward
def run_bn_bwd(r, offs=(0, 0, 0), halves=False, relu=None):
    """wtpse_bn_bwd (or its two halves) on the operands of D.bn_inputs -> dy, dgamma, dbeta (+ guards, + the amax table of dy)."""
    B, C, H, W = r["shape"]
    HW = H * W
    relu = int(r["relu"] if relu is None else relu)
    ns = L().query("wtpse_bn_bwd_nsplit", B, C, HW)
    dz, y, dy = dev(r["dz"], offs[0]), dev(r["y"], offs[1]), out(r["shape"], offs[2])
    ss, gm, mu, iv = dev(r["ss"]), dev(r["gamma"]), dev(r["mean"]), dev(r["invstd"])
    part, coef, dg, db, tab = out((ns * C * 2,)), out((C * 3,)), out((C,)), out((C,)), table()
    if halves:
        sums = out((C, 2))
        L().call("wtpse_bn_bwd_reduce", P(dz), P(y), P(ss), relu, P(mu), P(iv), P(part), P(sums), B, C, HW, S())
        L().call("wtpse_bn_bwd_apply", P(dz), P(y), P(ss), relu, P(gm), P(mu), P(iv), P(sums), P(sums), B * HW, P(coef), P(dg), P(db), 0,
                 P(dy), B, C, HW, P(tab), S())
        guards_ok(sums)
    else:
        L().call("wtpse_bn_bwd", P(dz), P(y), P(ss), relu, P(gm), P(mu), P(iv), P(part), P(coef), P(dg), P(db), 0, P(dy), B, C, HW,
                 P(tab), S())
    guards_ok(dy, dg, db, part, coef, tab, dz, y)
    assert amax_value(tab) == float(dy.abs().max()), "amax table of dy"
    dy.coef = coef.view(C, 3)                         # (the one-launch kernel leaves it untouched)
    return dy, dg, db


def check_bn(r, dy, dg, db, what):
    """test_batchnorm_train's comparisons: the ReLU-kink entries (|z| < 2e-6, at most max(2, numel // 100000)) are left out of dy."""
    kink = r["on_kink"]
    assert int(kink.sum()) <= D.kink_cap(kink.numel())
    zero = torch.zeros_like(r["dy"])
    close(torch.where(kink, zero, dy.cpu().double()), torch.where(kink, zero, r["dy"]), rtol=2e-4, atol=2e-5, what=what + " dy")
    close(dg, r["dgamma"], rtol=2e-4, atol=2e-4, what=what + " dgamma")
    close(db, r["dbeta"], rtol=2e-4, atol=2e-4, what=what + " dbeta")


@pytest.mark.parametrize("name", list(D.BN_CASES))
def test_batchnorm_backward_paths(name):
    """Segmented reduction, a split that owns several units, the paired float4 loop and its remainder, the scalar kernels, the
    1024-thread finalize, the one-launch kernel: fp64 autograd through F.batch_norm(train) [+ ReLU] on a seeded y."""
    shape, relu, expect = D.BN_CASES[name]
    B, C, H, W = shape
    halves = name in D.BN_HALVES
    br = D.bn_bwd_branch(B, C, H * W, halves=halves)
    subset(br, expect, name)
    if br["path"] == "three":
        assert L().query("wtpse_bn_bwd_nsplit", B, C, H * W) == br["nsplit"]
    r = D.bn_inputs(shape, relu)
    check_bn(r, *run_bn_bwd(r, halves=halves), what=name)


def test_batchnorm_backward_wide_finalize_from_stats():
    """bn_bwd_finalize_k<1024> through wtpse_bn_bwd_from_stats: 2051 rows of partials, a host-side split of the exact sums (one row
    per image: sum g and sum g (y - mean) in fp64, rounded once)."""
    shape, relu, _ = D.BN_CASES["wide"]
    B, C, H, W = shape
    assert B >= 2048                                  # bwd_finalize: nsplit >= 2048 -> 1024 threads
    r = D.bn_inputs(shape, relu)
    g64 = r["g_masked"]
    rows = torch.stack([g64.sum((2, 3)), (g64 * (r["y"].double() - r["mean"].double().view(1, C, 1, 1))).sum((2, 3))], 2).float().contiguous()
    assert rows.shape == (B, C, 2)
    gd, y, st = dev(g64.float()), dev(r["y"]), dev(rows)
    gm, mu, iv = dev(r["gamma"]), dev(r["mean"]), dev(r["invstd"])
    coef, dg, db, dy, tab = out((C * 3,)), out((C,)), out((C,)), out(shape), table()
    L().call("wtpse_bn_bwd_from_stats", P(gd), P(y), P(st), B, P(gm), P(mu), P(iv), P(coef), P(dg), P(db), 0, P(dy), B, C, H * W, P(tab), S())
    guards_ok(coef, dg, db, dy, tab)
    assert amax_value(tab) == float(dy.abs().max())
    check_bn(r, dy, dg, db, what="from_stats, 2051 rows")


def test_batchnorm_backward_one_launch_boundary():
    """C = 96 takes bn_bwd_small_k, C = 95 the three kernels: on the same per-channel data the 95 shared channels agree to the
    fused-vs-separate tolerances of test_maxpool_bwd_with_batchnorm_statistics (test_kernels_gpu.py: dy rtol 1e-4, atol 2e-5 * scale;
    dgamma / dbeta rtol 1e-4, atol 1e-4 * max + 1e-6), and each matches fp64."""
    assert D.bn_bwd_branch(2, 96, 256)["path"] == "small" and D.bn_bwd_branch(2, 95, 256)["path"] == "three"
    r96, r95 = D.bn_inputs((2, 96, 16, 16), True), D.bn_inputs((2, 96, 16, 16), True, channels=95)
    a, b = run_bn_bwd(r96), run_bn_bwd(r95)
    check_bn(r96, *a, what="C=96")
    check_bn(r95, *b, what="C=95")
    close(a[0][:, :95], b[0], rtol=1e-4, atol=2e-5 * float(b[0].abs().max()), what="one launch vs three: dy")
    close(a[1][:95], b[1], rtol=1e-4, atol=1e-4 * float(b[1].abs().max()) + 1e-6, what="one launch vs three: dgamma")
    close(a[2][:95], b[2], rtol=1e-4, atol=1e-4 * float(b[2].abs().max()) + 1e-6, what="one launch vs three: dbeta")


def test_batchnorm_backward_misaligned_operands():
    """(2, 3, 1, 1024) with dz, y and dy misaligned in turn.  A misaligned dy alone keeps the vector reduction: everything is bitwise
    equal to the aligned run.  A misaligned dz or y moves the reduction to the scalar kernel: the sums agree to the fused-vs-separate
    tolerance (test_kernels_gpu.py, as above), and given the same sums (wtpse_bn_bwd_apply) dy is bitwise equal for every form."""
    shape = (2, 3, 1, 1024)
    B, C, H, W = shape
    HW = H * W
    assert D.bn_bwd_branch(B, C, HW) == dict(D.bn_bwd_branch(B, C, HW, dy_aligned=False), apply="vec")
    assert D.bn_bwd_branch(B, C, HW, in_aligned=False)["reduce"] == "scalar"
    r = D.bn_inputs(shape, True)
    a = run_bn_bwd(r)
    check_bn(r, *a, what="aligned")
    for x, y in zip(run_bn_bwd(r, (0, 0, 1)), a):
        assert torch.equal(x, y), "dy misaligned"
    for offs in ((1, 0, 0), (0, 1, 0)):
        b = run_bn_bwd(r, offs)
        check_bn(r, *b, what=str(offs))
        close(b[0], a[0], rtol=1e-4, atol=2e-5 * float(a[0].abs().max()), what="dy")
        close(b[1], a[1], rtol=1e-4, atol=1e-4 * float(a[1].abs().max()) + 1e-6, what="dgamma")
        close(b[2], a[2], rtol=1e-4, atol=1e-4 * float(a[2].abs().max()) + 1e-6, what="dbeta")
    # the two halves: sums from the aligned and the misaligned reduction, then the apply pass of every form on the SAME sums
    ns = L().query("wtpse_bn_bwd_nsplit", B, C, HW)
    ss, gm, mu, iv = dev(r["ss"]), dev(r["gamma"]), dev(r["mean"]), dev(r["invstd"])
    sums = []
    for offs in ((0, 0), (1, 0), (0, 1)):
        dz, y, part, sm = dev(r["dz"], offs[0]), dev(r["y"], offs[1]), out((ns * C * 2,)), out((C, 2))
        L().call("wtpse_bn_bwd_reduce", P(dz), P(y), P(ss), 1, P(mu), P(iv), P(part), P(sm), B, C, HW, S())
        guards_ok(part, sm)
        sums.append(sm)
    for sm in sums[1:]:
        close(sm, sums[0], rtol=1e-4, atol=1e-4 * float(sums[0].abs().max()) + 1e-6, what="scalar vs vector reduction")
    dys = []
    for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        dz, y, dy = dev(r["dz"], offs[0]), dev(r["y"], offs[1]), out(shape, offs[2])
        coef, dg, db, tab = out((C * 3,)), out((C,)), out((C,)), table()
        L().call("wtpse_bn_bwd_apply", P(dz), P(y), P(ss), 1, P(gm), P(mu), P(iv), P(sums[0]), P(sums[0]), B * HW, P(coef), P(dg), P(db),
                 0, P(dy), B, C, HW, P(tab), S())
        guards_ok(dy, coef, dg, db, tab)
        assert amax_value(tab) == float(dy.abs().max())
        dys.append(dy)
    assert all(torch.equal(d, dys[0]) for d in dys[1:])
    close(dys[0], a[0], rtol=1e-4, atol=2e-5 * float(a[0].abs().max()), what="two halves vs one call")     # (sums rounded to fp32 between)


def check_finish(ref, what, coef=None, dgamma=None, dbeta=None, dbias=None):
    """The outputs of a BatchNorm-backward finisher against D.bn_finish_ref (bn_math.h in numpy float64, rounded once to fp32).  The
    bounds are derived, not measured: the sums are exact, so dbeta is; k1, k2, dgamma and dbias are one fp64 expression each, within a
    few 2^-53 of the reference fused or not, and the single rounding to fp32 can differ at a tie only: 1 ulp; k3 is a difference of
    two terms: 2^-23 (|k1 s1 / N| + |k2 mean|); frozen statistics: k2 == k3 == 0."""
    frozen = "dbias" in ref
    got = {"dgamma": dgamma, "dbeta": dbeta, "dbias": dbias}
    if coef is not None:
        got.update(k1=coef[:, 0], k2=coef[:, 1], k3=coef[:, 2])
    for k, v in got.items():
        if v is None:
            continue
        v = v.detach().cpu()
        assert bool(torch.isfinite(v).all()), (what, k, "not finite (unwritten or NaN)")
        n = D.ulps_apart(v, ref[k])
        err = float((v.double() - ref[k]).abs().max())
        print("%s %s: %d ulp, max |got - ref| %.3g" % (what, k, n, err))
        if k == "dbeta" or (frozen and k in ("k2", "k3")):
            assert torch.equal(v.double(), ref[k]), (what, k, "exact")
        elif k == "k3":
            assert bool(((v.double() - ref[k]).abs() <= ref["k3_tol"]).all()), (what, k, err, float(ref["k3_tol"].max()))
        else:
            assert n <= 1, (what, k, n)


@pytest.mark.parametrize("form", D.BN_EXACT_FORMS)
def test_batchnorm_backward_finishers_on_exact_sums(form):
    """Every place that finishes a BatchNorm backward — bn_bwd_small_k, bn_bwd_finalize_k<256> behind the reduction, <256> and <1024>
    on host-built rows (batch and frozen statistics), the tail of a data gradient (batch and frozen) — calls csrc/bn_math.h; here each
    runs on sums that are exact in any order (D.bn_exact_inputs, D.bn_exact_rows, class I of exact_cases) with arbitrary fp32 gamma and
    invstd, against the header's expressions in numpy float64 (check_finish); dy at check_bn's tolerances.  The 3-row and the 2051-row
    finalize are one template on the same sums: bitwise equal.  Whether a tail and the finalize kernel on the statistics the same launch
    left agree bitwise is printed, not asserted (profiles/bn_one_text.md records it)."""
    if form in ("one_launch", "three"):
        B, C0, H, W = D.BN_EXACT_SHAPE
        C = C0 if form == "one_launch" else D.BN_EXACT_CUT
        br = D.bn_bwd_branch(B, C, H * W)
        subset(br, {"path": "small"} if form == "one_launch" else {"path": "three", "reduce": "vec", "apply": "vec", "finalize": 256}, form)
        r = D.bn_exact_inputs(channels=None if form == "one_launch" else C)
        ref = D.bn_finish_ref(r["s1"], r["n2"], B * H * W, r["gamma"], r["mean"], r["invstd"])
        dy, dg, db = run_bn_bwd(r)
        check_finish(ref, form, coef=dy.coef if form == "three" else None, dgamma=dg, dbeta=db)
        ch = lambda k: ref[k].view(1, C, 1, 1)
        r.update(dy=ch("k1") * r["g_masked"] + ch("k2") * r["y"].double() + ch("k3"), dgamma=ref["dgamma"], dbeta=ref["dbeta"])
        check_bn(r, dy, dg, db, what=form)
    elif form in ("finalize", "finalize_frozen"):
        frozen = form == "finalize_frozen"
        C, count = D.BN_EXACT_C, 4 * D.BN_EXACT_ROWS[1]
        rows, s1, n2 = D.bn_exact_rows()
        gamma, invstd, mean = D.bn_exact_channels(C, 730)
        ref = D.bn_finish_ref(s1, n2, count, gamma, mean, invstd, frozen)
        gm, mu, iv = dev(gamma), dev(mean), dev(invstd)
        res = []
        for n in D.BN_EXACT_ROWS:
            assert D.bn_fold_width(n) == (1024 if n == D.BN_EXACT_ROWS[1] else 256)
            st, coef, dg, db, dbias = dev(rows[n]), out((C, 3)), out((C,)), out((C,)), out((C,))
            if frozen:
                L().call("wtpse_bn_bwd_finalize_coef_frozen", P(st), n, C, P(gm), P(iv), P(coef), P(dg), P(db), P(dbias), 0, S())
            else:
                L().call("wtpse_bn_bwd_finalize_coef", P(st), n, C, count, P(gm), P(mu), P(iv), P(coef), P(dg), P(db), 0, S())
            guards_ok(coef, dg, db, dbias, st)
            check_finish(ref, "%s, %d rows" % (form, n), coef=coef, dgamma=dg, dbeta=db, dbias=dbias if frozen else None)
            res.append((coef, dg, db) + ((dbias,) if frozen else ()))
        for a, b in zip(*res):
            assert torch.equal(a, b), "the same sums in 3 and in 2051 rows: one template, the same bits"
    else:
        import exact_cases as E
        from test_kernels_gpu import pack
        frozen = form == "tail_frozen"
        o = ops()
        p = E.bnb_problem(D.BN_EXACT_TAIL, "I")
        B, Cl, Co, bn_second, Cn, H, W, k, relu, x3 = p["case"]
        assert not x3 and p["d"] is not None and bool(p["check_stats"])
        gamma, invstd, _ = D.bn_exact_channels(Cl, 740)
        ref = D.bn_finish_ref(p["stats"][:, 0], p["stats"][:, 1], B * H * W, gamma, p["mean"], invstd, frozen)
        packed, _, off = pack(p["w"].float())
        gm, iv, mu = gamma.to(DEV), invstd.to(DEV), p["mean"].float().to(DEV)
        dg, db, dbias = out((Cl,)), out((Cl,)), out((Cl,))
        g0, g1, stats, coef = o.dgrad_bnb(p["du"].float().to(DEV), packed.data_ptr() + 4 * off, 0, Cl + Co, k, p["y"].float().to(DEV),
                                          p["ss"].float().to(DEV), mu, relu, p["split"], bn_second,
                                          tail=(gm, iv, dg, db) + ((dbias,) if frozen else ()))
        guards_ok(dg, db, dbias)
        assert torch.equal((g1 if (Co and bn_second) else g0).cpu().double(), p["g"]), "masked gradient: class I is exact"
        check_finish(ref, form, coef=coef, dgamma=dg, dbeta=db, dbias=dbias if frozen else None)
        # the finalize kernel on the partials the same launch left
        coef_f, dg_f, db_f, dbias_f = out((Cl, 3)), out((Cl,)), out((Cl,)), out((Cl,))
        if frozen:
            L().call("wtpse_bn_bwd_finalize_coef_frozen", P(stats), stats.shape[0], Cl, P(gm), P(iv), P(coef_f), P(dg_f), P(db_f), P(dbias_f), 0, S())
        else:
            L().call("wtpse_bn_bwd_finalize_coef", P(stats), stats.shape[0], Cl, B * H * W, P(gm), P(mu), P(iv), P(coef_f), P(dg_f), P(db_f), 0, S())
        guards_ok(coef_f, dg_f, db_f, dbias_f)
        check_finish(ref, form + ", finalize kernel on the launch's partials", coef=coef_f, dgamma=dg_f, dbeta=db_f, dbias=dbias_f if frozen else None)
        same = torch.equal(coef, coef_f) and torch.equal(dg, dg_f) and torch.equal(db, db_f) and (not frozen or torch.equal(dbias, dbias_f))
        print("%s: tail and finalize kernel agree bitwise: %s (%d rows of partials)" % (form, same, stats.shape[0]))
        torch.cuda.synchronize()
        E.clear_caches()


@pytest.mark.parametrize("hw", D.BN_VEC_HW + D.BN_SCALAR_HW)
def test_batchnorm_elementwise_forms(hw):
    """affine_act, bn_bwd_apply_coef, bn_bwd_scale_coef and bn_bwd_frozen on (2, 3, 1, hw): vector (hw % 4 == 0, aligned) against
    scalar with each pointer misaligned in turn, bitwise; fp64 at test_batchnorm_train's tolerances ("bn fwd": close() defaults,
    "bn dy": rtol 2e-4, atol 2e-5, dgamma / dbeta: rtol 2e-4, atol 2e-4); the amax tables against abs().max() of what was stored."""
    shape = (2, 3, 1, hw)
    B, C = 2, 3
    r = D.bn_inputs(shape, True)
    y, g, ss = r["y"], r["dz"], r["ss"]
    coef = torch.stack([D.rnd(C, seed=39) * 0.3 + 1, D.rnd(C, seed=40) * 0.2, D.rnd(C, seed=41) * 0.1], 1).contiguous()
    ssd, cd = dev(ss), dev(coef)
    k = coef.double().view(1, C, 3, 1, 1)
    s64 = ss.double().view(1, C, 2, 1, 1)
    forms2 = ((0, 0), (1, 0), (0, 1))
    forms3 = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
    assert D.flat_branch(hw) == ("vec" if hw % 4 == 0 else "scalar")

    res = []
    for offs in forms2:
        yd, z = dev(y, offs[0]), out(shape, offs[1])
        L().call("wtpse_affine_act", P(yd), P(ssd), 1, P(z), B, C, hw, S())
        guards_ok(z, yd)
        res.append(z)
    assert all(torch.equal(z, res[0]) for z in res[1:]), "affine_act"
    close(res[0], F.relu(y.double() * s64[:, :, 0] + s64[:, :, 1]), what="affine_act")

    res = []
    for offs in forms3:
        gd, yd, dy, tab = dev(g, offs[0]), dev(y, offs[1]), out(shape, offs[2]), table()
        L().call("wtpse_bn_bwd_apply_coef", P(gd), P(yd), P(cd), P(dy), B, C, hw, P(tab), S())
        guards_ok(dy, tab)
        assert amax_value(tab) == float(dy.abs().max()), "apply_coef amax"
        res.append(dy)
    assert all(torch.equal(d, res[0]) for d in res[1:]), "bn_bwd_apply_coef"
    close(res[0], k[:, :, 0] * g.double() + k[:, :, 1] * y.double() + k[:, :, 2], rtol=2e-4, atol=2e-5, what="bn_bwd_apply_coef")

    res = []
    for offs in forms2:
        gd, dy, tab = dev(g, offs[0]), out(shape, offs[1]), table()
        L().call("wtpse_bn_bwd_scale_coef", P(gd), P(cd), P(dy), B, C, hw, P(tab), S())
        guards_ok(dy, tab)
        assert amax_value(tab) == float(dy.abs().max()), "scale_coef amax"
        res.append(dy)
    assert all(torch.equal(d.cpu(), coef[:, 0].view(1, C, 1, 1) * g) for d in res), "bn_bwd_scale_coef: the fp32 product"

    # frozen statistics: dy = k1 g with k1 = gamma * invstd (independent of the sums: bitwise equal for every form)
    ns = L().query("wtpse_bn_bwd_nsplit", B, C, hw)
    gm, mu, iv = dev(r["gamma"]), dev(r["mean"]), dev(r["invstd"])
    res = []
    for offs in forms3:
        dz, yd, dy, tab = dev(g, offs[0]), dev(y, offs[1]), out(shape, offs[2]), table()
        part, cf, dg, db, dbias = out((ns * C * 2,)), out((C * 3,)), out((C,)), out((C,)), out((C,))
        L().call("wtpse_bn_bwd_frozen", P(dz), P(yd), P(ssd), 1, P(gm), P(mu), P(iv), P(part), P(cf), P(dg), P(db), P(dbias), 0, P(dy),
                 B, C, hw, P(tab), S())
        guards_ok(dy, tab, part, cf, dg, db, dbias)
        assert amax_value(tab) == float(dy.abs().max()), "frozen amax"
        res.append((dy, dg, db, dbias))
    assert all(torch.equal(t[0], res[0][0]) for t in res[1:]), "bn_bwd_frozen dy"
    for a, b in zip(res[3], res[0]):
        assert torch.equal(a, b), "bn_bwd_frozen, dy misaligned: same reduction, same bits"
    gmask = r["g_masked"]
    k1 = r["gamma"].double() * r["invstd"].double()
    kink = r["on_kink"]
    zero = torch.zeros_like(gmask)
    for dy, dg, db, dbias in res:
        close(torch.where(kink, zero, dy.cpu().double()), torch.where(kink, zero, k1.view(1, C, 1, 1) * gmask), rtol=2e-4, atol=2e-5, what="frozen dy")
        close(db, gmask.sum((0, 2, 3)), rtol=2e-4, atol=2e-4, what="frozen dbeta")
        close(dg, r["invstd"].double() * (gmask * (y.double() - r["mean"].double().view(1, C, 1, 1))).sum((0, 2, 3)), rtol=2e-4, atol=2e-4,
              what="frozen dgamma")
        close(dbias, k1 * gmask.sum((0, 2, 3)), rtol=2e-4, atol=2e-4, what="frozen dbias")


# =============================================================================================== WT loss
def wt_forward(z_dev, per_domain, margin, partial=None):
    """wtpse_wt_loss_fwd / _fwd_partials into guarded outputs -> an ops.WtLossState (what ops.wt_loss_bwd takes)."""
    o = ops()
    B, C, H, W = z_dev.shape
    HW, R = H * W, 3 * per_domain
    st = o.WtLossState()
    st.gram, st.v, st.offdiag, st.diag = out((B, 256)), out((B, 120)), out((B,)), out((B,))
    st.dmmd_dv, st.losses = out((R, 120)), out((3,))
    rowval = out((2 * (R + 1),))                      # R doubles + the tail launch's 8-byte ticket word
    assert rowval.data_ptr() % 8 == 0
    st_guarded = [rowval]
    if partial is None:
        Sq = L().query("wtpse_wt_split", B, HW, 0)
        ws = out((B * Sq * 256,))
        L().call("wtpse_wt_loss_fwd", P(z_dev), B, C, HW, 1e-5, float(margin), 3, per_domain, P(ws), P(st.gram), P(st.v), P(st.offdiag),
                 P(st.diag), P(rowval), P(st.dmmd_dv), P(st.losses), S())
        guards_ok(ws)
    else:
        part, Sq = partial
        L().call("wtpse_wt_loss_fwd_partials", P(part), Sq, B, HW, 1e-5, float(margin), 3, per_domain, P(st.gram), P(st.v), P(st.offdiag),
                 P(st.diag), P(rowval), P(st.dmmd_dv), P(st.losses), S())
    guards_ok(st.gram, st.v, st.offdiag, st.diag, st.dmmd_dv, st.losses, *st_guarded)
    st.z, st.B, st.HW, st.D, st.n, st.margin = z_dev, B, HW, 3, per_domain, float(margin)
    return st


def check_wt_forward(st, ref, what):
    """test_wt_loss_against_oracle_and_golden's tolerances: off / diag rtol 1e-5, atol 1e-7; dom 3e-7 + 1e-3 |ref|; Gram and v rtol
    1e-5, atol 1e-6."""
    B = st.B
    l = st.losses.cpu()
    close(l[0], ref["off"], rtol=1e-5, atol=1e-7, what=what + " off")
    close(l[1], ref["diag"], rtol=1e-5, atol=1e-7, what=what + " diag")
    assert abs(float(l[2]) - float(ref["dom"])) <= 3e-7 + 1e-3 * abs(float(ref["dom"])), (what, float(l[2]), float(ref["dom"]))
    close(st.gram.view(B, 16, 16), ref["gram"], rtol=1e-5, atol=1e-6, what=what + " gram")
    close(st.v, ref["v"], rtol=1e-5, atol=1e-6, what=what + " v")


def wt_backward(st, shape, base, acc, off=0, scaled=False, w_dom=None):
    """wtpse_wt_loss_bwd into a guarded dz, with a guarded M workspace.  scaled: device-scalar upstream gradients of 2 and host weights
    of 0.5, as the golden test passes them; w_dom: the host weight of the domain loss alone."""
    dz, M = out(shape, off, init=base if acc & 1 else None), out((st.B * 256,))
    g = torch.tensor(2.0, device=DEV) if scaled else None
    w = 0.5 if scaled else 1.0
    L().call("wtpse_wt_loss_bwd", P(st.z), st.B, 16, st.HW, st.margin, st.D, st.n, P(st.gram), P(st.offdiag), P(st.diag), P(st.dmmd_dv),
             P(g), P(g), P(g), w, w, w if w_dom is None else float(w_dom), P(M), P(dz), int(acc), S())
    guards_ok(dz, M)
    assert bool(torch.isfinite(M).all()) and bool(torch.isfinite(dz).all())
    return dz


@pytest.mark.parametrize("name", list(D.WT_CASES))
def test_wt_loss_paths(name):
    """Several partial Grams per image (vector and scalar, ragged last chunk), several backward blocks per image, the scalar backward
    with accumulate 0 / 1 / 3, a batch beyond the split target with R < B (images >= R get no MMD gradient): the forward triple,
    Gram, v and dL/dz against oracle.wtpse_cpu.whitening_loss in fp64, margin 0 and a margin that switches one image's clamp off.
    The features (scale 0.7, not whitened) and seeds keep every fp64 Gram entry more than 1e-5 from a sign kink
    (test_dispatch_paths_cpu.py), so no gradient entry is left out."""
    shape, pb, expect = D.WT_CASES[name]
    B, C, H, W = shape
    br = D.wt_branch(B, H * W)
    subset(br, expect, name)
    assert L().query("wtpse_wt_split", B, H * W, 0) == br["S"]
    z = D.wt_feature(shape, D.WT_SEEDS[name])
    assert D.wt_kink_distance(z) > D.KINK_MARGIN
    zd = dev(z)
    base = D.rnd(*shape, seed=40)
    for margin in (0.0, D.wt_margin_one_off(z)):
        ref = D.wt_ref(z, pb, margin)
        st = wt_forward(zd, pb, margin)
        check_wt_forward(st, ref, f"{name} margin={margin:.4g}")
        gmax = float(ref["dz"].abs().max())
        close(wt_backward(st, shape, base, 0), ref["dz"], rtol=2e-3, atol=1e-8 + 2e-4 * gmax, what=f"{name} dz")
        close(wt_backward(st, shape, base, 1, scaled=True), base.double() + ref["dz"], rtol=2e-3, atol=1e-6 + 2e-4 * gmax, what=f"{name} dz acc")
        close(wt_backward(st, shape, base, 3, scaled=True), base.double() * (z > 0) + ref["dz"], rtol=2e-3, atol=1e-6 + 2e-4 * gmax,
              what=f"{name} dz mask-in")
        # images >= R = 3 * per_domain take no part in the MMD (wt_dgram_k: `if (b < R)`): their dz is, bitwise, what a run without
        # the domain loss gives; the images below R do get its gradient
        R = 3 * pb
        with_dom, without = wt_backward(st, shape, base, 0), wt_backward(st, shape, base, 0, w_dom=0.0)
        assert torch.equal(with_dom[R:], without[R:]), f"{name}: an image >= R has an MMD gradient"
        assert all(not torch.equal(with_dom[b], without[b]) for b in range(R)), f"{name}: an image < R has no MMD gradient"


def test_wt_loss_misaligned_operands():
    """HW = 2052 with z, then dz, 4 bytes off: the forward takes gram_partial_k<false> (Gram to the golden test's rtol 1e-5, atol
    1e-6 of the aligned run), the backward gram_bwd_k<false> — bitwise equal to the vector kernel given the same state."""
    name = "hw2052"
    shape, pb, _ = D.WT_CASES[name]
    B, C, H, W = shape
    assert D.wt_branch(B, H * W, z_aligned=False)["fwd"] == "scalar" and D.wt_branch(B, H * W, dz_aligned=False)["bwd"] == "scalar"
    z = D.wt_feature(shape, D.WT_SEEDS[name])
    ref = D.wt_ref(z, pb, 0.0)
    za, zm = dev(z), dev(z, 1)
    st = wt_forward(za, pb, 0.0)
    st_m = wt_forward(zm, pb, 0.0)
    check_wt_forward(st_m, ref, "z misaligned")
    close(st_m.gram, st.gram, rtol=1e-5, atol=1e-6, what="gram, scalar vs vector")
    base = D.rnd(*shape, seed=40)
    for acc in (0, 1, 3):
        a = wt_backward(st, shape, base, acc)
        assert torch.equal(wt_backward(st, shape, base, acc, off=1), a), ("dz misaligned", acc)
        st.z = zm
        assert torch.equal(wt_backward(st, shape, base, acc), a), ("z misaligned", acc)
        st.z = za


@pytest.mark.parametrize("S", list(D.WT_FINALIZE_S))
def test_wt_loss_finalize_widths(S):
    """Partial Grams fed straight into the tail: gram_finalize_k<4> at S = 31, <16> from 32, the single-step remainder of the paired
    loop at 31, 33 and 47.  The pixels of a (3, 16, 8, S) map in S groups, each group's z z^T in fp64 rounded to fp32; the result
    against the oracle on the whole map at the golden test's tolerances."""
    nw, pairs, single = D.WT_FINALIZE_S[S]
    br = D.wt_branch(3, 8 * S, S=S)
    assert (br["finalize"], br["finalize_pairs"], br["finalize_single"]) == (nw, pairs, single)
    shape = (3, 16, 8, S)
    z = D.wt_feature(shape, D.WT_FINALIZE_SEEDS[S])
    part = dev(D.wt_partials(z, S))
    st = wt_forward(dev(z), 1, 0.0, partial=(part, S))
    check_wt_forward(st, D.wt_ref(z, 1, 0.0), f"S={S}")


def test_wt_combine_folds():
    """Both folds of wt_combine_k's header comment (mode 0: WT_PSE.update, mode 1: the student's accumulator overwrite).  No test
    covered this entry point: the tolerance is test_losses_roi_adam's "adam" one (rtol 1e-6, atol 1e-7), the suite's tolerance for a
    handful of fp32 operations on O(1) values."""
    for nmaps in (1, 2, 3):
        losses = D.rnd(nmaps, 3, seed=90).abs() + 0.1
        ld = dev(losses)
        for mode in (0, 1):
            o = out((4,))
            L().call("wtpse_wt_combine", P(ld), nmaps, 3.0, mode, P(o), S())
            guards_ok(o)
            close(o, D.wt_combine_ref(losses, 3.0, mode), rtol=1e-6, atol=1e-7, what=f"wt_combine nmaps={nmaps} mode={mode}")
