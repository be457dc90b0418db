"""Power-of-two equivariance on the GPU (-m gpu; tests/scale_cases.py holds the tables, profiles/scale_equivariance.md the prose).

Scaling by 2^k commutes with every fp32 and fp16 rounding, so if every scale of the x2h arithmetic follows its data, rescaling a
tensor by a power of two changes NO bit of any result once the power of two is undone — no reference and no tolerance needed.  A
fixed scale, a stale amax table, the wrong tensor's table or a missing one changes bits (the negative control shows that it does).
The oracle has the property on these inputs, bit for bit (test_scale_equivariance_cpu.py).

  1  backward of 2^k x loss for calls A and B, whole networks, batch and frozen statistics, all three arithmetics
  2  a BatchNorm's gamma, beta x 2^k and its consumer's weights / 2^k inside a ConvD and a ConvU block, through the engine's own
     schedule; the concat pair (one scale for both halves, by design) against fp64 with the derived bound instead
  3  negative control: the fixed 2^2 activation scale IS seen
  4  amax tables on caller-owned tensors: the attach / look-up / invalidate protocol of ops.py"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import scale_cases as S
from oracle.filler import fill_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from wtpse_hip import ops
    return ops


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _switch(terms):
    """wtpse_x3_terms is process-global: switch it for one test and put it back (as the bf16_mode fixture does)."""
    o = _ops()
    was = o.lib().query("wtpse_x3_terms", terms)
    assert was in (2, 3), "the library must default to an fp32-accuracy arithmetic (x2h or x3)"
    return o, was


@pytest.fixture(params=S.TERMS, ids=lambda t: {2: "x2h", 3: "x3", 1: "bf16"}[t])
def arithmetic(request):
    o, was = _switch(request.param)
    yield o
    o.lib().query("wtpse_x3_terms", was)


@pytest.fixture
def x2h():
    o, was = _switch(2)
    yield o
    o.lib().query("wtpse_x3_terms", was)


# ================================================================================================================ section 1
def _build_nets():
    import algorithms
    import shape_networks
    main = algorithms.WT_PSE(n_channels=3, n_classes=1, hparams=S.HP, device=DEV, two_step=False, per_domain_batch=S.CALL_PB,
                             source_domain_num=3).to(DEV)
    shape = shape_networks.ShapeVariationalDist_x(S.HP, DEV, n_classes=1, number_source_domain=3, batch_size=S.CALL_PB).to(DEV)
    fill_state_dict(main, S.CALL_SEED_W)
    fill_state_dict(shape, S.CALL_SEED_W + 3)
    return main, shape


def _run_calls(main, shape, k, img, od, eps):
    """Calls A and B as tests/test_frozen_bn_gpu.py runs them, the loss x 2^k.  -> {name: tensor}."""
    main.zero_grad(); shape.zero_grad()
    main.set_noise([eps])
    out, _, _, ins, dom = main.update(img, od, two_stage_inputs=img, sp_mask=od, two_step=True)
    seg = F.binary_cross_entropy(torch.sigmoid(out), od)
    (2.0 ** k * (seg + ins + dom)).backward()
    r = {"A.logits": out.detach().clone(), "A.loss": torch.stack([seg, ins, dom]).detach().clone(), "A.grads": main.flat_grads().clone()}
    shape.zero_grad(); main.zero_grad()
    main.set_noise([eps])
    kd, ins_t, ins_ij, ins_ii, dom_s = shape.update(main, img, od, two_stage_inputs=img, two_step=True)
    (2.0 ** k * (kd + ins_t + dom_s)).backward()
    r["B.loss"] = torch.stack([kd, ins_t, ins_ij, ins_ii, dom_s]).detach().clone()
    r["B.grads"] = shape.flat_grads().clone()
    main.set_noise([])
    return r


def _differing_parameters(net, got, want):
    """Names of the parameters whose slice of the flat gradient differs (the first step of narrowing a failure down)."""
    bad = []
    for n, p in net.named_parameters():
        off = net.param_offset(p)
        if not _same(got[off:off + p.numel()], want[off:off + p.numel()]):
            bad.append(n)
    return bad


@pytest.mark.parametrize("mode", S.MODES)
def test_gradient_scale_whole_calls(arithmetic, mode):
    """Backward of 2^k x loss, k in GRAD_KS, against k = 0: logits and loss scalars bitwise equal, flat gradients of both networks
    bitwise the k = 0 ones x 2^k."""
    img, od, eps = (t.to(DEV) for t in S.call_inputs())
    main, shape = _build_nets()
    for n in (main, shape):
        n.train(mode == "train")
    base = _run_calls(main, shape, 0, img, od, eps)
    assert bool(torch.isfinite(base["A.grads"]).all()) and bool(torch.isfinite(base["B.grads"]).all())
    assert float(base["A.grads"].abs().max()) > 0 and float(base["B.grads"].abs().max()) > 0
    for k in S.GRAD_KS:
        run = _run_calls(main, shape, k, img, od, eps)
        for n in ("A.logits", "A.loss", "B.loss"):
            assert _same(run[n], base[n]), "%s depends on the gradient scale (k = %d, %s)" % (n, k, mode)
        for call, net in (("A", main), ("B", shape)):
            got, want = run[call + ".grads"], base[call + ".grads"] * 2.0 ** k
            if not _same(got, want):
                bad = _differing_parameters(net, got, want)
                raise AssertionError("call %s, k = %d, %s: %d elements in %d parameters differ from 2^k x the k = 0 gradient: %s"
                                     % (call, k, mode, int((_bits(got) != _bits(want)).sum()), len(bad), bad[:12]))


# ================================================================================================================ section 2
def _holder(name):
    from wtpse_hip import nn as E
    b = S.BLOCKS[name]

    class Holder(E.HipNet):
        def __init__(self, blk):
            super().__init__()
            self.blk = blk
            self._finish_init()

    return Holder((E.ConvDBlock if b.kind == "convd" else E.ConvUBlock)(*b.args)).to(DEV)


def _run_block(h, name, sd, mode, scope=True, dz_scale=1.0):
    """The block with the state `sd` through the engine's own schedule, forward + backward of the seeded upstream gradient (x dz_scale).
    -> {"y", "dx", "dprev" (ConvU), "g.<parameter>"}; fresh input tensors on every call."""
    from wtpse_hip import nn as E
    o = _ops()
    training = mode == "train"
    h.blk.load_state_dict(sd)
    h.train(training)
    h.ensure_ready(repack=True)
    h.zero_grad()
    x, prev, dz = (t.to(DEV) if t is not None else None for t in S.block_inputs(name))
    dz = dz * dz_scale
    with (o.fwd_scope(torch.device(DEV, torch.cuda.current_device())) if scope else contextlib.nullcontext()):
        if prev is None:
            y, tape = E.convd_fwd(h.blk, x, training)
        else:
            y, tape = E.convu_fwd(h.blk, x, prev, training)
        out = {"y": y.dense().clone()}
    h.begin_backward()
    if prev is None:
        out["dx"] = E.convd_bwd(h.blk, tape, dz, None, need_dx=True)
    else:
        out["dx"], out["dprev"] = E.convu_bwd(h.blk, tape, dz)
    h.end_backward()
    torch.cuda.synchronize()
    for n, p in h.blk.named_parameters():
        if p.grad is not None:
            out["g." + n] = p.grad.detach().clone()
    return out


@pytest.mark.parametrize("scope", [True, False], ids=["fwd_scope", "no_scope"])
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("pair", S.BITWISE_PAIRS)
def test_activation_scale_blocks(arithmetic, pair, mode, scope):
    """gamma, beta of the pair's BatchNorm x 2^k, its consumer's weights / 2^k, k in BLOCK_KS, against k = 0: the block's output, dx and
    dprev bitwise unchanged, d gamma / d beta of that BatchNorm bitwise / 2^k, the consumer's dW bitwise x 2^k, every other gradient
    bitwise unchanged."""
    p = S.PAIRS[pair]
    h = _holder(p.block)
    sd = S.block_state(p.block)
    base = _run_block(h, p.block, sd, mode, scope)
    want_names = {"y", "dx"} | ({"dprev"} if S.BLOCKS[p.block].prev is not None else set())
    want_names |= {"g." + n for n in sd if not S.O.is_buffer(n) and not (mode == "train" and S.pre_bn_bias("g." + n))}
    assert set(base) == want_names, sorted(set(base) ^ want_names)
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in base.values())
    for k in S.BLOCK_KS:
        run = _run_block(h, p.block, S.rescale_state(sd, p, k), mode, scope)
        fac = S.expected_factors(p, k, base)
        assert sorted(run) == sorted(base)
        bad = []
        for n in sorted(base):
            f = fac[n].to(DEV) if torch.is_tensor(fac[n]) else fac[n]
            if not _same(run[n], base[n] * f):
                bad.append((n, int((_bits(run[n]) != _bits(base[n] * f)).sum()), run[n].numel()))
        assert not bad, "%s, k = %d, %s: tensors that differ (name, elements, of): %s" % (pair, k, mode, bad)


def _rel_l2(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize("mode", S.MODES)
def test_activation_scale_concat_pair(arithmetic, mode):
    """ConvU bn2 -> the second half of conv3's input columns.  Not bitwise by design in x2h: both halves of the concatenated input
    share max(in_amax, in_amax1) and the layer's weights share one pack scale, so the half that is 2^|k| smaller keeps |k| bits
    fewer.  Against an fp64 evaluation of the oracle's conv_u on the same rescaled state, relative L2 per tensor:
    everything finite and err(k) <= 2 x 2^|k| x err(0) (one bit per binade of imbalance, x 2 for rounding direction; err(0) is
    measured here, nothing is fixed in advance).  Prints the curve before it asserts.
    The x3 and bf16 arithmetics scale nothing (a bf16 term carries fp32's exponent: x3_in_scale is 1 for TERMS != 2 and the pack kernel
    packs at scale 1), so there the concat pair is held to the bitwise criterion of the other pairs as well."""
    p = S.PAIRS[S.CONCAT_PAIR]
    h = _holder(p.block)
    sd = S.block_state(p.block)
    err, runs = {}, {}
    for k in (0,) + S.BLOCK_KS:
        st = S.rescale_state(sd, p, k)
        run = runs[k] = _run_block(h, p.block, st, mode)
        ref = S.oracle_block(p.block, st, mode, torch.float64)
        assert all(bool(torch.isfinite(v).all()) for v in run.values()), (k, [n for n, v in run.items() if not bool(torch.isfinite(v).all())])
        err[k] = {n: _rel_l2(run[n], ref[n]) for n in run}
    for n in sorted(err[0]):
        print("[concat %s terms=%d] %-16s err(0) %.3e; err(k)/err(0): %s" % (
            mode, _ops().x3_terms(), n, err[0][n], "  ".join("k=%d %.2f" % (k, err[k][n] / err[0][n]) for k in S.BLOCK_KS)))
    bad = [(n, k, err[k][n], err[0][n]) for k in S.BLOCK_KS for n in err[0] if not S.concat_bound(err[k][n], err[0][n], k)]
    assert not bad, bad
    if _ops().x3_terms() != 2:
        for k in S.BLOCK_KS:
            fac = S.expected_factors(p, k, runs[0])
            diff = [n for n in sorted(runs[0])
                    if not _same(runs[k][n], runs[0][n] * (fac[n].to(DEV) if torch.is_tensor(fac[n]) else fac[n]))]
            assert not diff, "k = %d, %s: not bitwise without a shared scale: %s" % (k, mode, diff)


# ================================================================================================================ section 3
def test_fixed_activation_scale_is_seen(x2h, monkeypatch):
    """Negative control: with the forward amax tables switched off every activation is scaled by the fixed 2^2 fallback, which does NOT
    follow its data — the ConvD case at k = -16 must then differ from k = 0 in at least one bit of the block's output."""
    from wtpse_hip import nn as E
    monkeypatch.setattr(E, "FWD_AMAX", False)
    pair = "convd.bn1-conv2"
    p = S.PAIRS[pair]
    h = _holder(p.block)
    sd = S.block_state(p.block)
    base = _run_block(h, p.block, sd, "train")
    run = _run_block(h, p.block, S.rescale_state(sd, p, -16), "train")
    assert bool(torch.isfinite(run["y"]).all())
    assert not _same(run["y"], base["y"]), "a scale that does not follow its data went unseen"


def test_fixed_gradient_scale_is_seen(x2h, monkeypatch):
    """The same control on the gradients' side.  The ConvD block's upstream gradient x 2^-24: every gradient is bitwise 2^-24 x the
    unscaled one while the tables follow the data — and is NOT once every look-up answers with one fixed table (value 64: scale
    2^8, in range for the forward input and the unscaled gradients, fourteen bits short for the scaled ones)."""
    o = x2h
    k = min(S.GRAD_KS)
    h = _holder("convd")
    sd = S.block_state("convd")
    scaled = lambda base: {n: v * (1.0 if n == "y" else 2.0 ** k) for n, v in base.items()}
    base, run = _run_block(h, "convd", sd, "train"), _run_block(h, "convd", sd, "train", dz_scale=2.0 ** k)
    assert all(_same(run[n], v) for n, v in scaled(base).items())
    fixed = torch.zeros(o.AMAX_WORDS, dtype=torch.int32, device=DEV)
    fixed[0] = torch.tensor(64.0).view(torch.int32)
    monkeypatch.setattr(o, "amax_attached", lambda t: fixed)
    base, run = _run_block(h, "convd", sd, "train"), _run_block(h, "convd", sd, "train", dz_scale=2.0 ** k)
    assert all(bool(torch.isfinite(v).all()) for v in base.values())
    differ = [n for n, v in scaled(base).items() if not _same(run[n], v)]
    assert _same(run["y"], base["y"]) and {"dx", "g.conv1.weight", "g.conv2.weight"} <= set(differ), differ


# ================================================================================================================ section 4
AMAX_STRIDE = 16        # words between the shards of an amax table (one per 64-byte line)


def _table_value(tab):
    return float(tab[::AMAX_STRIDE].view(torch.float32).max())


def _two_layer_net():
    """The two-layer net of test_x2h_train_mode_batchnorm_bound."""
    from wtpse_hip import nn as E
    C = 64

    class Two(E.HipNet):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = E.ConvP(C, C, 3), E.BNP(C)
            self.conv2, self.bn2 = E.ConvP(C, C, 3), E.BNP(C)
            self._finish_init()
    net = Two().to(DEV)
    fill_state_dict(net, 181)
    net.train()
    net.ensure_ready(repack=True)
    return net


@pytest.mark.parametrize("k", [12, -12])
def test_forward_table_follows_a_reused_input(x2h, k):
    """A caller's x goes through convbn_fwd, is rescaled IN PLACE and goes through again: the result must be bitwise what a fresh
    x.clone() gives.  (A table cached on x by the first call describes the contents before: 2^12 larger data overflows fp16 under
    it, 2^-12 smaller data loses twelve bits.)"""
    from wtpse_hip import nn as E
    o = x2h
    net = _two_layer_net()
    x = S.make_noise(182, (4, 64, 32, 32)).to(DEV)

    def run(inp):
        with o.fwd_scope(torch.device(DEV, torch.cuda.current_device())):
            a1, _ = E.convbn_fwd(net.conv1, net.bn1, inp, None, True, True, want_tape=False)
            a2, _ = E.convbn_fwd(net.conv2, net.bn2, a1, None, True, True, want_tape=False)
            return a1.t.clone(), a2.dense().clone()

    first = run(x)
    assert all(bool(torch.isfinite(t).all()) for t in first)
    x.mul_(2.0 ** k)
    reused, fresh = run(x), run(x.clone())
    assert all(bool(torch.isfinite(t).all()) for t in fresh)
    assert _same(reused[0], fresh[0]) and _same(reused[1], fresh[1]), "the reused input ran under the scale of its earlier contents"
    assert _table_value(o.amax_of(x)) == float(x.abs().max())


def test_backward_table_follows_a_reused_gradient(x2h):
    """convd_bwd with a caller's dz that is rescaled in place (x 2^-12) and passed again: bitwise what a fresh clone gives; and the
    same for a data gradient launched on the caller's tensor directly (nn._dgrad: the launch that takes its scale from the table
    of the tensor it is handed)."""
    from wtpse_hip import nn as E
    o = x2h
    name = "convd"
    h = _holder(name)
    h.blk.load_state_dict(S.block_state(name))
    h.train()
    h.ensure_ready(repack=True)
    x, _, dz0 = (t.to(DEV) if t is not None else None for t in S.block_inputs(name))

    def run(dz):
        h.zero_grad()
        _, tape = E.convd_fwd(h.blk, x.clone(), True)
        h.begin_backward()
        dx = E.convd_bwd(h.blk, tape, dz, None, need_dx=True)
        h.end_backward()
        torch.cuda.synchronize()
        return [dx.clone()] + [p.grad.detach().clone() for p in h.blk.parameters() if p.grad is not None]

    dz = dz0.clone()
    run(dz)
    dz.mul_(2.0 ** -12)
    reused, fresh = run(dz), run(dz.clone())
    assert len(reused) == len(fresh) and all(_same(a, b) for a, b in zip(reused, fresh))

    net = _two_layer_net()
    g = S.make_noise(183, (4, 64, 32, 32)).to(DEV)
    d_first = E._dgrad(net.conv2, g)[0].clone()
    g.mul_(2.0 ** -12)
    d_reused, d_fresh = E._dgrad(net.conv2, g)[0].clone(), E._dgrad(net.conv2, g.clone())[0].clone()
    assert bool(torch.isfinite(d_first).all()) and _same(d_reused, d_fresh), "the reused gradient ran under the scale of its earlier contents"
    assert _same(d_fresh, d_first * 2.0 ** -12)               # (and the data gradient is itself equivariant)


def test_amax_table_protocol(x2h):
    """attach / look-up / invalidate (ops.amax_attach, amax_attached, amax_of, _amax_stale): a table is found again while the tensor
    keeps its contents, and never after a write — through torch (the version counter, shared by detached aliases) or through the
    library's own in-place launches."""
    o = x2h
    t = S.make_noise(184, (2, 8, 16, 16)).to(DEV)
    tab = o.amax_of(t)
    assert _table_value(tab) == float(t.abs().max())
    assert o.amax_of(t) is tab and o.amax_attached(t) is tab                  # cached: no second pass
    t.mul_(4.0)
    assert o.amax_attached(t) is None                                          # ... but not beyond the contents it was taken from
    tab2 = o.amax_of(t)
    assert tab2 is not tab and _table_value(tab2) == float(t.abs().max()) == 4.0 * _table_value(tab)
    t.copy_(S.make_noise(185, (2, 8, 16, 16)) * 1e-3)
    assert _table_value(o.amax_of(t)) == float(t.abs().max())
    alias = t.detach()                                                         # (what update() makes of its arguments)
    atab = o.amax_of(alias)
    t.add_(1.0)
    assert o.amax_attached(alias) is None and _table_value(o.amax_of(alias)) == float(t.abs().max()) != _table_value(atab)
    o.amax_of(t)
    o.axpy(t, t.clone(), 1.0)                                                  # the library's own write: no version, _amax_stale
    assert o.amax_attached(t) is None and _table_value(o.amax_of(t)) == float(t.abs().max())
    u = torch.empty_like(t)
    u.wt_amax = tab                                                            # attached past the protocol: never trusted
    assert o.amax_attached(u) is None
    # a producer's table stays with its result
    d = o.upsample2x_bwd(t)
    assert d.wt_amax is not None and o.amax_attached(d) is d.wt_amax and _table_value(d.wt_amax) == float(d.abs().max())


@pytest.mark.parametrize("entry", S.INPLACE_ENTRY_POINTS, ids=[n for n, _ in S.INPLACE_ENTRY_POINTS])
def test_inplace_entry_points_leave_no_stale_table(x2h, entry):
    """Every entry point of ops.py that writes into a caller-supplied float tensor: after the call the tensor carries no table, or
    one that holds its abs().max()."""
    o = x2h
    name, build = entry
    call, written = build(o, torch.device(DEV, torch.cuda.current_device()))
    before = [t.clone() for t in written]
    for t in written:
        wrong = torch.zeros(o.AMAX_WORDS, dtype=torch.int32, device=t.device)
        wrong[0] = torch.tensor(12345.0).view(torch.int32)
        o.amax_attach(t, wrong)
        assert o.amax_attached(t) is wrong
    call()
    torch.cuda.synchronize()
    assert any(not torch.equal(_bits(a), _bits(b)) for a, b in zip(written, before)), name + ": the call wrote nothing"
    for t in written:
        tab = o.amax_attached(t)
        assert tab is None or _table_value(tab) == float(t.abs().max()), name
        assert _table_value(o.amax_of(t)) == float(torch.nan_to_num(t).abs().max())
