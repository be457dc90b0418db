"""Frozen-BatchNorm training on the GPU (-m gpu): update() under .eval() followed by backward() — the backward through BatchNorm on
its running statistics (include/wtpse_hip.h: wtpse_bn_bwd_frozen and its siblings; wtpse_hip/nn.py: _bn_bwd) — against the
reference's own eval-mode modules (tests/golden/frozen_bn.npz, written by tools/make_golden_frozen.py), the folds against fp64 at
kernel level, and the step / run drivers with freeze_bn=True."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sketch
from oracle import wtpse_cpu as O
from oracle.filler import fill_state_dict, fill_value
from oracle.inputs import make_inputs, make_noise

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = dict(O.DEFAULT_HPARAMS)
TOL = 1e-4     # the project's bar for logits and loss values
CAL = 3.0      # the project's strict gradient rule (tests/test_parity_gpu.py: assert_calibrated(strict=True)): every tensor within
FLOOR = 5e-4   # CAL x the farthest of three fp32 evaluations of the reference + FLOOR, all gradients together within CAL x + 2e-4
FLOOR_TOTAL = 2e-4


def build_nets(pb, seed_w):
    import algorithms
    import shape_networks
    mk = lambda two_step: algorithms.WT_PSE(n_channels=3, n_classes=1, hparams=HP, device=DEV, two_step=two_step,
                                            per_domain_batch=pb, source_domain_num=3).to(DEV)
    mks = lambda: shape_networks.ShapeVariationalDist_x(HP, DEV, n_classes=1, number_source_domain=3, batch_size=pb).to(DEV)
    main, shape, main_oc, shape_oc = mk(False), mks(), mk(True), mks()
    for n, s in ((main, 0), (shape, 3), (main_oc, 7), (shape_oc, 11)):
        fill_state_dict(n, seed_w + s)
    return main, shape, main_oc, shape_oc


def close(a, b, rtol=TOL, atol=TOL, what=""):
    a = torch.as_tensor(np.asarray(a.detach().cpu()) if torch.is_tensor(a) else np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b.detach().cpu()) if torch.is_tensor(b) else np.asarray(b)).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e}, ref scale {b.abs().max():.3e}"


def _buffers(net):
    return {k: b.detach().clone() for k, b in net.named_buffers()}


def _check_grads(g, ci, call, net, sketch_seed):
    """The strict rule on EVERY tensor of the fixture (the pre-BatchNorm conv biases included).  Prints each figure before it asserts."""
    names = [str(n) for n in g["c%d_%s_names" % (ci, call)]]
    n2s, yard2 = g["c%d_%s_n2" % (ci, call)], g["c%d_%s_yard2" % (ci, call)]
    small, proj = g["c%d_%s_fp_small" % (ci, call)].astype(np.float64), g["c%d_%s_fp_proj" % (ci, call)].astype(np.float64)
    params = dict(net.named_parameters())
    so = pi = 0
    num_h = den = 0.0
    num_c = np.zeros(3)
    bad, ratios, worst = [], [], (0.0, 0.0, 0.0, "")
    for i, k in enumerate(names):
        n, n2 = int(n2s[i, 0]), float(n2s[i, 1])
        if n <= sketch.SMALL:
            data = small[so:so + n]
            so += n
        else:
            data = proj[pi]
            pi += 1
        p = params[k]
        assert p.grad is not None, "%s: no gradient" % k
        d2 = sketch.distance2(p.grad, {"n": n, "norm2": n2, "data": data}, sketch_seed + i)
        h, c = (d2 / (n2 + 1e-60)) ** 0.5, (float(yard2[i].max()) / (n2 + 1e-60)) ** 0.5
        if h > CAL * c + FLOOR:
            bad.append((h, c, k))
        ratios.append(h / max(c, 1e-30))
        worst = max(worst, (h, c, h / max(c, 1e-30), k))
        num_h += d2; den += n2; num_c += yard2[i]
    for k, p in params.items():            # what the reference's graph does not reach carries no gradient here either
        if k not in names:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    tot_h, tot_c = (num_h / den) ** 0.5, (float(num_c.max()) / den) ** 0.5
    print(f"[frozen case {ci} call {call}] all gradients: HIP {tot_h:.3e} vs the farthest of three reference-fp32 draws {tot_c:.3e} from "
          f"fp64 (ratio {tot_h / max(tot_c, 1e-30):.2f}); median per-tensor ratio {float(np.median(ratios)):.2f}; worst tensor "
          f"{worst[3]}: HIP {worst[0]:.3e} vs {worst[1]:.3e}; {len(bad)} of {len(names)} tensors beyond {CAL:.0f}x + {FLOOR:g}")
    assert not bad, f"{call}: {len(bad)} tensors beyond {CAL:.0f}x + {FLOOR:g}: {sorted(bad, reverse=True)[:4]}"
    assert tot_h <= CAL * tot_c + FLOOR_TOTAL, (tot_h, tot_c)


@pytest.mark.parametrize("ci", [0, 1])
def test_eval_update_backward_vs_reference(golden_dir, ci):
    """model.eval(); update(); loss.backward() for call A (WT_PSE.update + BCE + ins + dom) and call B (the student's update: kd + ins +
    dom) on the fixture's seeded inputs: logits and losses within 1e-4, EVERY gradient tensor inside the strict band, buffers
    bitwise unchanged, two runs bitwise equal."""
    g = np.load(os.path.join(golden_dir, "frozen_bn.npz"))
    B, pb, H, s_in, s_a, s_t, s_s = (int(v) for v in g["cases"][ci])
    K, small, seed_w, sketch_seed = (int(v) for v in g["meta"])
    assert (K, small) == (sketch.K, sketch.SMALL)
    img, od, _ = make_inputs(s_in, B, H, H)
    img, od = img.to(DEV), od.to(DEV)
    eps = make_noise(s_a, (B, 1, H, H))
    main, shape, _, _ = build_nets(pb, seed_w)
    main.eval(); shape.eval()
    before = {"A": _buffers(main), "B": _buffers(shape)}
    runs = []
    for rep in range(2):
        main.zero_grad(); shape.zero_grad()
        main.set_noise([eps])
        out, _, _, ins, dom = main.update(img, od, two_stage_inputs=img, sp_mask=od, two_step=True)
        seg = F.binary_cross_entropy(torch.sigmoid(out), od)
        (seg + ins + dom).backward()
        ga = main.flat_grads().clone()
        if rep == 0:
            ref = torch.from_numpy(g["c%d_logits" % ci])
            close(out if H <= 64 else out[:, :, ::4, ::4], ref, what="logits")
            close(O.checksum(out.float().cpu())[:2] / out.numel(), g["c%d_logits_cs" % ci][:2] / out.numel(), what="logits checksum")
            close(torch.stack([seg, ins, dom]), g["c%d_A_loss" % ci], what="call A losses")
            _check_grads(g, ci, "A", main, sketch_seed)
        shape.zero_grad(); main.zero_grad()
        kd, ins_t, ins_ij, ins_ii, dom_s = shape.update(main, img, od, two_stage_inputs=img, two_step=True)
        (kd + ins_t + dom_s).backward()
        if rep == 0:
            close(torch.stack([kd, ins_t, ins_ij, ins_ii, dom_s]), g["c%d_B_loss" % ci], what="call B losses")
            _check_grads(g, ci, "B", shape, sketch_seed)
        runs.append((out.clone(), ga, shape.flat_grads().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    for call, net in (("A", main), ("B", shape)):
        names = [str(n) for n in g["c%d_%s_buf_names" % (ci, call)]]
        now = _buffers(net)
        assert sorted(now) == names
        for i, k in enumerate(names):
            assert torch.equal(now[k], before[call][k]), "buffer %s changed" % k
            cs = O.checksum(now[k].float().cpu())[:2]
            assert np.allclose(cs, g["c%d_%s_buf_cs" % (ci, call)][i], rtol=1e-6, atol=0), k


# ------------------------------------------------------------------------------------------------------------ kernel level
def _layer(C, H, W, relu, seed, B=2):
    """A conv -> BatchNorm(eval) [-> ReLU] layer's tensors with no pre-activation within 1e-3 of zero: a = +-(2e-3 + |n|), and y the
    raw conv output that gives it."""
    gen = torch.Generator().manual_seed(seed)
    gamma = (0.5 + torch.rand(C, generator=gen)) * (torch.randint(0, 2, (C,), generator=gen) * 2 - 1).float()
    beta, rm, rv = 0.3 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen), 0.6 + 0.8 * torch.rand(C, generator=gen)
    gamma, beta, rm, rv = (t.to(DEV) for t in (gamma, beta, rm, rv))
    tgen = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(B, C, H, W, device=DEV, generator=tgen, dtype=torch.float64)
    a = torch.sign(a) * (2e-3 + a.abs())
    s = (gamma.double() / torch.sqrt(rv.double() + 1e-5)).view(1, -1, 1, 1)
    y = ((a - beta.double().view(1, -1, 1, 1)) / s + rm.double().view(1, -1, 1, 1)).float()
    dz = torch.randn(B, C, H, W, device=DEV, generator=tgen)
    return gamma, beta, rm, rv, y, dz


def _sum_bound(hip, t64, t32_sum, scale=None):
    """|HIP - fp64| <= max(3 |torch fp32 on the device - fp64|, log2(N) 2^-24 sum |t_i|) per channel: the second term is the
    first-order bound of pairwise summation of N terms in fp32 (derived, not tuned).  t64: the terms [B, C, H, W] in fp64;
    scale: a per-channel factor both sides carry (dgamma = r x the sum)."""
    N = t64.numel() // t64.shape[1]
    ref = t64.sum(dim=(0, 2, 3))
    bound = torch.maximum(3 * (t32_sum.double() - ref).abs(), math.log2(N) * 2.0 ** -24 * t64.abs().sum(dim=(0, 2, 3)))
    if scale is not None:
        ref, bound = ref * scale, bound * scale.abs()
    err = (hip.double() - ref).abs()
    return err, bound


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("hw", [(16, 16), (64, 48), (256, 256)])
@pytest.mark.parametrize("C", [16, 32, 64, 256])
def test_frozen_folds_at_kernel_level(C, hw, relu):
    """The plain-dz fold (wtpse_bn_bwd_frozen) and the from-stats fold on the partials of the max-pool backward
    (wtpse_maxpool2_bwd_bnb -> wtpse_bn_bwd_from_stats_frozen): dy = the fp32 product s_c g BITWISE, both reductions within the
    pairwise-summation bound, the conv-bias gradient = s_c sum g, the amax table = max |dy|, two runs bitwise equal."""
    from wtpse_hip import ops
    H, W = hw
    gamma, beta, rm, rv, y, dz = _layer(C, H, W, relu, seed=C * 1000 + H + relu)
    ss, mean, invstd = ops.bn_eval_coeffs_stats(gamma, beta, rm, rv)
    assert torch.equal(ss, ops.bn_eval_coeffs(gamma, beta, rm, rv)) and torch.equal(mean, rm)
    assert torch.allclose(invstd.double(), 1 / torch.sqrt(rv.double() + 1e-5), rtol=3e-7, atol=0)
    pre = y.double() * ss[:, 0].double().view(1, -1, 1, 1) + ss[:, 1].double().view(1, -1, 1, 1)
    assert float(pre.abs().min()) >= 1e-3, "a pre-activation within 1e-3 of zero"
    s = gamma * invstd                                     # fp32 product, as the fold forms k1

    def check(dy, dgamma, dbeta, dbias, g, what):
        assert torch.equal(dy.view(torch.int32), (s.view(1, -1, 1, 1) * g).view(torch.int32)), what + ": dy is not the fp32 product"
        g64 = g.double()
        t2_64 = g64 * (y.double() - mean.double().view(1, -1, 1, 1))
        t2_32 = (g * (y - mean.view(1, -1, 1, 1))).sum(dim=(0, 2, 3))
        for name, hip, (err, bound) in (("sum g", dbeta, _sum_bound(dbeta, g64, g.sum(dim=(0, 2, 3)))),
                                        ("sum g (y - m)", dgamma, _sum_bound(dgamma, t2_64, t2_32, invstd.double()))):
            k = int((err - bound).argmax())
            print(f"[{what} C={C} {H}x{W} relu={relu}] {name}: worst channel {k}: |HIP - fp64| {float(err[k]):.3e}, bound {float(bound[k]):.3e}")
            assert bool((err <= bound).all()), f"{what} {name}: channel {k}: {float(err[k]):.3e} > {float(bound[k]):.3e}"
        # the conv-bias gradient is the fold's s_c sum g: fp64 product of k1 and the folded sum, rounded once
        want = s.double() * g64.sum(dim=(0, 2, 3))
        err, bound = _sum_bound(dbias, g64, g.sum(dim=(0, 2, 3)), s.double())
        assert bool((err <= bound + 2.0 ** -23 * want.abs()).all()), what + ": conv-bias gradient"
        if dy.wt_amax is not None:                       # (x2h arithmetic: the consumers scale the gradient from it)
            assert float(dy.wt_amax.view(torch.float32).max()) == float(dy.abs().max()), what + ": amax table"

    g = torch.where(pre > 0, dz, torch.zeros_like(dz)) if relu else dz
    outs = []
    for rep in range(2):
        dgamma, dbeta, dbias = (torch.full((C,), 7.0, device=DEV) for _ in range(3))
        dy = ops.bn_bwd_frozen(dz, y, ss, relu, gamma, mean, invstd, dgamma, dbeta, dbias)
        outs.append((dy, dgamma, dbeta, dbias))
    check(*outs[0], g, "plain")
    assert all(torch.equal(a, b) for a, b in zip(*outs)), "plain: two runs differ"
    if relu and H % 2 == 0 and W % 4 == 0:
        # the max-pool variant: x = the raw output of the layer, dout at half resolution -> (masked gradient, partials)
        dout = torch.randn(y.shape[0], C, H // 2, W // 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
        outs = []
        for rep in range(2):
            r = ops.maxpool2_bwd_bnb(y, dout, None, ss, True, mean)
            assert r is not None
            gm, stats = r
            dgamma, dbeta, dbias = (torch.full((C,), 7.0, device=DEV) for _ in range(3))
            dy = ops.bn_bwd_from_stats_frozen(gm, stats, gamma, invstd, dgamma, dbeta, dbias)
            outs.append((dy, dgamma, dbeta, dbias))
            coef = ops.bn_bwd_finalize_coef_frozen(stats, gamma, invstd, *(torch.empty(C, device=DEV) for _ in range(3)))
            assert torch.equal(coef[:, 0], s) and not bool(coef[:, 1:].any())
            assert torch.equal(ops.bn_bwd_scale_coef(gm, coef), dy)
        assert bool((gm[pre <= 0] == 0).all())
        check(*outs[0], gm, "max-pool")
        assert all(torch.equal(a, b) for a, b in zip(*outs)), "max-pool: two runs differ"


def test_fused_and_stand_alone_routes_agree(monkeypatch):
    """A ConvD and a ConvU block in eval mode through the schedule's routes: the default (reductions in the producing data gradient's
    epilogue, folded by its tail, dy formed on load where a consumer can) against WTPSE_BN_IN=0, WTPSE_BN_TAIL=0 and
    WTPSE_BN_FUSED_STATS=0.  dy = k1 g has the same bits on every route, so data and weight gradients are BITWISE equal; dgamma, dbeta
    and the conv-bias gradients see another summation order: within 1e-5 of the sum of the terms' magnitudes, the tolerance of
    tests/test_conv_x3_gpu.py's switch tests."""
    from wtpse_hip import nn as E
    from wtpse_hip import ops

    class Holder(E.HipNet):
        def __init__(self):
            super().__init__()
            self.d = E.ConvDBlock(32, 128)
            self.u = E.ConvUBlock(64)
            self._finish_init()

    h = Holder().to(DEV)
    fill_state_dict(h, 77)
    h.eval()
    h.ensure_ready(repack=True)
    B, S = 4, 32
    x, prev = make_noise(1, (B, 32, 2 * S, 2 * S)).to(DEV), make_noise(2, (B, 32, 2 * S, 2 * S)).to(DEV)
    dout = make_noise(3, (B, 64, 2 * S, 2 * S)).to(DEV)
    mags = {}
    plain = ops.bn_bwd_frozen

    def spy(dz, y, ss, relu, gamma, mean, invstd, dgamma, dbeta, dbias, accumulate=False):
        pre = y.double() * ss[:, 0].double().view(1, -1, 1, 1) + ss[:, 1].double().view(1, -1, 1, 1)
        g = (dz.double() * (pre > 0)) if relu else dz.double()
        s1 = g.abs().sum(dim=(0, 2, 3))
        s2 = (g * (y.double() - mean.double().view(1, -1, 1, 1))).abs().sum(dim=(0, 2, 3)) * invstd.double()
        mags[dbeta.data_ptr()], mags[dgamma.data_ptr()], mags[dbias.data_ptr()] = s1, s2, s1 * (gamma * invstd).double().abs()
        return plain(dz, y, ss, relu, gamma, mean, invstd, dgamma, dbeta, dbias, accumulate)

    def run(**switches):
        for k, v in switches.items():
            monkeypatch.setattr(E, k, v)
        with ops.fwd_scope(x.device):
            mid, td = E.convd_fwd(h.d, x, False)              # [B, 128, S, S]
            out, tu = E.convu_fwd(h.u, mid, prev, False)
            h.zero_grad()
            h.begin_backward()
            dmid, dprev = E.convu_bwd(h.u, tu, dout, below_x=td.c3)
            dx = E.convd_bwd(h.d, td, dmid, None, need_dx=True)
            h.end_backward()
        torch.cuda.synchronize()
        for k in switches:
            monkeypatch.undo()
        return {"dx": dx.clone(), "dprev": dprev.clone(), **{k: p.grad.clone() for k, p in h.named_parameters()}}

    base = run()
    assert all(float(base[k].abs().max()) > 0 for k in base), "a gradient is missing"
    monkeypatch.setattr(ops, "bn_bwd_frozen", spy)
    alone = run(BN_FUSED_STATS=False)
    monkeypatch.setattr(ops, "bn_bwd_frozen", plain)
    params = dict(h.named_parameters())
    sums = {k for k in params if ".bn" in k or (k.endswith(".bias") and ".conv" in k)}
    assert len(sums) == 6 * 3
    for name, other in (("WTPSE_BN_FUSED_STATS=0", alone), ("WTPSE_BN_TAIL=0", run(BN_TAIL=False)), ("WTPSE_BN_IN=0", run(BN_IN=False))):
        for k in base:
            if k not in sums:
                assert torch.equal(base[k], other[k]), "%s: %s differs (max |d| %g)" % (name, k, float((base[k] - other[k]).abs().max()))
                continue
            scale = mags[h.grange(params[k], params[k].numel()).data_ptr()]
            rel = float(((base[k].double() - other[k].double()).abs() / (scale + 1e-30)).max())
            assert rel < 1e-5, "%s: %s differs by %.3e of the sum of its terms' magnitudes" % (name, k, rel)


# ------------------------------------------------------------------------------------------------------------ step and run
B_STEP = 6
RATES = (5e-4, 4e-4, 3e-4, 2e-4)


def _setup(seed=1, noise=1234):
    import bench
    from wtpse_hip.synth import default_hparams
    dev = torch.device("cuda:0")
    hp = default_hparams(True)
    torch.manual_seed(0)
    nets = list(bench.build_nets(hp, B_STEP // 3, dev, seed=seed))
    for n in nets:                           # running statistics that are not the initial (0, 1)
        for name, b in n.named_buffers():
            if name.endswith("running_mean") or name.endswith("running_var"):
                b.copy_(torch.from_numpy(fill_value(name, b.shape, 9)).to(dev))
        n.invalidate_packed()
        if noise is not None:
            n.seed_noise(noise)
    return dev, hp, nets


def _batch(dev, seed):
    from wtpse_hip.synth import make_batch
    return make_batch(B_STEP, 64, 64, dev, seed=seed)


def _snapshot(ts, nets):
    torch.cuda.synchronize()
    opts = [ts.opt[id(n)] for n in nets]
    return dict(params=[n.flat_params().clone() for n in nets], bufs=[torch.cat([b.detach().reshape(-1).double() for b in n.buffers()]) for n in nets],
                m=[o.m.clone() for o in opts], v=[o.v.clone() for o in opts], t=[o.t for o in opts],
                ctr=[int(n._noise_ctr.item()) for n in nets])


def _assert_same(a, b):
    for k in ("params", "bufs", "m", "v"):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), "%s of network %d differs" % (k, i)
    assert a["t"] == b["t"] and a["ctr"] == b["ctr"]


def _is_prebn_bias(k):
    return (".conv" in "." + k and k.endswith(".bias")) or "inc.double_conv.0.bias" in k or "inc.double_conv.3.bias" in k


def test_train_step_frozen_eager_plan_graph_bitwise():
    """Three steps of TrainStep(freeze_bn=True): eager, launch plan and hipGraph end bitwise equal; no buffer moves; the conv biases
    in front of a BatchNorm train (they do not on batch statistics); a mode toggled after recording raises."""
    from wtpse_hip.step import TrainStep
    snaps = []
    for graph in (False, "plan", True):
        dev, hp, nets = _setup()
        ts = TrainStep(*nets, hp, lr=RATES, graph=graph, freeze_bn=True)
        assert not any(m.training for n in nets for m in n.modules())
        bufs0 = [torch.cat([b.detach().reshape(-1).double() for b in n.buffers()]) for n in nets]
        p0 = {k: p.detach().clone() for k, p in nets[0].named_parameters()}
        res = None
        for k in range(3):
            res = ts.step(*_batch(dev, 40 + k))
        snap = _snapshot(ts, nets)
        assert all(torch.equal(a, b) for a, b in zip(bufs0, snap["bufs"])), "a buffer moved under freeze_bn"
        assert all(math.isfinite(float(v)) for v in res.values())
        moved = [k for k, p in nets[0].named_parameters() if _is_prebn_bias(k) and not torch.equal(p, p0[k])]
        assert len(moved) == sum(1 for k in p0 if _is_prebn_bias(k)) > 40
        snaps.append(snap)
        nets[1].train()
        with pytest.raises(RuntimeError, match="freeze_bn"):
            ts.step(*_batch(dev, 50))
        nets[1].eval()
        ts.close()
    _assert_same(snaps[0], snaps[1])
    _assert_same(snaps[0], snaps[2])
    # and a step built for batch statistics refuses networks in eval mode
    dev, hp, nets = _setup()
    ts = TrainStep(*nets, hp, lr=RATES)
    nets[0].eval()
    with pytest.raises(RuntimeError, match="freeze_bn"):
        ts.step(*_batch(dev, 40))


def _next_batch(dev):
    def feed(py_rng, np_rng):
        return _batch(dev, int(np_rng.randint(1 << 20)))
    return feed


def test_train_run_frozen_resume_bitwise(tmp_path):
    """TrainRun(freeze_bn=True): two epochs run through against one epoch, checkpoint, TrainRun.load into new networks, one more
    epoch — bitwise equal; the flag travels in the checkpoint's config and train_epoch() keeps the networks in eval mode."""
    from wtpse_hip.trainer import TrainRun
    kw = dict(iter_per_epoch=3, max_epoch=2, lr=RATES, graph="plan", seed=7, freeze_bn=True)
    dev, hp, nets = _setup()
    a = TrainRun(*nets, hp, _next_batch(dev), out_dir=str(tmp_path / "a"), **kw)
    a.train_epoch()
    ea = a.train_epoch()
    sa = _snapshot(a.train_step, nets)
    assert not any(m.training for n in nets for m in n.modules())

    dev, hp, nets1 = _setup()
    b1 = TrainRun(*nets1, hp, _next_batch(dev), out_dir=str(tmp_path / "b"), **kw)
    b1.train_epoch()
    path = str(tmp_path / "b" / "run.pth.tar")
    b1.save(path)
    assert torch.load(path, map_location="cpu", weights_only=True)["config"]["freeze_bn"] is True
    del b1
    dev, hp, nets2 = _setup(seed=5, noise=None)
    for n in nets2:
        n.train()
    b2 = TrainRun.load(path, *nets2, hp, _next_batch(dev), out_dir=str(tmp_path / "b"))
    assert b2.freeze_bn and b2.train_step.freeze_bn and (b2.epoch, b2.iteration) == (1, 3)
    eb = b2.train_epoch()
    _assert_same(sa, _snapshot(b2.train_step, nets2))
    assert ea["sums"] == eb["sums"]


def test_dropin_adam_trajectory_equals_train_step():
    """The drop-in path in eval mode — update() -> torch loss glue -> backward() -> torch.optim.Adam on the parameter views — against
    TrainStep(freeze_bn=True) on the same weights, inputs and noise.
    Step 0, call A: the two differ only in the loss glue (torch's BCE autograd vs the fused kernel), so every gradient tensor agrees to
    the project's 1e-4 (relative L2), the pre-BatchNorm conv biases included.
    Three steps: Adam's first steps move a weight by ~lr sign(grad), so an entry whose gradient is at rounding level goes either
    way; the trajectory rule is tests/test_parity_gpu.py::_check_params_vs_golden's: median < 1e-3, 90 % within 2 lr iters + 5e-4."""
    from wtpse_hip.step import TrainStep
    lr, iters = 5e-4, 3
    dev, hp, nets_a = _setup()
    dev, hp, nets_b = _setup()
    noises = [make_noise(900 + k, (B_STEP, 1, 64, 64)).to(dev) for k in range(2 * iters)]
    ts = TrainStep(*nets_a, hp, lr=lr, freeze_bn=True)
    model, shape, model_oc, shape_oc = nets_b
    for n in nets_b:
        n.eval()
    opts = [torch.optim.Adam(n.parameters(), lr=lr, betas=(0.9, 0.99)) for n in nets_b]
    gi, gd = float(hp['instance_wt_gm']), float(hp['domain_wt_gm'])
    for k in range(iters):
        image, od, oc = _batch(dev, 60 + k)
        ts.step(image, od, oc, {"a": noises[2 * k], "c": noises[2 * k + 1]})
        grads_a = nets_a[0].flat_grads().clone()
        # the same iteration through the drop-in surface (Trainer.py:766-914)
        opts[0].zero_grad(); model.zero_grad()
        model.set_noise([noises[2 * k]])
        out, _, _, ins, dom = model.update(image, od, two_stage_inputs=image, sp_mask=od, two_step=True)
        (F.binary_cross_entropy(torch.sigmoid(out), od) + gi * ins + gd * dom).backward()
        if k == 0:
            off = 0
            for name, p in model.named_parameters():
                ga = grads_a[off:off + p.numel()].double()
                off += p.numel()
                assert p.grad is not None, name
                rel = float((p.grad.reshape(-1).double() - ga).norm() / (ga.norm() + 1e-30))
                assert rel <= TOL, "%s: drop-in and TrainStep gradients differ by %.3e" % (name, rel)
        opts[0].step()
        opts[1].zero_grad(); shape.zero_grad()
        kd, ins_t, _, _, dom_s = shape.update(model, image, od, two_stage_inputs=image, two_step=True)
        (kd + gi * ins_t + gd * dom_s).backward(); opts[1].step()
        od_pred = (torch.sigmoid(out) > 0.75).float().detach()
        roi = (image + 1) * od_pred - 1
        opts[2].zero_grad(); model_oc.zero_grad()
        model_oc.set_noise([noises[2 * k + 1]])
        out_oc, _, _, ins_c, dom_c = model_oc.update(roi, oc, two_stage_inputs=roi, two_step=True)
        pw = torch.sum(od_pred) / torch.sum(od_pred * oc)
        if torch.isinf(pw) or torch.isnan(pw):
            pw = torch.tensor(1.).to(dev)
        (F.binary_cross_entropy_with_logits(out_oc * od_pred, oc, pos_weight=pw) + gi * ins_c + gd * dom_c).backward(); opts[2].step()
        opts[3].zero_grad(); shape_oc.zero_grad()
        kd2, ins_t2, _, _, dom_s2 = shape_oc.update(model_oc, roi, oc, two_stage_inputs=roi, two_step=True)
        (kd2 + gi * ins_t2 + gd * dom_s2).backward(); opts[3].step()
    torch.cuda.synchronize()
    pooled, pooled_bias = [], []
    for na, nb in zip(nets_a, nets_b):
        for (k, pa), (_, pb_) in zip(na.named_parameters(), nb.named_parameters()):
            d = (pa.detach() - pb_.detach()).abs().reshape(-1).cpu().numpy()
            (pooled_bias if _is_prebn_bias(k) else pooled).append(d)
        for (k, ba), (_, bb) in zip(na.named_buffers(), nb.named_buffers()):
            assert torch.equal(ba, bb), k
    for what, v in (("all other parameters", np.concatenate(pooled)), ("pre-BatchNorm conv biases", np.concatenate(pooled_bias))):
        print(f"[drop-in vs TrainStep, {what}] median |d| {np.median(v):.3e}, within 2 lr iters + 5e-4: {(v < 2 * lr * iters + 5e-4).mean():.4f}")
        assert np.median(v) < 1e-3 and (v < 2 * lr * iters + 5e-4).mean() >= 0.9
