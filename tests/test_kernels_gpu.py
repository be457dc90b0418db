"""Kernel-level parity (-m gpu): every C-ABI entry point against stock PyTorch fp32 ops on the host CPU,
on seeded inputs at sizes the CPU finishes in seconds — including ragged tiles, 1-/3-/8-channel layers, the
16x16 and 8x32 tile shapes, virtual concat, fused prologue/epilogue and all three MFMA modes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from wtpse_hip import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def close(a, b, rtol=1e-4, atol=1e-5, what=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    # 2e-6 of the tensor's scale: an fp32 sum of ~1e3 terms that cancels to ~0 carries that much rounding noise, and the
    # 16- and 32-wide MFMA paths (chosen by grid size) add the terms in different orders
    tol = atol + rtol * b.abs() + 2e-6 * float(b.abs().max())
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} at {int(err.argmax())}, ref scale {b.abs().max():.3e}"


def pack(w):
    """OIHW -> (packed buffer, wf_off, wd_off) through wtpse_pack_conv_weights."""
    o = ops()
    co, ci, k, _ = w.shape
    t = k * k
    wf = ((ci + 3) & ~3) * t * ((co + 15) & ~15)
    wd = ((co + 3) & ~3) * t * ((ci + 15) & ~15)
    flat = w.reshape(-1).contiguous().to(DEV)
    packed = torch.full((wf + wd,), float("nan"), device=DEV)
    desc = torch.tensor([0, co, ci, t, 0, wf, 0, 0], dtype=torch.int32, device=DEV)
    o.lib().call("wtpse_pack_conv_weights", flat.data_ptr(), desc.data_ptr(), 1, packed.data_ptr(), o.stream_ptr())
    return packed, 0, wf


CONV_CASES = [
    # B, C0, C1, Cout, H, W, k
    (2, 16, 0, 16, 16, 32, 3),     # MODE 0, one full 8x32 tile per 8 rows
    (2, 3, 0, 16, 20, 40, 3),      # 3-channel input, ragged tiles
    (1, 1, 0, 16, 9, 33, 3),       # 1-channel input
    (2, 16, 0, 32, 16, 16, 3),     # MODE 1, 16x16 tile
    (2, 32, 0, 64, 8, 8, 3),       # MODE 2, image smaller than a tile
    (1, 64, 64, 128, 16, 16, 3),   # concat, two cout blocks
    (2, 16, 16, 32, 24, 48, 3),    # concat at MODE 1, ragged
    (3, 32, 0, 16, 17, 35, 1),     # 1x1, MODE 0
    (2, 256, 0, 128, 4, 4, 1),     # 1x1, MODE 2, multi-chunk
    (2, 32, 0, 8, 16, 32, 1),      # head: Cout = 8
    (2, 8, 0, 1, 16, 32, 1),       # head: Cout = 1
    (1, 128, 0, 256, 2, 2, 3),     # deepest level of the 32x32 test network
    (2, 40, 0, 96, 12, 20, 3),     # non-power-of-two channels (MODE 1, 3 cout blocks)
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_forward(case):
    o = ops()
    B, C0, C1, Co, H, W, k = case
    x0 = rnd(B, C0, H, W, seed=1)
    x1 = rnd(B, C1, H, W, seed=2) if C1 else None
    w = rnd(Co, C0 + C1, k, k, seed=3, scale=0.2)
    b = rnd(Co, seed=4)
    ref = F.conv2d(torch.cat([x0, x1], 1) if C1 else x0, w, b, padding=k // 2)
    packed, wf, _ = pack(w)
    y, _, stats = o.conv_fwd(x0.to(DEV), x1.to(DEV) if C1 else None, packed.data_ptr() + 4 * wf, b.to(DEV), Co, k,
                             want_stats=True)
    close(y, ref, what="conv")
    s = stats.double().sum(0).cpu()
    close(s[:, 0], ref.double().sum((0, 2, 3)), rtol=1e-4, atol=1e-3, what="stat sum")
    close(s[:, 1], (ref.double() ** 2).sum((0, 2, 3)), rtol=1e-4, atol=1e-3, what="stat sumsq")
    yr, _, _ = o.conv_fwd(x0.to(DEV), x1.to(DEV) if C1 else None, packed.data_ptr() + 4 * wf, None, Co, k, relu_out=True)
    close(yr, F.relu(ref - b.view(1, -1, 1, 1)), what="conv relu nobias")


@pytest.mark.parametrize("case", [(2, 16, 16, 32, 16, 32, 3), (2, 16, 0, 16, 16, 32, 3), (1, 32, 32, 64, 8, 16, 1)])
def test_conv_prologue(case):
    """BatchNorm-apply + ReLU fused into the loader; zero padding applies after the activation."""
    o = ops()
    B, C0, C1, Co, H, W, k = case
    x0 = rnd(B, C0, H, W, seed=5)
    x1 = rnd(B, C1, H, W, seed=6) if C1 else None
    pro = torch.stack([rnd(C0 + C1, seed=7) * 0.5 + 1.0, rnd(C0 + C1, seed=8)], 1).contiguous()
    w = rnd(Co, C0 + C1, k, k, seed=9, scale=0.2)
    xin = torch.cat([x0, x1], 1) if C1 else x0
    act = xin * pro[:, 0].view(1, -1, 1, 1) + pro[:, 1].view(1, -1, 1, 1)
    act = torch.cat([F.relu(act[:, :C0]), act[:, C0:]], 1)      # ReLU on in0 only (bit 0)
    ref = F.conv2d(act, w, None, padding=k // 2)
    packed, wf, _ = pack(w)
    y, _, _ = o.conv_fwd(x0.to(DEV), x1.to(DEV) if C1 else None, packed.data_ptr() + 4 * wf, None, Co, k,
                         pro0=pro[:C0].contiguous().to(DEV), pro1=(pro[C0:].contiguous().to(DEV) if C1 else None), pro_relu=1)
    close(y, ref, what="prologue")


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_dgrad_wgrad(case):
    o = ops()
    B, C0, C1, Co, H, W, k = case
    x0 = rnd(B, C0, H, W, seed=11).requires_grad_(True)
    x1 = rnd(B, C1, H, W, seed=12).requires_grad_(True) if C1 else None
    w = rnd(Co, C0 + C1, k, k, seed=13, scale=0.2).requires_grad_(True)
    b = rnd(Co, seed=14).requires_grad_(True)
    dy = rnd(B, Co, H, W, seed=15)
    y = F.conv2d(torch.cat([x0, x1], 1) if C1 else x0, w, b, padding=k // 2)
    y.backward(dy)
    packed, _, wd = pack(w.detach())
    if C0 + C1 > 4:   # the data gradient of the 1-/3-channel input layers is never needed
        d0, d1, _ = o.conv_fwd(dy.to(DEV), None, packed.data_ptr() + 4 * wd, None, C0 + C1, k, split=(C0 if C1 else None))
        close(d0, x0.grad, what="dgrad0")
        if C1:
            close(d1, x1.grad, what="dgrad1")
    dw = torch.full_like(w, float("nan")).to(DEV)
    db = torch.full_like(b, float("nan")).to(DEV)
    o.conv_wgrad(dy.to(DEV), x0.detach().to(DEV), x1.detach().to(DEV) if C1 else None, k, dw, db)
    scale = float(w.grad.abs().max())
    close(dw, w.grad, rtol=2e-4, atol=2e-5 * max(scale, 1.0), what="wgrad")
    close(db, b.grad, rtol=2e-4, atol=1e-4, what="bgrad")
    o.conv_wgrad(dy.to(DEV), x0.detach().to(DEV), x1.detach().to(DEV) if C1 else None, k, dw, None, accumulate=True)
    close(dw, 2 * w.grad, rtol=2e-4, atol=4e-5 * max(scale, 1.0), what="wgrad accumulate")


@pytest.mark.parametrize("case", [(2, 32, 8, 16, 32, 1), (2, 8, 32, 17, 35, 1), (2, 16, 16, 20, 40, 3), (1, 64, 40, 8, 8, 3),
                                  (2, 32, 128, 4, 4, 1)])
def test_conv_dgrad_relu_mask(case):
    """mask_ref: the ReLU backward of the tensor the data gradient flows into rides in the epilogue (heads, DeepWT)."""
    o = ops()
    B, Co, Ci, H, W, k = case            # forward conv Ci -> Co; the data gradient has Ci output channels
    w = rnd(Co, Ci, k, k, seed=21, scale=0.2)
    dy = rnd(B, Co, H, W, seed=22)
    ref_act = rnd(B, Ci, H, W, seed=23)  # the (pre- or post-ReLU) activation whose sign gates the gradient
    ref_act[0, 0, 0, :4] = 0.0           # exactly zero counts as "not positive"
    want = F.conv_transpose2d(dy, w, padding=k // 2) * (ref_act > 0).float()
    packed, _, wd = pack(w)
    d0, _, _ = o.conv_fwd(dy.to(DEV), None, packed.data_ptr() + 4 * wd, None, Ci, k, mask_ref=ref_act.to(DEV))
    close(d0, want, what="masked dgrad")


@pytest.mark.parametrize("shape,relu", [((4, 16, 16, 32), True), ((3, 32, 9, 7), False), ((2, 64, 4, 4), True),
                                        ((4, 128, 8, 8), True), ((2, 256, 16, 16), False), ((32, 96, 32, 32), False)])   # last three: one-launch backward
def test_batchnorm_train(shape, relu):
    o = ops()
    B, C, H, W = shape
    xin = rnd(B, 8, H, W, seed=21)
    w = rnd(C, 8, 3, 3, seed=22, scale=0.3)
    bias = rnd(C, seed=23)
    gamma = (rnd(C, seed=24) * 0.2 + 1).requires_grad_(True)
    beta = (rnd(C, seed=25) * 0.2).requires_grad_(True)
    rm, rv = rnd(C, seed=26) * 0.1, rnd(C, seed=27).abs() + 0.5
    yref = F.conv2d(xin, w, bias, padding=1).requires_grad_(True)
    rm_ref, rv_ref = rm.clone(), rv.clone()
    zref = F.batch_norm(yref, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5)
    on_kink = zref.detach().abs() < 2e-6 if relu else torch.zeros_like(zref, dtype=torch.bool)
    if relu:
        zref = F.relu(zref)
    dz = rnd(*shape, seed=28)
    zref.backward(dz)
    packed, wf, _ = pack(w)
    y, _, stats = o.conv_fwd(xin.to(DEV), None, packed.data_ptr() + 4 * wf, bias.to(DEV), C, 3, want_stats=True)
    rm_d, rv_d = rm.to(DEV), rv.to(DEV)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    g_d, b_d = gamma.detach().to(DEV), beta.detach().to(DEV)
    ss, mean, invstd = o.bn_finalize(stats, B * H * W, g_d, b_d, rm_d, rv_d, nbt)
    z = o.affine_act(y, ss, relu)
    close(z, zref, what="bn fwd")
    close(rm_d, rm_ref, what="running_mean")
    close(rv_d, rv_ref, what="running_var")
    assert int(nbt.item()) == 1
    dg, dbt = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dy = o.bn_bwd(dz.to(DEV), y, ss, relu, g_d, mean, invstd, dg, dbt)
    # an output within rounding of the ReLU kink may take the other branch (the fused scale/shift rounds differently from
    # ATen's normalisation): its own gradient entry is skipped, at most a handful per million
    assert int(on_kink.sum()) <= max(2, on_kink.numel() // 100000)      # |z| < 2e-6 on unit-scale z: ~4 per million
    close(torch.where(on_kink.to(DEV), torch.zeros_like(dy), dy), torch.where(on_kink, torch.zeros_like(dy.cpu()), yref.grad),
          rtol=2e-4, atol=2e-5, what="bn dy")
    close(dg, gamma.grad, rtol=2e-4, atol=2e-4, what="dgamma")
    close(dbt, beta.grad, rtol=2e-4, atol=2e-4, what="dbeta")
    ss_e = o.bn_eval_coeffs(g_d, b_d, rm_d, rv_d)
    close(o.affine_act(y, ss_e, False), F.batch_norm(yref.detach(), rm_ref, rv_ref, gamma.detach(), beta.detach(), False, 0.1, 1e-5),
          what="bn eval")


@pytest.mark.parametrize("offset,amp", [(-1.0, 1e-1), (-1.0, 1e-3), (-1.0, 0.0), (10.0, 1e-2)])
def test_batchnorm_train_offset_input(offset, amp):
    """Train-mode statistics are folded from per-tile (sum, sum of squares) partials that the conv epilogue rounds to fp32; the
    variance E[y^2] - mean^2 loses digits when |mean| >> std.  The inputs that could do that here are the near-constant ones —
    the all -1 ROI image of an empty disc prediction (Trainer.py:842-853), offset images — but a zero-padded 3x3 conv of a
    constant map has borders: |mean| / std of its output stays near 5, and the normalised output stays within 5e-5 of the fp64
    result (tools/probe/bn_offset.py prints the table): 1-2e-6 as soon as the input carries any noise, 0.9-2.5e-5 for an EXACTLY
    constant input — every interior tile then holds the same values and rounds its 256-element sums the same way, so the
    partials' fp32 rounding (~1e-6 of E[y^2]) does not average out over the tiles and is multiplied by mean^2/var = 28.  Stock
    fp32 BatchNorm on the host: 1e-6.  Inside the path's 1e-4; the fix if it ever matters is a per-channel pivot (the previous
    step's batch mean) subtracted before the epilogue accumulates."""
    o = ops()
    B, C, H, W = 8, 32, 64, 64
    xin = offset + amp * rnd(B, 16, H, W, seed=41)
    w = rnd(C, 16, 3, 3, seed=42, scale=0.3)
    bias = rnd(C, seed=43)
    y64 = F.conv2d(xin.double(), w.double(), bias.double(), padding=1)
    z64 = F.batch_norm(y64, None, None, torch.ones(C).double(), torch.zeros(C).double(), True, 0.1, 1e-5)
    packed, wf, _ = pack(w)
    y, _, stats = o.conv_fwd(xin.to(DEV), None, packed.data_ptr() + 4 * wf, bias.to(DEV), C, 3, want_stats=True)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    ss, mean, invstd = o.bn_finalize(stats, B * H * W, torch.ones(C, device=DEV), torch.zeros(C, device=DEV),
                                     torch.zeros(C, device=DEV), torch.ones(C, device=DEV), nbt)
    z = o.affine_act(y, ss, False).cpu().double()
    err = float((z - z64).abs().max() / z64.abs().max())
    assert err <= (5e-5 if amp == 0.0 else 1e-5), err
    close(mean, y64.mean((0, 2, 3)).float(), rtol=1e-5, atol=1e-6, what="batch mean")


@pytest.mark.parametrize("shape", [(2, 5, 8, 12), (1, 3, 7, 9), (2, 16, 32, 32)])
def test_pool_and_upsample(shape):
    o = ops()
    x = rnd(*shape, seed=31).requires_grad_(True)
    p = F.max_pool2d(F.relu(x), 2)
    dp = rnd(*p.shape, seed=32)
    p.backward(dp)
    xd = x.detach().to(DEV)
    close(o.maxpool2_fwd(xd, None, True), p, what="pool fwd")
    # gradient wrt relu(x) (the tensor as loaded); the ReLU mask is the producer's job
    xr = F.relu(x.detach()).requires_grad_(True)
    F.max_pool2d(xr, 2).backward(dp)
    close(o.maxpool2_bwd(xd, dp.to(DEV), None, False, None, True), xr.grad, what="pool bwd")
    acc = rnd(*shape, seed=33)
    close(o.maxpool2_bwd(xd, dp.to(DEV), acc.clone().to(DEV), True, None, True), xr.grad + acc, what="pool bwd acc")
    # ... with the backward of the ReLU that produced the tensor fused in: (acc + pooled gradient) * [relu(x) > 0]
    live = (F.relu(x.detach()) > 0).float()
    close(o.maxpool2_bwd(xd, dp.to(DEV), acc.clone().to(DEV), True, None, True, mask=True), (xr.grad + acc) * live, what="pool bwd acc mask")
    close(o.maxpool2_bwd(xd, dp.to(DEV), None, False, None, True, mask=True), xr.grad * live, what="pool bwd mask")
    ref = rnd(*shape, seed=36)
    close(o.relu_mask(acc.to(DEV), ref.to(DEV)), acc * (ref > 0), what="relu mask")
    dst = acc.clone().to(DEV)
    o.axpy(dst, ref.to(DEV), 0.5)
    close(dst, acc + 0.5 * ref, what="axpy")
    x2 = rnd(*shape, seed=34).requires_grad_(True)
    u = F.interpolate(x2, scale_factor=2, mode="bilinear", align_corners=False)
    du = rnd(*u.shape, seed=35)
    u.backward(du)
    close(o.upsample2x_fwd(x2.detach().to(DEV)), u, what="up fwd")
    if shape[3] % 2 == 0:   # the BatchNorm-statistics variant (conv2 moved in front of the upsampling)
        uo, st = o.upsample2x_fwd_stats(x2.detach().to(DEV))
        close(uo, u, what="up fwd (stats variant)")
        tot = st.double().sum(0).cpu()
        close(tot[:, 0], u.detach().double().sum((0, 2, 3)), rtol=1e-5, atol=1e-3, what="up stat sum")
        close(tot[:, 1], (u.detach().double() ** 2).sum((0, 2, 3)), rtol=1e-5, atol=1e-3, what="up stat sumsq")
    close(o.upsample2x_bwd(du.to(DEV)), x2.grad, rtol=1e-4, atol=1e-5, what="up bwd")


def test_wt_loss_against_oracle_and_golden(golden_dir):
    """a-4 / a-5: forward triple and dL/dz against the CPU oracle and the reference-generated fixtures."""
    import os
    from oracle import wtpse_cpu as O
    from oracle.inputs import make_feature
    o = ops()
    g = np.load(os.path.join(golden_dir, "wtloss.npz"))
    for ci, (B, pb, H, white, margin, seed) in enumerate(g["cases"]):
        B, pb, H, seed = int(B), int(pb), int(H), int(seed)
        z = make_feature(seed, (B, 16, H, H), bool(white))
        zr = z.clone().requires_grad_(True)
        off, dg, dom = O.whitening_loss(zr, 3, pb, float(margin))
        (off + dg + dom).backward()
        st = o.wt_loss_fwd(z.to(DEV), 3, pb, float(margin))
        l = st.losses.cpu()
        p = f"c{ci}_"
        for got, ref, key in ((l[0], off, "off"), (l[1], dg, "diag")):
            close(got, ref.detach(), rtol=1e-5, atol=1e-7, what=p + key)
            assert abs(float(got) - float(g[p + key])) <= 1e-6 + 1e-5 * abs(float(g[p + key]))
        assert abs(float(l[2]) - float(g[p + "dom"])) <= 3e-7 + 1e-3 * abs(float(g[p + "dom"])), (float(l[2]), float(g[p + "dom"]))
        close(st.gram.view(B, 16, 16), torch.from_numpy(g[p + "gram"]), rtol=1e-5, atol=1e-6, what=p + "gram")
        close(st.v, torch.from_numpy(g[p + "v"]), rtol=1e-5, atol=1e-6, what=p + "v")
        dz = torch.zeros_like(z).to(DEV)
        o.wt_loss_bwd(st, dz, False)
        # |G_ij| and |G_ii - 1| have kinks at 0: for near-white features an entry can sit within rounding of the
        # kink, where the sign (hence the gradient) is decided by the last bit of the Gram.  Compare gradients only
        # when both Grams agree on every sign; otherwise require that each disagreement is within rounding of the kink.
        Gd = st.gram.view(B, 16, 16).cpu().double()
        Gr = torch.from_numpy(g[p + "gram"]).double()
        eye = torch.eye(16, dtype=torch.float64)
        kd, kr = Gd - eye * (Gd.diagonal(dim1=1, dim2=2).unsqueeze(-1) * 0 + 1), Gr - eye
        flips = torch.sign(kd) != torch.sign(kr)
        if flips.any():
            assert float(kr[flips].abs().max()) < 5e-6, "sign flip away from the kink"
            continue
        close(dz, zr.grad, rtol=2e-3, atol=1e-8 + 2e-4 * float(zr.grad.abs().max()), what=p + "dz")
        if H <= 8:
            close(dz, torch.from_numpy(g[p + "dz"]), rtol=2e-3, atol=1e-8 + 2e-4 * float(zr.grad.abs().max()), what=p + "dz golden")
        # accumulate + device-scalar upstream gradients + host weights
        base = rnd(*z.shape, seed=40)
        dz2 = base.clone().to(DEV)
        two = torch.tensor(2.0, device=DEV)
        o.wt_loss_bwd(st, dz2, True, g_off=two, g_diag=two, g_dom=two, w_off=0.5, w_diag=0.5, w_dom=0.5)
        close(dz2, base + zr.grad, rtol=2e-3, atol=1e-6 + 2e-4 * float(zr.grad.abs().max()), what=p + "dz acc")
        # accumulate & 2: the incoming gradient is wrt relu(z) and is masked with [z > 0] inside the same pass
        dz3 = base.clone().to(DEV)
        o.wt_loss_bwd(st, dz3, 3, g_off=two, g_diag=two, g_dom=two, w_off=0.5, w_diag=0.5, w_dom=0.5)
        close(dz3, base * (z > 0) + zr.grad, rtol=2e-3, atol=1e-6 + 2e-4 * float(zr.grad.abs().max()), what=p + "dz mask-in")


def test_wt_loss_unaligned_hw():
    from oracle import wtpse_cpu as O
    o = ops()
    z = rnd(3, 16, 5, 7, seed=41)
    off, dg, dom = O.whitening_loss(z, 3, 1, 0.0)
    st = o.wt_loss_fwd(z.to(DEV), 3, 1, 0.0)
    close(st.losses[:2], torch.stack([off, dg]), rtol=1e-5, atol=1e-7)
    # the domain loss, at the golden test's tolerance for `dom` (fp64 oracle: the value is a difference of O(1) kernel means)
    dom = O.whitening_loss(z.double(), 3, 1, 0.0)[2]
    assert abs(float(st.losses[2]) - float(dom)) <= 3e-7 + 1e-3 * abs(float(dom)), (float(st.losses[2]), float(dom))


@pytest.mark.parametrize("case", [(2, 8, 8, 1, True), (3, 16, 32, 1, False), (1, 4, 8, 3, True), (2, 16, 16, 0, True), (1, 8, 4, 0, False),
                                  (6, 64, 64, 1, True)])
def test_fused_head(case):
    """csrc/head.hip: the 1x1 heads as one kernel per direction against three (two) torch convolutions."""
    o = ops()
    B, H, W, nc, use_pro = case
    three = nc > 0
    x = rnd(B, 32, H, W, seed=61)
    pro = torch.stack([rnd(32, seed=62) * 0.5 + 1.0, rnd(32, seed=63) * 0.3], 1).contiguous() if use_pro else None
    w1 = rnd(32, 32, 1, 1, seed=64, scale=0.3).requires_grad_(True); b1 = rnd(32, seed=65, scale=0.2).requires_grad_(True)
    w2 = rnd(8, 32, 1, 1, seed=66, scale=0.3).requires_grad_(True); b2 = rnd(8, seed=67, scale=0.2).requires_grad_(True)
    w3 = rnd(nc, 8, 1, 1, seed=68, scale=0.5).requires_grad_(True) if three else None
    b3 = rnd(nc, seed=69, scale=0.2).requires_grad_(True) if three else None
    xa = (F.relu(x * pro[:, 0].view(1, -1, 1, 1) + pro[:, 1].view(1, -1, 1, 1)) if use_pro else x.clone()).requires_grad_(True)
    h1 = F.relu(F.conv2d(xa, w1, b1))
    h2 = F.conv2d(h1, w2, b2)
    out = F.conv2d(F.relu(h2), w3, b3) if three else h2
    dy = rnd(*out.shape, seed=70)
    out.backward(dy)
    D = lambda t: t.detach().to(DEV).contiguous() if t is not None else None
    got, h1d, h2d = o.head_fwd(D(x), D(pro), use_pro, D(w1), D(b1), D(w2), D(b2), D(w3), D(b3), True, want_h1=True)
    close(got, out, what="head out")
    close(h1d, h1, what="h1")
    close(h2d, F.relu(h2) if three else h2, what="h2")
    got2, none1, h2n = o.head_fwd(D(x), D(pro), use_pro, D(w1), D(b1), D(w2), D(b2), D(w3), D(b3), False)
    assert none1 is None and (h2n is None) == three
    assert torch.equal(got2, got)
    ns = 1320 + 9 * nc
    dpar = torch.full((ns,), float("nan"), device=DEV)
    dx = o.head_bwd(D(dy), D(x), D(pro), use_pro, h1d, h2d, D(w1), D(w2), D(w3), dpar, b1=D(b1))
    close(dx, xa.grad, what="dx")
    want = torch.cat([t.grad.reshape(-1) for t in (w1, b1, w2, b2) + ((w3, b3) if three else ())])
    scale = float(want.abs().max())
    close(dpar, want, rtol=2e-4, atol=2e-5 * max(scale, 1.0), what="head dparams")
    o.head_bwd(D(dy), D(x), D(pro), use_pro, h1d, h2d, D(w1), D(w2), D(w3), dpar, accumulate=True, b1=D(b1))
    close(dpar, 2 * want, rtol=2e-4, atol=4e-5 * max(scale, 1.0), what="head dparams accumulate")
    if o.x3_terms() == 2:
        # what the training step runs: no layer-1 tape (the backward forms h1 again), scales from the operands' amax tables
        xd = D(x)
        xam = o.amax_of(xd) if not use_pro else o.act_bound(D(pro), o.amax_of(xd))
        got3, none3, h2t = o.head_fwd(xd, D(pro), use_pro, D(w1), D(b1), D(w2), D(b2), D(w3), D(b3), True, x_amax=xam)
        assert none3 is None
        close(got3, out, what="head out (amax table)")
        dpar3 = torch.full((ns,), float("nan"), device=DEV)
        dx3 = o.head_bwd(D(dy), xd, D(pro), use_pro, None, h2t, D(w1), D(w2), D(w3), dpar3, b1=D(b1), x_amax=xam)
        close(dx3, xa.grad, what="dx (no tape, amax tables)")
        close(dpar3, want, rtol=2e-4, atol=2e-5 * max(scale, 1.0), what="head dparams (no tape, amax tables)")
        with pytest.raises(ValueError):
            o.head_bwd(D(dy), xd, D(pro), use_pro, None, h2t, D(w1), D(w2), D(w3), dpar3)


def test_fused_head_backward_is_repeatable():
    """Two runs of the head backward on the same operands give the same bits.  (Round 6's first x2h backward split its operands with
    inline assembly right next to matrix instructions — the compiler's hazard recogniser does not look inside — and its gradients moved
    by a remainder term's size from run to run; every accuracy test of the time passed at 1e-4.)"""
    o = ops()
    B, H, W, nc = 4, 64, 64, 1
    x = rnd(B, 32, H, W, seed=101).to(DEV)
    pro = torch.stack([rnd(32, seed=102) * 0.5 + 1.0, rnd(32, seed=103) * 0.3], 1).contiguous().to(DEV)
    w1, b1 = rnd(32, 32, 1, 1, seed=104, scale=0.3).to(DEV), rnd(32, seed=105, scale=0.2).to(DEV)
    w2, b2 = rnd(8, 32, 1, 1, seed=106, scale=0.3).to(DEV), rnd(8, seed=107, scale=0.2).to(DEV)
    w3, b3 = rnd(nc, 8, 1, 1, seed=108, scale=0.5).to(DEV), rnd(nc, seed=109, scale=0.2).to(DEV)
    dy = rnd(B, nc, H, W, seed=110).to(DEV)
    y, h1, h2 = o.head_fwd(x, pro, True, w1, b1, w2, b2, w3, b3, True, want_h1=True)
    ns = 1320 + 9 * nc
    outs = []
    for _ in range(3):
        dpar = torch.full((ns,), float("nan"), device=DEV)
        dx = o.head_bwd(dy, x, pro, True, h1, h2, w1, w2, w3, dpar, b1=b1)
        outs.append((dx.clone(), dpar.clone()))
    for dx, dpar in outs[1:]:
        assert torch.equal(dx, outs[0][0]) and torch.equal(dpar, outs[0][1])
    y2, _, h2b = o.head_fwd(x, pro, True, w1, b1, w2, b2, w3, b3, True, want_h1=True)
    assert torch.equal(y2, y) and torch.equal(h2b, h2)


def test_fused_head_keeps_a_nan_input_visible():
    """x2h heads: a NaN in the head's input reaches the output at its pixel as NaN (the inner ReLUs keep it, as torch.relu does), so the
    reference's isnan scrub of mu (shape_networks.py:490) still sees a diverged feature map; every other pixel stays finite."""
    o = ops()
    if o.x3_terms() != 2:
        pytest.skip("x2h arithmetic only")
    B, H, W = 2, 8, 8
    x = rnd(B, 32, H, W, seed=91)
    x[1, 5, 3, 4] = float("nan")
    D = lambda t: t.detach().to(DEV).contiguous()
    w1, b1 = rnd(32, 32, 1, 1, seed=92, scale=0.3), rnd(32, seed=93, scale=0.2)
    w2, b2 = rnd(8, 32, 1, 1, seed=94, scale=0.3), rnd(8, seed=95, scale=0.2)
    w3, b3 = rnd(1, 8, 1, 1, seed=96, scale=0.5), rnd(1, seed=97, scale=0.2)
    y, _, h2 = o.head_fwd(D(x), None, False, D(w1), D(b1), D(w2), D(b2), D(w3), D(b3), True)
    bad = torch.isnan(y.cpu())
    assert bool(bad[1, 0, 3, 4]) and int(bad.sum()) == 1
    assert bool(torch.isnan(h2.cpu())[1, :, 3, 4].all())
    y2, _, _ = o.head_fwd(D(x), None, False, D(w1), D(b1), D(w2), D(b2), None, None, True)
    bad2 = torch.isnan(y2.cpu())
    assert bool(bad2[1, :, 3, 4].all()) and int(bad2.sum()) == 8


@pytest.mark.parametrize("xs,gs", [(1e-4, 1e3), (300.0, 1e-5), (1.0, 1.0)])
def test_fused_head_scales_follow_the_data(xs, gs):
    """x2h heads: operands far from unit scale (inputs, weights, gradients) keep fp32-level accuracy — every operand is scaled by a
    bound of its own tensor (amax tables, absolute row sums of the weights), not by a fixed constant."""
    o = ops()
    if o.x3_terms() != 2:
        pytest.skip("x2h arithmetic only")
    B, H, W, nc = 2, 16, 32, 1
    x = (rnd(B, 32, H, W, seed=81) * xs).double()
    w1 = (rnd(32, 32, 1, 1, seed=82, scale=0.3) / xs * 3.0).double().requires_grad_(True); b1 = rnd(32, seed=83, scale=0.2).double().requires_grad_(True)
    w2 = rnd(8, 32, 1, 1, seed=84, scale=0.3).double().requires_grad_(True); b2 = rnd(8, seed=85, scale=0.2).double().requires_grad_(True)
    w3 = rnd(nc, 8, 1, 1, seed=86, scale=0.5).double().requires_grad_(True); b3 = rnd(nc, seed=87, scale=0.2).double().requires_grad_(True)
    xa = x.clone().requires_grad_(True)
    h2 = F.conv2d(F.relu(F.conv2d(xa, w1, b1)), w2, b2)
    out = F.conv2d(F.relu(h2), w3, b3)
    dy = (rnd(*out.shape, seed=88) * gs).double()
    out.backward(dy)
    D = lambda t: t.detach().float().to(DEV).contiguous()
    xd = D(x)
    xam = o.amax_of(xd)
    got, _, h2t = o.head_fwd(xd, None, False, D(w1), D(b1), D(w2), D(b2), D(w3), D(b3), True, x_amax=xam)
    rel = lambda g, w: float((g.double().cpu() - w).norm() / w.norm())
    assert rel(got, out.detach()) < 2e-6
    ns = 1320 + 9 * nc
    dpar = torch.full((ns,), float("nan"), device=DEV)
    dx = o.head_bwd(D(dy), xd, None, False, None, h2t, D(w1), D(w2), D(w3), dpar, b1=D(b1), x_amax=xam)
    assert rel(dx, xa.grad) < 2e-6
    off = 0
    for t in (w1, b1, w2, b2, w3, b3):
        k = t.numel()
        assert rel(dpar[off:off + k], t.grad.reshape(-1)) < 5e-6, t.shape
        off += k


@pytest.mark.parametrize("shape", [(3, 8, 9, 11), (5, 2, 256, 256)])   # the second takes the many-row reduction of (dw, db)
def test_attention_fuse_and_sampling(shape):
    o = ops()
    B, CE, H, W = shape
    z = rnd(B, 1, H, W, seed=51).requires_grad_(True)
    emb = rnd(B, CE, H, W, seed=52).requires_grad_(True)
    wb = torch.tensor([0.7, -0.2], requires_grad=True)
    pre = z * wb[0] + wb[1]
    att = torch.sigmoid(pre)
    fuse = 0.3 * emb + att * emb
    dfuse = rnd(B, CE, H, W, seed=53)
    fuse.backward(dfuse)
    wb_d = wb.detach().to(DEV)
    a, p, m, f = o.attn_fuse_fwd(z.detach().to(DEV), wb_d.data_ptr(), emb.detach().to(DEV), 0.3, True, True, True)
    close(a, att, what="att"); close(p, pre, what="pre"); close(f, fuse, what="fuse")
    assert torch.equal(m.cpu(), (att > 0.75).float())
    dwb = torch.zeros(2, device=DEV)
    demb, dz = o.attn_fuse_bwd(dfuse.to(DEV), z.detach().to(DEV), emb.detach().to(DEV), a, wb_d.data_ptr(), 0.3, dwb.data_ptr(), True)
    close(demb, emb.grad, what="demb"); close(dz, z.grad, what="dz"); close(dwb, wb.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(wb.grad.abs().max())), what="dwb")
    mu, lv, eps = rnd(B, 1, H, W, seed=54).requires_grad_(True), rnd(B, 1, H, W, seed=55).requires_grad_(True), rnd(B, 1, H, W, seed=56)
    zz = mu + torch.exp(lv / 2) * eps
    g = rnd(B, 1, H, W, seed=57)
    zz.backward(g)
    close(o.reparam_fwd(mu.detach().to(DEV), lv.detach().to(DEV), eps.to(DEV)), zz, what="reparam")
    close(o.reparam_bwd(g.to(DEV), lv.detach().to(DEV), eps.to(DEV)), lv.grad, what="dlogvar")
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    std = torch.exp(lv.detach() / 2)
    s = mu.detach() + std * eps
    close(o.reparam_student(mu.detach().to(DEV), lv.detach().to(DEV), eps.to(DEV), flag), s * std + mu.detach(), what="student sample")


def test_nan_scrub_only_when_nan_present():
    o = ops()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = torch.tensor([1.0, float("inf"), -2.0, 5.0] * 100, device=DEV)
    y = x.clone()
    o.nan_scrub_(y, flag)
    assert torch.equal(x.cpu(), y.cpu())            # inf alone is left in place (shape_networks.py:490)
    x[7] = float("nan")
    y = x.clone()
    o.nan_scrub_(y, flag)
    assert torch.equal(y.cpu(), torch.nan_to_num(x.cpu()))


def test_losses_roi_adam():
    o = ops()
    n = (4, 1, 13, 17)
    x = (rnd(*n, seed=61) * 3).requires_grad_(True)
    t = (rnd(*n, seed=62) > 0).float()
    ref = F.binary_cross_entropy(torch.sigmoid(x), t)
    ref.backward()
    close(o.bce_sigmoid_fwd(x.detach().to(DEV), t.to(DEV)), ref.detach(), rtol=1e-5, atol=1e-6, what="bce")
    close(o.bce_sigmoid_bwd(x.detach().to(DEV), t.to(DEV)), x.grad, rtol=1e-4, atol=1e-8, what="dbce")
    m = (rnd(*n, seed=63) > -0.5).float()
    x2 = (rnd(*n, seed=64) * 3).requires_grad_(True)
    pw = m.sum() / (m * t).sum()
    ref2 = F.binary_cross_entropy_with_logits(x2 * m, t, pos_weight=pw)
    ref2.backward()
    sums, pw_d = o.pos_weight_sums(m.to(DEV), t.to(DEV))
    close(pw_d, pw, rtol=1e-6, what="pos_weight")
    close(o.bce_logits_pw_fwd(x2.detach().to(DEV), m.to(DEV), t.to(DEV), pw_d), ref2.detach(), rtol=1e-5, atol=1e-6, what="bce pw")
    close(o.bce_logits_pw_bwd(x2.detach().to(DEV), m.to(DEV), t.to(DEV), pw_d), x2.grad, rtol=1e-4, atol=1e-8, what="dbce pw")
    _, pw1 = o.pos_weight_sums(torch.zeros(*n, device=DEV), t.to(DEV))
    assert float(pw1) == 1.0                            # 0/0 -> 1 (Trainer.py:866-867)
    a, b = rnd(*n, seed=65).requires_grad_(True), rnd(*n, seed=66)
    mse = F.mse_loss(b, a)
    mse.backward()
    close(o.mse_fwd(b.to(DEV), a.detach().to(DEV)), mse.detach(), rtol=1e-5, what="mse")
    close(o.mse_bwd(a.detach().to(DEV), b.to(DEV)), a.grad, rtol=1e-5, atol=1e-9, what="dmse")
    img = rnd(4, 3, 13, 17, seed=67)
    od = (torch.sigmoid(x.detach()) > 0.75).float()
    roi, od_d = o.roi(img.to(DEV), x.detach().to(DEV))
    assert torch.equal(od_d.cpu(), od)
    close(roi, (img + 1) * od - 1, what="roi")
    # Adam against torch.optim.Adam over 3 steps
    p = torch.nn.Parameter(rnd(1000, seed=68))
    opt = torch.optim.Adam([p], lr=5e-4, betas=(0.9, 0.99))
    pd, md, vd = p.detach().clone().to(DEV), torch.zeros(1000, device=DEV), torch.zeros(1000, device=DEV)
    for step in range(1, 4):
        gr = rnd(1000, seed=70 + step)
        p.grad = gr.clone()
        opt.step()
        o.adam_step(pd, gr.to(DEV), md, vd, 5e-4, 0.9, 0.99, 1e-8, step)
    close(pd, p.detach(), rtol=1e-6, atol=1e-7, what="adam")
    # the same three steps with the step number in device memory (what a captured launch uses)
    pd2, md2, vd2 = rnd(1000, seed=68).to(DEV), torch.zeros(1000, device=DEV), torch.zeros(1000, device=DEV)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step in range(1, 4):
        o.adam_step(pd2, rnd(1000, seed=70 + step).to(DEV), md2, vd2, 5e-4, 0.9, 0.99, 1e-8, 1, t_dev)
        o.counter_add(t_dev, 1)
    assert int(t_dev) == 3
    close(pd2, pd, rtol=1e-6, atol=1e-7, what="adam, device step counter")


def test_randn_stream_properties():
    o = ops()
    a = o.randn((1 << 20,), DEV, seed=7, offset=0)
    assert abs(float(a.mean())) < 5e-3 and abs(float(a.std()) - 1.0) < 5e-3
    assert float(a.abs().max()) < 7.0
    # a shard that starts at global element 4096 reproduces the same stream (data-parallel noise)
    b = o.randn((1000,), DEV, seed=7, offset=4096)
    assert torch.equal(a[4096:5096].cpu(), b.cpu())
    # the stream position may live in device memory (captured launches): offset + *counter
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    o.counter_add(ctr, 4000)
    c = o.randn((1000,), DEV, seed=7, offset=96, offset_dev=ctr)
    assert torch.equal(b.cpu(), c.cpu())
    assert not torch.equal(a[:1000].cpu(), o.randn((1000,), DEV, seed=8, offset=0).cpu())


def test_mmd_module():
    import algorithms
    from oracle import wtpse_cpu as O
    v = rnd(12, 120, seed=81) * 0.1
    got = algorithms.compute_MMD(3, 4).forward(v.to(DEV))
    ref = O.mmd(v, 3, 4)
    assert abs(float(got) - float(ref)) < 3e-7 + 1e-3 * abs(float(ref))


def test_rejects_bad_arguments():
    from wtpse_hip.lib import WtpseError
    o = ops()
    with pytest.raises(WtpseError):
        o.lib().call("wtpse_conv_fwd", 0, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 1, 8, 8, 16, 3, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        o.conv_fwd(torch.zeros(1, 16, 8, 8), None, 0, None, 16, 3)     # host tensor: no CPU fallback


def test_public_whitening_loss_is_differentiable():
    """WT_PSE.compute_whitening_loss / ShapeVariationalDist_x.compute_whitening_loss as public helpers: values and the
    gradient through autograd against the oracle's (reference algorithms.py:1277-1309, shape_networks.py:561-594)."""
    import algorithms
    import shape_networks
    from oracle import wtpse_cpu as O
    hp = dict(O.DEFAULT_HPARAMS)
    m = algorithms.WT_PSE(3, 1, hp, DEV, False, per_domain_batch=2, source_domain_num=3).to(DEV)
    sn = shape_networks.ShapeVariationalDist_x(hp, DEV, 1, 3, 2).to(DEV)
    z = rnd(6, 16, 24, 40, seed=91, scale=0.7)
    zr = z.clone().requires_grad_(True)
    off, dg, dom = O.whitening_loss(zr, 3, 2, 0.0)
    (off + dg + 2.0 * dom).backward()
    zd = z.to(DEV).requires_grad_(True)
    ins, d = m.compute_whitening_loss(zd)
    (ins + 2.0 * d).backward()
    close(ins, (off + dg).detach(), rtol=1e-5, atol=1e-7, what="ins")
    close(d, dom.detach(), rtol=1e-3, atol=1e-7, what="dom")
    close(zd.grad, zr.grad, rtol=1e-4, atol=1e-9, what="dz")
    zd2 = z.to(DEV).requires_grad_(True)
    o2, g2, d2 = sn.compute_whitening_loss(zd2)
    (o2 + g2 + 2.0 * d2).backward()
    close(zd2.grad, zr.grad, rtol=1e-4, atol=1e-9, what="dz (shape net)")


@pytest.mark.parametrize("shape", [(3, 16, 32, 64), (3, 16, 20, 40), (6, 3, 64, 64)])
def test_conv_gram_epilogue_and_wt_loss_from_partials(shape):
    """The DeepWT convs emit the per-tile partial Grams of their output (wtpse_conv_fwd_gram); compute_whitening_loss from
    those partials (wtpse_wt_loss_fwd_partials) must equal the loss computed from z itself and the oracle's."""
    from oracle import wtpse_cpu as O
    o = ops()
    B, Cin, H, W = shape
    x = rnd(B, Cin, H, W, seed=31)
    w = rnd(16, Cin, 3, 3, seed=32, scale=0.3)
    b = rnd(16, seed=33)
    packed, wf, _ = pack(w)
    z, (partial, S) = o.conv_fwd_gram(x.to(DEV), packed.data_ptr() + 4 * wf, b.to(DEV))
    ref = F.conv2d(x, w, b, padding=1)
    close(z, ref, what="conv (gram variant)")
    g_ref = torch.einsum("bip,bjp->bij", ref.reshape(B, 16, -1).double(), ref.reshape(B, 16, -1).double())
    g = partial.view(B, S, 16, 16).double().sum(1).cpu()
    close(g, g_ref, rtol=1e-5, atol=1e-5 * float(g_ref.abs().max()), what="partial Grams")
    pb = B // 3
    st_f = o.wt_loss_fwd(z, 3, pb, 0.0, gram_partial=(partial, S))
    st_d = o.wt_loss_fwd(z, 3, pb, 0.0)
    off, dg, dom = O.whitening_loss(ref, 3, pb, 0.0)
    for st in (st_f, st_d):
        close(st.losses[0], off, rtol=1e-4, atol=1e-7, what="off")
        close(st.losses[1], dg, rtol=1e-4, atol=1e-7, what="diag")
        close(st.losses[2], dom, rtol=2e-3, atol=1e-6, what="dom")
    close(st_f.gram, st_d.gram, rtol=1e-5, atol=1e-6, what="gram fused vs stand-alone")
    dz_f, dz_d = torch.empty_like(z), torch.empty_like(z)
    o.wt_loss_bwd(st_f, dz_f, False)
    o.wt_loss_bwd(st_d, dz_d, False)
    close(dz_f, dz_d, rtol=1e-4, atol=1e-7 * float(dz_d.abs().max()) + 1e-12, what="dL/dz fused vs stand-alone")


@pytest.mark.parametrize("shape,acc", [((4, 16, 32, 64), True), ((3, 8, 16, 8), False), ((2, 32, 64, 64), True)])
def test_maxpool_bwd_with_batchnorm_statistics(shape, acc):
    """The max-pool backward on the raw output of a conv + BatchNorm + ReLU layer that also forms that layer's BatchNorm-backward
    reductions (wtpse_maxpool2_bwd_bnb) + wtpse_bn_bwd_from_stats, against the separate passes (max-pool backward, then the
    three-kernel BatchNorm backward) and against autograd."""
    o = ops()
    B, C, H, W = shape
    y = rnd(*shape, seed=81).double().requires_grad_(True)
    gamma = (rnd(C, seed=82) * 0.2 + 1).double().requires_grad_(True)
    beta = (rnd(C, seed=83) * 0.2).double().requires_grad_(True)
    z = F.relu(F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5))
    skip = rnd(*shape, seed=84)
    dp = rnd(B, C, H // 2, W // 2, seed=85)
    loss = (F.max_pool2d(z, 2) * dp.double()).sum() + ((z * skip.double()).sum() if acc else 0.0)
    loss.backward()
    yd = y.detach().float().to(DEV)
    mean = yd.double().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(yd.double().var((0, 2, 3), unbiased=False) + 1e-5)
    g_d, b_d = gamma.detach().float().to(DEV), beta.detach().float().to(DEV)
    ss = torch.stack([g_d.double() * invstd, b_d.double() - mean * g_d.double() * invstd], 1).float().contiguous()
    mean_f, invstd_f = mean.float().contiguous(), invstd.float().contiguous()
    r = o.maxpool2_bwd_bnb(yd, dp.to(DEV), skip.clone().to(DEV) if acc else None, ss, True, mean_f)
    assert r is not None
    g, stats = r
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dy = o.bn_bwd_from_stats(g, yd, stats, g_d, mean_f, invstd_f, dg, db)
    # the separate passes
    g2 = o.maxpool2_bwd(yd, dp.to(DEV), skip.clone().to(DEV) if acc else None, acc, ss, True)
    dg2, db2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dy2 = o.bn_bwd(g2, yd, ss, True, g_d, mean_f, invstd_f, dg2, db2)
    sc = float(dy2.abs().max())
    close(dy, dy2, rtol=1e-4, atol=2e-5 * sc, what="fused vs separate dy")
    close(dg, dg2, rtol=1e-4, atol=1e-4 * float(dg2.abs().max()) + 1e-6, what="dgamma")
    close(db, db2, rtol=1e-4, atol=1e-4 * float(db2.abs().max()) + 1e-6, what="dbeta")
    on_kink = (F.batch_norm(y.detach(), None, None, gamma.detach(), beta.detach(), True, 0.1, 1e-5).abs() < 2e-6)
    kz = lambda t: torch.where(on_kink.to(t.device), torch.zeros_like(t), t)
    close(kz(dy), kz(y.grad.float()), rtol=1e-3, atol=2e-4 * float(y.grad.abs().max()), what="dy vs autograd")
    close(dg, gamma.grad, rtol=1e-3, atol=2e-4 * float(gamma.grad.abs().max()) + 1e-5, what="dgamma vs autograd")
