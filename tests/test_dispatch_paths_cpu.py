"""Host-side proof of tests/dispatch_cases.py: every case takes the branch it names — by the Python restatement of the launcher's
predicate and, where the library has a host query, by the C side — and the references are clear of the points where a last bit
decides a result (ReLU kinks of the BatchNorm cases within their cap, sign kinks of the Gram entries with nothing left out,
pooling windows without near-ties).  No GPU: the seeds are settled here before a kernel ever sees them."""
import pytest
import torch

import dispatch_cases as D


@pytest.fixture(scope="module")
def L():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    build.build()                                   # no-op when up to date
    return lib()


def test_plane_kernels_take_the_named_branch(L):
    for table, pred in ((D.POOL_FWD_CASES, D.pool_fwd_branch), (D.POOL_BWD_CASES, D.pool_bwd_branch),
                        (D.UP_FWD_CASES, D.up_fwd_branch), (D.UP_BWD_CASES, D.up_bwd_branch)):
        for name, ((B, C, H, W), branch, trips) in table.items():
            assert pred(H, W) == branch, (pred.__name__, name)
            assert pred(H, W, False) == "scalar", (pred.__name__, name)
            assert D.plane_trips(B * C) == trips, (pred.__name__, name)
    # the cap itself: 32768 planes are one trip, one more plane is a second trip
    assert D.plane_trips(D.PLANE_CAP) == 1 and D.plane_trips(D.PLANE_CAP + 1) == 2
    # both plane loops of the tables: the vector path, looped and not
    for table in (D.POOL_FWD_CASES, D.POOL_BWD_CASES, D.UP_FWD_CASES, D.UP_BWD_CASES):
        assert {t for _, b, t in table.values() if b == "vec"} == {1, 2}
        assert "scalar" in {b for _, b, _ in table.values()}
    # statistics rows of the plane kernels: gridDim.x * B
    for (B, C, H, W), branch, _ in D.POOL_BWD_CASES.values():
        assert L.query("wtpse_maxpool2_bwd_stats_blocks", B, H, W) == D.pool_stats_blocks(B, H, W)
    for (B, C, H, W), branch, _ in D.UP_FWD_CASES.values():
        assert L.query("wtpse_upsample2x_stats_blocks", B, H, W) == D.up_stats_blocks(B, H, W)
    for (B, C, H, W) in D.UP_BWD_BN_CASES.values():
        assert D.up_bwd_branch(H, W) == "vec"


def test_flat_kernels_take_both_forms():
    assert {D.flat_branch(n) for n in D.FLAT_SIZES} == {"vec", "scalar"}
    assert [D.flat_branch(n) for n in D.FLAT_SIZES] == ["scalar", "scalar", "vec", "scalar", "vec", "vec"]
    assert all(D.flat_branch(n, False) == "scalar" for n in D.FLAT_SIZES)
    assert [D.amax_branch(n) for n in D.AMAX_SIZES] == ["body+tail", "body+tail", "body", "body+tail", "body+tail", "body+tail"]
    assert all(D.amax_branch(n, False) == "misaligned" for n in D.AMAX_SIZES)
    assert all(n % 4 for n in D.RANDN_SIZES) and {n % 4 for n in D.RANDN_SIZES} == {1, 2, 3}


def test_loss_sizes_take_the_named_grid(L):
    for n, blocks in D.LOSS_SIZES.items():
        assert D.reduce_blocks(n) == blocks == L.query("wtpse_reduce_blocks", n), n
    big = max(D.LOSS_SIZES)
    assert D.loss_trips(big) == 17 and big <= 4_200_000       # the cap: grid-stride trips beyond the 16 of a full workgroup
    assert D.loss_trips(4097) == 9 and D.loss_trips(255) == 1
    for name, (B, CE, HW, rows, kernel) in D.ATTN_CASES.items():
        assert D.ceil_div(B * HW, 256) == rows and D.reduce_rows_branch(rows, 2) == kernel, name
    assert D.ATTN_CASES["tall_ragged"][2] % 256 == 5


def test_batchnorm_cases_take_the_named_branch(L):
    for name, ((B, C, H, W), relu, expect) in D.BN_CASES.items():
        br = D.bn_bwd_branch(B, C, H * W, halves=name in D.BN_HALVES)
        for k, v in expect.items():
            assert br[k] == v, (name, k, br)
        if name in D.BN_HALVES:
            assert D.bn_bwd_branch(B, C, H * W)["path"] == "small"
        if br["path"] == "three":
            assert L.query("wtpse_bn_bwd_nsplit", B, C, H * W) == br["nsplit"], name
    seen = [D.bn_bwd_branch(B, C, H * W, halves=n in D.BN_HALVES) for n, ((B, C, H, W), _, _) in D.BN_CASES.items()]
    assert {b["path"] for b in seen} == {"small", "three"}
    three = [b for b in seen if b["path"] == "three"]
    assert {b["finalize"] for b in three} == {256, 1024}
    assert {b["segs"] for b in three} >= {1, 2, 4}
    assert {b["remainder"] for b in three if b["reduce"] == "vec"} == {True, False}
    assert any(b["units_per_split"] > 1 for b in three)
    # a misaligned operand moves the reduction and / or the apply pass onto the scalar kernels, and the one-launch form off
    assert D.bn_bwd_branch(2, 3, 1024, in_aligned=False)["reduce"] == "scalar"
    assert D.bn_bwd_branch(2, 3, 1024, dy_aligned=False) == dict(D.bn_bwd_branch(2, 3, 1024), apply="scalar")
    assert D.bn_bwd_branch(2, 96, 256, dy_aligned=False)["path"] == "three"


def test_batchnorm_exact_sum_cases_take_the_named_branch(L):
    import exact_cases as E
    B, C, H, W = D.BN_EXACT_SHAPE
    assert D.bn_bwd_branch(B, C, H * W)["path"] == "small" and C == 96 and B * H * W <= 32768       # the smallest C of the one-launch form
    br = D.bn_bwd_branch(B, D.BN_EXACT_CUT, H * W)
    assert (br["path"], br["reduce"], br["apply"], br["finalize"], br["nsplit"]) == ("three", "vec", "vec", 256, B)
    assert L.query("wtpse_bn_bwd_nsplit", B, D.BN_EXACT_CUT, H * W) == B
    assert [D.bn_fold_width(n) for n in D.BN_EXACT_ROWS] == [256, 1024] and D.bn_fold_width(2047) == 256 and D.bn_fold_width(2048) == 1024
    # the operands: integers |v| <= 3, a mean of halves; per (image, channel) the products g (y - mean) are non-zero in at most one
    # float4, where they add up to +-2^k — the fp32 `* invstd` of a thread of bn_bwd_reduce_k and its butterfly are then exact
    r = D.bn_exact_inputs()
    d = r["y"].double() - r["mean"].double().view(1, C, 1, 1)
    assert float(d.abs().max()) <= 3 and float(r["dz"].abs().max()) <= 3 and bool((r["mean"] * 2 == (r["mean"] * 2).round()).all())
    assert bool((d == d.round()).all()) and bool((r["dz"] == r["dz"].round()).all())
    z = r["y"].double() * r["ss"][:, 0].double().view(1, C, 1, 1) + r["ss"][:, 1].double().view(1, C, 1, 1)
    assert torch.equal(r["g_masked"], r["dz"].double() * (z > 0)) and bool((z.float().double() == z).all())
    n = (r["g_masked"] * d).reshape(B, C, H * W // 4, 4).sum(3)
    assert bool(((n != 0).sum(2) <= 1).all()) and bool((torch.log2(n.abs().clamp(min=1)) % 1 == 0).all())
    assert int((r["n2"] != 0).sum()) > C // 2 and int((r["s1"] != 0).sum()) > C // 2
    cut = D.bn_exact_inputs(channels=D.BN_EXACT_CUT)
    assert cut["shape"] == (B, D.BN_EXACT_CUT, H, W) and torch.equal(cut["y"], r["y"][:, :D.BN_EXACT_CUT]) and torch.equal(cut["n2"], r["n2"][:D.BN_EXACT_CUT])
    rows, s1, n2 = D.bn_exact_rows()
    few, many = D.BN_EXACT_ROWS
    assert rows[many].shape == (many, D.BN_EXACT_C, 2) and rows[few].shape == (few, D.BN_EXACT_C, 2) and float(rows[many].abs().max()) <= 3
    assert torch.equal(rows[few].double().sum(0), rows[many].double().sum(0)) and torch.equal(rows[many].double().sum(0), torch.stack([s1, n2], 1))
    # the tail: the smallest case of the fp32 layout among the data gradients with the BatchNorm-backward epilogue
    fp32 = [(c[0] * c[1] * c[5] * c[6], i) for i, c in enumerate(E.TABLES["bnb"]) if not c[9]]
    assert min(fp32)[1] == D.BN_EXACT_TAIL and E.bnb_layouts(E.TABLES["bnb"][D.BN_EXACT_TAIL])[0] == 0
    # the reference helper: against the formulas written out independently, in fp64
    g, iv, mu = D.bn_exact_channels(D.BN_EXACT_C, 730)
    ref = D.bn_finish_ref(s1, n2, 100, g, mu, iv)
    k1 = g.double() * iv.double()
    k2 = -g.double() * iv.double() ** 2 * (n2 * iv.double()) / 100
    assert torch.allclose(ref["k1"], k1, rtol=1e-15) and torch.allclose(ref["k2"], k2, rtol=1e-14)
    assert torch.allclose(ref["k3"], -k1 * s1 / 100 - k2 * mu.double(), rtol=1e-12, atol=1e-18)
    fz = D.bn_finish_ref(s1, n2, 100, g, mu, iv, frozen=True)
    assert not bool(fz["k2"].any()) and not bool(fz["k3"].any()) and torch.allclose(fz["dbias"], k1 * s1, rtol=1e-15)
    assert D.ulps_apart(torch.tensor([1.0, -2.0]), torch.tensor([1.0 + 2.0 ** -23, -2.0], dtype=torch.float64)) == 1


def test_batchnorm_references_stay_off_the_relu_kink():
    for name, (shape, relu, _) in D.BN_CASES.items():
        r = D.bn_inputs(shape, relu)
        assert int(r["on_kink"].sum()) <= D.kink_cap(r["on_kink"].numel()), name
    r = D.bn_inputs((2, 96, 16, 16), True, channels=95)
    assert r["shape"] == (2, 95, 16, 16) and int(r["on_kink"].sum()) <= D.kink_cap(r["on_kink"].numel())
    for hw in D.BN_VEC_HW + D.BN_SCALAR_HW + (1024,):          # the element-wise and misalignment cases: sums include every entry
        assert int(D.bn_inputs((2, 3, 1, hw), True)["on_kink"].sum()) == 0, hw
    full = D.bn_inputs((2, 96, 16, 16), True)
    assert torch.equal(full["y"][:, :95], r["y"]) and torch.equal(full["dy"][:, :95], r["dy"])      # BatchNorm is per channel


def test_wt_cases_take_the_named_branch(L):
    for name, ((B, C, H, W), pb, expect) in D.WT_CASES.items():
        br = D.wt_branch(B, H * W)
        for k, v in expect.items():
            assert br[k] == v, (name, k, br)
        assert L.query("wtpse_wt_split", B, H * W, 0) == br["S"], name
        assert 3 * pb <= B
    assert D.wt_branch(3, 2052, z_aligned=False)["fwd"] == "scalar"
    assert D.wt_branch(3, 2052, dz_aligned=False) == dict(D.wt_branch(3, 2052), bwd="scalar", bwd_blocks=9)
    assert 768 // 770 == 0 and D.wt_split(770, 16) == (1, 2048)          # the split target clamps to 1
    for S, (nw, pairs, single) in D.WT_FINALIZE_S.items():
        br = D.wt_branch(3, 8 * S, S=S)
        assert (br["finalize"], br["finalize_pairs"], br["finalize_single"]) == (nw, pairs, single), S


def test_wt_references_stay_off_the_sign_kinks():
    """|G_ij| and |G_ii - 1| change sign at 0: no fp64 Gram entry of any case lies within KINK_MARGIN of it, so nothing is left
    out of the gradient comparison; and the margin that switches one image's clamp off sits between two per-image sums."""
    for name, (shape, pb, _) in D.WT_CASES.items():
        z = D.wt_feature(shape, D.WT_SEEDS[name])
        assert D.wt_kink_distance(z) > D.KINK_MARGIN, name
        m = D.wt_margin_one_off(z)
        g = D.wt_gram64(z)
        off = (g.abs() * torch.ones(16, 16, dtype=torch.float64).triu(1)).sum((1, 2))
        dg = (g.diagonal(dim1=1, dim2=2) - 1).abs().sum(1)
        # (an fp32 sum of up to 120 Gram entries carries at most ~120 * 2^-24 = 7e-6 of its value: 2e-5 of the margin is clear of it)
        assert int((off < m).sum()) == 1 and float((off - m).abs().min()) > 2e-5 * m, name
        assert float((dg - m).abs().min()) > 2e-5 * m, name
    for S, seed in D.WT_FINALIZE_SEEDS.items():
        assert D.wt_kink_distance(D.wt_feature((3, 16, 8, S), seed)) > D.KINK_MARGIN, S


def test_pool_references_have_no_near_ties():
    """A window's largest two values are either exactly equal (the first wins everywhere) or apart by far more than the rounding
    of the fused scale/shift."""
    for table in (D.POOL_FWD_CASES, D.POOL_BWD_CASES):
        for name, (shape, _, _) in table.items():
            x = D.pool_input(name, shape)
            for pro in (None, D.make_pro(shape[1], 7)):
                for relu in (0, 1):
                    assert D.pool_window_gap(x, pro, relu) > 1e-6, (name, pro is not None, relu)
    x = D.pool_input("ties", (2, 3, 6, 8))
    p, g = D.pool_ref(x, None, 1, torch.ones(2, 3, 3, 4), None, 0)
    assert float(p[0, 1, 1, 2]) == 0.0 and float(g[0, 1, 2, 4]) == 1.0 and float(g[0, 1, 2:4, 4:6].sum()) == 1.0    # all-negative: first wins
    assert float(g[0, 0, 0, 0]) == 1.0 and float(g[0, 0, 0:2, 0:2].sum()) == 1.0                                   # all-equal: first wins


def test_saturated_logits_keep_out_of_the_few_bit_band():
    x, t = D.saturated_inputs()
    assert not bool(((x.abs() > 9) & (x.abs() < 18)).any())
    for v in (0.0, 8.0, 20.0, 40.0, 90.0):
        for s in (1.0, -1.0):
            assert {float(u) for u in t[x == s * v]} == {0.0, 1.0}


def test_reference_helpers_agree_with_autograd():
    """The hand-written references against torch: the fp64 Adam recurrence against torch.optim.Adam, the wt_combine folds against
    their spelled-out sums, the partial Grams against the whole Gram."""
    p0, g = D.rnd(50, seed=1).double(), D.rnd(50, seed=2).double()
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=5e-4, betas=(0.9, 0.99))
    q, m, v = p0, torch.zeros(50), torch.zeros(50)
    for step in (1, 2, 3):
        p.grad = g.clone()
        opt.step()
        q, m, v = D.adam_ref(q, g, m, v, 5e-4, 0.9, 0.99, 1e-8, step)
    assert torch.allclose(q, p.detach(), rtol=1e-12, atol=1e-14)
    l = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    assert torch.allclose(D.wt_combine_ref(l, 3.0, 0), torch.tensor([12.0 / 3, 5.0 / 3, 7.0 / 3, 9.0 / 3], dtype=torch.float64))
    assert torch.allclose(D.wt_combine_ref(l, 3.0, 1), torch.tensor([5.0 / 3 + 10.0 / 3, 5.0 / 3, 10.0 / 3, 9.0 / 3], dtype=torch.float64))
    z = D.wt_feature((3, 16, 8, 33), 0)
    parts = D.wt_partials(z, 33).double().view(3, 33, 16, 16).sum(1) / (8 * 33 - 1) + 1e-5 * torch.eye(16, dtype=torch.float64)
    assert torch.allclose(parts, D.wt_gram64(z), rtol=1e-6, atol=1e-7)
