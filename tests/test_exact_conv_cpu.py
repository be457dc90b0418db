"""Host-side proof of tests/exact_cases.py.  Every weight-gradient case takes the branch it is listed under — by the Python
restatement of the launch plan and by the library's host query; every checked output of every case stays inside the exactness bound
(sum of |products| + |bias| + |accumulate base| < 2^22 units), every class-T case has teeth (dropping A's low part changes at least
90 % of the outputs that can change), every fp64 reference survives fp32, and every class-T operand splits exactly into two fp16
terms (none subnormal) at the scales the case will meet and into the bf16 terms of x3.  No GPU."""
import pytest
import torch

import exact_cases as E


@pytest.fixture(scope="module")
def L():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    build.build()                                   # no-op when up to date
    return lib()


# =============================================================================================== plans and branches
def test_fp32_wgrad_cases_take_the_named_branch(L):
    for name, (shape, k, expect, _) in E.WG32_CASES.items():
        B, C0, C1, Co, H, W = shape
        g = E.wgrad_geometry(B, H, W, C0 + C1, Co, k)
        for key, val in expect.items():
            assert g[key] == val, (name, key, g)
        assert E.wgrad_ksplit(B, H, W, C0 + C1, Co, k) == L.query("wtpse_wgrad_ksplit", B, H, W, C0 + C1, Co), name
        assert g["tiles"] == L.query("wtpse_conv_stats_blocks", B, H, W), name
        assert C1 == 0 or C0 % 16 == 0, name
    geo = {n: E.wgrad_geometry(c[0][0], c[0][4], c[0][5], c[0][1] + c[0][2], c[0][3], c[1]) for n, c in E.WG32_CASES.items()}
    k3 = [g for n, g in geo.items() if E.WG32_CASES[n][1] == 3]
    # every N-block instantiation, on both widths of the M block, and the forms with slack with nblk < NBLK
    for p32 in (False, True):
        assert {g["inst"] for g in k3 if g["P32"] == p32} == {1, 2, 5, 9}, p32
        assert {(g["nblk"], g["inst"]) for g in k3 if g["P32"] == p32 and g["slack"]} == {(4, 5), (7, 9)}, p32
        # the 9-block form: one tap per block (cg == MB) and mixed slots (cg < MB), the latter with and without slack
        assert {(g["full"], g["slack"]) for g in k3 if g["P32"] == p32 and g["inst"] == 9} == {(True, False), (False, False), (False, True)}, p32
    assert {g["TW"] for g in geo.values()} == {16, 32}
    assert {(g["P32"], g["TW"]) for n, g in geo.items() if E.WG32_CASES[n][1] == 1} == {(True, 16), (False, 32)}
    assert any(g["ragged_group"] and g["cout_blocks"] == 3 for g in k3)
    # the explicit split counts: one that does not divide the tile count, fewer than 8 slabs, more than 8 and no multiple of 8, all tiles
    for name, (shape, k, tiles, splits) in E.WG32_KSPLIT.items():
        B, C0, C1, Co, H, W = shape
        assert E.wgrad_geometry(B, H, W, C0 + C1, Co, k)["tiles"] == tiles == L.query("wtpse_conv_stats_blocks", B, H, W)
        assert all(1 <= s <= tiles for s in splits) and 1 in splits and tiles in splits
        assert any(tiles % s for s in splits) and any(s < 8 for s in splits) and any(s > 8 and s % 8 for s in splits)
        assert E.wgrad_geometry(B, H, W, C0 + C1, Co, k)["bias_wgs"] == 1
    assert geo["wide_ragged"]["bias_wgs"] == 3 and any(v.bias for v in E.WG32_CASES["wide_ragged"][3])


def test_x3_wgrad_cases_take_the_named_branch(L):
    for name, (shape, expect, _) in E.WGX3_CASES.items():
        B, C0, C1, Co, H, W = shape
        assert E.wgrad_x3_supported(C0 + C1, Co, 3, C0 if C1 else 8), name
        assert L.query("wtpse_wgrad_x3_supported", C0 + C1, Co, 3, C0 if C1 else 8) == 1, name
        g = E.wgrad_x3_geometry(B, H, W, C0 + C1, Co)
        for key, val in expect.items():
            assert g[key] == val, (name, key, g)
        assert E.wgrad_x3_ksplit(B, H, W, C0 + C1, Co) == L.query("wtpse_wgrad_x3_ksplit", B, H, W, C0 + C1, Co), name
    geo = [E.wgrad_x3_geometry(s[0], s[4], s[5], s[1] + s[2], s[3]) for s, _, _ in E.WGX3_CASES.values()]
    assert {g["Q"] for g in geo} == {False, True} and all(g["TW"] == 16 for g in geo)
    assert any(g["Q"] and g["tiles"] == 1 for g in geo) and any(g["Q"] and g["tiles"] == 18 for g in geo)
    # the predicate itself, against the library, around its edges
    for cin, cout, k, c0 in ((32, 32, 3, 8), (16, 32, 3, 8), (32, 48, 3, 8), (64, 64, 1, 8), (64, 64, 3, 12), (96, 64, 3, 32)):
        assert int(E.wgrad_x3_supported(cin, cout, k, c0)) == L.query("wtpse_wgrad_x3_supported", cin, cout, k, c0), (cin, cout, k, c0)


def test_tw32_wgrad_cases_change_their_tile_count():
    """WGX3_TW32_CASES (run by the tw32 job of tests/switch_worker.py): listed under conv_wgrad_x3_k<3, 5, Q> for both Q, with two and
    three tile columns, ragged last columns and rows — and each with another tile count, hence another default split count, than on the
    16-wide tiles: that is what lets a process prove the switch in force.  (The library's side of it needs a process started under
    the switch: test_switch_paths_cpu.py.)"""
    for name, (shape, expect, tiles16, _) in E.WGX3_TW32_CASES.items():
        B, C0, C1, Co, H, W = shape
        assert E.wgrad_x3_supported(C0 + C1, Co, 3, C0 if C1 else 8), name
        g = E.wgrad_x3_geometry(B, H, W, C0 + C1, Co, tw32=True)
        for key, val in expect.items():
            assert g[key] == val, (name, key, g)
        assert W % 32 != 0 and (H % g["TH"] != 0 or name == "tw32_cat"), name            # ragged last tile column (and row)
        assert E.wgrad_x3_geometry(B, H, W, C0 + C1, Co)["tiles"] == tiles16 != g["tiles"], name
        assert E.wgrad_x3_ksplit(B, H, W, C0 + C1, Co, tw32=True) == g["tiles"] and E.wgrad_x3_ksplit(B, H, W, C0 + C1, Co) == tiles16, name
    geo = [E.wgrad_x3_geometry(s[0], s[4], s[5], s[1] + s[2], s[3], tw32=True) for s, _, _, _ in E.WGX3_TW32_CASES.values()]
    assert {g["Q"] for g in geo} == {False, True}
    assert any(v.pro == 3 and v.acc for v in E.WGX3_TW32_CASES["tw32_cat"][3]) and E.WGX3_TW32_CASES["tw32_cat"][0][2]
    # 16-wide maps keep the 16-wide tiles under the switch
    assert E.wgrad_x3_geometry(2, 8, 16, 32, 32, tw32=True) == E.wgrad_x3_geometry(2, 8, 16, 32, 32)


X3_TABLES = ("x3", "x3r", "x3half", "x3sw", "x3k1")


def test_x3_tiling_restated(L):
    """x3_tiling of exact_cases against wtpse_conv_x3_stats_blocks for every case of every x3 table (and the layout-1 bnb cases) under
    the default switches, wtpse_x3_small_wide(1) and wtpse_x3r_enable(0) — the setters work on the host —; and every new case in the
    branch it is listed under."""
    shapes = [E.conv_shape(t, c) for t in X3_TABLES for c in E.TABLES[t]]
    shapes += [(c[0], c[1] + c[2], 0, c[1] + c[2], c[5], c[6], c[7]) for c in E.TABLES["bnb"] if c[9]]
    assert L.query("wtpse_x3_small_wide", -1) == 0 and L.query("wtpse_x3r_enable", -1) == 1
    try:
        for sw, x3r in ((0, 1), (1, 1), (0, 0), (1, 0), (1, 2)):
            L.query("wtpse_x3_small_wide", sw)
            L.query("wtpse_x3r_enable", x3r)
            for B, C0, C1, Co, H, W, k in shapes:
                for cout in (Co, C0 + C1):               # forward and data-gradient direction
                    t = E.x3_tiling(B, H, W, cout, k, small_wide=sw, x3r=x3r)
                    assert t["tiles"] == L.query("wtpse_conv_x3_stats_blocks", B, H, W, cout, k), ((B, C0, C1, Co, H, W, k), cout, sw, x3r, t)
    finally:
        L.query("wtpse_x3_small_wide", 0)
        L.query("wtpse_x3r_enable", 1)
    # the new cases in the branches they are listed under
    for case in E.X3_SMALL_WIDE_CASES:
        B, C0, C1, Co, H, W, k = case
        for cout in (Co, C0 + C1):
            for x3r in (1, 2):
                t = E.x3_tiling(B, H, W, cout, k, small_wide=1, x3r=x3r)
                assert (t["small"], t["half"], t["mt"], t["TW"], t["TH"]) == (1, 0, 1, 32, 4), (case, cout, t)
            off = E.x3_tiling(B, H, W, cout, k)
            assert (off["small"], off["half"], off["mt"], off["TH"]) == (0, 0, 1, 8), (case, cout, off)
    sw = [E.x3_tiling(c[0], c[4], c[5], c[3], c[6], small_wide=1) for c in E.X3_SMALL_WIDE_CASES]
    assert {t["tiles_x"] for t in sw} == {1, 2, 3}
    last_rows = {c[4] - (t["tiles_y"] - 1) * 4 for c, t in zip(E.X3_SMALL_WIDE_CASES, sw)}
    assert last_rows == {1, 2, 4}                         # ragged last tile rows of one and two rows, full ones, an image lower than a tile
    assert {c[6] for c in E.X3_SMALL_WIDE_CASES} == {1, 3} and any(c[2] for c in E.X3_SMALL_WIDE_CASES)
    assert any(c[3] == 64 for c in E.X3_SMALL_WIDE_CASES) and any(c[3] > 64 for c in E.X3_SMALL_WIDE_CASES) and any(c[3] <= 16 for c in E.X3_SMALL_WIDE_CASES)
    for case in E.BNB_SMALL_WIDE:
        B, Cl, Co, bn_second, Cn, H, W, k, relu, x3 = case
        assert case in E.TABLES["bnb"] and x3, case
        t = E.x3_tiling(B, H, W, Cl + Co, k, small_wide=1)
        assert (t["small"], t["mt"], t["TW"], t["TH"]) == (1, 1, 32, 4), (case, t)
    for B, C0, C1, Co, H, W, k in E.X3_K1_MT2_CASES:
        t = E.x3_tiling(B, H, W, Co, k)
        assert k == 1 and (t["mt"], t["half"], t["small"], t["tiles"]) == (2, 0, 0, 512), t
    # no 1x1 case of the older tables reaches the 64-channel blocks
    assert not any(E.x3_tiling(c[0], c[4], c[5], c[3], c[6])["mt"] == 2 for c in E.TABLES["x3"] if c[6] == 1)


def test_r_wgrad_cases_take_the_named_branch(L):
    plans = {}
    for name, (shape, expect, variants, _) in E.WGR_CASES.items():
        B, C0, C1, Co, H, W = shape
        assert E.wgrad_r_supported(C0 + C1, Co, 3, C0 if C1 else 16, W), name
        assert L.query("wtpse_wgrad_r_supported", C0 + C1, Co, 3, C0 if C1 else 16, W) == 1, name
        p = plans[name] = E.wgrad_r_plan(B, H, W, C0 + C1, Co)
        for key, val in expect.items():
            assert p[key] == val, (name, key, p)
        assert p["slabs"] == L.query("wtpse_wgrad_r_slabs", B, H, W, C0 + C1, Co), name
        for v in variants:
            assert not v.bias or p["mf"] * p["nf"] == 1, name           # the bias gradient: 16 x 16 blocks only
            assert not v.bn or (W != 16 and not v.bias), name            # the fused-BatchNorm form: no twin, no bias
            assert v.amax != "dyx" or v.pro is None, name                # amax_of(x) bounds x as stored, not behind a prologue
    P = plans.values()
    assert {(p["mf"], p["nf"]) for p in P} == {(1, 1), (2, 1), (1, 2), (2, 2)}
    # each block shape with a prologue, without one and in the fused-BatchNorm form
    for blk in ("blk11", "blk21_h1", "blk12", "blk22"):
        vs = E.WGR_CASES[blk][2]
        assert any(v.pro and not v.bn for v in vs) and any(v.pro is None for v in vs) and any(v.bn for v in vs), blk
    # segment heights 1 .. 5 (3k + 1 above 3 included), short last segments, X rows a unit walks in every residue of the unrolled loop
    assert {p["rseg"] for p in P} >= {1, 2, 3, 4, 5}
    assert {(p["rseg"], p["last"]) for p in P} >= {(4, 2), (5, 2), (4, 1), (3, 1), (5, 1)}
    assert set().union(*[p["xrows_mod4"] for p in P]) == {0, 1, 2, 3}
    assert any(p["idle"] for p in P) and any(p["per_wave"] == (1, 2) for p in P)
    assert plans["h1"]["nseg"] == 1 and plans["h2"]["nseg"] == 2
    twins = [p for p in P if p["twin"]]
    assert {p["odd_pair"] for p in twins} == {True, False} and any(p["rseg"] > 1 for p in twins)
    assert any(p["strips"] == 3 for p in P) and any(p["strips"] == 2 and p["rseg"] > 1 for p in P)
    # the predicate and the slab count against the library off the table too
    for cin, cout, k, c0, w in ((64, 64, 3, 16, 64), (256, 256, 3, 16, 16), (16, 16, 3, 16, 16), (64, 64, 3, 16, 24), (48, 32, 3, 16, 32),
                                (32, 32, 1, 16, 32), (32, 32, 3, 8, 32)):
        assert int(E.wgrad_r_supported(cin, cout, k, c0, w)) == L.query("wtpse_wgrad_r_supported", cin, cout, k, c0, w), (cin, cout, k, c0, w)
    for B, H, W, cin, cout in ((32, 16, 16, 256, 256), (24, 32, 64, 64, 64), (1, 3, 32, 16, 16), (7, 9, 96, 48, 16)):
        assert E.wgrad_r_slabs(B, H, W, cin, cout) == L.query("wtpse_wgrad_r_slabs", B, H, W, cin, cout), (B, H, W, cin, cout)


def test_which_arithmetic_a_wgrad_r_call_runs():
    """wgrad_r_terms(): x2h needs mode 2, a materialised dY and — on the 16 x 16 blocks — dY's amax table; the one-term mode skips the
    16 x 16 blocks and the fused-BatchNorm form."""
    small, big, twin = (E.wgrad_r_plan(2, 4, 32, 16, 16), E.wgrad_r_plan(2, 8, 32, 32, 32), E.wgrad_r_plan(3, 5, 16, 32, 32))
    V = E.V
    assert E.wgrad_r_terms(2, small, V(3)) == 3 and E.wgrad_r_terms(2, small, V(3, amax="dy")) == 2
    assert E.wgrad_r_terms(2, big, V(3)) == 2 and E.wgrad_r_terms(2, big, V(3, bn=True)) == 3
    assert E.wgrad_r_terms(2, twin, V(3)) == 2 and E.wgrad_r_terms(3, twin, V(3)) == 3 and E.wgrad_r_terms(1, twin, V(None)) == 1
    assert E.wgrad_r_terms(1, small, V(3)) == 3 and E.wgrad_r_terms(1, big, V(3)) == 1 and E.wgrad_r_terms(1, big, V(3, bn=True)) == 3
    assert all(E.wgrad_r_terms(3, p, V(3)) == 3 for p in (small, big, twin))


def test_fold_cases_take_both_loops_of_the_fold():
    """wgrad_fold4_k: fewer than 8 slabs (empty lane groups), the tail loop alone, exactly 32 (the strided loop once, no tail), 33 and 34
    (once + a tail in one / two lane groups), many; wgrad_reduce_k (with a bias gradient): fewer than 8, and counts 8 does not divide."""
    for slabs, name in E.FOLD4_SLABS.items():
        B, C0, C1, Co, H, W = E.WGR_CASES[name][0]
        assert E.wgrad_r_plan(B, H, W, C0 + C1, Co)["slabs"] == slabs, name
        assert any(not v.bias for v in E.WGR_CASES[name][2]), name
        assert (Co * (C0 + C1) * 9) % 128 == 0, name           # n % 4 != 0 and a ragged last workgroup: unreachable from the entry points
    f = {s: E.fold_branch(s, False) for s in E.FOLD4_SLABS}
    assert f[1]["empty_groups"] == 7 and f[3]["empty_groups"] == 5 and f[7]["empty_groups"] == 1
    assert f[12] == dict(f[12], strided=(0, 0), tail=(1, 2))
    assert f[32] == dict(f[32], strided=(1, 1), tail=(0, 0))
    assert f[33] == dict(f[33], strided=(1, 1), tail=(0, 1)) and f[34]["tail"] == (0, 1)
    assert f[220]["strided"] == (6, 7) and f[220]["tail"] == (0, 3)
    # the x3 entry point reaches the same fold; its cases bring 2, 4, 6, 18 and 1 slabs
    assert sorted(E.wgrad_x3_ksplit(s[0], s[4], s[5], s[1] + s[2], s[3]) for s, _, _ in E.WGX3_CASES.values()) == [1, 2, 4, 6, 18]
    with_bias = {E.wgrad_r_plan(s[0], s[4], s[5], s[1] + s[2], s[3])["slabs"] for s, _, vs, _ in E.WGR_CASES.values() if any(v.bias for v in vs)}
    assert with_bias >= {3, 12, 34, 220}


# =============================================================================================== exactness, teeth, splits
def _check_splits(what, operands, scales):
    """Every operand as the matrix cores see it: three bf16 terms exact (x3); two fp16 terms exact and normal at each x2h scale."""
    for key, t in operands.items():
        assert E.fp32_exact(t), (what, key)
        assert E.split_bf16_exact(t, 3), (what, key, "three bf16 terms")
        if key in scales:
            exact, normal = E.split2h_exact(t, scales[key])
            assert exact and normal, (what, key, scales[key], exact, normal)


def _wgrad_checks(fam):
    for name in E.wgrad_cases(fam):
        (B, C0, C1, Co, H, W), k, variants, classes = E.wgrad_case(fam, name)
        plan = E.wgrad_r_plan(B, H, W, C0 + C1, Co) if fam == "r" else None
        for cls in E.wgrad_classes(classes):
            for v in variants:
                what = (fam, name, cls, E.vid(v))
                p = E.wgrad_problem(fam, name, cls, v)
                assert p["d"] is not None, what + ("no density of B keeps the case inside the bound",)
                extra = 3.0 if v.acc else 0.0
                assert float(p["absdw"].max()) / p["unit"] + extra / p["unit"] < E.BOUND, what
                assert E.fp32_exact(p["dw"]), what
                if v.bias:
                    assert E.fp32_exact(p["db"]), what
                    assert p["check_db"] or cls == "TD", what          # dense class-T dY: the bias gradient stays class I's and TX's
                    if p["check_db"]:
                        assert float(p["absdb"].max()) / p["unit"] + extra / p["unit"] < E.BOUND, what
                if v.bn:
                    for t in (p["g"], p["y"], p["coef"]):
                        assert E.fp32_exact(t), what
                modes = E.MODES_I if cls == "I" else E.MODES_T
                if cls == "I":
                    # one bf16 term has to hold every operand as loaded
                    assert all(E.split_bf16_exact(t, 1) for t in p["loaded"].values()), what
                    continue
                assert E.teeth(p["dw"], p["round"](), p["absdw"]) >= E.TEETH, what
                # A as stored is two terms of either split; as loaded (prologue, BatchNorm form) it meets these scales
                raw = torch.cat([p["x0"].reshape(-1), p["x1"].reshape(-1) if p["x1"] is not None else p["x0"].new_zeros(0)]) \
                    if cls == "TX" else (p["g"] if v.bn else p["dy"]).reshape(-1)
                assert E.split_bf16_exact(raw, 2) and all(E.split2h_exact(raw, 2.0 ** e) == (True, True) for e in (2, 6, 12, 13)), what
                for mode in modes:
                    _check_splits(what + (mode,), p["loaded"], E.wgrad_scales(fam, plan, mode, v, p) if plan else {})
        E.clear_caches()


def test_fp32_wgrad_cases_are_exact_and_have_teeth():
    _wgrad_checks("fp32")


def test_x3_wgrad_cases_are_exact_and_have_teeth():
    _wgrad_checks("x3")


def test_tw32_wgrad_cases_are_exact_and_have_teeth():
    _wgrad_checks("x3tw32")
    for name in E.WGX3_TW32_CASES:
        shape, k, variants, classes = E.wgrad_case("x3tw32", name)
        for cls in ("TX", "TD"):
            for v in variants:
                # (the concat sums 720 pixels x 64 channels per weight — twice the pixels of the other two — and takes the next density)
                assert E.wgrad_problem("x3tw32", name, cls, v)["d"] >= (0.125 if name == "tw32_cat" else 0.25), (name, cls, E.vid(v))
    E.clear_caches()


def test_r_wgrad_cases_are_exact_and_have_teeth():
    _wgrad_checks("r")


def test_explicit_ksplit_case_is_exact_and_has_teeth():
    _wgrad_checks("ksplit")


@pytest.mark.parametrize("table", [t for t in E.TABLES if t != "bnb"])
def test_forward_and_dgrad_cases_are_exact_and_have_teeth(table):
    left_out = set()
    for idx, case in enumerate(E.TABLES[table]):
        B, C0, C1, Co, H, W, k = E.conv_shape(table, case)
        for variant in E.conv_variants(table, case):
            for cls in E.conv_classes(variant):
                what = (table, case, cls, variant)
                p = E.conv_problem(table, idx, cls, variant)
                if cls != "I" and B >= 20 and (p["d"] is None or p["d"] < E.MIN_DENSITY_EXISTING):
                    left_out.add((idx, cls, variant))
                    continue
                assert p["d"] is not None and (cls == "I" or p["d"] >= E.MIN_DENSITY_EXISTING), what
                assert table != "x3sw" or p["d"] >= E.MIN_DENSITY_SMALL_WIDE, what
                assert float(p["absout"].max()) / p["unit"] < E.BOUND and E.fp32_exact(p["out"]), what
                if variant in ("bias", "stats") and cls == "I":
                    # (the rows of partials are compared through their fp64 sum: each row exact, the total need not fit fp32)
                    assert p["check_sum"], what
                    assert variant != "stats" or p["check_sq"], what
                    if variant == "stats":
                        assert float((p["out"] != 0).double().mean()) > 0.9, what           # sparse operands, not empty outputs
                if cls == "I":
                    assert all(E.split_bf16_exact(t, 1) for t in p["loaded"].values()), what
                    continue
                assert E.teeth(p["out"], p["round"](), p["absout"], p["zeroed"]) >= E.TEETH, what
                raw = p["w"] if cls == "TB" else (p["inp0"] if p["inp1"] is None else torch.cat([p["inp0"], p["inp1"]], 1))
                assert E.split_bf16_exact(raw, 2) and all(E.split2h_exact(raw, 2.0 ** e) == (True, True) for e in (2, 6, 12, 13)), what
                for mode in E.MODES_T:
                    for with_table in (False, True) if E.conv_with_table(table, variant) else (False,):
                        _check_splits(what + (mode, with_table), p["loaded"], E.conv_scales(table, mode, p, with_table))
        E.clear_caches()
    assert left_out == E.CLASS_I_ONLY.get(table, set()), left_out


def test_dgrad_bnb_cases_are_exact_and_have_teeth():
    layouts = set()
    for idx, case in enumerate(E.TABLES["bnb"]):
        B, Cl, Co, bn_second, Cn, H, W, k, relu, x3 = case
        layouts.update(E.bnb_layouts(case))
        for cls in E.CONV_CLASSES:
            what = (case, cls)
            p = E.bnb_problem(idx, cls)
            assert p["d"] is not None and p["d"] >= E.MIN_DENSITY_EXISTING, what
            assert float(p["absout"].max()) / p["unit"] < E.BOUND and E.fp32_exact(p["g"]), what
            assert p["other"] is None or E.fp32_exact(p["other"]), what
            for t in (p["y"], p["ss"], p["mean"]):
                assert E.fp32_exact(t), what
            assert bool((p["mean"] * 2 == (p["mean"] * 2).round()).all()), what               # integers or halves
            if cls == "I":
                assert p["check_stats"], what                                                 # sum g and sum g (y - mean), per tile
                continue
            assert E.teeth(p["out"], p["round"](), p["absout"]) >= E.TEETH, what
            for mode in E.MODES_T:
                _check_splits(what + (mode,), p["loaded"], {})
        E.clear_caches()
    assert layouts == {0, 1, 2}


def test_the_scale_restatement():
    """x3_scale_from_amax: amax * S in [2^14, 2^15), a power of two; and what the issue states about A: two fp16 terms at 2^2, 2^6,
    2^12 and 2^13, no low term subnormal, two bf16 terms."""
    for amax in (1.0, 3.0 + 3.0 / 4096, 0.5, 9.0, 21.0, 1e-5, 3e4):
        s = E.scale_from_amax(amax)
        assert 2.0 ** 14 <= amax * s < 2.0 ** 15 and s == 2.0 ** round(__import__("math").log2(s)), amax
    assert E.scale_from_amax(0.0) == 1.0
    a = torch.tensor([i + j / 4096.0 for i in range(-3, 4) for j in range(-3, 4)], dtype=torch.float64)
    for e in (2, 6, 12, 13):
        assert E.split2h_exact(a, 2.0 ** e) == (True, True), e
    assert E.split_bf16_exact(a, 2) and not E.split_bf16_exact(a, 1)
    h0, h1 = E.split2h(a, 4.0)
    assert bool((h1 != 0).any()), "A must need its second term"
