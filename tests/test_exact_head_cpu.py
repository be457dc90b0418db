"""Host-side proof of tests/exact_head_cases.py.  Every case has the launch geometry it is listed for (the restated head_grid against
the library's host query); every stage of every chain and every compared per-workgroup partial stays inside the exactness bound
(sum of |products| + |bias| < 2^22 units); every operand splits into two exact, normal fp16 terms at the restated device scales;
every compared output a class-T setting reaches has teeth (at least 90 % of the outputs that can change do when A is rounded); each of
the 14 cross products of the x2h kernels is shown by some compared output; class I holds a few percent exact zeros on both ReLUs.
No GPU."""
import pytest
import torch

import exact_cases as E
import exact_head_cases as HC


@pytest.fixture(scope="module")
def L():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    build.build()                                   # no-op when up to date
    return lib()


@pytest.fixture(autouse=True)
def _drop_problems():
    yield
    HC.clear_caches()


def problems(name, classes=HC.SETTINGS):
    for cls in classes:
        for v in HC.HEAD_CASES[name][2]:
            yield cls, v, HC.head_problem(name, cls, v)


# =============================================================================================== geometry and variants
def test_cases_have_the_listed_geometry(L):
    geo = {}
    for name, ((B, H, W), expect, _, small) in HC.HEAD_CASES.items():
        g = geo[name] = HC.geometry(B, H, W)
        for key, val in expect.items():
            assert g[key] == val, (name, key, g[key])
        assert g["slabs"] == g["grid"] == L.query("wtpse_head_slabs", B, H * W), name
        assert not small or (g["wg_pixels"] == 128 and g["rounds"] == 1), name
    for nblk in (1, 4, 5, 2047, 2048, 2049, 4100, 10 ** 6):           # head_grid off the table too
        assert HC.head_grid(nblk) == L.query("wtpse_head_slabs", 1, 32 * nblk), nblk
    # the fold: 1 slab, fewer than 8, exactly 8, 8 k + 1, 512
    assert [g["slabs"] for g in geo.values()] == [1, 1, 2, 7, 8, 9, 512, 512, 512]
    # waves without a block (they still zero their share of the slab), every wave busy exactly once, two and three rounds
    assert geo["b1"]["idle_waves"] == 3 and geo["b1"]["one_block_waves"] == 1
    assert geo["cap"]["one_block_waves"] == 2048 and geo["cap+4"]["one_block_waves"] == 2044 and geo["3rounds"]["one_block_waves"] == 0
    assert geo["cap+4"]["wg_pixels"] == 256 and geo["3rounds"]["wg_pixels"] == 384
    # 3rounds: block 2050, the first of image 1, is wave 2's second block in workgroup 0
    g = geo["3rounds"]
    assert g["bpi"] + 0 == 2050 and 2050 - g["stride"] == 2 and 4096 + 3 < g["nblk"] <= 4096 + 4


def test_variants_cover_every_axis_on_every_kernel():
    """Every value of every axis with the two-layer AND the three-layer instantiation (each variant runs in modes 3 and 2: the fp32-input
    and the x2h kernel, forward and backward); nc = 1 .. 4; the large cases one variant of each head."""
    vs = [v for _, _, variants, _ in HC.HEAD_CASES.values() for v in variants]
    for three in (False, True):
        mine = [v for v in vs if (v.nc > 0) == three]
        assert {v.pro for v in mine} == {None, 0, 1}, three
        assert {v.acc for v in mine} == {False, True}, three
    assert {v.nc for v in vs} == {0, 1, 2, 3, 4}
    small = [v for _, _, variants, s in HC.HEAD_CASES.values() if s for v in variants]
    assert {v.nc for v in small} == {0, 1, 2, 3, 4} and {v.pro for v in small} == {None, 0, 1} and {v.acc for v in small} == {False, True}
    for name, (_, _, variants, s) in HC.HEAD_CASES.items():
        assert s or sorted(v.nc > 0 for v in variants) == [False, True], name
    assert HC.HEAD_CASES[HC.MODE1_CASE][3]
    assert any(v.nc == HC.HEAD_MAXNC for v in HC.HEAD_CASES["3rounds"][2] + HC.HEAD_CASES["cap+4"][2] + HC.HEAD_CASES["cap"][2])


# =============================================================================================== exactness, splits, teeth, zeros
@pytest.mark.parametrize("name", list(HC.HEAD_CASES))
def test_cases_are_exact_split_exactly_and_have_teeth(name):
    small = HC.HEAD_CASES[name][3]
    for cls, v, p in problems(name):
        what = (name, cls, HC.hvid(v))
        if what in HC.CLASS_I_ONLY:
            assert p["d"] is None, what
            continue
        assert p["d"] is not None, what + ("no density keeps the case inside the bound with teeth",)
        r, o, units, check = p["r"], p["o"], p["units"], p["check"]
        # ---- exactness: every stage of the chain, and every compared output's own sums (y; the per-workgroup partials)
        for k in HC.STAGES:
            assert units[k] < 1.0, what + (k, units[k])
        for k, on in check.items():
            assert not on or k not in HC.OWN_SUM or units[k] < 1.0, what + (k,)
        for k in ("h1", "h2", "dx") + (("y",) if (v.nc and check["y"]) else ()):
            assert check[k] and E.fp32_exact(r[k]), what + (k,)
        for t in (p["x"], p["pro"], o["xa"], o["w1"], o["b1"], o["w2"], o["b2"], o["w3"], o["b3"], o["dy"], p["base"]):
            assert t is None or E.fp32_exact(t), what
        # ---- what is compared: everything in class I; forward and dx everywhere (y not in TW2: see exact_head_cases._requirements)
        if cls == "I":
            assert all(check.values()) and not p["why"], what + (p["why"],)
            assert all(E.split_bf16_exact(o[k], 1) for k in ("xa", "w1", "w2", "dy")), what
        else:
            assert check.get("y", True) or cls == "TW2" or p["why"]["y"] == "bound", what
            assert small or not any(check[k] for k in HC.PARAM_OUT if k in check), what
            a = {"x": p["x"], "dy": o["dy"], "w1": o["w1"], "w2": o["w2"]}[HC.A_OF[cls]]
            assert bool(((a - a.round()) != 0).all()), what                 # every element of A carries a low part
            # ---- teeth: every compared output A reaches
            for k in HC.DEPENDS[cls]:
                if check.get(k):
                    assert p["share"][k] is not None and p["share"][k] >= E.TEETH, what + (k, p["share"][k])
        # ---- splits at the restated scales: with the amax tables always; without x_amax in class I always, in class T where they hold
        assert p["scales"][True]["robust"] and p["scales"][False]["robust"], what
        for k, (exact, normal) in p["splits"][True].items():
            assert exact and normal, what + (k, p["scales"][True])
        assert p["notable"] or cls in ("TX", "TW1"), what                    # (only h1 * sh fails there: sh follows xbound = 8192)
        assert p["notable"] or [k for k, (e, n) in p["splits"][False].items() if not (e and n)] == ["h1"], what
        # ---- zeros on the masks: class I, pre-activations of h1 and (three-layer heads) of h2
        if cls == "I":
            for k in ("a1",) + (("a2",) if v.nc else ()):
                assert float((r[k] == 0).double().mean()) >= HC.ZERO_SHARE, what + (k,)


def test_every_cross_product_is_shown_by_a_compared_output():
    """The 14 places: each has a (small case, setting, variant, compared output) whose reference changes in at least 90 % of the elements
    that can change when that product alone loses the operand's low fp16 term.  The four accW operands and the layer-1-again products
    are shown by the parameter gradients, which class T compares in the small cases only."""
    shown = {pl: [] for pl in HC.PLACES}
    for name, (_, _, _, small) in HC.HEAD_CASES.items():
        if not small:
            continue
        for cls, v, p in problems(name, HC.SETTINGS[1:]):
            if p["d"] is None:
                continue
            for pl, (setting, _, _, outs, _) in HC.PLACES.items():
                if setting != cls or not any(p["check"].get(k) for k in outs):
                    continue
                _, share = HC.perturbed(p, pl)
                shown[pl] += [(name, HC.hvid(v), k) for k in outs if p["check"].get(k) and share.get(k) is not None and share[k] >= E.TEETH]
        HC.clear_caches()
    assert len(HC.PLACES) == 14 and sorted(pl[:2] for pl in HC.PLACES) == sorted(t for t in ("f1", "f2", "r1", "d3", "d4", "w1", "w2") for _ in "AB")
    for pl, where in shown.items():
        assert where, pl
        if pl in HC.SLAB_PLACES:
            assert {k for _, _, k in where} <= set(HC.PARAM_OUT), pl
        assert len({n for n, _, _ in where}) >= 2, (pl, where)               # in more than one geometry


def test_the_scale_restatement():
    """head_scales on operands small enough to do by hand: dense |W1| <= 3 without a table — rows of up to 96, times xbound = 8192, is
    below 2^20: sh = 2^-5; the table's sx follows the data; dy's amax times W3's largest column sum, then W2's."""
    o = {"w1": torch.full((32, 32), 3.0, dtype=torch.float64), "b1": torch.full((32,), -3.0, dtype=torch.float64),
         "w2": torch.full((8, 32), -2.0, dtype=torch.float64), "w3": torch.tensor([[1.0] * 8, [-3.0] * 8], dtype=torch.float64),
         "dy": torch.full((1, 2, 32), 1.5, dtype=torch.float64)}
    x = torch.full((1, 32, 32), 3.0, dtype=torch.float64)
    s = HC.head_scales(o, None, x, None, False)
    assert (s["sx"], s["sw1"], s["sw2"], s["sh"]) == (4.0, 2.0 ** 13, 2.0 ** 13, 2.0 ** -5)
    assert s["sd2"] == 2.0 ** 12 and s["sd1"] == 2.0 ** 8                    # 1.5 * 4 = 6 -> 2^12; 6 * 16 = 96 -> 2^8
    s = HC.head_scales(o, None, x, None, True)
    assert s["sx"] == 2.0 ** 13 and s["sh"] == 2.0 ** 6                      # 96 * 3 + 3 = 291 -> 2^6
    pro = torch.tensor([[2.0, -1.0]] * 32, dtype=torch.float64)
    assert HC.head_scales(o, None, x, pro, True)["sx"] == 2.0 ** 12          # act_bound: 2 * 3 + 1 = 7
    assert HC.head_scales(dict(o, w3=None), None, x, None, True)["sd2"] == 2.0 ** 14
    assert HC.head_ns(0) == 1320 and HC.head_ns(4) == 1356 and HC.sections(3)[-1] == ("db3", 1320 + 24, (3,))
