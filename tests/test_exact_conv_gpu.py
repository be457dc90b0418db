"""The convolution kernels on operands they must get exactly right (tests/exact_cases.py; proved on the host by
test_exact_conv_cpu.py): forward, data gradient, the three weight-gradient families and the slab folds behind them, compared BIT FOR
BIT with an fp64 reference — no tolerance, in every arithmetic mode the operand class is exact in.  Outputs an entry point overwrites
start as a sentinel NaN, and so do the slabs: a pixel, tap, row, slab or cross product that is dropped, doubled or misplaced, a wrong
seam or a wrong scale-back changes bits somewhere and fails the case, whatever its magnitude."""
import contextlib

import pytest
import torch

import exact_cases as E
from test_kernels_gpu import ops, pack, DEV
from test_conv_x3_gpu import pack_x3, pack_x16, small_wide

pytestmark = pytest.mark.gpu


_DEV = {}


def dev(t):
    """fp32 device copy of a (cached, hence long-lived) host tensor of a problem, made once per test."""
    if t is None:
        return None
    c = _DEV.get(id(t))
    if c is None:
        c = _DEV[id(t)] = (t, t.float().contiguous().to(DEV))
    return c[1]


@pytest.fixture(autouse=True)
def _fresh_device_copies():
    _DEV.clear()
    yield
    _DEV.clear()
    E.clear_caches()


def differs(got, ref64, what, rows=False):
    """None when `got` holds the bits of the reference (compared on the device; the host-side proof has shown that the reference
    survives fp32), else the message of exact_cases.first_difference."""
    if not rows and got.shape == ref64.shape and torch.equal(got, dev(ref64)):
        return None
    return E.first_difference(got, ref64, what, rows)


def sentinel(*shape):
    return E.nan_fill(*shape).to(DEV)


@contextlib.contextmanager
def x3_terms(mode):
    """wtpse_x3_terms is process-global: set for the block, restored behind it."""
    L = ops().lib()
    was = L.query("wtpse_x3_terms", mode)
    try:
        yield
    finally:
        L.query("wtpse_x3_terms", was)


@contextlib.contextmanager
def x3r_enable(setting):
    L = ops().lib()
    L.query("wtpse_x3r_enable", setting)
    try:
        yield
    finally:
        L.query("wtpse_x3r_enable", 1)


def finish(failures):
    torch.cuda.synchronize()
    assert not failures, "%d call(s) not bit-exact:\n  %s" % (len(failures), "\n  ".join(failures[:12]))


# =============================================================================================== weight gradient
def run_wgrad(fam, p, v, ksplit=None):
    """One call through the C ABI with slabs and outputs of our own (sentinel NaN, or class-I integers under accumulate).
    -> (dw, db or None)"""
    o = ops()
    L = o.lib()
    B, C0, C1, Co, H, W = p["shape"]
    k, Cin = p["k"], C0 + C1
    n = Co * Cin * k * k
    x0, x1, pro0, pro1 = dev(p["x0"]), dev(p["x1"]), dev(p["pro0"]), dev(p["pro1"])
    pro_relu = 0 if v.pro is None else v.pro
    dw = dev(p["base"]).clone() if v.acc else sentinel(Co, Cin, k, k)
    db = (dev(p["base_b"]).clone() if v.acc else sentinel(Co)) if v.bias else None
    ptr, st = o.ptr, o.stream_ptr()
    if fam in ("fp32", "ksplit"):
        ns = ksplit or L.query("wtpse_wgrad_ksplit", B, H, W, Cin, Co)
    elif fam in ("x3", "x3tw32"):
        ns = L.query("wtpse_wgrad_x3_ksplit", B, H, W, Cin, Co)
    else:
        ns = L.query("wtpse_wgrad_r_slabs", B, H, W, Cin, Co)
    slab = sentinel(ns * n)
    dbs = sentinel(ns * Co) if v.bias else None
    if v.bn:
        g, y, coef = dev(p["g"]), dev(p["y"]), dev(p["coef"])
        L.call("wtpse_conv_wgrad_r_bn", ptr(g), ptr(y), ptr(coef), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), pro_relu, ptr(slab), ns,
               ptr(dw), int(v.acc), B, H, W, Co, st)
        return dw, db
    dy = dev(p["dy"])
    if fam in ("fp32", "ksplit"):
        L.call("wtpse_conv_wgrad", ptr(dy), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), pro_relu, ptr(slab), ptr(dbs), ns, ptr(dw),
               ptr(db), int(v.acc), B, H, W, Co, k, st)
    elif fam in ("x3", "x3tw32"):
        L.call("wtpse_conv_wgrad_x3", ptr(dy), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), pro_relu, ptr(slab), ns, ptr(dw), int(v.acc),
               B, H, W, Co, k, st)
    else:
        dya = o.amax_of(dy) if v.amax else None
        xa0 = o.amax_of(x0) if v.amax == "dyx" else None
        xa1 = o.amax_of(x1) if (v.amax == "dyx" and x1 is not None) else None
        L.call("wtpse_conv_wgrad_r", ptr(dy), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), pro_relu, ptr(slab), ptr(dbs), ns, ptr(dw),
               ptr(db), int(v.acc), B, H, W, Co, ptr(dya), ptr(xa0), ptr(xa1), st)
    return dw, db


def check_wgrad(fam, name, modes_of, ksplit=None):
    """Every class, variant and mode of one case; the failures of all calls in one message."""
    finish(wgrad_failures(fam, name, modes_of, ksplit))


def wgrad_failures(fam, name, modes_of, ksplit=None):
    shape, k, variants, classes = E.wgrad_case(fam, name)
    failures = []
    for cls in E.wgrad_classes(classes):
        for v in variants:
            p = E.wgrad_problem(fam, name, cls, v)
            for mode in modes_of(cls):
                if v.amax and mode != 2:
                    continue                                   # the amax tables matter to x2h only
                what = "%s %s class %s %s mode %s%s" % (fam, name, cls, E.vid(v), mode, "" if ksplit is None else " ksplit %d" % ksplit)
                with x3_terms(mode) if mode else contextlib.nullcontext():
                    dw, db = run_wgrad(fam, p, v, ksplit)
                f = differs(dw, p["dw"], what + ": dW (cout, cin, ky, kx)")
                if f:
                    failures.append(f)
                if v.bias and p["check_db"]:
                    f = differs(db, p["db"], what + ": dbias (cout)")
                    if f:
                        failures.append(f)
    return failures


def all_modes(cls):
    return E.MODES_I if cls == "I" else E.MODES_T


def current_mode(cls):
    return (0,)              # the fp32-input MFMA kernels do not look at the mode: whatever is on


@pytest.mark.parametrize("name", list(E.WG32_CASES))
def test_wgrad_fp32(name):
    check_wgrad("fp32", name, current_mode)


@pytest.mark.parametrize("ksplit", E.WG32_KSPLIT["ksplit18"][3])
def test_wgrad_fp32_explicit_ksplit(ksplit):
    """Any 1 <= ksplit <= tiles is legal at the C ABI: counts that do not divide the tiles, wgrad_reduce_k with fewer than 8 slabs and
    with a count 8 does not divide, the bias section behind the weight section."""
    check_wgrad("ksplit", "ksplit18", current_mode, ksplit)


@pytest.mark.parametrize("name", list(E.WGX3_CASES))
def test_wgrad_x3(name):
    check_wgrad("x3", name, all_modes)


@pytest.mark.parametrize("name", list(E.WGR_CASES))
def test_wgrad_r(name):
    check_wgrad("r", name, all_modes)


# =============================================================================================== forward / data gradient
def conv_call(entry, layout, p, wptr, in_amax=(None, None), grad_in=False):
    """One forward / data-gradient launch through the C ABI with sentinel outputs.  -> (out [B, C, H, W], stats rows or None, gram rows
    or None)"""
    o = ops()
    L = o.lib()
    B, C0, C1, Co, H, W, k = p["shape"]
    cout = (C0 + C1) if p["back"] else Co
    in0, in1 = dev(p["inp0"]), dev(p["inp1"])
    ptr, st = o.ptr, o.stream_ptr()
    want_stats = "stat_sum" in p
    bias, pro0, pro1, mask = dev(p["bias"]), dev(p["pro0"]), dev(p["pro1"]), dev(p["mask"])
    if entry == "wtpse_conv16_x3":
        out = sentinel(B, cout, H, W)
        rows = o._stats_blocks(2, B, H, W)
        stats = sentinel(rows, cout, 2) if want_stats else None
        gram = sentinel(rows, 256) if "gram" in p else None
        L.call(entry, ptr(in0), in0.shape[1], wptr, ptr(bias), ptr(pro0), p["pro_relu"], ptr(out), ptr(stats), ptr(gram), ptr(mask), 0, 0, 0,
               B, H, W, cout, int(p["relu_out"]), int(grad_in), ptr(in_amax[0]), 0, st)
        return out, stats, gram
    if p["split"] is None:
        out0, out1, csplit = sentinel(B, cout, H, W), None, cout
    else:
        csplit = p["split"]
        out0, out1 = sentinel(B, csplit, H, W), sentinel(B, cout - csplit, H, W)
    stats = sentinel(o._stats_blocks(layout, B, H, W, cout, k), cout, 2) if want_stats else None
    amax = (ptr(in_amax[0]), ptr(in_amax[1])) if layout == 1 else ()
    L.call(entry, ptr(in0), in0.shape[1], ptr(in1), 0 if in1 is None else in1.shape[1], wptr, ptr(bias), ptr(pro0), ptr(pro1), p["pro_relu"],
           ptr(out0), ptr(out1), csplit, ptr(stats), B, H, W, cout, k, int(p["relu_out"]), ptr(mask), *amax, 0, st)
    return (out0 if out1 is None else torch.cat([out0, out1], 1)), stats, None


def compare_conv(p, out, stats, gram, what, failures):
    B, C0, C1, Co, H, W, k = p["shape"]
    f = differs(out, p["out"], what + ": output (image, channel, row, column)")
    if f:
        failures.append(f)
    if stats is not None:
        assert stats.shape[0] * E.STAT_TILE >= B * H * W, (what, stats.shape)       # a row covers a tile of at most STAT_TILE pixels
        for col, key, ok in ((0, "stat_sum", p["check_sum"]), (1, "stat_sq", p["check_sq"])):
            if ok:
                f = differs(stats[:, :, col], p[key], what + ": statistics partials, %s (channel)" % key, rows=True)
                if f:
                    failures.append(f)
    if gram is not None and p["check_sq"]:
        G = gram.double().view(B, -1, 16, 16).sum(1).cpu()
        if not torch.equal(G, p["gram"]):
            failures.append(what + ": Gram partials differ in %d of %d entries" % (int((G != p["gram"]).sum()), G.numel()))


def amax_tables(p):
    o = ops()
    a0 = dev(p["inp0"])
    return (o.amax_of(a0), o.amax_of(dev(p["inp1"])) if p["inp1"] is not None else None)


def table_runs(table, variant, mode):
    """Without an amax table, and in mode 2 once more with the input's own from amax_of where the entry point takes one."""
    return (False, True) if (mode == 2 and E.conv_with_table(table, variant)) else (False,)


@pytest.mark.parametrize("idx", range(len(E.TABLES["conv"])))
def test_conv_fp32(idx):
    """CONV_CASES on the fp32-input MFMA path: forward (bias, statistics, output ReLU, prologue) and data gradient (split, mask)."""
    case = E.TABLES["conv"][idx]
    failures = []
    for variant in E.conv_variants("conv", case):
        for cls in E.conv_classes(variant):
            p = E.conv_problem("conv", idx, cls, variant)
            assert p["d"] is not None, (case, cls, variant)
            packed, wf, wd = pack(p["w"].float())
            out, stats, _ = conv_call("wtpse_conv_fwd", 0, p, packed.data_ptr() + 4 * (wd if p["back"] else wf))
            compare_conv(p, out, stats, None, "conv_fwd %s class %s %s" % (case, cls, variant), failures)
    finish(failures)


def _x3_tables():
    return [(t, i, c) for t in ("x3", "x3r", "x3half") for i in range(len(E.TABLES[t])) for c in E.CONV_CLASSES]


@pytest.mark.parametrize("table,idx,cls", _x3_tables())
def test_conv_x3(table, idx, cls):
    """X3_CASES, X3R_CASES (conv_x3r_k forced on every 3x3 launch / off) and X3_HALF_CASES (default / conv_x3r_k off) through
    wtpse_conv_fwd_x3 in every mode the class is exact in, every call of every case in every class (one test per class: the fp64
    references of the largest cases are the time); the weights are packed under the mode they are used in."""
    case = E.TABLES[table][idx]
    settings = {"x3": (1,), "x3r": (2, 0), "x3half": (1, 0)}[table]
    failures = []
    for variant in E.conv_variants(table, case):
        if cls not in E.conv_classes(variant):
            continue
        p = E.conv_problem(table, idx, cls, variant)
        assert p["d"] is not None, (table, case, cls, variant)
        for mode in all_modes(cls):
            with x3_terms(mode):
                packed, xf, xd = pack_x3(p["w"].float())
                for with_table in table_runs(table, variant, mode):
                    tabs = amax_tables(p) if with_table else (None, None)
                    for setting in settings:
                        with x3r_enable(setting):
                            out, stats, _ = conv_call("wtpse_conv_fwd_x3", 1, p, packed.data_ptr() + 2 * (xd if p["back"] else xf), tabs)
                        compare_conv(p, out, stats, None, "conv_fwd_x3 %s %s class %s %s mode %d x3r %d%s"
                                     % (table, case, cls, variant, mode, setting, " amax" if with_table else ""), failures)
    finish(failures)


def x3_failures(table, idx, cls, x3r_settings, sw_settings=(0,)):
    """Every variant of one case of an x3 table in one class through wtpse_conv_fwd_x3: every mode the class is exact in, with an amax
    table where the entry point takes one, under every wtpse_x3r_enable setting of x3r_settings and wtpse_x3_small_wide setting of
    sw_settings.  -> the first_difference messages."""
    case = E.TABLES[table][idx]
    failures = []
    for variant in E.conv_variants(table, case):
        if cls not in E.conv_classes(variant):
            continue
        p = E.conv_problem(table, idx, cls, variant)
        assert p["d"] is not None, (table, case, cls, variant)
        for mode in all_modes(cls):
            with x3_terms(mode):
                packed, xf, xd = pack_x3(p["w"].float())
                for with_table in table_runs("x3", variant, mode):
                    tabs = amax_tables(p) if with_table else (None, None)
                    for sw in sw_settings:
                        for setting in x3r_settings:
                            with x3r_enable(setting), small_wide(sw):
                                out, stats, _ = conv_call("wtpse_conv_fwd_x3", 1, p, packed.data_ptr() + 2 * (xd if p["back"] else xf), tabs)
                            compare_conv(p, out, stats, None, "conv_fwd_x3 %s %s class %s %s mode %d x3r %d small_wide %d%s"
                                         % (table, case, cls, variant, mode, setting, sw, " amax" if with_table else ""), failures)
    return failures


@pytest.mark.parametrize("idx,cls", [(i, c) for i in range(len(E.X3_SMALL_WIDE_CASES)) for c in E.CONV_CLASSES])
def test_conv_x3_small_wide(idx, cls):
    """X3_SMALL_WIDE_CASES: the 32-channel blocks on 32 x 4 tiles that only wtpse_x3_small_wide(1) reaches — conv_x3_k<KS, 1, 5, EPI, 1,
    TERMS> (wtpse_x3r_enable 1) and, for the 3x3 cases, conv_x3r_k<1, 1, 1, 5, ...> (2) — and the same calls with the switch off, so
    that a failure tells the tiling from the case."""
    B, C0, C1, Co, H, W, k = E.X3_SMALL_WIDE_CASES[idx]
    finish(x3_failures("x3sw", idx, cls, (1, 2) if k == 3 else (1,), (1, 0)))
    assert ops().lib().query("wtpse_x3_small_wide", -1) == 0


@pytest.mark.parametrize("idx,cls", [(i, c) for i in range(len(E.X3_K1_MT2_CASES)) for c in E.CONV_CLASSES])
def test_conv_x3_k1_mt2(idx, cls):
    """X3_K1_MT2_CASES: the 64-channel blocks on a 1x1 layer, conv_x3_k<1, 2, ...> — what up2.conv2 runs in the step at B = 32."""
    finish(x3_failures("x3k1", idx, cls, (1,)))


@pytest.mark.parametrize("case", E.BNB_SMALL_WIDE)
def test_dgrad_bnb_small_wide(case):
    """EPI 2 on the 32 x 4 tiles: the bnb cases on wide maps with W % 32 == 0 once more under wtpse_x3_small_wide(1), compared as
    test_dgrad_bnb compares them (masked gradient, other half, class-I partials through their fp64 sum)."""
    B, Cl, Co, bn_second, Cn, H, W, k, relu, x3 = case
    L = ops().lib()
    with small_wide(1):
        assert L.query("wtpse_conv_x3_stats_blocks", B, H, W, Cl + Co, k) == E.x3_tiling(B, H, W, Cl + Co, k, small_wide=1)["tiles"]
        assert E.x3_tiling(B, H, W, Cl + Co, k, small_wide=1)["small"] == 1 and x3
        test_dgrad_bnb(E.TABLES["bnb"].index(case))
    assert L.query("wtpse_x3_small_wide", -1) == 0


@pytest.mark.parametrize("idx", range(len(E.TABLES["x16"])))
def test_conv16_x3(idx):
    """X16_CASES: forward and gradient direction of the 16-channel kernel; a gradient input comes with grad_in — without a table it
    stays on x3, with amax_of it runs x2h in mode 2; Gram partials at 16 output channels."""
    case = E.TABLES["x16"][idx]
    failures = []
    for variant in E.conv_variants("x16", case):
        for cls in E.conv_classes(variant):
            p = E.conv_problem("x16", idx, cls, variant)
            assert p["d"] is not None, (case, cls, variant)
            for mode in all_modes(cls):
                with x3_terms(mode):
                    packed, xf, xd = pack_x16(p["w"].float())
                    for with_table in table_runs("x16", variant, mode):
                        tabs = amax_tables(p) if with_table else (None, None)
                        out, stats, gram = conv_call("wtpse_conv16_x3", 2, p, packed.data_ptr() + 2 * (xd if p["back"] else xf), tabs,
                                                     grad_in=p["back"])
                        compare_conv(p, out, stats, gram, "conv16_x3 %s class %s %s mode %d%s" % (case, cls, variant, mode, " amax" if with_table else ""),
                                     failures)
    finish(failures)


def bnb_call(layout, p, wptr, in_amax):
    """The data gradient with the BatchNorm-backward epilogue, without the in-launch tail.  -> (out0, out1 or None, stats)"""
    o = ops()
    L = o.lib()
    B, Cl, Co, bn_second, Cn, H, W, k, relu, _ = p["case"]
    Ct = Cl + Co
    du, y, ss, mean = dev(p["du"]), dev(p["y"]), dev(p["ss"]), dev(p["mean"])
    ptr, st = o.ptr, o.stream_ptr()
    if p["split"] is None:
        out0, out1, csplit = sentinel(B, Ct, H, W), None, Ct
    else:
        csplit = p["split"]
        out0, out1 = sentinel(B, csplit, H, W), sentinel(B, Ct - csplit, H, W)
    stats = sentinel(o._stats_blocks(layout, B, H, W, Ct, k), Cl, 2)
    if layout == 2:
        L.call("wtpse_conv16_x3", ptr(du), Cn, wptr, 0, 0, 0, ptr(out0), ptr(stats), 0, ptr(y), ptr(ss), ptr(mean), int(relu), B, H, W, Ct, 0, 1,
               ptr(in_amax), 0, st)
    elif layout == 1:
        L.call("wtpse_dgrad_x3_bnb", ptr(du), Cn, wptr, ptr(out0), ptr(out1), csplit, ptr(y), ptr(ss), ptr(mean), int(relu), p["c0"], p["c1"],
               ptr(stats), B, H, W, Ct, k, ptr(in_amax), st)
    else:
        L.call("wtpse_dgrad_bnb", ptr(du), Cn, wptr, ptr(out0), ptr(out1), csplit, ptr(y), ptr(ss), ptr(mean), int(relu), p["c0"], p["c1"],
               ptr(stats), B, H, W, Ct, k, st)
    return out0, out1, stats


@pytest.mark.parametrize("idx", range(len(E.TABLES["bnb"])))
def test_dgrad_bnb(idx):
    """The test_dgrad_bnb cases: the masked gradient, the other half of a split, and the partials sum g, sum g (y - mean) with an integer
    (or half) mean — layouts 0, 1 and, where the layer fits, 2; the statistics in class I (per tile inside the bound)."""
    case = E.TABLES["bnb"][idx]
    B, Cl, Co, bn_second, Cn, H, W, k, relu, _ = case
    failures = []
    for layout in E.bnb_layouts(case):
        for cls in E.CONV_CLASSES:
            p = E.bnb_problem(idx, cls)
            for mode in ((0,) if layout == 0 else all_modes(cls)):
                with x3_terms(mode) if mode else contextlib.nullcontext():
                    w = p["w"].float()
                    if layout == 0:
                        packed, _, off = pack(w)
                        wptr = packed.data_ptr() + 4 * off
                    else:
                        packed, _, off = pack_x3(w) if layout == 1 else pack_x16(w)
                        wptr = packed.data_ptr() + 2 * off
                    for with_table in ((False, True) if (mode == 2 and layout) else (False,)):
                        tab = ops().amax_of(dev(p["du"])) if with_table else None
                        out0, out1, stats = bnb_call(layout, p, wptr, tab)
                        what = "dgrad_bnb %s layout %d class %s mode %d%s" % (case, layout, cls, mode, " amax" if with_table else "")
                        g = out1 if (Co and bn_second) else out0
                        f = differs(g, p["g"], what + ": masked gradient (image, channel, row, column)")
                        if f:
                            failures.append(f)
                        if Co:
                            f = differs(out0 if bn_second else out1, p["other"], what + ": other half")
                            if f:
                                failures.append(f)
                        if cls == "I":
                            assert stats.shape[0] * E.STAT_TILE >= B * H * W, (what, stats.shape)
                            f = differs(stats, p["stats"], what + ": partials (channel, [sum g, sum g (y - mean)])", rows=True)
                            if f:
                                failures.append(f)
    finish(failures)
