"""Case tables, seeded operands, the fp64 reference chain and a Python restatement of the launch geometry and of the device-side
scale derivation for the exact-arithmetic tests of the fused 1x1 heads (csrc/head.hip; profiles/exact_head.md is the table in prose).
The machinery is exact_cases.py's, extended to a CHAIN: 32 -> 32 (ReLU) -> 8 [-> (ReLU) -> nc] forward, and backward through it with
four more power-of-two scales derived on the device.  Imports neither the product nor the GPU: test_exact_head_cpu.py proves the
tables on the host, test_exact_head_gpu.py runs them and compares BITS.

  class I   every operand an integer, |v| <= 3 (prologue scale from {1, 2, -1, 0.5}, integer shift); the weights of layers 1 and 2
            are kept at the densities I_DENSITY so that a few percent of the pre-activations of h1 AND of h2 are exactly 0 — the
            test of the ReLU masks (the x2h backward takes the mask of h1 from an h1 it forms again)
  class T   exactly one tensor is "A" = i + j / 4096 (every element with a low part): TX x, TD dy, TW1 W1, TW2 W2; x, W1, W2 and dy
            are otherwise integers kept with probability d (the largest of DENSITIES that keeps every checked sum inside the bound);
            W3 and the biases are dense integers.  A x A is not exact, so a chain needs the four settings; together they put a low part
            on either side of each of the seven MFMA triples of the x2h kernels (PLACES)."""
import functools
import math
from collections import namedtuple

import torch

from dispatch_cases import ceil_div
from exact_cases import BOUND, DENSITIES, TEETH, UNIT_T, ints, operand, pro_table, scale_from_amax, seed_of, split2h_exact

HEAD_MAXNC = 4
X_FIXED_SCALE, X_FIXED_BOUND = 4.0, 8192.0          # head_*_h_k without x_amax: X3_FWD_SCALE and 32768 / X3_FWD_SCALE
# class I: share of W1 / W2 kept.  A pre-activation is a sum of n products of variance s^2: it is exactly 0 with probability about
# 1 / sqrt(2 pi n s^2) — dense layers (n = 32) give 1.8 % for h1 and 0.3 % for h2; with about 3.4 and 1.7 non-zero weights per row and the
# small h1 that follows, both shares are a few percent in most draws (_operands keeps a draw that has them).  x and dy stay dense: the
# geometry is theirs.
I_DENSITY = {"w1": 0.125, "w2": 0.0625}
ZERO_SHARE = 0.02                                   # "a few percent": at least 2 % of the pre-activations exactly 0, in every class-I problem

# HV: one head and how it is called.  nc: 0 the two-layer head, 1..4 the three-layer head's output channels; pro: None no prologue,
# 0 affine, 1 affine + ReLU; acc: accumulate onto class-I integers (else dparams starts as the sentinel NaN)
HV = namedtuple("HV", "nc pro acc")


def hvid(v):
    return "%s-%s%s" % ("L2" if v.nc == 0 else "L3nc%d" % v.nc, {None: "nopro", 0: "affine", 1: "affine+relu"}[v.pro], "-acc" if v.acc else "")


# name -> ((B, H, W), expected subset of geometry(), variants, small).  small: a workgroup owns at most 128 pixels — the cases whose
# class-T calls compare the parameter gradients as well (the per-workgroup partials of the large cases leave the bound in class T)
HEAD_CASES = {
    "b1":      ((1, 4, 8), {"nblk": 1, "grid": 1, "idle_waves": 3, "rounds": 1}, (HV(0, None, False), HV(1, 1, True), HV(4, 0, False)), True),
    "b3":      ((3, 4, 8), {"nblk": 3, "grid": 1, "bpi": 1, "idle_waves": 1}, (HV(0, 0, True), HV(2, 1, False), HV(4, None, True)), True),
    "b5":      ((1, 10, 16), {"nblk": 5, "grid": 2, "last_wg_busy": 1}, (HV(0, 1, False), HV(3, 0, True), HV(4, 1, False)), True),
    "b28":     ((1, 28, 32), {"nblk": 28, "grid": 7, "fold_empty_groups": 1}, (HV(0, None, True), HV(1, 0, False)), True),
    "b32":     ((2, 16, 32), {"nblk": 32, "grid": 8, "fold_empty_groups": 0, "fold_trips": (1, 1)}, (HV(2, None, False), HV(0, 1, True)), True),
    "b33":     ((3, 11, 32), {"nblk": 33, "grid": 9, "bpi": 11, "wg_straddles_image": True, "fold_trips": (1, 2)},
                (HV(3, 1, True), HV(4, 0, False), HV(0, None, False)), True),
    "cap":     ((2, 128, 256), {"nblk": 2048, "grid": 512, "rounds": 1, "idle_waves": 0, "blocks_per_wave": (1, 1)},
                (HV(0, None, False), HV(4, 1, True)), False),
    "cap+4":   ((3, 171, 128), {"nblk": 2052, "grid": 512, "rounds": 2, "blocks_per_wave": (1, 2), "waves_with_most": 4, "wave_changes_image": True,
                                "second_round_images": (2, 2), "first_round_image_wg0": 0}, (HV(0, 1, True), HV(4, None, False)), False),
    "3rounds": ((2, 100, 656), {"nblk": 4100, "grid": 512, "rounds": 3, "blocks_per_wave": (2, 3), "waves_with_most": 4, "bpi": 2050,
                                "second_round_images": (0, 1), "wave_changes_image": True}, (HV(0, 0, False), HV(3, 1, True)), False),
}
MODE1_CASE = "b5"                      # one small case in mode 1 as well: its class-T calls are exact only on the fp32-input kernels (one bf16 term is not)
# (case, setting, variant id) no density keeps inside the bound with teeth: class I only
CLASS_I_ONLY = {("b1", "TW2", "L3nc1-affine+relu-acc")}
SETTINGS = ("I", "TX", "TD", "TW1", "TW2")
A_OF = {"TX": "x", "TD": "dy", "TW1": "w1", "TW2": "w2"}
FWD_OUT, BWD_OUT = ("y", "h2", "h1"), ("dx", "dW1", "db1", "dW2", "db2", "dW3", "db3")
PARAM_OUT = BWD_OUT[1:]
# what a class-T setting can move at all: the outputs with a product of A (or of something derived from A) in them
DEPENDS = {"TX": ("h1", "h2", "y", "dW1", "dW2", "dW3"), "TD": ("dx", "dW1", "db1", "dW2", "db2", "dW3", "db3"),
           "TW1": ("h1", "h2", "y", "dx", "dW2", "dW3"), "TW2": ("h2", "y", "dx", "dW1", "db1", "dW3")}
# the 14 cross products of the x2h kernels: place -> (setting that puts a low part there, the operand [key of the chain's result] and
# its scale, the outputs that show it, what it is in csrc/head.hip).  Side A is the MFMA's first operand.
PLACES = {
    "f1B": ("TX", "xa", "sx", ("h1", "h2", "y"), "head_fwd_h_k acc1: A1[s][0] x B1[s][1]"),
    "f2B": ("TX", "h1", "sh", ("h2", "y"), "head_fwd_h_k acc2: A2[s][0] x B2[s][1] (h1 carries the low part)"),
    "r1B": ("TX", "xa", "sx", ("dW2",), "head_bwd_h_k acc1 (layer 1 again): A1[s][0] x B1[s][1]"),
    "w1B": ("TX", "xa", "sx", ("dW1",), "head_bwd_h_k accW1: qa[0] x qb[1] (Tx)"),
    "w2B": ("TX", "h1", "sh", ("dW2",), "head_bwd_h_k accW2: qa[0] x qb[1] (Th1)"),
    "d3B": ("TD", "dh2", "sd2", ("dx", "dW1", "db1"), "head_bwd_h_k acc3: A2T[0] x Bd2[1]"),
    "d4B": ("TD", "dh1", "sd1", ("dx",), "head_bwd_h_k acc4: A1T[s][0] x Bd1[s][1]"),
    "w1A": ("TD", "dh1", "sd1", ("dW1",), "head_bwd_h_k accW1: qa[1] x qb[0] (Tdh1)"),
    "w2A": ("TD", "dh2", "sd2", ("dW2",), "head_bwd_h_k accW2: qa[1] x qb[0] (Tdh2)"),
    "f1A": ("TW1", "w1", "sw1", ("h1", "h2", "y"), "head_fwd_h_k acc1: A1[s][1] x B1[s][0]"),
    "r1A": ("TW1", "w1", "sw1", ("dW2",), "head_bwd_h_k acc1 (layer 1 again): A1[s][1] x B1[s][0]"),
    "d4A": ("TW1", "w1", "sw1", ("dx",), "head_bwd_h_k acc4: A1T[s][1] x Bd1[s][0]"),
    "f2A": ("TW2", "w2", "sw2", ("h2", "y"), "head_fwd_h_k acc2: A2[s][1] x B2[s][0]"),
    "d3A": ("TW2", "w2", "sw2", ("dx", "dW1", "db1"), "head_bwd_h_k acc3: A2T[1] x Bd2[0]"),
}
SLAB_PLACES = ("r1A", "r1B", "w1A", "w1B", "w2A", "w2B")         # seen through the parameter gradients only: the small cases


# =============================================================================================== launch geometry, restated
def head_grid(nblk):
    """head_grid (csrc/head.hip): workgroups of four waves, one 32-pixel block per wave and round, at most 512 workgroups."""
    return max(1, min(ceil_div(nblk, 4), 512))


def geometry(B, H, W):
    """What the strided block loop `for (blk = 4 * wg + wave; blk < nblk; blk += 4 * grid)` does on a shape."""
    assert (H * W) % 32 == 0
    bpi = H * W // 32
    nblk = B * bpi
    grid = head_grid(nblk)
    stride = 4 * grid
    blocks = [len(range(w, nblk, stride)) for w in range(stride)]
    most = max(blocks)
    second = [(w + stride) // bpi for w in range(stride) if w + stride < nblk]
    slabs = grid
    trips = [len(range(kq, slabs, 8)) for kq in range(8)]               # head_fold_k: lane group kq adds slabs kq, kq + 8, ...
    return {"bpi": bpi, "nblk": nblk, "grid": grid, "stride": stride, "rounds": ceil_div(nblk, stride), "idle_waves": blocks.count(0),
            "blocks_per_wave": (min(blocks), most), "waves_with_most": blocks.count(most), "last_wg_busy": sum(1 for b in blocks[-4:] if b),
            "wg_straddles_image": any((4 * g) // bpi != min(4 * g + 3, nblk - 1) // bpi for g in range(grid)),
            "wave_changes_image": any(w // bpi != (w + stride) // bpi for w in range(stride) if w + stride < nblk),
            "second_round_images": (min(second), max(second)) if second else None, "first_round_image_wg0": 0,
            "one_block_waves": blocks.count(1),         # their only prefetch is past the end: clamped to the last block, never used
            "wg_pixels": 4 * ceil_div(nblk, stride) * 32, "slabs": slabs, "fold_empty_groups": trips.count(0),
            "fold_trips": (min(trips), max(trips))}


def head_ns(nc):
    """Floats of dparams / of one slab: dW1 [32][32] | db1 [32] | dW2 [8][32] | db2 [8] | dW3 [nc][8] | db3 [nc]."""
    return 1024 + 32 + 256 + 8 + 9 * nc


def sections(nc):
    """-> [(name, offset, shape)] of dparams."""
    out, off = [], 0
    for name, shape in (("dW1", (32, 32)), ("db1", (32,)), ("dW2", (8, 32)), ("db2", (8,))) + ((("dW3", (nc, 8)), ("db3", (nc,))) if nc else ()):
        out.append((name, off, shape))
        off += math.prod(shape)
    assert off == head_ns(nc)
    return out


# =============================================================================================== the chain in fp64
def _mm(w, t):
    return torch.einsum("mk,bkp->bmp", w, t)


def _outer(a, b):
    return torch.einsum("bmp,bkp->mk", a, b)


def _col(b):
    return b.view(1, -1, 1)


ONES = {"m1": 1.0, "m2": 1.0, "m1r": 1.0}


def chain(o, masks=None, sub=None):
    """Forward and backward of one head on [B, C, HW] tensors.  o: xa (the ACTIVATED input: the gradient is with respect to it), w1, b1,
    w2, b2, w3, b3 (None: two layers), dy.  masks: None — the ReLUs, by `> 0` on the fp64 values; or {m1, m2, m1r} to multiply with
    instead (ONES: the chain on absolute values).  sub: {place of PLACES: f(operand) -> the operand to use in THAT product}.
    m1r / h1r: layer 1 as the x2h backward forms it again — the same numbers unless a product of that triple is tampered with."""
    sub = sub or {}

    def g(place, v):
        f = sub.get(place)
        return v if f is None else f(v)

    three = o["w3"] is not None
    r = {}
    a1 = _mm(g("f1A", o["w1"]), g("f1B", o["xa"])) + _col(o["b1"])
    m1 = (a1 > 0) if masks is None else masks["m1"]
    h1 = a1 * m1
    a2 = _mm(g("f2A", o["w2"]), g("f2B", h1)) + _col(o["b2"])
    if three:
        m2 = (a2 > 0) if masks is None else masks["m2"]
        h2 = a2 * m2
        r["y"] = _mm(o["w3"], h2) + _col(o["b3"])
    else:
        m2, h2 = None, a2
    if "r1A" in sub or "r1B" in sub:
        a1r = _mm(g("r1A", o["w1"]), g("r1B", o["xa"])) + _col(o["b1"])
        m1r = (a1r > 0) if masks is None else masks["m1r"]
        h1r = a1r * m1r
    else:
        m1r, h1r = m1, h1
    dy = o["dy"]
    dh2 = _mm(o["w3"].t(), dy) * m2 if three else dy
    acc3 = _mm(g("d3A", o["w2"]).t(), g("d3B", dh2))
    dh1 = acc3 * m1r
    r.update(a1=a1, m1=m1, h1=h1, a2=a2, m2=m2, h2=h2, m1r=m1r, h1r=h1r, dh2=dh2, acc3=acc3, dh1=dh1, xa=o["xa"], w1=o["w1"], w2=o["w2"],
             dx=_mm(g("d4A", o["w1"]).t(), g("d4B", dh1)),
             dW1=_outer(g("w1A", dh1), g("w1B", o["xa"])), db1=dh1.sum((0, 2)),
             dW2=_outer(g("w2A", dh2), g("w2B", h1r)), db2=dh2.sum((0, 2)))
    if three:
        r.update(dW3=_outer(dy, h2), db3=dy.sum((0, 2)))
    return r


def activated(x, pro, relu):
    v = x if pro is None else x * pro[:, 0].view(1, -1, 1) + pro[:, 1].view(1, -1, 1)
    return torch.relu(v) if relu else v


def _abs(o):
    return {k: (None if t is None else t.abs()) for k, t in o.items()}


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float64).float())


def _topk_sum(flat, k):
    return flat.topk(min(k, flat.shape[1]), dim=1).values.sum(1)


def wg_bound(a, b, npix, limit):
    """No workgroup's partial of sum_px |a[m][px]| |b[c][px]| (b None: of sum_px |a[m][px]|) can be larger than this: the sum of the
    npix largest terms, npix = the pixels one workgroup can own.  Past `limit` by the cheap form (the npix largest of one factor times
    the largest of the other), the sums of the npix largest products themselves are formed."""
    af = a.transpose(0, 1).reshape(a.shape[1], -1)
    if b is None:
        return float(_topk_sum(af, npix).max())
    bf = b.transpose(0, 1).reshape(b.shape[1], -1)
    if af.shape[1] <= npix:
        return float((af @ bf.t()).max())
    cheap = min(float(_topk_sum(af, npix).max() * bf.max()), float(af.max() * _topk_sum(bf, npix).max()))
    if cheap < limit:
        return cheap
    return max(float(_topk_sum(af[m:m + 1] * bf, npix).max()) for m in range(af.shape[0]))


def stage_units(ra, unit):
    """Largest sum of |products| + |bias| of every stage of the chain on absolute values, in units of BOUND."""
    keys = ("a1", "a2", "dh2", "acc3", "dx") + (("y",) if "y" in ra else ())
    return {k: float(ra[k].max()) / unit / BOUND for k in keys}


def slab_units(ra, oa, npix, unit):
    """The same for the per-workgroup fp32 partials of the parameter gradients (the fold behind them adds in fp64 and rounds once)."""
    lim = BOUND * unit
    u = {"dW1": wg_bound(ra["dh1"], oa["xa"], npix, lim), "db1": wg_bound(ra["dh1"], None, npix, lim),
         "dW2": wg_bound(ra["dh2"], ra["h1"], npix, lim), "db2": wg_bound(ra["dh2"], None, npix, lim)}
    if oa["w3"] is not None:
        u.update(dW3=wg_bound(oa["dy"], ra["h2"], npix, lim), db3=wg_bound(oa["dy"], None, npix, lim))
    return {k: v / unit / BOUND for k, v in u.items()}


# =============================================================================================== the device's scales, restated
def head_scales(o, r, x_raw, pro, table):
    """The power-of-two scales head_fwd_h_k / head_bwd_h_k derive (every wave for itself, in registers: nothing on the host can read
    them back — the bit comparison on the GPU is the check of this restatement).  table: x_amax / dy_amax as the step passes them
    (amax_of(x) for a raw input, act_bound(pro, amax_of(x)) behind a prologue) or x_amax = None (the fixed scale).
    -> {sx, sw1, sw2, sh, sd2, sd1, robust}: robust = no bound sits so close to a power of two that fp32 rounding (or a fused
    multiply-add) of its formula could move its exponent."""
    robust = True

    def bound(exact):
        nonlocal robust
        v = _f32(exact)
        robust = robust and (exact == 0 or math.frexp(v)[1] == math.frexp(exact)[1])
        return v

    s = {"sw1": scale_from_amax(float(o["w1"].abs().max())), "sw2": scale_from_amax(float(o["w2"].abs().max()))}
    if table:
        xam = float(x_raw.abs().max())
        if pro is not None:                            # act_bound_k: max_c |scale_c| * amax + |shift_c|
            xam = max(bound(abs(float(pro[c, 0])) * xam + abs(float(pro[c, 1]))) for c in range(pro.shape[0]))
        s["sx"], xbound = scale_from_amax(xam), xam
    else:
        s["sx"], xbound = X_FIXED_SCALE, X_FIXED_BOUND
    hbound = bound(float(o["w1"].abs().sum(1).max()) * xbound + float(o["b1"].abs().max()))
    s["sh"] = scale_from_amax(hbound)
    c3 = float(o["w3"].abs().sum(0).max()) if o["w3"] is not None else 1.0
    d2bound = bound(float(o["dy"].abs().max()) * c3)
    s["sd2"] = scale_from_amax(d2bound)
    s["sd1"] = scale_from_amax(bound(float(o["w2"].abs().sum(0).max()) * d2bound))
    s["robust"] = robust
    return s


# the operands as the matrix cores see them (the four transpose tiles Tdh1, Tx, Th1, Tdh2 and the transposed weights A1T, A2T hold the
# same values at the same scales): key of the chain's result -> scale
SPLIT_OPERANDS = {"xa": "sx", "w1": "sw1", "w2": "sw2", "h1": "sh", "dh2": "sd2", "dh1": "sd1"}


def splits_hold(r, s):
    """{operand: (exact, normal)} of split2h_exact at the restated scales."""
    return {k: split2h_exact(r[k], s[sk]) for k, sk in SPLIT_OPERANDS.items()}


def high_term(v, scale):
    """The operand with its low fp16 term dropped: what a product computes when the cross product with that low term is missing."""
    return (v * scale).float().half().double() / scale


# =============================================================================================== problems
def _operands(name, cls, v, d, salt=None):
    (B, H, W), _, _, _ = HEAD_CASES[name]
    sd = seed_of("head", name, cls, hvid(v))
    P = H * W
    three = v.nc > 0
    if cls == "I" and salt is None:
        # the weights and biases of layers 1 and 2 are drawn again until both ReLUs see their share of exact zeros (eight rows of W2 are
        # a small sample: one draw in three misses it) — looked for on the first pixels, asserted on all of them by the host test
        for salt in range(64):
            x, pro, o = _operands(name, cls, v, d, salt)
            n = max(1, min(B, 8192 // P))
            a1 = _mm(o["w1"], o["xa"][:n, :, :8192]) + _col(o["b1"])
            a2 = _mm(o["w2"], torch.relu(a1)) + _col(o["b2"])
            if min(float((a1 == 0).double().mean()), float((a2 == 0).double().mean()) if three else 1.0) >= 1.5 * ZERO_SHARE:
                return x, pro, o
        raise AssertionError("no draw of the class-I weights of %s %s has the zeros" % (name, hvid(v)))
    sw = sd + 1000 * (salt or 0)

    def make(t, shape, k):
        if cls == "I":
            return operand("B", shape, k, I_DENSITY[t]) if t in I_DENSITY else ints(shape, k)
        if cls == "TW2" and t == "x":
            return ints(shape, k)                   # x multiplies nothing of A there; dense, it keeps h1 from being the same at every pixel
        return operand("A" if A_OF[cls] == t else "B", shape, k, d)

    x = make("x", (B, 32, P), sd + 1)
    pro = pro_table(32, sd + 9, shift=cls == "I") if v.pro is not None else None
    o = {"xa": activated(x, pro, bool(v.pro)), "w1": make("w1", (32, 32), sw + 2), "b1": ints((32,), sw + 4), "w2": make("w2", (8, 32), sw + 3),
         "b2": ints((8,), sw + 5), "w3": ints((v.nc, 8), sd + 6) if three else None, "b3": ints((v.nc,), sd + 7) if three else None,
         "dy": make("dy", (B, v.nc if three else 8, P), sd + 8)}
    return x, pro, o


# the sums an output needs inside the bound besides the stages every call needs (a1, a2, dh2, acc3, dx): its own
OWN_SUM = ("y",) + PARAM_OUT
STAGES = ("a1", "a2", "dh2", "acc3", "dx")


def _requirements(cls, small):
    """What the density of a class-T problem is chosen for, in this order of preference: every sum of every output; without the
    per-workgroup partials of the bias and W3 gradients; without any partial; without y (TW2: W2 is dense there, and the chain on
    absolute values through |b1|, |W2| and a dense W3 leaves the bound at every density)."""
    full = STAGES + ("y",)
    if cls == "I":
        return (full + PARAM_OUT,)
    return ((full + PARAM_OUT, full + ("dW1", "dW2")) if small else ()) + (full, STAGES)


@functools.lru_cache(maxsize=None)
def head_problem(name, cls, v):
    """Operands and fp64 references of one (case, setting, variant).  -> dict: x (raw, [B, 32, HW]), pro, o (the chain's operands), r (the
    chain's result: the references), base (accumulate: class-I integers [ns]), dparams (float32: float32(exact sum), with the base added
    in fp32), d, unit, units (every checked sum / BOUND), check (output -> it is compared: its sums are inside the bound and, where the
    setting's A reaches it, it has teeth), why (output left out -> "bound" / "teeth" / "large case": class T compares no
    parameter gradient there, their partials are not looked at), share (class T: output -> share of the outputs
    that can change which do when A is rounded), scales / splits (with the amax tables: True, without: False), notable (the operands split
    exactly without x_amax too: the call runs in mode 2 with x_amax = None as well), geo."""
    (B, H, W), _, _, small = HEAD_CASES[name]
    geo = geometry(B, H, W)
    unit = 1.0 if cls == "I" else UNIT_T
    three = v.nc > 0
    out = {"d": None, "unit": unit, "geo": geo, "name": name, "cls": cls, "v": v, "shape": (B, H, W)}

    def attempt(d, req):
        x, pro, o = _operands(name, cls, v, d)
        oa = _abs(o)
        ra = chain(oa, masks=ONES)
        units = stage_units(ra, unit)
        if max(units[k] for k in req if k in units) >= 1.0:
            return None
        if cls == "I" or small:
            units.update(slab_units(ra, oa, geo["wg_pixels"], unit))
        if max(units.get(k, 0.0) for k in req) >= 1.0:
            return None
        inside = {k: (k not in OWN_SUM or units.get(k, 2.0) < 1.0) for k in FWD_OUT + BWD_OUT if three or k not in ("y", "dW3", "db3")}
        r = chain(o)
        share, why = {}, {k: "bound" if (k in units or cls == "I" or small) else "large case" for k, ok in inside.items() if not ok}
        if cls != "I":
            _, share = perturbed(dict(out, x=x, pro=pro, o=o, r=r), "A")
            for k in DEPENDS[cls]:
                if inside.get(k) and (share.get(k) is None or share[k] < TEETH):
                    if k in req or k in ("h1", "h2"):
                        return None                  # an output this level asks for: try the next density
                    why[k] = "teeth"
        check = {k: k not in why for k in inside}
        return x, pro, o, r, units, check, share, why

    for req in _requirements(cls, small):
        for d in DENSITIES if cls != "I" else (1.0,):
            got = attempt(d, req)
            if got is not None:
                break
        if got is not None:
            break
    if got is None:
        return out
    x, pro, o, r, units, check, share, why = got
    ns = head_ns(v.nc)
    flat = torch.cat([r[k].reshape(-1) for k, _, _ in sections(v.nc)])
    base = ints((ns,), seed_of("head-base", name, cls, hvid(v))) if v.acc else None
    dparams = flat.float() if base is None else base.float() + flat.float()          # head_fold_k: out[i] + (float) t, in fp32
    scales = {t: head_scales(o, r, x, pro, t) for t in (True, False)}
    splits = {t: splits_hold(r, scales[t]) for t in (True, False)}
    out.update(d=d, x=x, pro=pro, o=o, r=r, base=base, dparams=dparams, units=units, check=check, share=share, why=why, req=req,
               scales=scales, splits=splits, notable=all(e and n for e, n in splits[False].values()))
    return out


def perturbed(p, what):
    """(reference with a low part dropped, share of the outputs that can change which do, per output).  what: "A" — the setting's A
    rounded to integers; or a place of PLACES — that product alone computed with the operand's high fp16 term (scales as with the
    tables).  "Can change": a chain on absolute values, with the ReLUs of either reference open, that carries only the dropped part."""
    o, r, cls = p["o"], p["r"], p["cls"]
    oa = _abs(o)
    if what == "A":
        key = {"x": "xa", "dy": "dy", "w1": "w1", "w2": "w2"}[A_OF[cls]]
        o2 = dict(o, xa=activated(p["x"].round(), p["pro"], bool(p["v"].pro))) if key == "xa" else dict(o, **{key: o[key].round()})
        rp = chain(o2)
        low = (o[key] - o2[key]).abs()
        masks = {k: (r[k] | rp[k]) if r[k] is not None else None for k in ("m1", "m2", "m1r")}
        ra, rb = chain(oa, masks=masks), chain(dict(oa, **{key: oa[key] + low}), masks=masks)
    else:
        _, opk, sk, _, _ = PLACES[what]
        s = head_scales(o, r, p["x"], p["pro"], True)
        rp = chain(o, sub={what: lambda t: high_term(t, s[sk])})
        masks = {k: (r[k] | rp[k]) if r[k] is not None else None for k in ("m1", "m2", "m1r")}
        low = (r[opk] - high_term(r[opk], s[sk])).abs()
        ra, rb = chain(oa, masks=masks), chain(oa, masks=masks, sub={what: lambda t: t + low})
    share = {}
    for k in FWD_OUT + BWD_OUT:
        if k in r and k in rp:
            live = (rb[k] - ra[k]) > 0
            share[k] = (float(((r[k] != rp[k]) & live).sum()) / int(live.sum())) if bool(live.any()) else None
    return rp, share


def clear_caches():
    head_problem.cache_clear()
