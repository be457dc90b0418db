"""Case tables, seeded operands, fp64 references and a Python restatement of the weight-gradient launch plans for the exact-arithmetic
tests of the convolution kernels (profiles/exact_conv.md is the table in prose).  Imports neither the product nor the GPU — the
case tables of the existing forward tests are read from test_kernels_gpu / test_conv_x3_gpu, which import both lazily:
test_exact_conv_cpu.py proves the tables on the host (restated plan == the library's host query == the branch a case is listed
under; the exactness bound, the teeth condition and the exact splits of every class-T operand), test_exact_conv_gpu.py runs them
and compares BITS.

Why bits: every scale in these kernels is a power of two and every operand is split by exact subtraction, so an input whose terms
are all representable — and whose sums stay inside fp32's 24 bits with room to spare — goes through the fp32-input MFMA, x3 (three
bf16 terms), x2h (two fp16 terms) and the one-term bf16 mode without a single rounding.  The result is then the rational number
an fp64 reference gives, and the kernel has to return exactly that.

  class I   every operand an integer, |v| <= 3 (prologue scales from {1, 2, -1, 0.5}): exact in all three modes, finds geometry errors
  class T   one operand of each product "A" = i + j / 4096 (|i|, |j| <= 3: 14 significant bits, exactly two fp16 or two bf16 terms),
            the other "B" a class-I integer, kept with probability d: every cross product x2h / x3 keep is exact, the ones they drop
            are zero; each family runs with A on either side, so either missing cross product changes the bits.  Modes 3 and 2."""
import functools
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from dispatch_cases import NAN_BITS, ceil_div

UNIT_T = 2.0 ** -12             # common unit of the products of class T
BOUND = 2 ** 22                 # units: sum of |products| (+ |bias|, + |accumulate base|) per checked output, two bits under fp32's 24
TEETH = 0.90                    # fraction of a case's outputs that must change when A's low part is dropped
DENSITIES = (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125)       # of B: the largest one that keeps a case inside BOUND is taken
MIN_DENSITY_EXISTING = 0.0625   # a case of the existing forward tables that needs less stays in class I only
MODES_I, MODES_T = (3, 2, 1), (3, 2)
X3_FWD_SCALE = 4.0


def nan_fill(*shape):
    """A tensor of the sentinel NaN (a payload no kernel produces): outputs an entry point overwrites start as this."""
    return torch.full(shape, NAN_BITS, dtype=torch.int32).view(torch.float32)


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(shape, seed, lim=3):
    return torch.randint(-lim, lim + 1, tuple(shape), generator=_gen(seed)).double()


def tvals(shape, seed):
    """Class-T operand A: i + j / 4096 with |i| <= 3 and 1 <= |j| <= 3 — every element of A carries a low part, so that a single
    product is enough to show a dropped one."""
    g = _gen(seed + 7919)
    j = torch.randint(1, 4, tuple(shape), generator=g) * (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1)
    return ints(shape, seed) + j.double() / 4096.0


def keep(shape, seed, d):
    """Nested in d: an element kept at density d is kept at every larger one."""
    return (torch.rand(tuple(shape), generator=_gen(seed), dtype=torch.float64) < d).double()


def operand(kind, shape, seed, d=1.0):
    """kind: 'I' integer, 'A' i + j / 4096, 'B' integer kept with probability d."""
    if kind == "A":
        return tvals(shape, seed)
    v = ints(shape, seed)
    return v * keep(shape, seed + 104729, d) if kind == "B" and d < 1.0 else v


def pro_table(C, seed, shift=True):
    """Prologue coefficients [C, 2]: scale from {1, 2, -1, 0.5}, integer shift.  Class T runs without the shift: a sparse B has to
    stay sparse, and on A a shift only adds to the bound (so lowers the density of B, hence the teeth) without adding a low part;
    the shift — and with it the order of zero padding and activation — is class I's."""
    s = torch.tensor([1.0, 2.0, -1.0, 0.5], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=_gen(seed))]
    t = ints((C,), seed + 1) if shift else torch.zeros(C, dtype=torch.float64)
    return torch.stack([s, t], 1).contiguous()


def act64(x, pro, relu):
    v = x
    if pro is not None:
        v = v * pro[:, 0].view(1, -1, 1, 1) + pro[:, 1].view(1, -1, 1, 1)
    return F.relu(v) if relu else v


def act_cat(x0, x1, pro0, pro1, pro_relu):
    """The input of a convolution as loaded: prologue and ReLU per half of the (virtual) concat."""
    a = act64(x0, pro0, pro_relu & 1)
    return a if x1 is None else torch.cat([a, act64(x1, pro1, pro_relu & 2)], 1)


def fp32_exact(t64):
    return bool((t64.float().double() == t64).all())


# =============================================================================================== the splits, restated
def scale_from_amax(amax):
    """x3_scale_from_amax: the power of two S with amax * S in [2^14, 2^15); 1 for 0."""
    if amax == 0:
        return 1.0
    return 2.0 ** (14 - (math.frexp(float(amax))[1] - 1))


def split2h(v64, scale):
    """split2h_pair on v * scale: (h0, h1) fp16, h1 = fp16(v * scale - h0)."""
    s = (v64 * scale).float()
    h0 = s.half()
    return h0, (s - h0.float()).half()


def split2h_exact(v64, scale):
    """-> (h0 + h1 == v * scale everywhere, no non-zero term below fp16's smallest normal 2^-14 and none infinite)."""
    h0, h1 = split2h(v64, scale)
    exact = bool((h0.double() + h1.double() == v64 * scale).all())
    normal = all(bool(torch.isfinite(h).all()) and bool((h[h != 0].double().abs() >= 2.0 ** -14).all()) for h in (h0, h1))
    return exact, normal


def split_bf16_exact(v64, terms):
    """split3_pair cut after `terms` terms: do the bf16 terms add up to v?"""
    r = v64.float()
    tot = torch.zeros_like(v64)
    for _ in range(terms):
        p = r.bfloat16()
        tot = tot + p.double()
        r = r - p.float()
    return bool((tot == v64).all())


# =============================================================================================== launch plans, restated
def tiling(B, H, W, narrow, pixels):
    """make_tiling (internal.h)."""
    TW = 16 if narrow else 32
    TH = pixels // TW
    tx, ty = ceil_div(W, TW), ceil_div(H, TH)
    return {"TW": TW, "TH": TH, "tiles_x": tx, "tiles_y": ty, "tiles": B * tx * ty}


def wgrad_geometry(B, H, W, Cin, Cout, k=3):
    """wgrad_geometry + the N-block choice of wtpse_conv_wgrad (conv.hip)."""
    t = tiling(B, H, W, W <= 16, 256)
    MB = 32 if Cout > 16 else 16
    cg = min(Cin, MB)
    ngroups = ceil_div(Cin, cg)
    nblk = ceil_div(cg * k * k, MB)
    inst = 1 if k == 1 else (1 if nblk <= 1 else 2 if nblk <= 2 else 5 if nblk <= 5 else 9)
    return dict(t, MB=MB, P32=MB == 32, cg=cg, full=cg == MB, ngroups=ngroups, ragged_group=Cin % cg != 0, nblk=nblk, inst=inst, slack=nblk < inst,
                cout_blocks=ceil_div(Cout, MB), bias_wgs=ceil_div(Cout, 32))


def wgrad_ksplit(B, H, W, Cin, Cout, k=3):
    g = wgrad_geometry(B, H, W, Cin, Cout, k)
    return max(1, min(512 // (g["cout_blocks"] * g["ngroups"]), g["tiles"]))


def wgrad_x3_supported(Cin, Cout, k, C0):
    return k == 3 and Cin >= 32 and Cout >= 32 and Cin % 32 == 0 and Cout % 32 == 0 and C0 % 8 == 0


def wgrad_x3_geometry(B, H, W, Cin, Cout, tw32=False):
    """wgrad_x3_geometry (conv_x3.hip): 16-wide tiles by default; tw32: the 32-wide tiles a process started under
    WTPSE_X3_WGRAD_TW32=1 takes on maps wider than 16 (conv_wgrad_x3_k<3, 5, Q>; read once per process)."""
    q = Cin % 64 == 0 and Cout % 64 == 0
    return dict(tiling(B, H, W, not (tw32 and W > 16), 64 if q else 128), Q=q, blk=64 if q else 32)


def wgrad_x3_ksplit(B, H, W, Cin, Cout, tw32=False):
    g = wgrad_x3_geometry(B, H, W, Cin, Cout, tw32)
    return max(1, min(512 // ((Cout // g["blk"]) * (Cin // g["blk"])), g["tiles"]))


def x3_mt2(B, H, W, CoutP, mt=0):
    """x3_mt2 (conv_x3.hip): 64-channel blocks where they give 512 workgroups; mt: the once-per-process override WTPSE_X3_MT (1 | 2)."""
    mt2 = CoutP % 64 == 0 and tiling(B, H, W, W <= 16, 256)["tiles"] * (CoutP // 64) >= 512
    if mt == 1:
        mt2 = False
    if mt == 2 and CoutP % 64 == 0:
        mt2 = True
    return mt2


def x3_half(B, H, W, CoutP, k, mt2, x3r=1, half_min=256):
    """x3_half: 64-channel blocks on 128-pixel tiles (3x3, conv_x3r_k allowed); half_min: WTPSE_X3_HALF_MIN (0: WTPSE_X3_HALF=0)."""
    if k != 3 or half_min == 0 or x3r == 0 or CoutP % 64 != 0 or mt2:
        return False
    return tiling(B, H, W, W <= 16, 128)["tiles"] * (CoutP // 64) >= half_min


def x3_small_tiles(B, H, W, CoutP, mt2, small_wide=0):
    """x3_small_tiles: 32-channel blocks on 128-pixel tiles — few workgroups on a 16-wide map, or wtpse_x3_small_wide(1) at W % 32 == 0."""
    if mt2:
        return False
    if W > 16:
        return bool(small_wide) and W % 32 == 0
    return tiling(B, H, W, True, 256)["tiles"] * (CoutP // 32) < 512


def x3_tiling(B, H, W, Cout, k, small_wide=0, x3r=1, mt=0, half_min=256):
    """x3_tiling (conv_x3.hip), the switches as parameters: wtpse_x3_small_wide, wtpse_x3r_enable and the once-per-process
    WTPSE_X3_MT / WTPSE_X3_HALF_MIN.  -> the tiling plus mt (32-channel blocks per workgroup), px, half, small."""
    CoutP = (Cout + 31) & ~31
    mt2 = x3_mt2(B, H, W, CoutP, mt)
    half = x3_half(B, H, W, CoutP, k, mt2, x3r, half_min)
    small = (not half) and x3_small_tiles(B, H, W, CoutP, mt2, small_wide)
    px = 128 if (half or small) else 256
    return dict(tiling(B, H, W, W <= 16, px), mt=2 if (mt2 or half) else 1, px=px, half=int(half), small=int(small))


def wgrad_r_supported(Cin, Cout, k, C0, W):
    if W == 16 and (Cin % 32 or Cout % 32):
        return False
    return k == 3 and Cin % 16 == 0 and Cout % 16 == 0 and C0 % 16 == 0 and (W % 32 == 0 or W == 16)


def wgrad_r_plan(B, H, W, Cin, Cout):
    """wgrad_r_plan (wgrad_r.hip) plus what follows from it inside wgrad_r_k: rows of the last segment, X rows a unit walks
    (rlast - rfirst + 1: the row loop is unrolled by four with a tail of up to three), units per wave."""
    if not (W % 32 == 0 or W == 16) or H < 1 or Cin % 16 or Cout % 16:
        return None
    mf, nf = (2 if Cout % 32 == 0 else 1), (2 if Cin % 32 == 0 else 1)
    nci = Cin // (16 * nf)
    pairs = (Cout // (16 * mf)) * nci
    strips = 1 if W == 16 else W // 32
    nw = 4 if mf * nf >= 2 else 8
    target = 1024 if mf * nf >= 2 else 2048
    wpp = max((target // pairs) // nw * nw, nw)
    cols = ((B + 1) // 2 if W == 16 else B) * strips
    nseg = ceil_div(wpp, cols) if cols < wpp else 1
    nseg = min(nseg, H)
    rseg = ceil_div(H, nseg)
    nseg = ceil_div(H, rseg)
    units = cols * nseg
    if wpp > units:
        wpp = ceil_div(units, nw) * nw
    per_wave = [(wv + 1) * units // wpp - wv * units // wpp for wv in range(wpp)]
    xrows = set()
    for seg in range(nseg):
        y0, y1 = seg * rseg, min(H, seg * rseg + rseg)
        xrows.add(min(y1, H - 1) - max(y0 - 1, 0) + 1)
    return {"mf": mf, "nf": nf, "nw": nw, "pairs": pairs, "nci": nci, "wpp": wpp, "nseg": nseg, "rseg": rseg, "units": units,
            "strips": strips, "twin": W == 16, "slabs": wpp // nw, "last": H - (nseg - 1) * rseg, "idle": per_wave.count(0),
            "per_wave": (min(per_wave), max(per_wave)), "xrows_mod4": sorted({r % 4 for r in xrows}), "odd_pair": W == 16 and B % 2 == 1}


def wgrad_r_slabs(B, H, W, Cin, Cout):
    p = wgrad_r_plan(B, H, W, Cin, Cout)
    return 0 if p is None else p["slabs"]


def wgrad_r_terms(mode, plan, v):
    """16-bit terms per operand of the wgrad_r_k a call runs (csrc/wgrad_r.hip: wgrad_r_variant): 2 = x2h (PRO always on),
    1 = one bf16 term, 3 = x3.  v: the call's variant."""
    big = plan["mf"] * plan["nf"] >= 2
    if mode == 2 and not v.bn and (v.amax != "" or big):
        return 2
    if plan["twin"]:
        return 1 if mode == 1 else 3
    if mode == 1 and not v.bn and big:
        return 1
    return 3


def fold_branch(slabs, bias):
    """The fold behind an entry point without / with a bias gradient, and the trips of wgrad_fold4_k's two loops."""
    if bias:
        return {"kernel": "wgrad_reduce_k", "partial": slabs % 8 != 0, "short": slabs < 8}
    strided, tails = [], []
    for kq in range(8):                                # the lane group kq of a workgroup takes slabs kq, kq + 8, ...
        k, n = kq, 0
        while k + 24 < slabs:
            k, n = k + 32, n + 1
        strided.append(n)
        tails.append(len(range(k, slabs, 8)))
    return {"kernel": "wgrad_fold4_k", "strided": (min(strided), max(strided)), "tail": (min(tails), max(tails)),
            "empty_groups": sum(1 for kq in range(8) if kq >= slabs)}


# =============================================================================================== weight-gradient cases
# V: one call of an entry point.  pro: None (no prologue at all) or the pro_relu bits with both coefficient tables given;
# bias: with dbias; acc: accumulate onto class-I integers; bn: the fused-BatchNorm form (wtpse_conv_wgrad_r_bn);
# amax: "" none, "dy" dy_amax from amax_of, "dyx" dy_amax and x_amax0 / x_amax1 from amax_of (mode 2 only, no prologue)
V = namedtuple("V", "pro bias acc bn amax", defaults=(None, False, False, False, ""))


def vid(v):
    return "%s%s%s%s%s" % ("nopro" if v.pro is None else "pro%d" % v.pro, "+bias" if v.bias else "", "+acc" if v.acc else "",
                           "+bn" if v.bn else "", "+amax_" + v.amax if v.amax else "")


_FP32_V = (V(None, bias=True), V(1, acc=True))
# name -> ((B, C0, C1, Cout, H, W), ksize, expected subset of wgrad_geometry(), variants)
WG32_CASES = {
    "p16_nb1":      ((2, 1, 0, 16, 5, 9), 3, {"P32": False, "TW": 16, "tiles": 2, "nblk": 1, "inst": 1}, _FP32_V),
    "p16_nb2":      ((2, 3, 0, 16, 5, 9), 3, {"P32": False, "nblk": 2, "inst": 2}, _FP32_V),
    "p16_nb4of5":   ((2, 6, 0, 16, 5, 9), 3, {"P32": False, "nblk": 4, "inst": 5, "slack": True}, _FP32_V),
    "p16_nb7of9":   ((2, 12, 0, 16, 5, 9), 3, {"P32": False, "nblk": 7, "inst": 9, "slack": True}, _FP32_V),
    "p16_nb9":      ((2, 16, 0, 16, 5, 9), 3, {"P32": False, "nblk": 9, "inst": 9, "slack": False, "full": True}, _FP32_V),
    "p16_nb9_mix":  ((2, 15, 0, 16, 5, 9), 3, {"P32": False, "nblk": 9, "inst": 9, "slack": False, "full": False}, _FP32_V),
    "p16_cout5":    ((2, 6, 0, 5, 5, 9), 3, {"P32": False, "nblk": 4, "inst": 5}, _FP32_V),
    "p32_nb1":      ((2, 3, 0, 20, 5, 9), 3, {"P32": True, "nblk": 1, "inst": 1}, _FP32_V),
    "p32_nb2":      ((2, 5, 0, 20, 5, 9), 3, {"P32": True, "nblk": 2, "inst": 2}, _FP32_V),
    "p32_nb4of5":   ((2, 12, 0, 20, 5, 9), 3, {"P32": True, "nblk": 4, "inst": 5, "slack": True}, _FP32_V),
    "p32_nb7of9":   ((2, 24, 0, 40, 5, 9), 3, {"P32": True, "nblk": 7, "inst": 9, "slack": True, "cout_blocks": 2}, _FP32_V),
    "p32_nb9_mix":  ((2, 30, 0, 20, 5, 9), 3, {"P32": True, "nblk": 9, "inst": 9, "slack": False, "full": False}, _FP32_V),
    "wide_ragged":  ((2, 40, 0, 96, 9, 33), 3, {"P32": True, "TW": 32, "ragged_group": True, "cout_blocks": 3, "bias_wgs": 3, "tiles": 8,
                                                "nblk": 9, "full": True}, _FP32_V + (V(None, bias=True, acc=True),)),
    "k1_ragged":    ((2, 40, 0, 20, 5, 9), 1, {"P32": True, "TW": 16, "ragged_group": True, "inst": 1}, _FP32_V),
    "k1_wide":      ((2, 20, 0, 8, 17, 35), 1, {"P32": False, "TW": 32, "tiles": 12, "ragged_group": True, "inst": 1}, _FP32_V),
    "concat":       ((2, 16, 16, 32, 9, 33), 3, {"P32": True, "TW": 32, "ngroups": 1},
                     (V(None, bias=True), V(1), V(2, acc=True), V(3, bias=True))),
}
# explicit ksplit through the C ABI: name -> (case of WG32_CASES or a shape, ksize, tiles, the split counts)
WG32_KSPLIT = {"ksplit18": ((3, 32, 0, 32, 20, 40), 3, 18, (1, 5, 7, 18))}

_X3W_V = (V(3), V(None, acc=True))
# name -> (shape, expected subset of wgrad_x3_geometry() [+ ksplit], variants)
WGX3_CASES = {
    "q0_small":  ((2, 32, 0, 32, 5, 9), {"Q": False, "TH": 8, "tiles": 2}, _X3W_V),
    "q0_96":     ((3, 96, 0, 64, 7, 24), {"Q": False, "tiles": 6}, _X3W_V),
    "q1_18":     ((3, 64, 0, 64, 9, 20), {"Q": True, "TH": 4, "tiles": 18}, _X3W_V),
    "q1_one":    ((1, 128, 0, 128, 2, 2), {"Q": True, "tiles": 1}, (V(0), V(None, acc=True))),      # four pixels: no ReLU on load
    "concat":    ((2, 32, 32, 64, 5, 9), {"Q": True, "tiles": 4}, (V(1), V(2), V(3, acc=True))),
}

# conv_wgrad_x3_k<3, 5, Q>: reached only by a process started under WTPSE_X3_WGRAD_TW32=1 (tests/switch_worker.py, job tw32); each case
# changes its tile count between the 16- and the 32-wide tiles.  name -> (shape, expected subset of wgrad_x3_geometry(tw32=True),
# tiles on the default 16-wide tiles, variants)
WGX3_TW32_CASES = {
    "tw32_q0":  ((2, 32, 0, 32, 5, 40), {"Q": False, "TW": 32, "TH": 4, "tiles_x": 2, "tiles_y": 2, "tiles": 8}, 6, _X3W_V),
    "tw32_q1":  ((2, 64, 0, 64, 3, 72), {"Q": True, "TW": 32, "TH": 2, "tiles_x": 3, "tiles_y": 2, "tiles": 12}, 10, _X3W_V),
    "tw32_cat": ((2, 32, 32, 64, 5, 72), {"Q": True, "TW": 32, "tiles": 18}, 20, (V(1), V(2), V(3, acc=True))),
}

_BLK_V = (V(3), V(None), V(3, bn=True), V(3, amax="dy"), V(None, amax="dyx"))
_SEG_V = (V(3),)
# name -> (shape, expected subset of wgrad_r_plan(), variants, classes)
WGR_CASES = {
    # block shapes
    "blk11":       ((2, 16, 0, 16, 4, 32), {"mf": 1, "nf": 1, "nw": 8, "slabs": 1, "rseg": 1}, _BLK_V, "IT"),
    "blk21_h1":    ((2, 16, 0, 32, 1, 32), {"mf": 2, "nf": 1, "nw": 4, "units": 2, "idle": 2, "slabs": 1}, _BLK_V, "IT"),
    "blk12":       ((2, 32, 0, 16, 4, 64), {"mf": 1, "nf": 2, "strips": 2}, _BLK_V, "IT"),
    "blk22":       ((2, 32, 0, 32, 8, 32), {"mf": 2, "nf": 2}, _BLK_V, "IT"),
    # bias gradient (16 x 16 blocks)
    "bias_21u":    ((3, 16, 0, 16, 7, 32), {"mf": 1, "nf": 1, "units": 21, "wpp": 24, "idle": 3, "slabs": 3},
                    (V(3, bias=True), V(None, bias=True, acc=True), V(None), V(3, bias=True, amax="dy")), "IT"),
    "bias_3x3":    ((3, 16, 0, 48, 10, 96), {"mf": 1, "nf": 1, "pairs": 3, "strips": 3}, (V(3, bias=True), V(None, bias=True)), "IT"),
    # row segments: heights 2, 3, 4, 5 of the segment, short last segments, waves without a unit
    "rseg2":       ((2, 256, 0, 256, 16, 32), {"rseg": 2, "last": 2}, _SEG_V, "IT"),
    "rseg3":       ((2, 256, 0, 256, 24, 32), {"rseg": 3, "last": 3}, _SEG_V, "IT"),
    "rseg4_l2":    ((2, 256, 0, 256, 26, 32), {"rseg": 4, "last": 2, "idle": 2}, _SEG_V + (V(None),), "IT"),
    "rseg5_l2":    ((2, 256, 0, 256, 37, 32), {"rseg": 5, "last": 2}, _SEG_V + (V(3, bn=True),), "IT"),
    "rseg4_l1_s2": ((2, 256, 0, 256, 13, 64), {"rseg": 4, "last": 1, "strips": 2}, _SEG_V + (V(3, bn=True),), "IT"),
    "rseg3_24":    ((2, 128, 0, 128, 70, 32), {"rseg": 3, "nseg": 24, "last": 1, "slabs": 12}, _SEG_V, "IT"),
    "h1":          ((2, 32, 0, 32, 1, 32), {"rseg": 1, "nseg": 1}, _SEG_V + (V(None),), "IT"),
    "h2":          ((2, 32, 0, 32, 2, 32), {"rseg": 1, "nseg": 2}, _SEG_V + (V(None),), "IT"),
    # more than one unit per wave, unequal shares
    "twin_18on16": ((5, 256, 0, 256, 26, 16), {"twin": True, "units": 18, "wpp": 16, "rseg": 5, "last": 1, "per_wave": (1, 2),
                                               "odd_pair": True}, _SEG_V, "IT"),
    # twin (W = 16)
    "twin_odd":    ((3, 32, 0, 32, 5, 16), {"twin": True, "odd_pair": True}, (V(3), V(None, acc=True), V(3, amax="dy")), "IT"),
    "twin_rseg4":  ((4, 256, 0, 256, 26, 16), {"twin": True, "rseg": 4}, _SEG_V, "IT"),
    "twin_concat": ((5, 64, 64, 128, 16, 16), {"twin": True, "odd_pair": True}, (V(3), V(1), V(None)), "IT"),
    # concat whose halves are one 16-channel fragment each
    "concat16":    ((2, 16, 16, 32, 12, 64), {"mf": 2, "nf": 2, "strips": 2}, (V(3), V(1), V(2, bn=True), V(None, amax="dyx")), "IT"),
    # slab counts of the fold (the other counts come with the cases above)
    "fold7":       ((3, 32, 0, 64, 9, 32), {"slabs": 7}, _SEG_V, "IT"),
    "fold32":      ((5, 16, 0, 32, 25, 32), {"slabs": 32}, _SEG_V, "IT"),
    "fold33":      ((3, 16, 0, 32, 43, 32), {"slabs": 33}, _SEG_V, "IT"),
    "fold34":      ((5, 16, 0, 16, 27, 64), {"slabs": 34}, (V(3), V(3, bias=True)), "IT"),
    "fold220":     ((40, 16, 0, 16, 64, 64), {"slabs": 220, "rseg": 3}, (V(3), V(3, bias=True)), "I"),
}
# slab count -> the case (without bias) that folds it with wgrad_fold4_k
FOLD4_SLABS = {1: "blk11", 3: "bias_21u", 7: "fold7", 12: "rseg3_24", 32: "fold32", 33: "fold33", 34: "fold34", 220: "fold220"}


def wgrad_cases(fam):
    return {"fp32": WG32_CASES, "ksplit": WG32_KSPLIT, "x3": WGX3_CASES, "x3tw32": WGX3_TW32_CASES, "r": WGR_CASES}[fam]


def wgrad_case(fam, name):
    """-> (shape, ksize, variants, classes)."""
    c = wgrad_cases(fam)[name]
    if fam == "ksplit":
        return c[0], c[1], (V(None, bias=True),), "IT"
    if fam == "fp32":
        return c[0], c[1], c[3], "IT"
    if fam == "x3":
        return c[0], 3, c[2], "IT"
    if fam == "x3tw32":
        return c[0], 3, c[3], "IT"
    return c[0], 3, c[2], c[3]


def wgrad_classes(classes):
    """The operand settings of a case: class I, and class T with A = X (B = dY) and with A = dY (B = X)."""
    return ("I", "TX", "TD") if "T" in classes else ("I",)


def teeth(ref, ref_round, absref, zeroed=False):
    """Fraction of the outputs that change when A's low part is dropped, among the outputs that have a non-zero product at all
    (an output the geometry leaves empty — the vertical taps of a one-row image — cannot change).  zeroed: the call has an output
    ReLU or a mask; the outputs those set to zero either way are left out as well."""
    live = absref > 0
    if zeroed:
        live = live & ((ref != 0) | (ref_round != 0))
    return float(((ref != ref_round) & live).sum()) / max(1, int(live.sum()))


def choose_density(sparse, try_d, power=1, probe=None):
    """try_d(d) -> (state, worst): the operands at density d of B and the largest checked sum in units of BOUND.  -> (d, state) for
    the first density of DENSITIES that try_d finds inside the bound (None, None if none does).  Not tried: densities at which the
    bound of d = 1, scaled down in proportion (d ** power: a sum of squares of products of two sparse operands falls as d^4), still
    cannot fit, and densities that probe(d) — the same bound on a few images of a large batch — already finds outside."""
    first = None
    for d in DENSITIES if sparse else (1.0,):
        if first is not None and d ** power * first >= 1.0:
            continue
        if probe is not None:
            w = probe(d)
            first = w if first is None else first
            if w >= 1.0:
                continue
        state, w = try_d(d)
        first = w if first is None else first
        if w < 1.0:
            return d, state
    return None, None


def _units(absval, unit, extra=0.0):
    return (float(absval.max()) + extra) / unit / BOUND


def _bound_ok(absval, unit, extra=0.0):
    return float(absval.max()) / unit + extra / unit < BOUND


@functools.lru_cache(maxsize=None)
def wgrad_problem(fam, name, cls, v):
    """Operands and fp64 references of one call.  -> dict: x0, x1, pro0, pro1, dy | (g, y, coef), base, dw (reference, base included),
    db, and for the CPU proof: absdw / absdb (the same sums over absolute values), round() (the reference with A's low part dropped), d, unit, loaded
    (name -> operand as the matrix cores see it)."""
    (B, C0, C1, Co, H, W), k, _, _ = wgrad_case(fam, name)
    Cin = C0 + C1
    sd = seed_of(fam, name, cls, vid(v))
    unit = 1.0 if cls == "I" else UNIT_T
    xk, dk = {"I": ("I", "I"), "TX": ("A", "B"), "TD": ("B", "A")}[cls]

    def build(d):
        x = operand(xk, (B, Cin, H, W), sd + 1, d)
        pro = pro_table(Cin, sd + 2, shift=cls == "I") if v.pro is not None else None
        if v.bn:
            # dY = k1 g + k2 y + k3, formed on load: g carries the class of dY, y and the coefficients are integers; k3 = 0 where dY
            # must stay sparse
            g = operand(dk, (B, Co, H, W), sd + 3, d)
            y = operand("B" if dk == "B" else "I", (B, Co, H, W), sd + 4, d)
            lim = 2 if cls == "I" else 1
            coef = torch.stack([ints((Co,), sd + 5, lim), ints((Co,), sd + 6, lim), ints((Co,), sd + 7, lim) * (0.0 if dk == "B" else 1.0)], 1)
            coef[:, 0] = torch.where(coef[:, 0] == 0, torch.ones(Co, dtype=torch.float64), coef[:, 0])
            dy = coef[:, 0].view(1, -1, 1, 1) * g + coef[:, 1].view(1, -1, 1, 1) * y + coef[:, 2].view(1, -1, 1, 1)
        else:
            g = y = coef = None
            dy = operand(dk, (B, Co, H, W), sd + 3, d)
        if cls == "I" and W == 16:
            # twin: columns 15 and 0 of every image non-zero on both sides, so that a leak across the seam between two images shows
            for t in (x, dy) if not v.bn else (x,):
                for col in (0, 15):
                    t[..., col] = torch.where(t[..., col] == 0, torch.ones_like(t[..., col]), t[..., col])
        return x, pro, g, y, coef, dy

    def loaded(x, pro):
        pr = 0 if v.pro is None else v.pro
        return act_cat(x[:, :C0], x[:, C0:] if C1 else None, None if pro is None else pro[:C0], None if pro is None or not C1 else pro[C0:], pr)

    shape = (Co, Cin, k, k)
    grad = lambda xa, dy: torch.nn.grad.conv2d_weight(xa, shape, dy, padding=k // 2)
    base = ints(shape, sd + 8) if v.acc else None
    base_b = ints((Co,), sd + 9) if v.acc and v.bias else None
    def try_d(d):
        x, pro, g, y, coef, dy = build(d)
        xa = loaded(x, pro)
        absdw = grad(xa.abs(), dy.abs())
        return (x, pro, g, y, coef, dy, xa, absdw), _units(absdw, unit, 3.0 if v.acc else 0.0)

    chosen, state = choose_density(cls != "I", try_d)
    out = {"d": chosen, "unit": unit, "shape": (B, C0, C1, Co, H, W), "k": k}
    if chosen is None:
        return out
    x, pro, g, y, coef, dy, xa, absdw = state
    dw = grad(xa, dy)
    db = dy.sum((0, 2, 3))
    absdb = dy.abs().sum((0, 2, 3))
    out.update(x0=x[:, :C0].contiguous(), x1=x[:, C0:].contiguous() if C1 else None,
               pro0=None if pro is None else pro[:C0].contiguous(), pro1=None if pro is None or not C1 else pro[C0:].contiguous(),
               dy=dy, g=g, y=y, coef=coef, base=base, base_b=base_b, dw=dw if base is None else dw + base,
               db=db if base_b is None else db + base_b, absdw=absdw, absdb=absdb, loaded={"x": xa, "dy": dy},
               check_db=v.bias and _bound_ok(absdb, unit, 3.0 if v.acc else 0.0))
    if cls != "I":
        def dw_round():                                     # the reference with A's low part dropped: for the host-side proof only
            if cls == "TX":
                return grad(loaded(x.round(), pro), dy)
            if v.bn:
                return grad(xa, coef[:, 0].view(1, -1, 1, 1) * g.round() + coef[:, 1].view(1, -1, 1, 1) * y + coef[:, 2].view(1, -1, 1, 1))
            return grad(xa, dy.round())
        out["round"] = dw_round
    return out


def wgrad_scales(fam, plan, mode, v, p):
    """The power-of-two scales the operands of a weight-gradient call meet where the call runs x2h: {operand name: scale}."""
    if fam != "r" or wgrad_r_terms(mode, plan, v) != 2:
        return {}
    sx = scale_from_amax(float(torch.cat([p["x0"].abs().reshape(-1), p["x1"].abs().reshape(-1) if p["x1"] is not None else p["x0"].new_zeros(1)]).max())) \
        if v.amax == "dyx" else X3_FWD_SCALE
    sdy = scale_from_amax(float(p["dy"].abs().max())) if v.amax else X3_FWD_SCALE
    return {"x": sx, "dy": sdy}


# =============================================================================================== forward / data-gradient cases
def _existing_tables():
    # (the two test modules import the product and touch the device inside their functions only; should either start doing so at
    # module level, copy the tables here instead)
    import test_conv_x3_gpu as TX
    import test_kernels_gpu as TK
    bnb = [m for m in TX.test_dgrad_bnb.pytestmark if m.name == "parametrize"][0].args[1]
    return {"conv": list(TK.CONV_CASES), "x3": list(TX.X3_CASES), "x16": list(TX.X16_CASES), "x3r": list(TX.X3R_CASES),
            "x3half": list(TX.X3_HALF_CASES), "bnb": list(bnb)}


# 32-channel blocks on 32 x 4 tiles: conv_x3_k<KS, 1, 5, EPI, 1, TERMS> and (wtpse_x3r_enable(2), 3x3) conv_x3r_k<1, 1, 1, 5, ...>,
# reached only under wtpse_x3_small_wide(1) at W % 32 == 0.  (B, C0, C1, Cout, H, W, k)
X3_SMALL_WIDE_CASES = [
    (2, 16, 0, 32, 6, 32, 3),      # one chunk, one tile column, the last tile row 2 of 4 rows
    (2, 16, 16, 32, 9, 64, 3),     # concat, two tile columns, the last tile row a single row
    (2, 40, 0, 96, 8, 32, 3),      # ragged chunk (40 -> 48), three output-channel blocks
    (3, 64, 0, 64, 5, 32, 3),      # 64 outputs that stay on 32-channel blocks (neither mt2 nor half: 6 tiles), grid.y = 2, four chunks
    (2, 64, 0, 32, 5, 32, 1),      # 1x1, multi-chunk
    (2, 3, 0, 8, 4, 96, 3),        # 3-channel input, Cout <= 16 on a 32-row tile, three tile columns, exactly one full tile row
    (1, 32, 0, 32, 1, 32, 3),      # image lower than a tile
]
# 64-channel blocks on a 1x1 layer (conv_x3_k<1, 2, ...>), default path: 512 tiles x one block, the step's own instantiation
# (up2.conv2 at B = 32).  A table of its own: the tolerance tests iterate X3_CASES.
X3_K1_MT2_CASES = [(32, 16, 0, 64, 64, 64, 1)]
# the EPI 2 cases (of the bnb table) that take the 32 x 4 tiles under wtpse_x3_small_wide(1)
BNB_SMALL_WIDE = ((2, 32, 0, False, 32, 16, 32, 3, False, True), (2, 32, 0, False, 32, 6, 32, 3, True, True),
                  (2, 32, 32, True, 64, 6, 64, 3, True, True))
MIN_DENSITY_SMALL_WIDE = 0.125  # every call of X3_SMALL_WIDE_CASES with a sparse operand keeps it at least this dense

TABLES = dict(_existing_tables(), x3sw=X3_SMALL_WIDE_CASES, x3k1=X3_K1_MT2_CASES)
BIG_BATCH = 16          # from this batch size on the density of B is looked for on two images first (the bound does not grow with the batch)


def conv_shape(table, case):
    """-> (B, C0, C1, Cout, H, W, k) of a case of one of the existing tables."""
    if table in ("conv", "x3", "x3sw", "x3k1"):
        return tuple(case)
    if table == "x16":
        B, Ci, Co, H, W = case
        return (B, Ci, 0, Co, H, W, 3)
    return tuple(case) + (3,)


STAT_TILE = 256         # pixels of the largest tile a row of statistics partials covers (internal.h: 256 or 128 pixels per tile)


def tile_bound(absval):
    """Per channel: the sum of the STAT_TILE largest values over (batch, rows, columns) — no tile's sum can be larger."""
    C = absval.shape[1]
    flat = absval.transpose(0, 1).reshape(C, -1)
    return flat.topk(min(STAT_TILE, flat.shape[1]), dim=1).values.sum(1)


CONV_CLASSES = ("I", "TA", "TB")         # class I; class T with A = the input (B = weights); class T with A = the weights (B = input)


def conv_classes(variant):
    return ("I",) if variant == "stats" else CONV_CLASSES


def conv_variants(table, case):
    """The calls every case runs, whatever its batch.  Forward: 'bias' (bias, statistics partials [, Gram partials at 16 output
    channels of the 16-channel kernel] — compared where their bound holds), 'stats' (class I, both operands sparse so that the sums of
    squares hold the bound too), 'relu' (no bias, output ReLU), 'pro' (prologue on both inputs, ReLU on the first).  Data-gradient
    direction (layers with more than 4 input channels): 'dgrad' (split output for a concat), 'dmask' (mask_ref with exact zeros)."""
    B, C0, C1, Co, H, W, k = conv_shape(table, case)
    return ("bias", "stats", "relu", "pro") + ((("dgrad",) if C1 else ("dgrad", "dmask")) if C0 + C1 > 4 else ())


def conv_with_table(table, variant):
    """Calls that run a second time in mode 2 with the amax table of their input from amax_of (x3 / 16-channel entry points): the
    scale then follows the data.  The 16-channel kernel takes a gradient input with grad_in: x3 without a table, x2h with one."""
    return table != "conv" and variant in ("bias", "dgrad")


@functools.lru_cache(maxsize=None)
def conv_problem(table, idx, cls, variant):
    """Operands and fp64 references of one forward / data-gradient call.  -> dict: inp0, inp1 (the launch's input, halves of a concat),
    w (OIHW of the FORWARD convolution), bias, pro0, pro1, pro_relu, relu_out, split, mask, out (reference), absout, round(),
    stat_sum / stat_sq and their absolute bounds (class I), d, unit, loaded."""
    B, C0, C1, Co, H, W, k = conv_shape(table, TABLES[table][idx])
    Cin = C0 + C1
    back = variant in ("dgrad", "dmask")
    sd = seed_of(table, idx, cls, variant)
    unit = 1.0 if cls == "I" else UNIT_T
    ik, wk = {"I": ("I", "I"), "TA": ("A", "B"), "TB": ("B", "A")}[cls]
    Ci_l, Co_l = (Co, Cin) if back else (Cin, Co)          # channels of the launch's input / output
    use_pro = variant == "pro"

    def build(d):
        inp = operand(ik, (B, Ci_l, H, W), sd + 1, d)
        w = operand(wk, (Co, Cin, k, k), sd + 2, d)
        if variant == "stats":                             # both operands sparse: the squares of the outputs have to fit a tile's sum
            inp, w = operand("B", (B, Ci_l, H, W), sd + 1, d), operand("B", (Co, Cin, k, k), sd + 2, d)
        pro = pro_table(Ci_l, sd + 3, shift=cls == "I") if use_pro else None
        return inp, w, pro

    def load(inp, pro):
        if back:
            return inp
        return act_cat(inp[:, :C0], inp[:, C0:] if C1 else None, None if pro is None else pro[:C0],
                       None if pro is None or not C1 else pro[C0:], 1 if use_pro else 0)

    def conv(a, w, bias):
        return F.conv_transpose2d(a, w, None, padding=k // 2) if back else F.conv2d(a, w, bias, padding=k // 2)

    bias = ints((Co,), sd + 4) if variant in ("bias", "pro", "stats") else None
    def try_d(d):
        inp, w, pro = build(d)
        a = load(inp, pro)
        absout = conv(a.abs(), w.abs(), None if bias is None else bias.abs())
        worst = _units(absout, unit)
        if variant == "stats":
            worst = max(worst, _units(tile_bound(absout * absout), 1.0))
        return (inp, w, pro, a, absout), worst

    def probe(d):                                          # the same bound on the first two images
        inp, w, pro = build(d)
        a2 = load(inp[:2], pro)
        ab = conv(a2.abs(), w.abs(), None if bias is None else bias.abs())
        worst = _units(ab, unit)
        return max(worst, _units(tile_bound(ab * ab), 1.0)) if variant == "stats" else worst

    sparse = cls != "I" or variant == "stats"
    chosen, state = choose_density(sparse, try_d, 4 if variant == "stats" else 1, probe if (sparse and B >= BIG_BATCH) else None)
    out = {"d": chosen, "unit": unit, "shape": (B, C0, C1, Co, H, W, k), "back": back}
    if chosen is None:
        return out
    inp, w, pro, a, absout = state
    ref = conv(a, w, bias)
    relu_out = variant == "relu"
    if relu_out:
        ref = F.relu(ref)
    mask = None
    if variant == "dmask":
        mask = ints((B, Cin, H, W), sd + 5)          # a seventh of it exact zeros: "not positive"
        ref = ref * (mask > 0)
    split = C0 if (back and C1) else None
    out.update(inp0=(inp if back else inp[:, :C0]).contiguous(), inp1=None if back or not C1 else inp[:, C0:].contiguous(), w=w, bias=bias,
               pro0=None if pro is None else pro[:C0].contiguous(), pro1=None if pro is None or not C1 else pro[C0:].contiguous(),
               pro_relu=1 if use_pro else 0, relu_out=relu_out, split=split, mask=mask, out=ref, absout=absout, loaded={"in": a, "w": w},
               zeroed=relu_out or mask is not None)
    if cls == "I" and variant in ("bias", "stats"):
        # statistics partials: one row of (sum y, sum y^2) [and of the 16 x 16 Gram] per tile of at most STAT_TILE pixels, summed in
        # fp32 — exact in any order while the sum of the STAT_TILE largest |y| (y^2) of a channel stays inside the bound
        out["stat_sum"], out["stat_sq"] = ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3))
        out["check_sum"], out["check_sq"] = _bound_ok(tile_bound(absout), 1.0), _bound_ok(tile_bound(absout * absout), 1.0)
        if table == "x16" and Co == 16:
            f = ref.reshape(B, 16, -1)
            out["gram"] = torch.bmm(f, f.transpose(1, 2))          # (|G_ij| of a tile <= the larger of the two channels' sums of squares)
    if cls != "I":
        def out_round():                                    # the reference with A's low part dropped: for the host-side proof only
            r = conv(load(inp.round(), pro), w, bias) if cls == "TA" else conv(a, w.round(), bias)
            if relu_out:
                r = F.relu(r)
            return r if mask is None else r * (mask > 0)
        out["round"] = out_round
    return out


def conv_scales(table, mode, p, with_table=False):
    """{operand: scale} where a forward / data-gradient call of the x3 or 16-channel entry point runs x2h (mode 2): the input at
    2^2 without a table or the x3_scale_from_amax value of its own amax with one, the weights at the pack kernel's scale."""
    if table == "conv" or mode != 2:
        return {}
    if table == "x16" and p["back"] and not with_table:
        return {}                                      # a gradient input without a table: the 16-channel kernel stays on x3
    raw = p["inp0"] if p["inp1"] is None else torch.cat([p["inp0"], p["inp1"]], 1)
    return {"in": scale_from_amax(float(raw.abs().max())) if with_table else X3_FWD_SCALE, "w": scale_from_amax(float(p["w"].abs().max()))}


# cases of the existing tables (B = 20 ... 64) that no density of B from 1/16 up keeps inside the bound stay in class I only:
# table -> {(index, class, variant)}.  None needs it: the bound of a forward / data-gradient output grows with Cin * k^2, not with B.
CLASS_I_ONLY = {}


def bnb_layouts(case):
    """Weight layouts a test_dgrad_bnb case runs in: the one the existing test uses (0 fp32, 1 x3) and, where the layer fits the
    16-channel kernel, its fragments (2)."""
    B, Cl, Co, bn_second, Cn, H, W, k, relu, x3 = case
    return (int(x3),) + ((2,) if (Co == 0 and Cl <= 16 and Cn <= 16 and k == 3) else ())


# ---- data gradient with the BatchNorm-backward epilogue (the test_dgrad_bnb cases)
@functools.lru_cache(maxsize=None)
def bnb_problem(idx, cls):
    """conv -> BatchNorm(+ReLU) -> [cat] -> conv, the data gradient of the second conv with the first one's BatchNorm backward in its
    epilogue.  y (the raw output below), the BatchNorm's scale / shift and its mean are integers (or halves) in every class: the mask
    [ss0 y + ss1 > 0] and the products g (y - mean) are exact.  -> du, w, y, ss, mean, g (masked gradient), other, stats [Cl, 2]."""
    B, Cl, Co, bn_second, Cn, H, W, k, relu, x3 = TABLES["bnb"][idx]
    sd = seed_of("bnb", idx, cls)
    unit = 1.0 if cls == "I" else UNIT_T
    ik, wk = {"I": ("I", "I"), "TA": ("A", "B"), "TB": ("B", "A")}[cls]
    Ct = Cl + Co
    y = ints((B, Cl, H, W), sd + 3)
    ss = torch.stack([torch.tensor([1.0, 2.0, -1.0, 0.5], dtype=torch.float64)[torch.randint(0, 4, (Cl,), generator=_gen(sd + 4))],
                      ints((Cl,), sd + 5) * 0.5], 1).contiguous()
    mean = ints((Cl,), sd + 6, 2) * 0.5
    c0, c1 = (Co, Ct) if (Co and bn_second) else (0, Cl)
    def try_d(d):
        du = operand(ik, (B, Cn, H, W), sd + 1, d)
        w = operand(wk, (Cn, Ct, k, k), sd + 2, d)
        absout = F.conv_transpose2d(du.abs(), w.abs(), None, padding=k // 2)
        return (du, w, absout), _units(absout, unit)

    chosen, state = choose_density(cls != "I", try_d)
    out = {"d": chosen, "unit": unit, "case": TABLES["bnb"][idx]}
    if chosen is None:
        return out
    du, w, absout = state
    full = F.conv_transpose2d(du, w, None, padding=k // 2)
    z = y * ss[:, 0].view(1, -1, 1, 1) + ss[:, 1].view(1, -1, 1, 1)
    live = (z > 0).double() if relu else torch.ones_like(z)
    g = full[:, c0:c1] * live
    other = None if not Co else (full[:, :Co] if bn_second else full[:, Cl:])
    ym = y - mean.view(1, -1, 1, 1)
    ga = absout[:, c0:c1]
    stats = torch.stack([g.sum((0, 2, 3)), (g * ym).sum((0, 2, 3))], 1)
    abs_stats = torch.stack([tile_bound(ga), tile_bound(ga * ym.abs())], 1)          # per tile, as the forward statistics
    out.update(du=du, w=w, y=y, ss=ss, mean=mean, g=g, other=other, stats=stats, absout=absout, abs_stats=abs_stats,
               check_stats=_bound_ok(abs_stats, unit * 0.5), loaded={"in": du, "w": w},
               split=None if not Co else (Co if bn_second else Cl), c0=c0, c1=c1)
    if cls != "I":
        out["round"] = lambda: F.conv_transpose2d(du.round() if cls == "TA" else du, w.round() if cls == "TB" else w, None, padding=k // 2)
        out["out"] = full
    return out


def clear_caches():
    """The problems are cached for the calls of ONE test (modes, settings); a test drops them behind itself — the largest hold
    hundreds of MB."""
    for f in (wgrad_problem, conv_problem, bnb_problem):
        f.cache_clear()


# =============================================================================================== comparison
def first_difference(got, ref64, what, rows=False):
    """None if got (fp32, host) holds exactly the bits of the fp64 reference; else how many elements differ and where the first is.
    rows: got is [rows, ...] of fp32 partials, each exact — their fp64 sum is compared with the reference as it is."""
    if rows:
        ref, got = ref64, got.detach().cpu().double().sum(0)
    else:
        ref = ref64.float()
        assert bool((ref.double() == ref64).all()), what + ": the reference does not survive fp32"
    got = got.detach().cpu().reshape(ref.shape)
    if torch.equal(got, ref):
        return None
    bad = ~(got == ref)                               # (a NaN differs from everything)
    flat = int(bad.reshape(-1).to(torch.uint8).argmax())
    idx = []
    for n in reversed(ref.shape):
        idx.append(flat % n)
        flat //= n
    idx = tuple(reversed(idx))
    return "%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(ref[idx]))
