"""Case table, inputs, fp32 yardstick and a Python restatement of the host dispatcher of csrc/dwt.hip (wtpse_dwt2_fwd /
wtpse_dwt2_inv); profiles/dwt_paths.md is the table in prose.  Imports neither the product nor the GPU: test_dwt_paths_cpu.py
proves the table on the host (every branch of the restated dispatcher is claimed by a case, every case takes the branch it is
listed under, the bound has teeth), test_dwt_paths_gpu.py runs it.

The bound.  The specification is oracle/dwt_cpu.py in float64.  The same lifting steps in numpy float32 (constants rounded once,
the oracle's operation order: lift_fwd32 / lift_inv32 below) are the YARDSTICK: what a correct fp32 implementation loses on this
input.  Per sub-band and level
    err_band <= K * max(yard_band, 2^-24 * max|ref_band|),    K = 4,
err_band / yard_band: largest absolute distance of the device / of the fp32 restatement to the oracle in that band.  K = 4: the
device may contract to FMA and the inverse multiplies by rounded reciprocals where the oracle divides (up to twice the roundings
per lifting step); the fused paths recompute neighbours in another order (up to another factor of two).  The inverse and the round
trip use the same form on the whole image.  The yardstick is measured against the reference arithmetic, never against the device.
One measured exception, band_k below: bands of fewer than 16 coefficients on the generic forward path."""
import functools
import re

import numpy as np

from oracle import dwt_cpu as O

K = 4
K_FWD = {"generic": K, "fast256": K, "fast512": K}      # per forward path; the inverse (always generic) and the round trip: K
# Thin bands of the generic forward path.  In a band of a few coefficients yard_band is a few draws of a rounding error, not its
# scale, and after eight or nine levels such a coefficient can be much smaller than the LL values it was formed from: on the MI355X
# the deepest bands of 256^2 L8 / 512^2 L9 (one coefficient per plane) came out at 4.16 (db2 256^2 L8), 5.40 (haar 512^2 L9) and 7.33
# (db2 512^2 L9) with absolute errors of 1.6e-7 .. 4.6e-7 — what every other band of the same launches shows — while the worst band of
# the fp32 restatement itself moves between 6 and 304 x 2^-24 max|band| on 512^2 L9 over twenty seeds.  Same kernel, same arithmetic as the
# levels above it: legitimate rounding.  Such bands get twice the measured worst (profiles/dwt_paths.md); every other band keeps K.
THIN_BAND = 16                  # coefficients in the band, all planes together
K_THIN_GENERIC = 2 * 7.33


def band_k(path, count):
    return K_THIN_GENERIC if path == "generic" and count < THIN_BAND else K_FWD[path]


EPS = 2.0 ** -24
WAVELETS = {"haar": 0, "db2": 1}

# ================================================================================================ the dispatcher, restated
COLS_PER_BLOCK = 62             # dwt2_fwd_k / dwt2_inv_k: 64 lanes = 62 column pairs + a halo lane on either side
RP = 16                         # row pairs per wave
ROWS_PER_BLOCK = 4 * RP         # four waves per workgroup
FAST_LIMITS = {256: 7, 512: 8}  # dwt_fast_shape: square W x W planes up to this many levels take the streaming path
MAX_LEVELS, MAX_PLANES = 12, 65535


def ceil_div(a, b):
    return (a + b - 1) // b


def fast_shape(H, W, levels):
    return H == W and W in FAST_LIMITS and levels <= FAST_LIMITS[W]


def accepted(planes, H, W, wavelet, levels, offs=(0, 0, 0), same=False, null=False):
    """The WTPSE_REQUIREs of both entry points (offs: float offsets of x, coef, tmp from a 16-byte boundary)."""
    return (not null and 0 < planes <= MAX_PLANES and H > 0 and W > 0 and 1 <= levels <= MAX_LEVELS and wavelet in (0, 1)
            and H % (1 << levels) == 0 and W % (1 << levels) == 0 and not same and all((4 * o) % 8 == 0 for o in offs))


def level_geometry(h, w, planes):
    """One launch of dwt2_fwd_k / dwt2_inv_k on an h x w region: dwt_grid and what its last blocks hold."""
    npairs, nrp = w // 2, h // 2
    gx, gy = ceil_div(npairs, COLS_PER_BLOCK), ceil_div(nrp, ROWS_PER_BLOCK)
    live = npairs - COLS_PER_BLOCK * (gx - 1)
    rows = nrp - ROWS_PER_BLOCK * (gy - 1)
    return {"h": h, "w": w, "grid": (gx, gy, planes),
            "col_last": "full" if live == COLS_PER_BLOCK else "partial", "col_live": live,
            "row_last": "full" if rows == ROWS_PER_BLOCK else "partial", "row_live": rows,
            "empty_waves": 4 - ceil_div(rows, RP), "cut_wave": rows % RP != 0}


def generic_levels(planes, H, W, levels):
    return [level_geometry(H >> lv, W >> lv, planes) for lv in range(levels)]


def fwd_branch(planes, H, W, levels, offs=(0, 0, 0)):
    """wtpse_dwt2_fwd -> the launches it makes.  path: generic / fast256 / fast512; why (generic only): what kept it off the
    streaming path; levels: one level_geometry per generic launch; launches (fast only): (NPL, KEEP, nrest, grid) each."""
    assert accepted(planes, H, W, 0, levels, offs)
    aligned = all((4 * o) % 16 == 0 for o in offs)
    if fast_shape(H, W, levels) and aligned:
        if W == 512:
            launches = [{"NPL": 4, "KEEP": False, "nrest": 0, "grid": (1, (H // 2) // 128, planes)}]
            if levels > 1:
                launches.append({"NPL": 2, "KEEP": True, "nrest": levels - 2, "grid": (1, 1, planes)})
        else:
            launches = [{"NPL": 2, "KEEP": True, "nrest": levels - 1, "grid": (1, 1, planes)}]
        return {"path": "fast%d" % W, "why": None, "launches": launches, "levels": []}
    if fast_shape(H, W, levels):
        why = "align:" + "+".join(n for n, o in zip(("x", "coef", "tmp"), offs) if (4 * o) % 16)
    elif H == W and W in FAST_LIMITS:
        why = "levels"
    elif H in FAST_LIMITS or W in FAST_LIMITS:
        why = "nonsquare"
    else:
        why = "shape"
    return {"path": "generic", "why": why, "launches": [], "levels": generic_levels(planes, H, W, levels)}


def inv_branch(planes, H, W, levels, offs=(0, 0, 0)):
    """wtpse_dwt2_inv: always the generic kernel, the deepest level first."""
    assert accepted(planes, H, W, 0, levels, offs)
    return {"path": "generic", "why": "inverse", "launches": [], "levels": generic_levels(planes, H, W, levels)[::-1]}


def branch_keys(br, kind="fwd"):
    """The branches of the dispatcher and of the kernels' index arithmetic that a call exercises, as a set of names."""
    keys = {"%s:%s" % (kind, br["path"])}
    if br["path"] == "generic" and kind == "fwd":
        keys.add("fwd:why=" + br["why"])
    for g in br["levels"]:
        gx, gy, _ = g["grid"]
        keys.add("%s:col_last=%s" % (kind, g["col_last"]))
        keys.add("%s:row_last=%s" % (kind, g["row_last"]))
        if gx > 1:
            keys.add(kind + ":grid_x>1")
        if gy > 1:
            keys.add(kind + ":grid_y>1")
        if gy > 1 and g["row_last"] == "partial":
            keys.add(kind + ":grid_y>1,row_last=partial")
        if g["empty_waves"]:
            keys.add(kind + ":empty_waves")
        if g["cut_wave"]:
            keys.add(kind + ":cut_wave")
        if g["w"] == 2:
            keys.add(kind + ":npairs=1")
        if g["h"] == 2:
            keys.add(kind + ":nrp=1")
        if (g["h"] // 2) % 2 and g["h"] > 2:
            keys.add(kind + ":odd_nrp")
    for l in br["launches"]:
        if l["KEEP"]:
            keys.add("fwd:keep,nrest=%d" % l["nrest"])
        else:
            keys.add("fwd:stream,NPL=%d" % l["NPL"])
    if br["path"].startswith("fast") and br["launches"][0]["grid"][2] % 2:
        keys.add("fwd:fast,odd_planes")
    return keys


# every branch the restated dispatcher has; the table below must claim each one (test_dwt_paths_cpu.py)
ALL_BRANCHES = frozenset(
    ["fwd:generic", "fwd:fast256", "fwd:fast512", "inv:generic"]
    + ["fwd:why=" + w for w in ("shape", "nonsquare", "levels", "align:x", "align:coef", "align:tmp")]
    + ["%s:%s" % (k, b) for k in ("fwd", "inv") for b in (
        "col_last=full", "col_last=partial", "row_last=full", "row_last=partial", "grid_x>1", "grid_y>1",
        "grid_y>1,row_last=partial", "empty_waves", "cut_wave", "npairs=1", "nrp=1", "odd_nrp")]
    + ["fwd:stream,NPL=4", "fwd:fast,odd_planes"] + ["fwd:keep,nrest=%d" % n for n in (0, 1, 2, 6)])
# dwt2_stream_k<WV, 2, false> (a 256-wide level streamed to memory) is not a branch: dwt_stream_launch(keep = false) is only
# called with w = 512, and the instance was removed from csrc/dwt.hip rather than given an invented caller.


# ================================================================================================ the cases
def _case(shape, levels, offs=(0, 0, 0), seed=0, expect=None, claims=()):
    return {"shape": shape, "levels": levels, "offs": offs, "seed": seed, "expect": expect or {}, "claims": frozenset(claims)}


G, F256, F512 = {"path": "generic"}, {"path": "fast256"}, {"path": "fast512"}

# name -> shape, levels, float offsets of (x, coef, tmp) from a 16-byte boundary, the seed of the input, what fwd_branch must
# say (a subset of its dict; "grids": the generic grids level by level) and the branch keys the case is there for
CASES = {
    "2x2": _case((1, 1, 2, 2), 1, seed=44, expect=dict(G, why="shape", grids=[(1, 1, 1)]),
                 claims=["fwd:npairs=1", "fwd:nrp=1", "inv:npairs=1", "inv:nrp=1"]),
    "144x16_L1": _case((1, 1, 144, 16), 1, seed=12, expect=dict(G, why="shape", grids=[(1, 2, 1)]),
                       claims=["fwd:grid_y>1", "fwd:grid_y>1,row_last=partial", "fwd:empty_waves", "fwd:cut_wave", "inv:grid_y>1",
                               "inv:grid_y>1,row_last=partial", "inv:empty_waves", "inv:cut_wave", "fwd:why=shape", "fwd:generic",
                               "inv:generic", "fwd:row_last=partial", "inv:row_last=partial"]),
    "144x16_L4": _case((1, 1, 144, 16), 4, seed=13, expect=dict(G, grids=[(1, 2, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1)]),
                       claims=["fwd:odd_nrp", "inv:odd_nrp", "fwd:npairs=1", "fwd:grid_y>1,row_last=partial"]),
    "8x248_L3": _case((1, 1, 8, 248), 3, seed=14, expect=dict(G, grids=[(2, 1, 1), (1, 1, 1), (1, 1, 1)]),
                      claims=["fwd:col_last=full", "inv:col_last=full", "fwd:grid_x>1", "inv:grid_x>1", "fwd:nrp=1"]),
    "16x128_L3": _case((2, 1, 16, 128), 3, seed=15, expect=dict(G, grids=[(2, 1, 2), (1, 1, 2), (1, 1, 2)]),
                       claims=["fwd:grid_x>1", "fwd:col_last=partial", "inv:col_last=partial"]),
    "256x512_L4": _case((1, 1, 256, 512), 4, seed=16, expect=dict(G, why="nonsquare", grids=[(5, 2, 1), (3, 1, 1), (2, 1, 1), (1, 1, 1)]),
                        claims=["fwd:why=nonsquare", "fwd:grid_y>1", "fwd:row_last=full", "inv:row_last=full"]),
    "512x256_L2": _case((1, 1, 512, 256), 2, seed=17, expect=dict(G, why="nonsquare", grids=[(3, 4, 1), (2, 2, 1)]),
                        claims=["fwd:why=nonsquare", "fwd:grid_y>1", "inv:grid_y>1"]),
    "256_L8": _case((1, 2, 256, 256), 8, seed=52, expect=dict(G, why="levels", grids=[(3, 2, 2), (2, 1, 2)] + [(1, 1, 2)] * 6),
                    claims=["fwd:why=levels", "fwd:nrp=1", "fwd:npairs=1"]),
    "512_L9": _case((1, 1, 512, 512), 9, seed=56, expect=dict(G, why="levels", grids=[(5, 4, 1), (3, 2, 1), (2, 1, 1)] + [(1, 1, 1)] * 6),
                    claims=["fwd:why=levels", "fwd:grid_y>1"]),
    "256_L3_x+8": _case((1, 2, 256, 256), 3, offs=(2, 0, 0), seed=20, expect=dict(G, why="align:x"), claims=["fwd:why=align:x"]),
    "256_L3_coef+8": _case((1, 2, 256, 256), 3, offs=(0, 2, 0), seed=20, expect=dict(G, why="align:coef"), claims=["fwd:why=align:coef"]),
    "256_L3_tmp+8": _case((1, 2, 256, 256), 3, offs=(0, 0, 2), seed=20, expect=dict(G, why="align:tmp"), claims=["fwd:why=align:tmp"]),
    "256_L3_aligned": _case((1, 2, 256, 256), 3, seed=20, expect=dict(F256, launches=[(2, True, 2)]), claims=["fwd:fast256"]),
    "f256_L1": _case((1, 3, 256, 256), 1, seed=21, expect=dict(F256, launches=[(2, True, 0)]), claims=["fwd:keep,nrest=0", "fwd:fast,odd_planes"]),
    "f256_L2": _case((1, 3, 256, 256), 2, seed=22, expect=dict(F256, launches=[(2, True, 1)]), claims=["fwd:keep,nrest=1"]),
    "f256_L3": _case((1, 3, 256, 256), 3, seed=23, expect=dict(F256, launches=[(2, True, 2)]), claims=["fwd:keep,nrest=2", "fwd:fast256"]),
    "f256_L7": _case((1, 3, 256, 256), 7, seed=24, expect=dict(F256, launches=[(2, True, 6)]), claims=["fwd:keep,nrest=6"]),
    "f512_L1": _case((1, 3, 512, 512), 1, seed=25, expect=dict(F512, launches=[(4, False, 0)]), claims=["fwd:stream,NPL=4", "fwd:fast512"]),
    "f512_L2": _case((1, 3, 512, 512), 2, seed=26, expect=dict(F512, launches=[(4, False, 0), (2, True, 0)]), claims=["fwd:keep,nrest=0"]),
    "f512_L3": _case((1, 3, 512, 512), 3, seed=27, expect=dict(F512, launches=[(4, False, 0), (2, True, 1)]), claims=["fwd:keep,nrest=1"]),
    "f512_L4": _case((1, 3, 512, 512), 4, seed=28, expect=dict(F512, launches=[(4, False, 0), (2, True, 2)]), claims=["fwd:keep,nrest=2"]),
    "f512_L8": _case((1, 3, 512, 512), 8, seed=29, expect=dict(F512, launches=[(4, False, 0), (2, True, 6)]), claims=["fwd:keep,nrest=6"]),
    "planes": _case((3, 5, 32, 64), 2, seed=30, expect=dict(G, why="shape", grids=[(1, 1, 15), (1, 1, 15)]), claims=["fwd:why=shape"]),
}
ALIGNMENT_CASES = ("256_L3_x+8", "256_L3_coef+8", "256_L3_tmp+8")      # each against "256_L3_aligned": the same input
INDEPENDENCE_CASES = ("planes", "f256_L3")
REPEAT_CASES = ("16x128_L3", "f256_L3", "f512_L4")

# The fast-path limits as data: square 256 / 512 planes up to 7 / 8 levels, 16-byte aligned, stream; one level more is generic.
# (shape, levels) -> path.  A change to dwt_fast_shape fails test_dwt_paths_cpu.py before it silently moves a case.
FAST_TABLE = {((256, 256), 1): "fast256", ((256, 256), 7): "fast256", ((256, 256), 8): "generic",
              ((512, 512), 1): "fast512", ((512, 512), 8): "fast512", ((512, 512), 9): "generic",
              ((256, 512), 4): "generic", ((512, 256), 2): "generic", ((128, 128), 3): "generic", ((1024, 1024), 3): "generic"}


def planes_of(case):
    return case["shape"][0] * case["shape"][1]


def case_branch(name, kind="fwd"):
    c = CASES[name]
    H, W = c["shape"][2:]
    return (fwd_branch if kind == "fwd" else inv_branch)(planes_of(c), H, W, c["levels"], c["offs"])


def matches(br, expect):
    """A case's `expect` against fwd_branch's answer -> the first mismatch or None."""
    for k, v in expect.items():
        if k == "grids":
            got = [g["grid"] for g in br["levels"]]
        elif k == "launches":
            got = [(l["NPL"], l["KEEP"], l["nrest"]) for l in br["launches"]]
        else:
            got = br[k]
        if got != v:
            return (k, got, v)
    return None


def dispatcher_source_constants(text):
    """What csrc/dwt.hip itself says about the numbers restated above -> dict, for test_dwt_paths_cpu.py."""
    m = re.search(r"W == 256 \|\| W == 512\) && levels <= \(W == 256 \? (\d+) : (\d+)\)", text)
    return {"limits": {256: int(m.group(1)), 512: int(m.group(2))} if m else None,
            "RP": int(re.search(r"constexpr int RP = (\d+);", text).group(1)),
            "cols": [int(v) for v in re.findall(r"ceil_div\(w / 2, (\d+)\)", text)],
            "rows_expr": "ceil_div(h / 2, 4 * RP)" in text,
            "align16": text.count("(uintptr_t)x | (uintptr_t)coef | (uintptr_t)tmp) & 15) == 0"),
            "align8": text.count("(uintptr_t)x | (uintptr_t)coef | (uintptr_t)tmp) & 7) == 0"),
            "stream_instances": sorted(set(re.findall(r"dwt2_stream_k<WV, (\d), (true|false)>", text)))}


# ================================================================================================ inputs and references
def case_input(name):
    """The case's input, float32 [B, C, H, W]: unit normal, seeded per case."""
    c = CASES[name]
    return np.random.RandomState(1000 + c["seed"]).randn(*c["shape"]).astype(np.float32)


F32 = np.float32
R3_32, A_32, B_32, C1_32, C2_32, S2_32 = (F32(v) for v in (O.R3, O.A, O.B, O.C1, O.C2, np.sqrt(2.0)))
MUTANTS = ("clamp", "swap_hl_lh", "lb_scaled", "short_region", "offsets_exchanged")


def lift_fwd32(x, wavelet, axis, clamp=False, lb=B_32):
    """oracle.dwt_cpu.lift_fwd in float32: constants rounded once, the same operation order.  clamp (mutant): the right
    neighbour of the last pair is the pair itself instead of pair 0."""
    assert x.dtype == np.float32
    x = np.moveaxis(x, axis, -1)
    e, o = x[..., 0::2], x[..., 1::2]
    if wavelet == "haar":
        s, d = (e + o) / S2_32, (o - e) / S2_32
    else:
        d1 = o - R3_32 * e
        d1n = np.roll(d1, -1, axis=-1)
        if clamp and d1.shape[-1]:
            d1n[..., -1] = d1[..., -1]
        s1 = e + A_32 * d1 + lb * d1n
        d2 = d1 + np.roll(s1, 1, axis=-1)
        s, d = C1_32 * s1, C2_32 * d2
    out = np.moveaxis(np.concatenate([s, d], axis=-1), -1, axis)
    assert out.dtype == np.float32
    return out


def lift_inv32(y, wavelet, axis):
    assert y.dtype == np.float32
    y = np.moveaxis(y, axis, -1)
    n = y.shape[-1] // 2
    s, d = y[..., :n], y[..., n:]
    if wavelet == "haar":
        e, o = (s - d) / S2_32, (s + d) / S2_32
    else:
        s1, d2 = s / C1_32, d / C2_32
        d1 = d2 - np.roll(s1, 1, axis=-1)
        e = s1 - A_32 * d1 - B_32 * np.roll(d1, -1, axis=-1)
        o = d1 + R3_32 * e
    out = np.empty_like(y)
    out[..., 0::2], out[..., 1::2] = e, o
    return np.moveaxis(out, -1, axis)


def dwt2_f32(x, wavelet, levels, mutant=None):
    """oracle.dwt_cpu.dwt2 in float32.  mutant: one of MUTANTS — a wrong transform of the kind a kernel's index arithmetic
    produces; test_dwt_paths_cpu.py shows that the bound rejects each one on every case where it changes a bit.
      clamp             db2: the right neighbour of the last column pair clamped instead of wrapped (horizontal pass only)
      swap_hl_lh        the HL and LH quadrants of every level exchanged
      lb_scaled         db2: LB * (1 + 2^-16)
      short_region      level >= 2 transforms a region one column pair short: the last pair of every row stays as it was
      offsets_exchanged the quadrant offsets (h/2 for rows, w/2 for columns) exchanged, indices wrapped to the region"""
    assert mutant is None or mutant in MUTANTS
    out = np.array(x, dtype=np.float32, copy=True)
    H, W = out.shape[-2:]
    h, w = H, W
    lb = F32(B_32 * F32(1.0 + 2.0 ** -16)) if mutant == "lb_scaled" else B_32
    assert mutant != "lb_scaled" or lb != B_32
    for lv in range(levels):
        reg = out[..., :h, :w]
        if mutant == "short_region" and lv >= 1:
            n = w // 2
            hz = reg.copy()
            part = lift_fwd32(reg[..., :w - 2], wavelet, -1)
            hz[..., :n - 1], hz[..., n - 1] = part[..., :n - 1], reg[..., w - 2]
            hz[..., n:2 * n - 1], hz[..., 2 * n - 1] = part[..., n - 1:], reg[..., w - 1]
        else:
            hz = lift_fwd32(reg, wavelet, -1, clamp=mutant == "clamp", lb=lb)
        res = lift_fwd32(hz, wavelet, -2, lb=lb)
        h2, w2 = h // 2, w // 2
        if mutant == "swap_hl_lh":
            hl, lh = res[..., :h2, w2:].copy(), res[..., h2:, :w2].copy()
            res[..., :h2, w2:], res[..., h2:, :w2] = lh, hl
        elif mutant == "offsets_exchanged":
            q = {(a, b): res[..., a * h2:(a + 1) * h2, b * w2:(b + 1) * w2].copy() for a in (0, 1) for b in (0, 1)}
            r, c = np.arange(h2)[:, None], np.arange(w2)[None, :]
            for (a, b), v in q.items():          # ll first, hh last, as the kernel's stores
                res[..., (a * w2 + r) % h, (b * h2 + c) % w] = v
        out[..., :h, :w] = res
        h, w = h2, w2
    return out


def idwt2_f32(c, wavelet, levels):
    out = np.array(c, dtype=np.float32, copy=True)
    H, W = out.shape[-2:]
    for lv in reversed(range(levels)):
        h, w = H >> lv, W >> lv
        out[..., :h, :w] = lift_inv32(lift_inv32(out[..., :h, :w], wavelet, -2), wavelet, -1)
    return out


def bands(H, W, levels):
    """The sub-bands of the Mallat layout: (level, name, row slice, column slice); level 1 is the finest.  hl: high horizontal /
    low vertical (top right), lh: bottom left, hh: bottom right; ll: what the last level leaves."""
    for lv in range(1, levels + 1):
        h, w = H >> lv, W >> lv
        yield lv, "hl", slice(0, h), slice(w, 2 * w)
        yield lv, "lh", slice(h, 2 * h), slice(0, w)
        yield lv, "hh", slice(h, 2 * h), slice(w, 2 * w)
    yield levels, "ll", slice(0, H >> levels), slice(0, W >> levels)


def band_ratios(got, ref, yard, levels, against=None):
    """Per band: err / max(yard_band, 2^-24 max|ref_band|) -> [(level, band, ratio, err, yard_band, max|ref_band|, size)].  got / yard:
    device (or mutant) and fp32-restatement coefficients, ref: the float64 oracle's, all [..., H, W].  against: measure err as the
    distance to this array instead of ref (two device results against one another, in the oracle's units)."""
    H, W = ref.shape[-2:]
    got = np.asarray(got, dtype=np.float64)
    other = ref if against is None else np.asarray(against, dtype=np.float64)
    assert got.shape == ref.shape == yard.shape == other.shape
    rows = []
    for lv, nm, rs, cs in bands(H, W, levels):
        r = ref[..., rs, cs]
        err = float(np.abs(got[..., rs, cs] - other[..., rs, cs]).max())
        yb = float(np.abs(yard[..., rs, cs].astype(np.float64) - r).max())
        top = float(np.abs(r).max())
        unit = max(yb, EPS * top)
        rows.append((lv, nm, (err / unit) if unit > 0 else (0.0 if err == 0 else np.inf), err, yb, top, r.size))
    return rows


def over_bound(rows, path):
    """The bands of band_ratios' answer that break the bound of forward path `path` -> [(level, band, ratio, K of the band)]."""
    return [(t[0], t[1], round(t[2], 2), band_k(path, t[6])) for t in rows if not t[2] <= band_k(path, t[6])]


def worst(rows):
    return max(rows, key=lambda r: r[2])


def image_ratio(got, ref, yard):
    """The whole-image form (inverse, round trip): max|got - ref| / max(max|yard - ref|, 2^-24 max|ref|) -> (ratio, err, yard)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.abs(got - ref).max())
    yd = float(np.abs(np.asarray(yard, dtype=np.float64) - ref).max())
    return err / max(yd, EPS * float(np.abs(ref).max())), err, yd


@functools.lru_cache(maxsize=None)
def _reference(shape, seed, levels, wavelet):
    x = np.random.RandomState(1000 + seed).randn(*shape).astype(np.float32)
    ref = O.dwt2(x, wavelet, levels)
    c32 = ref.astype(np.float32)
    r = {"x": x, "ref": ref, "yard": dwt2_f32(x, wavelet, levels), "coef32": c32,
         "inv_yard": idwt2_f32(c32, wavelet, levels)}
    r["trip_yard"] = idwt2_f32(r["yard"], wavelet, levels)
    for v in r.values():
        v.setflags(write=False)
    return r


def reference(name, wavelet):
    """x (float32), ref = oracle.dwt2(x) (float64), yard = dwt2_f32(x), coef32 = float32(ref), inv_yard = idwt2_f32(coef32),
    trip_yard = idwt2_f32(dwt2_f32(x)); computed once per (case, wavelet), read-only."""
    c = CASES[name]
    return _reference(c["shape"], c["seed"], c["levels"], wavelet)


def reference_of(x, wavelet, levels):
    """The same dict for an input of the caller's (tests/test_dwt.py)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ref = O.dwt2(x, wavelet, levels)
    c32 = ref.astype(np.float32)
    return {"x": x, "ref": ref, "yard": dwt2_f32(x, wavelet, levels), "coef32": c32, "inv_yard": idwt2_f32(c32, wavelet, levels)}


# ================================================================================================ the ramp
RAMP = (0.3125, 0.1875, 3.0)     # a, b, c0: dyadic, so the float32 ramp is exact and the oracle's detail bands vanish
RAMP_SIZES = (64, 256)


def ramp_input(n):
    a, b, c0 = RAMP
    r, c = np.arange(n, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
    x = a * r + b * c + c0
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return x.astype(np.float32).reshape(1, 1, n, n)


def ramp_interior(coef):
    """The three level-1 detail bands at least two pairs from the periodic seam -> one flat array."""
    n = coef.shape[-1] // 2
    i, d = slice(2, n - 2), n
    return np.concatenate([np.asarray(coef)[..., i, d + 2:2 * d - 2].ravel(), np.asarray(coef)[..., d + 2:2 * d - 2, i].ravel(),
                           np.asarray(coef)[..., d + 2:2 * d - 2, d + 2:2 * d - 2].ravel()])


def ramp_yardstick(n):
    """max |detail| of the fp32 restatement on the ramp, away from the seam: pure rounding (the oracle's are < 1e-10)."""
    return float(np.abs(ramp_interior(dwt2_f32(ramp_input(n), "db2", 1))).max())
