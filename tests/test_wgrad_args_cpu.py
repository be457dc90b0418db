"""The argument tuples the four weight-gradient entry points refuse (csrc/conv.hip, csrc/conv_x3.hip, csrc/wgrad_r.hip), on a host
without a GPU, in the manner of tests/test_conv_args_cpu.py: placeholder pointers that nothing dereferences, a base tuple per entry
point and form that satisfies every precondition (asserted to reach the launch: neither 0 nor -1 on a host without a device), and
cases that change a base so that one clause fails and expect WTPSE_EINVAL (-1).

The slab count of a tuple is what the size query of its family answers for the tuple's own sizes (QUERY), asked for the base and
kept by its cases; a case that needs the count of its own sizes says QUERY again, one that breaks the count gives a function of
the base's.

What cannot be isolated through the ABI:
  * a non-positive size or channel count also fails what is derived from it: the tile count that bounds the k-split,
    wtpse_wgrad_x3_supported / wtpse_wgrad_r_supported, the slab count of the plan;
  * `!(dbias && bn_y)`: no entry point passes both (wtpse_conv_wgrad_r has no bn_y, wtpse_conv_wgrad_r_bn no dbias);
  * `(bn_y == nullptr) == (bn_coef == nullptr)`: wtpse_conv_wgrad_r_bn asks for both first, wtpse_conv_wgrad_r passes neither;
  * the twin form (W == 16) needing 2 x 2 blocks and no bias gradient: wtpse_wgrad_r_supported refuses the other blocks at that
    width and `!dbias || mf * nf == 1` refuses the bias; its third part, no _bn form, has a case;
  * wgrad_r_plan refusing a tuple: it restates conditions of wtpse_wgrad_r_supported."""
import ctypes

import pytest

from test_conv_args_cpu import P, raw  # noqa: F401  (the placeholder pointer; `raw` is that module's fixture, and its skip where a GPU is visible)

QUERY = "query"

ARGS = {
    "wtpse_conv_wgrad": "dy x0 C0 x1 C1 pro0 pro1 pro_relu slab dbias_slab ksplit dw dbias accumulate B H W Cout ksize stream",
    "wtpse_conv_wgrad_x3": "dy x0 C0 x1 C1 pro0 pro1 pro_relu slab ksplit dw accumulate B H W Cout ksize stream",
    "wtpse_conv_wgrad_r": "dy x0 C0 x1 C1 pro0 pro1 pro_relu slab dbias_slab nslab dw dbias accumulate B H W Cout dy_amax x_amax0 "
                          "x_amax1 stream",
    "wtpse_conv_wgrad_r_bn": "g bn_y bn_coef x0 C0 x1 C1 pro0 pro1 pro_relu slab nslab dw accumulate B H W Cout stream",
}
ARGS = {k: v.split() for k, v in ARGS.items()}
# entry point -> (its size query, the name of its slab-count argument)
COUNT = {"wtpse_conv_wgrad": ("wtpse_wgrad_ksplit", "ksplit"), "wtpse_conv_wgrad_x3": ("wtpse_wgrad_x3_ksplit", "ksplit"),
         "wtpse_conv_wgrad_r": ("wtpse_wgrad_r_slabs", "nslab"), "wtpse_conv_wgrad_r_bn": ("wtpse_wgrad_r_slabs", "nslab")}

SHAPE = dict(B=1, H=8, W=8)          # one tile in every tiling of conv_wgrad_k and of the 32-channel blocks of conv_wgrad_x3_k
BIAS = dict(dbias=P, dbias_slab=P)
ONE_INPUT = dict(x1=None, C1=0)


def _base(dy="dy", **kw):
    """16 + 16 -> 32 channels with a prologue on both inputs, accumulating."""
    d = {dy: P}
    d.update(x0=P, C0=16, x1=P, C1=16, pro0=P, pro1=P, pro_relu=3, slab=P, dw=P, accumulate=1, Cout=32, **SHAPE)
    d.update(kw)
    return d


def _shared(d, count):
    """The clauses every entry point states: required pointers, positive sizes, the second input and its channel count."""
    dy = "dy" if "dy" in d else "g"
    cases = [("no_" + n, {n: None}) for n in (dy, "x0", "slab", "dw")] + [(n + "_0", {n: 0}) for n in ("B", "H", "W", "C0", "Cout")]
    if d["C1"]:
        cases += [("C1_negative", dict(C1=-d["C1"])), ("x1_without_C1", {"C1": 0, count: QUERY}), ("C1_without_x1", dict(x1=None))]
    else:
        cases += [("x1_without_C1", dict(x1=P)), ("C1_without_x1", {"C1": d["C0"], count: QUERY})]
    return cases


BIAS_PAIR = [("dbias_without_slab", dict(dbias_slab=None)), ("slab_without_dbias", dict(dbias=None))]
NO_BIAS_PAIR = [("dbias_without_slab", dict(dbias=P)), ("slab_without_dbias", dict(dbias_slab=P))]
# B = 1, 8 x 8: the query answers the tile count (one tile, and at least one slab), so one more is one above the tiles
KSPLIT = [("ksplit_0", dict(ksplit=0)), ("ksplit_over_tiles", dict(ksplit=lambda n: n + 1))]
NSLAB = [("nslab_minus_1", dict(nslab=lambda n: n - 1)), ("nslab_plus_1", dict(nslab=lambda n: n + 1))]

# name -> [(tag, base tuple, [(case, overrides)])]
ENTRIES = {}

b = _base(ksize=3, ksplit=QUERY, **BIAS)
ENTRIES["wtpse_conv_wgrad"] = [
    ("", b, _shared(b, "ksplit") + BIAS_PAIR + KSPLIT + [("ksize_2", dict(ksize=2)), ("ksize_5", dict(ksize=5)),
                                                         ("C0_splits_a_group", dict(C0=8, C1=24))]),
    ("1x1", dict(b, ksize=1), KSPLIT + [("C0_splits_a_group", dict(C0=8, C1=24))]),
    ("one_input", dict(b, dbias=None, dbias_slab=None, **ONE_INPUT),
     _shared(dict(b, **ONE_INPUT), "ksplit") + NO_BIAS_PAIR + KSPLIT),
    ("1x1_one_input", dict(b, ksize=1, dbias=None, dbias_slab=None, **ONE_INPUT), NO_BIAS_PAIR),
    ("one_input_bias", dict(b, C0=8, **ONE_INPUT), []),      # C0 % 16 binds behind a concat only
]

b = _base(ksize=3, ksplit=QUERY)
b1 = dict(b, C0=32, **ONE_INPUT)
ENTRIES["wtpse_conv_wgrad_x3"] = [
    ("blocks", b1, _shared(b1, "ksplit") + KSPLIT + [("ksize_1", dict(ksize=1)), ("Cin_48", dict(C0=48)), ("Cout_48", dict(Cout=48)),
                                                     ("Cin_16", dict(C0=16))]),
    ("blocks_two_inputs", b, KSPLIT + [("ksize_1", dict(ksize=1)), ("Cin_48", dict(C1=32)),
                                                              ("Cout_48", dict(Cout=48)), ("C0_4_behind_concat", dict(C0=4, C1=28))]),
    ("blocks_concat_64", dict(b, C0=32, C1=32), _shared(dict(b, C0=32, C1=32), "ksplit")),
    ("blocks_C0_8", dict(b, C0=8, C1=24), []),               # the x3 kernel takes a concat at every multiple of 8
    ("quadrants", dict(b1, C0=64, Cout=64), [("ksplit_0", dict(ksplit=0)), ("Cin_80", dict(C0=80, ksplit=QUERY)),
                                            ("Cout_80", dict(Cout=80, ksplit=QUERY))]),
    ("quadrants_two_inputs", dict(b, C0=32, C1=32, Cout=64), [("C0_4_behind_concat", dict(C0=4, C1=60))]),
]

b = _base(nslab=QUERY, W=32, dy_amax=P, x_amax0=P, x_amax1=P)
b16 = dict(b, C0=16, Cout=16, x_amax1=None, **ONE_INPUT)
b32 = dict(b, C0=32, x_amax1=None, **ONE_INPUT)
BIG = dict(C0=32, Cout=32, H=4096, W=4096, nslab=QUERY)     # a plane of 32 channels: 2^31 bytes
ENTRIES["wtpse_conv_wgrad_r"] = [
    ("c16_bias", dict(b16, **BIAS), BIAS_PAIR + NSLAB + [
        ("W_16_with_16_channels", dict(W=16, nslab=QUERY)), ("W_24", dict(W=24)), ("Cin_8", dict(C0=8)), ("Cout_24", dict(Cout=24))]),
    ("c16", b16, _shared(b16, "nslab") + NO_BIAS_PAIR + NSLAB),
    ("c16_no_amax", dict(b16, dy_amax=None, x_amax0=None), NSLAB),
    ("blocks_2x2", b32, _shared(b32, "nslab") + NSLAB + [
        ("bias_with_32_channels", dict(BIAS)), ("bias_with_32_inputs", dict(BIAS, Cout=16, nslab=QUERY)),
        ("bias_with_32_outputs", dict(BIAS, C0=16, nslab=QUERY)), ("W_24", dict(W=24)), ("W_48", dict(W=48)),
        ("x_plane_2G", dict(BIG, Cout=16)), ("dy_plane_2G", dict(BIG, C0=16))]),
    ("blocks_2x2_under_2G", dict(b32, H=4096, W=4064), []),
    ("twin", dict(b32, W=16), NSLAB + [("bias", dict(BIAS)), ("Cin_48", dict(C0=48, nslab=QUERY)), ("Cout_16", dict(Cout=16, nslab=QUERY))]),
    ("concat", b, _shared(b, "nslab") + NSLAB + [("C0_8_behind_concat", dict(C0=8, C1=24)), ("x1_plane_2G", dict(BIG, C0=16, C1=32, Cout=16))]),
]

b = _base(dy="g", nslab=QUERY, W=32, bn_y=P, bn_coef=P)
b32 = dict(b, C0=32, **ONE_INPUT)
ENTRIES["wtpse_conv_wgrad_r_bn"] = [
    ("", b32, _shared(b32, "nslab") + NSLAB + [("no_bn_y", dict(bn_y=None)), ("no_bn_coef", dict(bn_coef=None)), ("W_24", dict(W=24)),
                                               ("twin", dict(W=16, nslab=QUERY)), ("dy_plane_2G", dict(BIG, C0=16))]),
    ("c16", dict(b32, C0=16, Cout=16), NSLAB + [("no_bn_y", dict(bn_y=None))]),
    ("concat", b, _shared(b, "nslab") + [("C0_8_behind_concat", dict(C0=8, C1=24)), ("no_bn_coef", dict(bn_coef=None))]),
]

BASES = [pytest.param(name, base, {}, id="%s%s" % (name[6:], "-" + tag if tag else ""))
         for name, groups in ENTRIES.items() for tag, base, _ in groups]
CASES = [pytest.param(name, base, over, id="%s%s-%s" % (name[6:], "-" + tag if tag else "", case))
         for name, groups in ENTRIES.items() for tag, base, cases in groups for case, over in cases]


def _count(raw, name, d):
    return raw(COUNT[name][0])(d["B"], d["H"], d["W"], d["C0"] + d["C1"], d["Cout"])


def _call(raw, name, base, over):
    names, key = ARGS[name], COUNT[name][1]
    fn = raw(name)
    assert len(names) == len(fn.argtypes), name
    assert base[key] == QUERY and set(base) | set(over) <= set(names), sorted((set(base) | set(over)) - set(names))
    values = dict(base, **over)
    n = over.get(key, _count(raw, name, base))
    values[key] = _count(raw, name, values) if n == QUERY else n(_count(raw, name, base)) if callable(n) else n
    if not over:
        assert values[key] >= 1, (name, values[key])
    args = [values.get(n, None if t is ctypes.c_void_p else 0) for n, t in zip(names, fn.argtypes)]
    return fn(*args)


def test_every_entry_point_is_covered():
    assert sorted(ENTRIES) == sorted(ARGS) == sorted(COUNT) and len(ARGS) == 4
    ids = [p.id for p in BASES + CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)
    for name, groups in ENTRIES.items():
        assert any(cases for _, _, cases in groups), name


def test_one_tile_bounds_the_default_split(raw):
    """ksplit_over_tiles is one above the tiles: at the bases' shape the query answers the tile count."""
    assert raw("wtpse_wgrad_ksplit")(1, 8, 8, 32, 32) == raw("wtpse_conv_stats_blocks")(1, 8, 8) == 1
    assert raw("wtpse_wgrad_x3_ksplit")(1, 8, 8, 32, 32) == 1          # 128 pixels of an 8 x 8 map: one tile


@pytest.mark.parametrize("name,base,over", BASES)
def test_base_tuple_passes_every_precondition(raw, name, base, over):
    """Nothing is refused: the call gets as far as the launch, which has no device to run on."""
    assert _call(raw, name, base, over) not in (0, -1)


@pytest.mark.parametrize("name,base,over", CASES)
def test_one_broken_precondition_is_refused(raw, name, base, over):
    assert _call(raw, name, base, over) == -1
