"""The argument tuples the nine convolution entry points refuse (csrc/conv.hip, csrc/conv_x3.hip: every WTPSE_REQUIRE clause that
can be reached through the C ABI), on a host without a GPU.

Every entry point (and every `layout` of the three that take one) has a base tuple that satisfies all of its preconditions; a case
changes the base so that exactly one clause fails and expects WTPSE_EINVAL (-1).  The clauses are checked before anything is launched,
so the pointers are placeholders into one 16-byte-aligned host buffer that nothing dereferences.  The base tuples themselves pass the
checks and reach the launch, which on a host without a device comes back with a HIP status (not -1): that is asserted too — it is what
shows that a case fails for its own clause and not for one the base already broke.  A validator that wrongly accepts a placeholder
tuple must never reach a device: the module skips itself where a GPU is visible."""
import ctypes

import numpy as np
import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("placeholder pointers: host without a GPU only", allow_module_level=True)

_BUF = np.zeros(64, dtype=np.float64)
P = (_BUF.ctypes.data + 15) & ~15          # a 16-byte-aligned placeholder for every pointer argument
ODD = P + 8                                # ... and one that is not 16-byte aligned
MOM, EPS = 0.1, 1e-5

FWD = "in0 C0 in1 C1 wpacked bias pro0 pro1 pro_relu out0 out1 Csplit stats B H W Cout ksize relu_out mask_ref"
DGRAD = "dy C wpacked out0 out1 Csplit bn_y bn_ss bn_mean bn_relu bn_c0 bn_c1 stats B H W Cout ksize"
COEF = "dy C wpacked layout out0 out1 Csplit bn_y bn_ss bn_mean bn_relu bn_c0 bn_c1 stats gamma invstd coef dgamma dbeta %s" \
       "accumulate partial2 tickets B H W Cout ksize in_amax stream"
ARGS = {
    "wtpse_conv_fwd": FWD + " out_amax stream",
    "wtpse_conv_fwd_x3": FWD + " in_amax in_amax1 out_amax stream",
    "wtpse_conv_fwd_gram": "in0 C0 wpacked bias pro0 pro_relu out0 gram_partial B H W Cout relu_out out_amax stream",
    "wtpse_conv16_x3": "in0 C0 wx16 bias pro0 pro_relu out0 stats gram_partial mask_ref bn_ss bn_mean bn_relu B H W Cout relu_out "
                       "in_is_grad in_amax out_amax stream",
    "wtpse_dgrad_bnb": DGRAD + " stream",
    "wtpse_dgrad_x3_bnb": DGRAD + " in_amax stream",
    "wtpse_conv_fwd_bnf": "in0 C0 in1 C1 wpacked layout bias pro0 pro1 pro_relu out0 stats gamma beta running_mean running_var "
                          "num_batches momentum eps scale_shift save_mean save_invstd partial2 tickets B H W Cout ksize in_amax0 "
                          "in_amax1 act_amax stream",
    "wtpse_dgrad_bnb_coef": COEF % "",
    "wtpse_dgrad_bnb_coef_frozen": COEF % "dbias ",
}
ARGS = {k: v.split() for k, v in ARGS.items()}

SHAPE = dict(B=1, H=8, W=8)
# 64-channel blocks of the x3 kernels (512 workgroups of them): the only launches that stage up to 512 prologue coefficients
SHAPE_MT2 = dict(B=8, H=64, W=64, Cout=256)
# 64-channel blocks on 128-pixel tiles (3x3, 512 workgroups of them where the 256-pixel tiling gives 256): 256 coefficients like the rest
SHAPE_HALF = dict(B=8, H=64, W=64, Cout=128)


def _fwd_base(**kw):
    """Two inputs of 16 channels, two outputs of 16 channels, bias, ReLU."""
    d = dict(in0=P, C0=16, in1=P, C1=16, wpacked=P, bias=P, pro_relu=0, out0=P, out1=P, Csplit=16, Cout=32, ksize=3, relu_out=1, **SHAPE)
    d.update(kw)
    return d


def _dgrad_base(**kw):
    """48 -> 32 channels in two outputs of 16, BatchNorm statistics over the second."""
    d = dict(dy=P, C=48, wpacked=P, out0=P, out1=P, Csplit=16, bn_y=P, bn_ss=P, bn_mean=P, bn_relu=1, bn_c0=16, bn_c1=32, stats=P,
             Cout=32, ksize=3, **SHAPE)
    d.update(kw)
    return d


def _one_output(d):
    return dict(d, out1=None, Csplit=d["Cout"])


def _first(d):        # the null pointers and non-positive sizes of an implementation's first clause
    inp, cin, w = ("dy", "C", "wpacked") if "dy" in d else ("in0", "C0", "wx16" if "wx16" in d else "wpacked")
    return [("no_" + n, {n: None}) for n in (inp, w, "out0")] + [(n + "_0", {n: 0}) for n in ("B", "H", "W", cin)]


TWO_INPUTS = [("C1_negative", dict(C1=-16)), ("in1_without_C1", dict(C1=0)), ("C1_without_in1", dict(in1=None)),
              ("C0_splits_a_chunk", dict(C0=8))]
KSIZE = [("ksize_2", dict(ksize=2)), ("ksize_5", dict(ksize=5))]
SPLIT = [("Csplit_0", dict(Csplit=0)), ("Csplit_over_Cout", dict(Csplit=48)), ("out1_without_split", dict(Csplit=32)),
         ("split_without_out1", dict(out1=None)), ("Csplit_mod_16", dict(Csplit=8))]
BN_RANGE = [("bn_c0_negative", dict(bn_c0=-16)), ("bn_range_empty", dict(bn_c0=32)), ("bn_c1_over_Cout", dict(bn_c1=48)),
            ("bn_c0_mod_16", dict(bn_c0=8)), ("bn_c1_mod_16", dict(bn_c1=24))]
BN_PTRS = [("no_" + n, {n: None}) for n in ("bn_y", "bn_ss", "bn_mean", "stats")]
COEF_PTRS = [("no_" + n, {n: None}) for n in ("gamma", "invstd", "coef", "dgamma", "dbeta", "partial2", "tickets")]
BNF_PTRS = [("no_" + n, {n: None}) for n in ("stats", "gamma", "beta", "scale_shift", "save_mean", "save_invstd", "partial2", "tickets")]
LAYOUT = [("layout_negative", dict(layout=-1)), ("layout_3", dict(layout=3))]
RUNNING = [("running_mean_alone", dict(running_var=None)), ("running_var_alone", dict(running_mean=None))]


def _fwd_options(d):
    """The exclusions between stats, relu_out, mask_ref, out1 and out_amax that every forward implementation states."""
    one = _one_output(d)
    return [("stats_with_relu", dict(stats=P)),
            ("stats_with_mask", dict(one, stats=P, relu_out=0, mask_ref=P)),
            ("mask_with_out1", dict(mask_ref=P)),
            ("out_amax_with_mask", dict(one, mask_ref=P, out_amax=P))]


# name -> [(tag, base tuple, [(case, overrides)])]
ENTRIES = {}

b = _fwd_base()
ENTRIES["wtpse_conv_fwd"] = [("", b, _first(b) + TWO_INPUTS + KSIZE + SPLIT + _fwd_options(b))]

ENTRIES["wtpse_conv_fwd_x3"] = [
    ("", b, _first(b) + TWO_INPUTS + KSIZE + SPLIT + _fwd_options(b) + [
        ("in_amax1_without_in1", dict(in1=None, C1=0, in_amax1=P)),
        ("CinP_over_256", dict(C0=272, in1=None, C1=0))]),
    ("mt2", _fwd_base(C0=512, in1=None, C1=0, Csplit=128, **SHAPE_MT2), [("CinP_over_512", dict(C0=528))]),
    ("mt2_two_inputs", _fwd_base(C0=256, C1=256, Csplit=128, **SHAPE_MT2), [("CinP_over_512", dict(C1=272))]),
    ("half", _fwd_base(C0=256, in1=None, C1=0, Csplit=64, **SHAPE_HALF), [("CinP_over_256", dict(C0=272))]),
]

b = dict(in0=P, C0=8, wpacked=P, bias=P, pro0=P, pro_relu=1, out0=P, gram_partial=P, Cout=16, relu_out=0, out_amax=P, **SHAPE)
ENTRIES["wtpse_conv_fwd_gram"] = [("", b, _first(b) + [("no_gram", dict(gram_partial=None)), ("Cout_8", dict(Cout=8)),
                                                       ("Cout_32", dict(Cout=32)), ("relu_out", dict(relu_out=1))])]

b = dict(in0=P, C0=16, wx16=P, bias=P, pro0=P, pro_relu=1, out0=P, Cout=16, relu_out=1, in_amax=P, out_amax=P, **SHAPE)
bn = dict(b, bias=None, relu_out=0, out_amax=None, stats=P, mask_ref=P, bn_ss=P, bn_mean=P, bn_relu=1, in_is_grad=1)
ENTRIES["wtpse_conv16_x3"] = [
    ("", b, _first(b) + [("C0_17", dict(C0=17)), ("Cout_17", dict(Cout=17)), ("Cout_0", dict(Cout=0)),
                         ("stats_with_relu", dict(stats=P)),
                         ("gram_with_Cout_8", dict(gram_partial=P, Cout=8, relu_out=0)),
                         ("gram_with_relu", dict(gram_partial=P)),
                         ("fragments_misaligned", dict(wx16=ODD)),
                         ("stats_with_mask", dict(stats=P, mask_ref=P, relu_out=0, out_amax=None)),
                         ("out_amax_with_mask", dict(mask_ref=P))]),
    ("bnb", bn, [("no_mask_ref", dict(mask_ref=None)), ("no_stats", dict(stats=None)), ("no_bn_ss", dict(bn_ss=None)),
                 ("bias", dict(bias=P)), ("gram", dict(gram_partial=P)), ("C0_17", dict(C0=17)), ("fragments_misaligned", dict(wx16=ODD))]),
]

b = _dgrad_base()
ENTRIES["wtpse_dgrad_bnb"] = [("", b, BN_PTRS + _first(b) + KSIZE + SPLIT + BN_RANGE)]
ENTRIES["wtpse_dgrad_x3_bnb"] = [
    ("", b, BN_PTRS + _first(b) + KSIZE + SPLIT + BN_RANGE + [("CinP_over_256", dict(C=272))]),
    ("mt2", _dgrad_base(C=512, Csplit=128, bn_c0=128, bn_c1=256, **SHAPE_MT2), [("CinP_over_512", dict(C=528))]),
    ("half", _dgrad_base(C=256, Csplit=64, bn_c0=64, bn_c1=128, **SHAPE_HALF), [("CinP_over_256", dict(C=272))]),
]

b = dict(in0=P, C0=16, in1=P, C1=16, wpacked=P, bias=P, pro0=P, pro1=P, pro_relu=3, out0=P, stats=P, gamma=P, beta=P, running_mean=P,
         running_var=P, num_batches=P, momentum=MOM, eps=EPS, scale_shift=P, save_mean=P, save_invstd=P, partial2=P, tickets=P, Cout=32,
         ksize=3, in_amax0=P, in_amax1=P, act_amax=P, **SHAPE)
b16 = dict(b, in1=None, C1=0, pro1=None, Cout=16)        # in_amax1 stays: the 16-channel layout ignores it
ENTRIES["wtpse_conv_fwd_bnf"] = [
    ("fp32", dict(b, layout=0), BNF_PTRS + LAYOUT + RUNNING + _first(b) + TWO_INPUTS + KSIZE + [("Cout_0", dict(Cout=0))]),
    ("x3", dict(b, layout=1, in_amax1=None), BNF_PTRS + RUNNING + _first(b) + TWO_INPUTS + KSIZE + [
        ("in_amax1_without_in1", dict(in1=None, C1=0, in_amax1=P)), ("CinP_over_256", dict(C0=272, in1=None, C1=0)),
        ("Cout_0", dict(Cout=0))]),
    ("x3_two_amax", dict(b, layout=1), []),
    ("x3_mt2", dict(b, layout=1, C0=512, in1=None, C1=0, in_amax1=None, **SHAPE_MT2), [("CinP_over_512", dict(C0=528))]),
    ("x3_half", dict(b, layout=1, C0=256, in1=None, C1=0, in_amax1=None, **SHAPE_HALF), [("CinP_over_256", dict(C0=272))]),
    ("c16", dict(b16, layout=2), BNF_PTRS + RUNNING + _first(b16) + [
        ("ksize_1", dict(ksize=1)), ("in1", dict(in1=P)), ("C1", dict(C1=16)), ("second_input", dict(in1=P, C1=16)), ("pro1", dict(pro1=P)), ("C0_17", dict(C0=17)),
        ("Cout_17", dict(Cout=17)), ("Cout_0", dict(Cout=0)), ("fragments_misaligned", dict(wpacked=ODD))]),
]

for name, extra in (("wtpse_dgrad_bnb_coef", {}), ("wtpse_dgrad_bnb_coef_frozen", dict(dbias=P))):
    b = _dgrad_base(gamma=P, invstd=P, coef=P, dgamma=P, dbeta=P, accumulate=1, partial2=P, tickets=P, in_amax=P, **extra)
    b16 = dict(_one_output(b), C=16, Cout=16, Csplit=16, bn_c0=0, bn_c1=16)
    ptrs = BN_PTRS + COEF_PTRS + [("no_" + n, {n: None}) for n in extra]
    ENTRIES[name] = [
        ("fp32", dict(b, layout=0), ptrs + LAYOUT + _first(b) + KSIZE + SPLIT + BN_RANGE),
        ("x3", dict(b, layout=1), ptrs + _first(b) + KSIZE + SPLIT + BN_RANGE + [("CinP_over_256", dict(C=272))]),
        ("x3_mt2", dict(b, layout=1, C=512, Csplit=128, bn_c0=128, bn_c1=256, **SHAPE_MT2), [("CinP_over_512", dict(C=528))]),
        ("x3_half", dict(b, layout=1, C=256, Csplit=64, bn_c0=64, bn_c1=128, **SHAPE_HALF), [("CinP_over_256", dict(C=272))]),
        ("c16", dict(b16, layout=2), ptrs + _first(b16) + [
            ("ksize_1", dict(ksize=1)), ("out1", dict(out1=P)), ("Csplit_8", dict(Csplit=8)), ("bn_c0_8", dict(bn_c0=8)),
            ("bn_c1_8", dict(bn_c1=8)), ("C_17", dict(C=17)), ("Cout_32", dict(Cout=32, Csplit=32, bn_c1=32)),
            ("fragments_misaligned", dict(wpacked=ODD))]),
    ]

BASES = [pytest.param(name, base, id="%s%s" % (name[6:], "-" + tag if tag else ""))
         for name, groups in ENTRIES.items() for tag, base, _ in groups]
CASES = [pytest.param(name, dict(base, **over), id="%s%s-%s" % (name[6:], "-" + tag if tag else "", case))
         for name, groups in ENTRIES.items() for tag, base, cases in groups for case, over in cases]


@pytest.fixture(scope="module")
def raw():
    from wtpse_hip import build, lib
    build.build()
    return lib.lib().raw


def _call(raw, name, values):
    names = ARGS[name]
    fn = raw(name)
    assert len(names) == len(fn.argtypes), name
    assert set(values) <= set(names), sorted(set(values) - set(names))
    args = [values.get(n, 0.0 if t is ctypes.c_float else (None if t is ctypes.c_void_p else 0)) for n, t in zip(names, fn.argtypes)]
    return fn(*args)


def test_every_entry_point_is_covered():
    assert sorted(ENTRIES) == sorted(ARGS) and len(ARGS) == 9
    for name in ("wtpse_conv_fwd_bnf", "wtpse_dgrad_bnb_coef", "wtpse_dgrad_bnb_coef_frozen"):
        assert {base["layout"] for _, base, _ in ENTRIES[name]} == {0, 1, 2}


@pytest.mark.parametrize("name,values", BASES)
def test_base_tuple_passes_every_precondition(raw, name, values):
    """Nothing is refused: the call gets as far as the launch, which has no device to run on."""
    assert _call(raw, name, values) not in (0, -1)


@pytest.mark.parametrize("name,values", CASES)
def test_one_broken_precondition_is_refused(raw, name, values):
    assert _call(raw, name, values) == -1
