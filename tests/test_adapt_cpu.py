"""wtpse_hip/adapt.py on the host: the float64 specification of the blended BatchNorm statistics (weight rule, blend, divergence,
activation bound), the adapted checkpoint's dict, shift.csv / shift.json through tables.py, the switches of the run programs, and the
new entry point's place in the header and the binding."""
import argparse

import numpy as np
import pytest
import torch

from wtpse_hip import adapt as A


def _stats(rng, C, lo=0.5, hi=2.0):
    return rng.normal(size=C), rng.uniform(lo, hi, size=C)


# ---- the specification ------------------------------------------------------------------------------------------------------------
def test_blend_returns_source_at_0_and_target_at_1():
    rng = np.random.default_rng(0)
    (ms, vs), (mt, vt) = _stats(rng, 7), _stats(rng, 7)
    m, v = A.blend_host(ms, vs, mt, vt, 0.0)
    assert np.array_equal(m, ms) and np.array_equal(v, vs)
    m, v = A.blend_host(ms, vs, mt, vt, 1.0)
    assert np.array_equal(m, mt) and np.array_equal(v, vt)
    m, v = A.blend_host(ms, vs, mt, vt, 0.25)
    assert np.allclose(m, 0.75 * ms + 0.25 * mt, rtol=1e-15) and np.allclose(v, 0.75 * vs + 0.25 * vt, rtol=1e-15)
    assert m.dtype == np.float64
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            A.blend_host(ms, vs, mt, vt, bad)
    # float32 inputs are widened, not computed in
    m32, _ = A.blend_host(ms.astype(np.float32), vs, mt, vt, 0.3)
    assert m32.dtype == np.float64


def test_weight_rule():
    assert A.DEFAULT_PRIOR == 16.0
    assert A.blend_weight(9) == 9.0 / 25.0 == 0.36
    assert A.blend_weight(16, 16) == 0.5
    assert A.blend_weight(1, 0) == 1.0 and A.blend_weight(1000, 0) == 1.0
    assert A.blend_weight(0, 16) == 0.0
    assert A.blend_weight(5, 2) == 5.0 / 7.0
    ws = [A.blend_weight(n, 16) for n in range(1, 200)]
    assert all(a < b for a, b in zip(ws, ws[1:])) and ws[-1] < 1.0
    for bad in ((0, 0), (-1, 16), (3, -1)):
        with pytest.raises(ValueError):
            A.blend_weight(*bad)


def test_target_pools_with_history():
    rng = np.random.default_rng(1)
    x, y = rng.normal(3.0, 2.0, size=(4, 500)), rng.normal(-1.0, 0.5, size=(4, 300))
    m, v = A.target_host(x.sum(1), (x * x).sum(1), 500)
    assert np.allclose(m, x.mean(1), rtol=1e-13) and np.allclose(v, x.var(1), rtol=1e-11)
    both = np.concatenate((x, y), 1)
    m, v = A.target_host(y.sum(1), (y * y).sum(1), 300, x.sum(1), (x * x).sum(1), 500)
    assert np.allclose(m, both.mean(1), rtol=1e-13) and np.allclose(v, both.var(1), rtol=1e-11)
    # cancellation never leaves a negative variance
    m, v = A.target_host(np.array([3e8]), np.array([9e16 - 1e3]), 1.0)
    assert v[0] == 0.0


def test_coefficients_are_float64_rounded_once():
    rng = np.random.default_rng(2)
    g, b = rng.normal(size=5), rng.normal(size=5)
    mb, vb = _stats(rng, 5)
    ss = A.coeffs_host(g, b, mb, vb)
    assert ss.dtype == np.float32 and ss.shape == (5, 2)
    scale = g / np.sqrt(vb + np.float64(np.float32(1e-5)))
    assert np.array_equal(ss[:, 0], scale.astype(np.float32)) and np.array_equal(ss[:, 1], (b - mb * scale).astype(np.float32))


def test_divergence_on_constructed_numbers():
    m, v = np.array([0.0, 1.5, -2.0]), np.array([1.0, 0.25, 4.0])
    assert np.array_equal(A.divergence_host(m, v, m, v), np.zeros(3))
    # a mean offset alone: D = d^2 / (2 (v + eps)), growing with |d|
    offs = [A.divergence_host(m, v, m + d, v) for d in (0.1, 0.5, 1.0, -2.0)]
    for d, got in zip((0.1, 0.5, 1.0, -2.0), offs):
        assert np.allclose(got, d * d / (2 * (v + A.EPS)), rtol=1e-12)
    assert all((a < b).all() for a, b in zip(offs, offs[1:]))
    # a variance ratio r > 1 alone: D = (r - 1 - ln r) / 2, growing with r
    ratios = [A.divergence_host(m, v, m, r * (v + A.EPS) - A.EPS) for r in (1.5, 2.0, 4.0, 10.0)]
    for r, got in zip((1.5, 2.0, 4.0, 10.0), ratios):
        assert np.allclose(got, 0.5 * (r - 1.0 - np.log(r)), rtol=1e-12)
    assert all((a < b).all() for a, b in zip(ratios, ratios[1:]))
    assert (A.divergence_host(m, v, m + 0.3, 0.5 * v) > 0).all()              # a KL divergence: positive off the diagonal
    # KL between the two normals, checked against numerical integration on one channel
    ms, vs, mt, vt = 0.3, 1.7, -0.4, 0.6
    x = np.linspace(-12, 12, 400001)
    pt = np.exp(-(x - mt) ** 2 / (2 * (vt + A.EPS))) / np.sqrt(2 * np.pi * (vt + A.EPS))
    logratio = -(x - mt) ** 2 / (2 * (vt + A.EPS)) + (x - ms) ** 2 / (2 * (vs + A.EPS)) + 0.5 * np.log((vs + A.EPS) / (vt + A.EPS))
    assert abs(float(np.sum(pt * logratio) * (x[1] - x[0])) - float(A.divergence_host(ms, vs, mt, vt))) < 1e-8


BOUND_CASES = ["centred", "offset100", "outlier", "offset100_outlier", "history"]


@pytest.mark.parametrize("case", BOUND_CASES)
def test_bound_covers_the_activated_output(case):
    rng = np.random.default_rng(40 + BOUND_CASES.index(case))
    C, M = 6, 4096
    y = rng.normal(size=(C, M))
    if "offset100" in case:
        y = y + 100.0                                   # |mean| / std = 100
    if "outlier" in case:
        y[:, 17] += 60.0 * np.array([1, -1, 1, -1, 1, -1])          # one sample 60 standard deviations out
    g, b = rng.normal(size=C) * 3.0, rng.normal(size=C)
    ms, vs = _stats(rng, C)
    s1, s2 = y.sum(1), (y * y).sum(1)
    mc, vc = A.target_host(s1, s2, M)
    if case == "history":                                # pooled with an earlier call far away: the call's own mean is off mean_b
        h = rng.normal(5.0, 3.0, size=(C, 1000))
        mt, vt = A.target_host(s1, s2, M, h.sum(1), (h * h).sum(1), 1000)
    else:
        mt, vt = mc, vc
    for w in (0.0, 0.36, 1.0):
        mb, vb = A.blend_host(ms, vs, mt, vt, w)
        ss = A.coeffs_host(g, b, mb, vb).astype(np.float64)
        z = np.abs(ss[:, :1] * y + ss[:, 1:]).max(1)
        bound = A.bound_host(g, b, mb, vb, mc, vc, M)
        assert np.isfinite(bound).all() and (bound >= z).all(), (case, w, bound / z)
        # the headroom is one binade over the inequality itself
        assert np.allclose(A.bound_host(g, b, mb, vb, mc, vc, M, headroom=1.0) * 2.0, bound, rtol=1e-15)


# ---- the adapted checkpoint -------------------------------------------------------------------------------------------------------
def _toy_state_dicts():
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    gen = torch.Generator().manual_seed(3)
    sds = []
    for i, _ in enumerate(CHECKPOINT_KEYS):
        sds.append({"inc.conv1.weight": torch.randn(4, 3, 3, 3, generator=gen), "inc.bn1.weight": torch.randn(4, generator=gen),
                    "inc.bn1.bias": torch.randn(4, generator=gen), "inc.bn1.running_mean": torch.randn(4, generator=gen),
                    "inc.bn1.running_var": torch.rand(4, generator=gen) + 0.5, "inc.bn1.num_batches_tracked": torch.tensor(7 + i)})
    return sds


def _toy_site():
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    layers = {k: {"inc.bn1": dict(images=5, divergence=[0.1 * (i + 1), 0.2, 0.3, 0.5])} for i, k in enumerate(CHECKPOINT_KEYS)}
    layers["model"]["prior_dist.inc.double_conv.1"] = dict(images=0, divergence=[0.0] * 16)
    return dict(prior=16.0, images=5, source="checkpoint_3.pth.tar", layers=layers)


def test_checkpoint_dict_round_trip(tmp_path):
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    sds, site = _toy_state_dicts(), _toy_site()
    before = [{k: v.clone() for k, v in sd.items()} for sd in sds]
    mean_b, var_b = np.array([0.1, 0.2, 0.3, 1 / 3]), np.array([1.0, 2.0, 3.0, 2 / 3])
    ck = A.site_checkpoint(sds, {"model": {"inc.bn1": (mean_b, var_b)}, "model_oc_shape": {"inc.bn1": (2 * mean_b, var_b)}}, site)
    assert list(ck) == list(CHECKPOINT_KEYS) + ["site"]
    for sd, old in zip(sds, before):                      # the inputs are untouched, the outputs are copies
        assert all(torch.equal(sd[k], old[k]) for k in old)
    for key, sd in zip(CHECKPOINT_KEYS, sds):
        for k, v in sd.items():
            assert ck[key][k].data_ptr() != v.data_ptr()
            changed = key in ("model", "model_oc_shape") and k in ("inc.bn1.running_mean", "inc.bn1.running_var")
            assert torch.equal(ck[key][k], v) != changed, (key, k)
    assert np.array_equal(ck["model"]["inc.bn1.running_mean"].numpy(), mean_b.astype(np.float32))
    assert np.array_equal(ck["model"]["inc.bn1.running_var"].numpy(), var_b.astype(np.float32))
    assert ck["model"]["inc.bn1.running_mean"].dtype == torch.float32
    assert np.array_equal(ck["model_oc_shape"]["inc.bn1.running_mean"].numpy(), (2 * mean_b).astype(np.float32))
    with pytest.raises(ValueError):
        A.site_checkpoint(sds, {"model": {"inc.bn1": (mean_b[:3], var_b[:3])}}, site)
    # through a file, as the program writes it and load_checkpoint reads it: every tensor and the "site" entry come back
    path = str(tmp_path / "adapted_checkpoint.pth.tar")
    torch.save(ck, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert back["site"] == site
    for key in CHECKPOINT_KEYS:
        assert list(back[key]) == list(ck[key]) and all(torch.equal(back[key][k], ck[key][k]) for k in ck[key])


def test_shift_tables(tmp_path):
    from wtpse_hip import tables as T
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    site = _toy_site()
    rows = A.shift_rows(site)
    assert len(rows) == 5 and [r["network"] for r in rows] == ["model", "model", "model_shape", "model_oc", "model_oc_shape"]
    assert rows[0] == dict(network="model", name="inc.bn1", channels=4, images=5, div_mean=float(np.mean([0.1, 0.2, 0.3, 0.5])), div_max=0.5)
    assert rows[1]["images"] == 0 and rows[1]["channels"] == 16 and rows[1]["div_mean"] == 0.0 and rows[1]["div_max"] == 0.0
    summary = A.write_shift(str(tmp_path), site)
    with open(tmp_path / "shift.csv") as f:
        assert f.readline().strip() == ",".join(A.SHIFT_COLUMNS)
    got_rows, got_summary = A.read_shift(str(tmp_path))
    assert got_rows == rows and got_summary == summary == T.read_json(str(tmp_path / "shift.json"))
    # the means run over the channels of the visited layers only
    assert summary["networks"]["model"] == float(np.mean([0.1, 0.2, 0.3, 0.5]))
    pooled = [d for i in range(4) for d in (0.1 * (i + 1), 0.2, 0.3, 0.5)]
    assert summary["mean_divergence"] == float(np.mean(pooled)) and set(summary["networks"]) == set(CHECKPOINT_KEYS)
    assert (summary["prior"], summary["images"], summary["source"]) == (16.0, 5, "checkpoint_3.pth.tar")


# ---- the switches -----------------------------------------------------------------------------------------------------------------
BASE = ["--images", "d", "--checkpoint", "c", "--out", "o"]


def test_segment_parser_defaults_and_refusals(capsys):
    from wtpse_hip import locate, segment
    for ap in (locate.parser(), None):
        if ap is None:
            ap = argparse.ArgumentParser()
            segment.add_arguments(ap)
        args = ap.parse_args(BASE)
        assert args.adapt == "none" and args.prior == 16.0
        kw = segment.segmenter_arguments(ap, args)
        assert "adapt" not in kw and "prior" not in kw                                  # off: the keywords are what they were
        kw = segment.segmenter_arguments(ap, ap.parse_args(BASE + ["--adapt", "stream", "--prior", "4"]))
        assert kw["adapt"] == "stream" and kw["prior"] == 4.0 and kw["views"] is None
        kw = segment.segmenter_arguments(ap, ap.parse_args(BASE + ["--adapt", "batch", "--views", "flips"]))
        assert kw["adapt"] == "batch" and kw["prior"] == 16.0 and len(kw["views"]) > 1
        with pytest.raises(SystemExit):
            segment.segmenter_arguments(ap, ap.parse_args(BASE + ["--adapt", "stream", "--views", "flips"]))
        assert "--adapt stream cannot be combined with --views" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            segment.segmenter_arguments(ap, ap.parse_args(BASE + ["--adapt", "batch", "--prior", "-1"]))
        with pytest.raises(SystemExit):
            ap.parse_args(BASE + ["--adapt", "site"])


def test_driver_keywords():
    from wtpse_hip.segment import Segmenter
    s = Segmenter(None, None, None, None, out_dir=None)
    assert s.adapt is None and s.prior == 16.0
    assert Segmenter(None, None, None, None, out_dir=None, adapt="none").adapt is None
    s = Segmenter(None, None, None, None, out_dir=None, adapt="stream", prior=0)
    assert (s.adapt, s.prior) == ("stream", 0.0)
    assert Segmenter(None, None, None, None, out_dir=None, adapt="batch", views="flips").adapt == "batch"
    with pytest.raises(ValueError):
        Segmenter(None, None, None, None, out_dir=None, adapt="stream", views="flips")
    with pytest.raises(ValueError):
        Segmenter(None, None, None, None, out_dir=None, adapt="site")
    with pytest.raises(ValueError):
        Segmenter(None, None, None, None, out_dir=None, adapt="batch", prior=-2)


def test_adapt_parser_and_the_test_split_programs():
    from wtpse_hip.programs import test_run_parser
    args = A.parser().parse_args(BASE)
    assert (args.prior, args.batch_size, args.images, args.checkpoint, args.out) == (16.0, 9, "d", "c", "o")
    args = A.parser().parse_args(BASE + ["--prior", "0", "--batch-size", "2"])
    assert (args.prior, args.batch_size) == (0.0, 2)
    with pytest.raises(SystemExit):
        A.parser().parse_args(["--images", "d"])
    # the test-split programs have no switch (a site checkpoint, or AdaptedTestRun from Python): an unknown option ends them
    split = ["--data-dir", "D", "--datasetTest", "3", "--checkpoint", "c", "--out", "o"]
    assert test_run_parser("test_run", "doc").parse_args(split).batch_size == 9
    with pytest.raises(SystemExit):
        test_run_parser("test_run", "doc").parse_args(split + ["--adapt", "batch"])


def test_adapted_test_run_keywords():
    from wtpse_hip.test_run import TestRun
    t = A.AdaptedTestRun(None, None, None, None, out_dir=None)
    assert isinstance(t, TestRun) and t.adapt is None and t.prior == 16.0 and (t.overlay, t.metrics) == ("device", "device")
    assert A.AdaptedTestRun(None, None, None, None, out_dir=None, adapt="none").adapt is None
    t = A.AdaptedTestRun(None, None, None, None, out_dir=None, adapt="stream", prior=3, metrics="host", morphometry=True, sectors=32)
    assert (t.adapt, t.prior, t.metrics, t.morphometry, t.sectors) == ("stream", 3.0, "host", True, 32)
    for bad in (dict(adapt="both"), dict(adapt="batch", prior=-1), dict(adapt="batch", metrics="gpu")):
        with pytest.raises(ValueError):
            A.AdaptedTestRun(None, None, None, None, out_dir=None, **bad)


def test_state_and_context_without_a_device():
    class Root:
        bn_blend = None
    nets = [Root(), Root(), None, Root()]
    st = A.BlendState(4, "stream")
    assert (st.prior, st.mode, st.report, st.n_seen, st.slots) == (4.0, "stream", False, 0, {})
    assert A.BlendState(report=True).report is True
    with A.blended(nets, st) as got:
        assert got is st and all(n.bn_blend is st for n in nets if n is not None)
    assert all(n.bn_blend is None for n in nets if n is not None)
    with pytest.raises(KeyError):
        with A.blended(nets, st):
            raise KeyError("x")
    assert all(n.bn_blend is None for n in nets if n is not None)                 # restored whatever ends the block
    inner = A.BlendState()
    with A.blended(nets, st):
        with A.blended(nets[:1], inner):
            assert nets[0].bn_blend is inner and nets[1].bn_blend is st
        assert nets[0].bn_blend is st
    with A.blended(nets, None) as got:                                             # the switch off: nothing is set
        assert got is None and all(n.bn_blend is None for n in nets if n is not None)
    assert A.make_state(None) is None and A.make_state("none") is None
    st = A.make_state("batch", 3)
    assert (st.mode, st.prior) == ("batch", 3.0)
    for bad in (dict(mode="site"), dict(prior=-1)):
        with pytest.raises(ValueError):
            A.BlendState(**bad)


def test_hipnet_has_the_switch_off_by_default():
    import algorithms
    from oracle.wtpse_cpu import DEFAULT_HPARAMS as HP
    m = algorithms.WT_PSE(3, 1, HP, "cpu", False, per_domain_batch=1)
    assert m.bn_blend is None and m.bn_momentum == 0.1
    assert "bn_blend" not in m.state_dict() and "bn_blend" not in dict(m.named_buffers())


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_has_the_entry_point():
    import ctypes
    from wtpse_hip import build
    from wtpse_hip.lib import parse_header
    types = build.parse_prototypes()["wtpse_bn_finalize_blend"]
    assert types == ["const float*", "int", "int", "long long", "const float*", "const float*", "const float*", "const float*", "double",
                     "float", "double*", "double", "float*", "double*", "double*", "unsigned*", "void*"]
    # the running statistics are read-only at the boundary, as the sibling's gamma / beta are
    assert build.parse_prototypes()["wtpse_bn_finalize"][6] == "float*" and types[6] == types[7] == "const float*"
    bound = parse_header()["wtpse_bn_finalize_blend"]
    assert len(bound) == 17 and bound[8] is ctypes.c_double and bound[9] is ctypes.c_float and bound[11] is ctypes.c_double
    assert bound[3] is ctypes.c_longlong and bound[-1] is ctypes.c_void_p
    build.generate_thunks()
    assert "wtpse_bn_finalize_blend" in open(build.THUNKS).read()


def test_library_binds_the_entry_point_and_checks_arguments():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    build.build()
    L = lib()
    assert "wtpse_bn_finalize_blend" in L.protos
    raw = L.raw("wtpse_bn_finalize_blend")
    # argument validation happens before any launch: null partials; a weight outside [0, 1]; history without a buffer
    assert raw(0, 1, 1, 1, 0, 0, 0, 0, 0.5, 1e-5, 0, 0.0, 0, 0, 0, 0, 0) == -1
    assert raw(8, 1, 1, 1, 8, 8, 8, 8, 1.5, 1e-5, 0, 0.0, 8, 0, 0, 0, 0) == -1
    assert raw(8, 1, 1, 1, 8, 8, 8, 8, 0.5, 1e-5, 0, 4.0, 8, 0, 0, 0, 0) == -1
    assert raw(8, 1, 1, 0, 8, 8, 8, 8, 0.5, 1e-5, 0, 0.0, 8, 0, 0, 0, 0) == -1
