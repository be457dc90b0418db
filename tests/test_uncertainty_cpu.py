"""Sampled shape latents, host side: the fp64 specification of the sampling launch against the reference-pinned fixture
(tests/golden/uncertainty.npz, tools/make_golden_uncertainty.py), its degenerate scale = 0 case, the argument checks of
wtpse_shape_samples (no launch is made without a GPU) and the arithmetic of uncertainty.csv."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import wtpse_cpu as O
from oracle.filler import fill_state_dict
from oracle.inputs import make_inputs
from oracle.wtpse_cpu import DEFAULT_HPARAMS as HP

from wtpse_hip import segment as S
from wtpse_hip import uncertainty as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uncertainty.npz")
LN3 = math.log(3.0)


def fixture_case(fx, ci):
    """-> (two_step, cat_shape, seed_in, B, H, K, seed_main, seed_shape) of case ci."""
    B, H, K, seed_main, seed_shape = (int(v) for v in fx["meta"])
    two_step, cat_shape, seed_in, _ = (int(v) for v in fx["cases"][ci])
    return bool(two_step), bool(cat_shape), seed_in, B, H, K, seed_main, seed_shape


def fixture_inputs(two_step, seed_in, B, H):
    """The `inputs_all` of the fixture's predict call (tools/make_golden_uncertainty.py)."""
    img = make_inputs(seed_in, B, H, H)[0]
    return torch.stack((img, make_inputs(seed_in + 500, B, H, H)[0]), 0) if two_step else img


def oracle_tensors(ci, fx):
    """emb, mu, logvar and the pointwise weights of case ci from the oracle's CPU restatement, in float64."""
    import algorithms
    import shape_networks
    two_step, cat_shape, seed_in, B, H, K, seed_main, seed_shape = fixture_case(fx, ci)
    hp = dict(HP, cat_shape=cat_shape)
    main = algorithms.WT_PSE(3, 1, hp, "cpu", two_step, per_domain_batch=1, source_domain_num=3)
    shape = shape_networks.ShapeVariationalDist_x(hp, "cpu", 1, 3, 1)
    fill_state_dict(main, seed_main)
    fill_state_dict(shape, seed_shape)
    dbl = lambda net: {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in net.state_dict().items()}
    sd, sds = dbl(main), dbl(shape)
    data = fixture_inputs(two_step, seed_in, B, H).double()
    inputs, wt_in = (data[0], data[1]) if two_step else (data, data)
    with torch.no_grad():
        emb = O.main_unet(sd, inputs, False)
        fmap = O.unet_body(sds, "", O.deep_wt(sds, "wt_model.", wt_in)[-1], False)
        mu = O._scrub_nan(O.head3(sds, "mu_prior.", fmap))
        logvar = O.head3(sds, "logvar_prior.", fmap)
    wout = sd["outc.0.weight"].reshape(-1).numpy()
    return dict(emb=emb.numpy(), mu=mu.numpy(), logvar=logvar.numpy(), w=float(sd["attention_layer.layer1.weight"]),
                b=float(sd["attention_layer.layer1.bias"]), coef=float(hp["shape_attention_coeffient"]), wout=wout[:8],
                bout=float(sd["outc.0.bias"]), wz=float(wout[8]) if cat_shape else None)


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_host_specification_reproduces_the_reference(ci):
    fx = np.load(GOLDEN)
    t = oracle_tensors(ci, fx)
    res = U.shape_samples_host(eps=fx["c%d_eps" % ci], **t)
    ref = fx["c%d_logits64" % ci]
    err = float(np.abs(res["logits"] - ref).max())
    spread = float(ref.std(axis=1).max())
    print("case %d: max |host - reference fp64| = %.3e; largest spread of a pixel's logits over the samples %.3e" % (ci, err, spread))
    assert res["logits"].shape == ref.shape and res["logits"].dtype == np.float64
    assert err <= 1e-10
    assert spread > 1e-3                                   # the samples do differ: the latent reaches the logits
    # the fixture's own promise: the logits keep away from the vote threshold
    assert float((np.abs(ref - LN3) < 1e-3).mean()) <= 1e-3
    p = 1.0 / (1.0 + np.exp(-ref))
    assert np.abs(res["mean"] - p.mean(1)).max() <= 1e-12 and np.abs(res["std"] - p.std(1)).max() <= 1e-12
    assert np.array_equal(res["votes"], (p > 0.75).sum(1).astype(np.uint8))


def synthetic(seed=5, B=2, CE=8, HW=24, K=6):
    r = np.random.RandomState(seed)
    return dict(emb=r.standard_normal((B, CE, HW)), mu=r.standard_normal((B, HW)), logvar=r.uniform(-4, 1, (B, HW)), w=1.3, b=-0.2,
                coef=0.3, wout=r.standard_normal(CE), bout=0.1, wz=None, eps=r.standard_normal((B, K, HW)))


def test_host_scale_zero_is_degenerate():
    t = synthetic()
    K = t["eps"].shape[1]
    for wz in (None, 0.7):
        res = U.shape_samples_host(**dict(t, wz=wz), scale=0.0)
        assert np.all(res["std"] == 0.0)
        assert np.all((res["votes"] == 0) | (res["votes"] == K)) and (res["votes"] == K).any() and (res["votes"] == 0).any()
        assert all(np.array_equal(res["logits"][:, k], res["logits"][:, 0]) for k in range(K))
    # a non-finite standard deviation counts as 0: the pixel repeats its deterministic prediction
    lv = t["logvar"].copy()
    lv[0, :3] = (np.inf, np.nan, 1e6)
    res, det = U.shape_samples_host(**dict(t, logvar=lv)), U.shape_samples_host(**t, scale=0.0)
    assert np.isfinite(res["logits"]).all() and np.all(res["std"][0, :3] == 0.0)
    assert np.array_equal(res["logits"][0, :, :3], det["logits"][0, :, :3])
    assert np.all(res["std"][0, 3:] > 0.0)


def test_argument_checks_come_before_any_launch():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    build.build()
    fn = lib().raw("wtpse_shape_samples")
    P = 4096                                               # never dereferenced: every call below is refused on its arguments

    def call(emb=P, K=4, HW=64, offset=0, CE=8, scale=1.0):
        return fn(emb, CE, P, P, P, 0.3, P, P, 0, scale, K, 1, offset, 0, 0.75, P, P, P, 0, 2, HW, 0)

    assert call(K=0) == -1 and call(K=65) == -1
    assert call(HW=66) == -1
    assert call(offset=6) == -1
    assert call(emb=0) == -1
    assert call(CE=0) == -1 and call(CE=17) == -1
    assert call(scale=-1.0) == -1 and call(scale=float("nan")) == -1
    assert lib().raw("wtpse_shape_samples_mask")(P, P, P, P, 0, 4, 2, 66, 0) == -1


def geometry(area, top, bottom, left, right):
    return (area, top, bottom, left, right, 0, 0, 0)


def test_ratio_statistics():
    disc = geometry(400, 10, 29, 10, 29)                   # 20 x 20
    cups = [geometry(100, 15, 24, 15, 24), geometry(64, 16, 23, 16, 23), geometry(0, 64, -1, 64, -1), geometry(144, 14, 25, 14, 25)]
    samples = [S.measure(disc, c, 64, 64) for c in cups]
    samples.insert(2, S.measure(geometry(0, 64, -1, 64, -1), cups[0], 64, 64))        # an empty disc: no ratio
    st = U.ratio_statistics(samples)
    assert st["n_samples"] == 5 and st["n_defined"] == 4
    v = np.array([0.5, 0.4, 0.0, 0.6])
    for r, vals in (("vcdr", v), ("hcdr", v), ("acdr", np.array([0.25, 0.16, 0.0, 0.36]))):
        assert st[r + "_mean"] == pytest.approx(vals.mean(), abs=1e-15)
        assert st[r + "_std"] == pytest.approx(vals.std(), abs=1e-15)
        assert st[r + "_p05"] == float(np.percentile(vals, 5)) and st[r + "_p95"] == float(np.percentile(vals, 95))
    assert st["vcdr_p05"] == pytest.approx(0.06, abs=1e-15) and st["vcdr_p95"] == pytest.approx(0.585, abs=1e-15)
    empty = U.ratio_statistics([S.measure(geometry(0, 64, -1, 64, -1), cups[0], 64, 64)] * 3)
    assert empty["n_samples"] == 3 and empty["n_defined"] == 0
    assert all(math.isnan(empty["%s_%s" % (r, s)]) for r in U.RATIOS for s in U.STATS)
    one = U.ratio_statistics(samples[:1])
    assert one["vcdr_std"] == 0.0 and one["vcdr_p05"] == one["vcdr_p95"] == one["vcdr_mean"] == 0.5


def test_map_statistics_picture_and_table(tmp_path):
    votes = np.array([[0, 4, 1], [3, 4, 0]], np.uint8)
    std = np.array([[0.0, 0.0, 0.25], [0.5, 0.1, 0.75]], np.float32)
    assert U.map_statistics(votes, std, 4) == (2, float(std.astype(np.float64).mean()))
    pic = U.std_picture(std, std[::-1])
    assert pic.shape == (2, 3, 3) and pic.dtype == np.uint8 and not pic[..., 2].any()
    assert pic[..., 0].tolist() == [[0, 0, 128], [255, 51, 255]] and np.array_equal(pic[..., 1], pic[::-1, :, 0])
    row = dict(U.ratio_statistics([]), index=1, name='a,"b".png', disc_disagree_px=2, cup_disagree_px=0, disc_std_mean=0.1, cup_std_mean=0.0)
    row2 = dict(row, index=2, name="c.png", n_samples=4, n_defined=4, **{"%s_%s" % (r, s): 0.1 * i for i, r in enumerate(U.RATIOS) for s in U.STATS})
    U.write_csv(str(tmp_path), [row, row2])
    back = U.read_csv(str(tmp_path))
    assert list(back[0]) == list(U.CSV_COLUMNS) and back[1] == {k: row2[k] for k in U.CSV_COLUMNS}
    assert back[0]["name"] == row["name"] and math.isnan(back[0]["vcdr_mean"]) and back[0]["n_defined"] == 0
