"""Sampled shape latents on the device (-m gpu): wtpse_shape_samples against its fp64 specification on synthetic tensors, the
in-kernel generator against injected ops.randn noise bit for bit, WT_PSE.predict_samples against the reference-pinned fixture
(tests/golden/uncertainty.npz), validate.predict_pair_samples against predict_pair, and Segmenter(samples=K) end to end."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.filler import fill_state_dict
from oracle.inputs import make_inputs
from test_segment_cpu import content
from test_uncertainty_cpu import GOLDEN, fixture_case, fixture_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LN3 = math.log(3.0)
TOL = 1e-4                     # the project's logit bar; the sigmoid is 1/4-Lipschitz, so it bounds mean and std as well


class Case:
    """Synthetic inputs of one launch, on the host in fp32 and on the device: emb, mu O(1), logvar in [-4, 1]."""

    def __init__(self, seed, B=3, H=16, W=20, CE=8, cat_shape=False):
        r = np.random.RandomState(seed)
        self.B, self.H, self.W, self.CE = B, H, W, CE
        self.emb = r.standard_normal((B, CE, H, W)).astype(np.float32)
        self.mu = r.standard_normal((B, 1, H, W)).astype(np.float32)
        self.logvar = r.uniform(-4.0, 1.0, (B, 1, H, W)).astype(np.float32)
        self.wb = np.array([1.3, -0.2], np.float32)
        self.wout = np.concatenate([r.standard_normal(CE), [0.6]]).astype(np.float32)       # the last: the latent's own weight
        self.bout = np.array([0.1], np.float32)
        self.coef, self.cat_shape = 0.3, cat_shape
        self.upload()

    def upload(self):
        self.d = {k: torch.from_numpy(getattr(self, k)).to(DEV) for k in ("emb", "mu", "logvar", "wb", "wout", "bout")}

    def run(self, K, noise=None, seed=0, offset=0, scale=1.0, want_logits=True):
        from wtpse_hip import ops
        d = self.d
        wz = d["wout"].data_ptr() + 4 * self.CE if self.cat_shape else 0
        return ops.shape_samples(d["emb"], d["mu"], d["logvar"], d["wb"].data_ptr(), self.coef, d["wout"].data_ptr(), d["bout"].data_ptr(),
                                 wz, K, seed, offset, scale, noise, 0.75, want_logits)

    def host(self, eps, scale=1.0):
        from wtpse_hip.uncertainty import shape_samples_host
        return shape_samples_host(self.emb, self.mu, self.logvar, self.wb[0], self.wb[1], self.coef, self.wout[:self.CE], self.bout[0],
                                  self.wout[self.CE] if self.cat_shape else None, eps, scale)


def check_against_host(got, want, K, what):
    mean, std, votes, logits = (t.cpu().numpy() for t in got)
    B = logits.shape[0]
    e_l = float(np.abs(logits - want["logits"]).max())
    e_m = float(np.abs(mean[:, 0] - want["mean"]).max())
    e_s = float(np.abs(std[:, 0] - want["std"]).max())
    near = np.abs(want["logits"] - LN3) <= TOL                  # (pixel, sample) pairs whose vote the rounding may decide
    ok = ~near.any(axis=1)
    print("%s: max |logit - fp64| %.3e, mean %.3e, std %.3e; %.4f %% of the logits within %g of ln 3; votes 0..%d, %d pixels compared"
          % (what, e_l, e_m, e_s, 100.0 * near.mean(), TOL, votes.max(), ok.sum()))
    assert np.isfinite(logits).all() and np.isfinite(mean).all() and np.isfinite(std).all()
    assert e_l <= TOL and e_m <= TOL and e_s <= TOL
    assert near.mean() <= 1e-3
    assert votes.dtype == np.uint8 and np.array_equal(votes[:, 0][ok], want["votes"][ok])
    assert 0 < want["votes"].sum() < K * want["votes"].size      # there is something to count
    assert tuple(mean.shape) == tuple(std.shape) == tuple(votes.shape) == (B, 1) + logits.shape[2:]


# ---- kernel level -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 64])
def test_kernel_matches_host_specification(K):
    from wtpse_hip import ops
    c = Case(100 + K)
    assert c.H * c.W == 320 and (c.H * c.W // 4) % 256 != 0     # images straddle workgroups, the last workgroup is partial
    noise = ops.randn((c.B, K, c.H, c.W), DEV, 7, 4 * K)
    check_against_host(c.run(K, noise=noise), c.host(noise.cpu().numpy()), K, "K = %d" % K)
    if K == 1:
        assert float(c.run(K, noise=noise)[1].abs().max()) == 0.0               # one sample has no spread


def test_kernel_cat_shape_and_nonfinite_logvar():
    from wtpse_hip import ops
    K = 5
    c = Case(200, cat_shape=True)
    noise = ops.randn((c.B, K, c.H, c.W), DEV, 8, 0)
    check_against_host(c.run(K, noise=noise), c.host(noise.cpu().numpy()), K, "cat_shape")
    plain = Case(200, cat_shape=False)
    assert float((c.run(K, noise=noise)[3] - plain.run(K, noise=noise)[3]).abs().max()) > 0.1       # wz is used
    bad = [(0, 0, 3), (1, 7, 19), (2, 15, 0), (2, 15, 1)]
    for (b, y, x), v in zip(bad, (np.inf, np.nan, np.inf, np.nan)):
        c.logvar[b, 0, y, x] = v
    c.upload()
    got = c.run(K, noise=noise)
    check_against_host(got, c.host(noise.cpu().numpy()), K, "cat_shape, inf / nan in logvar")
    std, logits = got[1].cpu().numpy(), got[3].cpu().numpy()
    for b, y, x in bad:                                                         # the standard deviation scrubbed to 0: z = mu
        assert std[b, 0, y, x] == 0.0 and np.all(logits[b, :, y, x] == logits[b, 0, y, x])


def test_generator_equals_injected_noise_bitwise():
    from wtpse_hip import ops
    K, seed, offset = 5, 0x123456789ABCDEF, 2 ** 33 + 28                        # a counter truncated to 32 bits fails here
    c = Case(300)
    noise = ops.randn((c.B, K, c.H, c.W), DEV, seed, offset)
    assert not torch.equal(noise, ops.randn((c.B, K, c.H, c.W), DEV, seed, 28))
    gen, inj = c.run(K, seed=seed, offset=offset), c.run(K, noise=noise)
    for a, b, name in zip(gen, inj, ("mean", "std", "votes", "logits")):
        assert torch.equal(a, b), name
    again = c.run(K, seed=seed, offset=offset)
    assert all(torch.equal(a, b) for a, b in zip(gen, again))                   # two launches of the same call
    other = c.run(K, seed=seed, offset=offset + 4)
    assert not torch.equal(gen[3], other[3])
    without = c.run(K, seed=seed, offset=offset, want_logits=False)             # the logits are an optional output
    assert without[3] is None and all(torch.equal(a, b) for a, b in zip(gen[:3], without[:3]))
    # one launch per image at a stride of its own: image b draws from offset + b * stride
    stride = 2 * K * c.H * c.W
    per = ops.shape_samples(c.d["emb"], c.d["mu"], c.d["logvar"], c.d["wb"].data_ptr(), c.coef, c.d["wout"].data_ptr(), c.d["bout"].data_ptr(),
                            0, K, seed, offset, 1.0, None, 0.75, True, image_stride=stride)
    eps = torch.stack([ops.randn((K, c.H, c.W), DEV, seed, offset + b * stride) for b in range(c.B)])
    assert all(torch.equal(a, b) for a, b in zip(per, c.run(K, noise=eps)))


def test_scale_zero_repeats_the_deterministic_prediction():
    K = 5
    c = Case(400)
    mean, std, votes, logits = c.run(K, seed=3, offset=0, scale=0.0)
    assert all(torch.equal(logits[:, k], logits[:, 0]) for k in range(K))
    assert float(std.abs().max()) == 0.0
    v = votes.cpu().numpy()
    assert np.all((v == 0) | (v == K)) and (v == 0).any() and (v == K).any()
    want = c.host(np.zeros((c.B, K, c.H, c.W)), scale=0.0)
    assert float(np.abs(logits.cpu().numpy() - want["logits"]).max()) <= TOL
    assert float((mean[:, 0] - torch.sigmoid(logits[:, 0])).abs().max()) <= 1e-6           # a few ulps of a value below 1


def test_binding_argument_checks():
    from wtpse_hip import ops
    from wtpse_hip.lib import WtpseError
    c = Case(500)
    with pytest.raises(WtpseError):
        c.run(0)
    with pytest.raises(WtpseError):
        c.run(65)
    with pytest.raises(WtpseError):
        c.run(4, offset=6)
    with pytest.raises(ValueError):
        c.run(4, noise=torch.zeros(c.B, 3, c.H, c.W, device=DEV))
    odd = Case(501, H=3, W=5)                                                   # HW = 15
    with pytest.raises(WtpseError):
        odd.run(4)


# ---- network level: the reference under a substituted latent --------------------------------------------------------------------
def fixture_nets(ci, fx):
    import algorithms
    import shape_networks
    from oracle.wtpse_cpu import DEFAULT_HPARAMS
    two_step, cat_shape, seed_in, B, H, K, seed_main, seed_shape = fixture_case(fx, ci)
    hp = dict(DEFAULT_HPARAMS, cat_shape=cat_shape)
    main = algorithms.WT_PSE(3, 1, hp, DEV, two_step, per_domain_batch=1, source_domain_num=3).to(DEV)
    shape = shape_networks.ShapeVariationalDist_x(hp, DEV, 1, 3, 1).to(DEV)
    fill_state_dict(main, seed_main)
    fill_state_dict(shape, seed_shape)
    main.eval()
    shape.eval()
    return main, shape, fixture_inputs(two_step, seed_in, B, H).to(DEV), K


@pytest.mark.parametrize("ci", [0, 1, 2], ids=["plain", "two_step", "cat_shape"])
def test_predict_samples_matches_the_reference(ci):
    fx = np.load(GOLDEN)
    main, shape, data, K = fixture_nets(ci, fx)
    eps = torch.from_numpy(fx["c%d_eps" % ci]).to(DEV)
    with torch.no_grad():
        res = main.predict_samples(shape, data, K, noise=eps, want_logits=True)
        logit, pre = main.predict(shape, data)
    assert torch.equal(res.logit, logit) and torch.equal(res.pre, pre)          # the unchanged path, from the same U-Net pass
    ref32, ref64 = fx["c%d_logits" % ci], fx["c%d_logits64" % ci]
    p = 1.0 / (1.0 + np.exp(-ref64))
    e_l = float(np.abs(res.logits.cpu().numpy() - ref32).max())
    e_m = float(np.abs(res.mean.cpu().numpy()[:, 0] - p.mean(1)).max())
    e_s = float(np.abs(res.std.cpu().numpy()[:, 0] - p.std(1)).max())
    print("case %d: max |logit - reference fp32| %.3e, mean %.3e, std %.3e (largest std %.3e)" % (ci, e_l, e_m, e_s, p.std(1).max()))
    assert e_l <= TOL and e_m <= TOL and e_s <= TOL
    assert np.array_equal(res.votes.cpu().numpy()[:, 0], (p > 0.75).sum(1))    # the fixture keeps its logits away from ln 3
    assert tuple(res.logits.shape) == ref32.shape and tuple(res.mean.shape) == tuple(logit.shape)


def test_predict_samples_needs_a_shape_prior():
    import algorithms
    from oracle.wtpse_cpu import DEFAULT_HPARAMS
    net = algorithms.WT_PSE(3, 1, dict(DEFAULT_HPARAMS, whitening=False, shape_prior=False), DEV, False).to(DEV)
    with pytest.raises(ValueError, match="shape_prior"):
        net.predict_samples(None, torch.zeros(1, 3, 32, 32, device=DEV), 4)


# ---- both stages ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from test_parity_gpu import build_nets
    nets = build_nets(1)
    for n in nets:
        n.eval()
    return nets


def test_predict_pair_samples(nets):
    from wtpse_hip import ops, validate as V
    data = make_inputs(61, 2, 64, 64)[0].to(DEV)
    K = 4
    pred, pred_oc = V.predict_pair(*nets, data)
    p1, p1_oc, disc, cup = V.predict_pair_samples(*nets, data, K, seed=9, offset=8 * K * 64 * 64, scale=1.0, want_logits=True)
    assert torch.equal(p1, pred) and torch.equal(p1_oc, pred_oc)
    od_pred = ops.roi(data.contiguous(), pred)[1]
    outside = od_pred <= 0
    print("od_pred covers %.1f %% of the pixels; cup votes inside it: %d" % (100.0 * float((~outside).float().mean()), int(cup.votes[~outside].sum())))
    assert int(cup.votes[outside].sum()) == 0
    assert bool((cup.logits[outside.expand(-1, K, -1, -1)] == 0).all()) and bool((cup.std[outside] == 0).all())
    assert bool((cup.mean[outside] == 0.5).all())
    z0 = V.predict_pair_samples(*nets, data, K, seed=9, offset=0, scale=0.0)
    assert torch.equal(z0[0], pred) and torch.equal(z0[1], pred_oc) and z0[2].logits is None
    for s, logit in ((z0[2], pred), (z0[3], pred_oc)):
        assert float((s.mean - torch.sigmoid(logit)).abs().max()) <= TOL and float(s.std.abs().max()) == 0.0


# ---- the driver ------------------------------------------------------------------------------------------------------------------
SIZES = [(70, 90), (100, 64), (70, 90), (100, 64), (100, 64), (70, 90)]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("crops"))
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(content(h, w, "random" if i % 2 else "smooth")).save(os.path.join(root, "crop %02d.png" % i))
    return root


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_segmenter_without_samples_is_unchanged(nets, folder, tmp_path):
    from wtpse_hip.segment import Segmenter
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    sa = Segmenter(*nets, out_dir=a, batch_size=2).run(folder)
    sb = Segmenter(*nets, out_dir=b, batch_size=2, samples=0, seed=5, scale=2.0).run(folder)
    ta = tree(a)
    assert sa == sb and ta == tree(b) and "n_samples" not in sa
    assert sorted(os.path.dirname(k) for k in ta) == [""] * 2 + ["mask"] * 6 + ["overlay"] * 6          # no new file


def test_segmenter_with_samples(nets, folder, tmp_path, monkeypatch):
    import json
    from wtpse_hip import ops, uncertainty as U
    from wtpse_hip.segment import Segmenter
    K, S = 4, 256
    plain = str(tmp_path / "plain")
    Segmenter(*nets, out_dir=plain, batch_size=2).run(folder)
    draws, real = [], ops.shape_samples

    def spy(emb, *a):
        draws[-1].append([a[9] + b * a[14] for b in range(emb.shape[0])])       # a[9]: offset, a[14]: image_stride
        return real(emb, *a)

    monkeypatch.setattr(ops, "shape_samples", spy)
    outs = {}
    for bs in (2, 6):
        draws.append([])
        out = str(tmp_path / ("k4_b%d" % bs))
        seg = Segmenter(*nets, out_dir=out, batch_size=bs, samples=K, seed=3)
        summary = seg.run(folder)
        assert seg.sample_offsets == [i * 2 * K * S * S for i in range(6)]
        outs[bs] = (out, summary, U.read_csv(out))
    # the offset every image was given, per stage, whatever the batch size: disc at 2 K S^2 i, cup K S^2 behind it
    for calls in draws:
        disc, cup = sum(calls[0::2], []), sum(calls[1::2], [])
        assert disc == [i * 2 * K * S * S for i in range(6)] and cup == [o + K * S * S for o in disc]
    out, summary, rows = outs[2]
    got, want = tree(out), tree(plain)
    for k, v in want.items():
        if k != "summary.json":
            assert got[k] == v, k                                               # mask/, overlay/, measurements.csv byte for byte
    assert sorted(set(got) - set(want)) == ["uncertainty.csv"] + sorted(os.path.join("uncertainty", "crop %02d.png" % i) for i in range(6))
    with open(os.path.join(plain, "summary.json")) as f:
        base = json.load(f)
    assert {k: v for k, v in summary.items() if k not in ("n_samples", "mean_vcdr_std")} == base and summary["n_samples"] == K
    defined = [r["vcdr_std"] for r in rows if r["vcdr_std"] == r["vcdr_std"]]
    assert summary["mean_vcdr_std"] == (float(np.mean(np.array(defined, np.float64))) if defined else None)
    assert len(rows) == 6 and [r["index"] for r in rows] == list(range(1, 7)) and [r["name"] for r in rows] == ["crop %02d.png" % i for i in range(6)]
    for r, (h, w) in zip(rows, SIZES):
        assert r["n_samples"] == K and 0 <= r["n_defined"] <= K
        assert 0 <= r["disc_disagree_px"] <= S * S and 0 <= r["cup_disagree_px"] <= S * S
        assert 0.0 <= r["disc_std_mean"] <= 0.5 and 0.0 <= r["cup_std_mean"] <= 0.5
        if r["n_defined"]:
            assert r["vcdr_p05"] <= r["vcdr_mean"] <= r["vcdr_p95"] and r["vcdr_std"] >= 0.0
        else:
            assert math.isnan(r["vcdr_mean"]) and math.isnan(r["acdr_p95"])
        png = Image.open(os.path.join(out, "uncertainty", r["name"]))
        assert png.mode == "RGB" and png.size == (w, h) and not np.array(png)[..., 2].any()
    print("rows:", [(r["n_defined"], r["disc_disagree_px"], r["cup_disagree_px"], round(r["disc_std_mean"], 5)) for r in rows])
    assert len(outs[6][2]) == 6 and outs[6][1]["n_samples"] == K
