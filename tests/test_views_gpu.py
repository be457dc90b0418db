"""Test-time views on the device (-m gpu): wtpse_dihedral_views and wtpse_views_merge against views.view_host / views.merge_host at
S = 20 (less than one 32-tile) and S = 68 (two full tiles and a 4-wide partial one, whose mirrored and transposed partners are
partial on the other side), validate.predict_pair_views against predict_pair / predict_pair_samples of each view, and
Segmenter(views=...) / CalibrationRun(views=...) end to end."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.fundus_tree import _sample
from oracle.inputs import make_inputs
from test_calibration_gpu import SIZES as CAL_SIZES, _feed
from test_segment_cpu import content
from test_uncertainty_gpu import SIZES, TOL, tree

pytestmark = pytest.mark.gpu
DEV = "cuda"
LN3 = math.log(3.0)
CODES = (0, 5, 3, 6, 1, 7, 2, 4)
SS = (20, 68)


def torch_view(x, c):
    """views.view_host with torch ops, on the last two axes."""
    if c & 4:
        x = x.transpose(-1, -2)
    if c & 2:
        x = x.flip(-2)
    if c & 1:
        x = x.flip(-1)
    return x.contiguous()


def torch_unview(x, c):
    if c & 1:
        x = x.flip(-1)
    if c & 2:
        x = x.flip(-2)
    if c & 4:
        x = x.transpose(-1, -2)
    return x.contiguous()


# ---- kernel level -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SS)
def test_generator_is_view_host_bitwise(S):
    from wtpse_hip import ops, views as VW
    B, C = 2, 3
    x = np.arange(B * C * S * S, dtype=np.float32).reshape(B, C, S, S)          # every element unique (exact below 2^24)
    assert x.max() < 2 ** 24
    got = ops.dihedral_views(torch.from_numpy(x).to(DEV), CODES)
    assert tuple(got.shape) == (8, B, C, S, S)
    got = got.cpu().numpy()
    for v, c in enumerate(CODES):
        assert np.array_equal(got[v], VW.view_host(x, c)), (S, c)
    one = ops.dihedral_views(torch.from_numpy(x).to(DEV), (0,))
    assert tuple(one.shape) == (1, B, C, S, S) and np.array_equal(one.cpu().numpy()[0], x)


def merge_inputs(S, V=8, K=3, B=2, seed=0):
    r = np.random.default_rng(1000 + S + seed)
    logits = (2.0 * r.standard_normal((V, B, K, S, S))).astype(np.float32)
    logits[np.abs(logits - LN3) < 1e-3] += np.float32(0.01)                     # no vote is left to the rounding of a sigmoid
    assert not (np.abs(logits.astype(np.float64) - LN3) < 1e-3).any()
    return logits


@pytest.fixture(scope="module", params=SS)
def merged(request):
    """One merge of V = 8, K = 3, B = 2 at S: (S, host logits, device logits, the host specification)."""
    from wtpse_hip import views as VW
    S = request.param
    logits = merge_inputs(S)
    return S, logits, torch.from_numpy(logits).to(DEV), VW.merge_host(logits, CODES)


def test_merge_matches_host_specification(merged):
    from wtpse_hip import ops
    S, logits, dev, want = merged
    mean, std, votes, out, mean_logit = (t.cpu().numpy() for t in ops.views_merge(dev, CODES))
    assert out.shape == (2, 24, S, S) and mean.shape == std.shape == votes.shape == mean_logit.shape == (2, 1, S, S)
    assert votes.dtype == np.uint8 and mean_logit.dtype == np.float32
    assert np.array_equal(out, want["logits"])                                  # a pure permutation
    assert mean_logit[:, 0].tobytes() == want["mean_logit"].tobytes()           # the float32 mean rule, bit for bit
    e_m, e_s = float(np.abs(mean[:, 0] - want["mean"]).max()), float(np.abs(std[:, 0] - want["std"]).max())
    print("S = %d: max |mean - fp64| %.3e, |std - fp64| %.3e (largest std %.3e); votes 0..%d" % (S, e_m, e_s, want["std"].max(), votes.max()))
    assert e_m <= TOL and e_s <= TOL
    assert np.array_equal(votes[:, 0], want["votes"])                           # every pixel, none excused
    assert 0 < int(want["votes"].sum()) < 24 * want["votes"].size


def test_merge_optional_outputs_and_repeatability(merged):
    from wtpse_hip import ops
    S, logits, dev, want = merged
    full = ops.views_merge(dev, CODES)
    again = ops.views_merge(dev, CODES)
    assert all(torch.equal(a, b) for a, b in zip(full, again))                  # two launches of one call
    none = ops.views_merge(dev, CODES, want_logits=False, want_mean_logit=False)
    assert none[3] is None and none[4] is None and all(torch.equal(a, b) for a, b in zip(full[:3], none[:3]))
    only = ops.views_merge(dev, CODES, want_logits=False)
    assert only[3] is None and torch.equal(only[4], full[4]) and all(torch.equal(a, b) for a, b in zip(full[:3], only[:3]))
    other = ops.views_merge(dev, CODES, threshold=0.5)                          # the threshold moves the votes alone
    assert torch.equal(other[0], full[0]) and torch.equal(other[1], full[1]) and not torch.equal(other[2], full[2])


@pytest.mark.parametrize("S", SS)
def test_merge_single_map_and_equal_samples(S):
    from wtpse_hip import ops, views as VW
    x = merge_inputs(S, 1, 1, 2, seed=1)
    x[0, 0, 0, 0, 0] = -0.0
    mean, std, votes, out, mean_logit = ops.views_merge(torch.from_numpy(x).to(DEV), (0,))
    assert float(std.abs().max()) == 0.0
    assert mean_logit.cpu().numpy().tobytes() == x.tobytes() and out.cpu().numpy().tobytes() == x.tobytes()
    assert np.array_equal(votes.cpu().numpy()[:, 0], x[0, :, 0] > LN3)
    # one map under all eight views, K times each: every un-viewed sample is the map itself
    V, K = 8, 3
    base = x[0, :, 0]                                                           # [B,S,S]
    logits = np.stack([np.repeat(np.ascontiguousarray(VW.view_host(base, c))[:, None], K, 1) for c in CODES])
    mean, std, votes, out, mean_logit = (t.cpu().numpy() for t in ops.views_merge(torch.from_numpy(logits).to(DEV), CODES))
    for s in range(V * K):
        assert out[:, s].tobytes() == base.tobytes(), (S, s)
    assert np.all(std == 0.0)
    assert np.all((votes == 0) | (votes == V * K)) and (votes == 0).any() and (votes == V * K).any()


def test_binding_argument_checks():
    from wtpse_hip import ops
    from wtpse_hip.lib import WtpseError
    x = torch.zeros(2, 3, 20, 20, device=DEV)
    with pytest.raises(WtpseError):
        ops.dihedral_views(x, (0, 8))
    with pytest.raises(WtpseError):
        ops.dihedral_views(x, tuple(range(8)) + (0,))
    with pytest.raises(WtpseError):
        ops.dihedral_views(torch.zeros(1, 1, 18, 18, device=DEV), (0,))
    with pytest.raises(ValueError):
        ops.dihedral_views(torch.zeros(1, 1, 20, 24, device=DEV), (0,))
    lg = torch.zeros(5, 1, 13, 20, 20, device=DEV)
    with pytest.raises(WtpseError):
        ops.views_merge(lg, (0, 1, 2, 3, 4))                                    # 65 maps
    with pytest.raises(ValueError):
        ops.views_merge(lg, (0, 1))
    with pytest.raises(WtpseError):
        ops.views_merge(torch.zeros(1, 1, 1, 18, 18, device=DEV), (0,))


# ---- both stages ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from test_parity_gpu import build_nets
    nets = build_nets(1)
    for n in nets:
        n.eval()
    return nets


@pytest.fixture(scope="module")
def disc_nets():
    """The same networks with the disc head's output bias left to the test (set_disc_bias): the filler weights predict no disc at
    all, so od_pred is empty, the cup is masked everywhere and no cup pixel is scored — true but vacuous for what is inside."""
    from test_parity_gpu import build_nets
    nets = build_nets(1)
    for n in nets:
        n.eval()
    return nets, nets[0].outc[0].bias.detach().clone()


def set_disc_bias(disc_nets, images, level):
    """Moves the disc head's output bias so that `level` (min / median) of predict_pair's disc logit over `images` sits at ln 3 + 2
    (min: every pixel well inside od_pred) or at ln 3 (median: half the pixels inside)."""
    from wtpse_hip import validate as V
    nets, bias0 = disc_nets
    with torch.no_grad():
        nets[0].outc[0].bias.copy_(bias0)
        logit = torch.cat([V.predict_pair(*nets, im)[0].reshape(-1) for im in images])
        shift = LN3 + 2.0 - float(logit.min()) if level == "min" else LN3 - float(logit.median())
        nets[0].outc[0].bias.add_(shift)
    return nets


def check_views_without_samples(nets, data):
    """predict_pair_views(n_samples = 0) against predict_pair of every view -> the fraction of pixels inside the merged od_pred."""
    from wtpse_hip import ops, validate as V
    keep = data.clone()
    pred, pred_oc = V.predict_pair(*nets, data)
    p0, p0_oc, d0, c0 = V.predict_pair_views(*nets, data, (0,))
    assert torch.equal(p0, pred) and torch.equal(p0_oc, pred_oc) and torch.equal(data, keep)
    assert d0.n_samples == 1 and torch.equal(d0.logits, pred) and float(d0.std.abs().max()) == 0.0 and d0.pre is None
    p, p_oc, disc, cup = V.predict_pair_views(*nets, data, "d4")
    assert disc.n_samples == cup.n_samples == 8 and tuple(disc.logits.shape) == tuple(cup.logits.shape) == (2, 8, 64, 64)
    assert disc.logit is p and cup.logit is p_oc
    per_view = [V.predict_pair(*nets, torch_view(data, c)) for c in range(8)]
    for v in range(8):
        assert torch.equal(disc.logits[:, v:v + 1], torch_unview(per_view[v][0], v)), v
    # pred: the float32 mean rule (sequential sum from the first, one multiplication by 1 / 8)
    acc = disc.logits[:, 0].clone()
    for v in range(1, 8):
        acc = acc + disc.logits[:, v]
    assert torch.equal(p[:, 0], acc * torch.tensor(1.0 / 8.0, dtype=torch.float32, device=DEV))
    # the merged cup is restricted to the merged disc
    od_pred = ops.roi(data.contiguous(), p)[1]
    outside = od_pred <= 0
    print("merged od_pred covers %.1f %% of the pixels; disc std max %.3e; cup votes inside: %d"
          % (100.0 * float((~outside).float().mean()), float(disc.std.max()), int(cup.votes[~outside].sum())))
    assert bool((p_oc[outside] == 0).all()) and bool((cup.logits[outside.expand(-1, 8, -1, -1)] == 0).all())
    assert int(cup.votes[outside].sum()) == 0 and bool((cup.mean[outside] == 0.5).all()) and bool((cup.std[outside] == 0).all())
    inside = ~outside
    cup_views = torch.cat([torch_unview(per_view[v][1], v) for v in range(8)], 1)
    assert torch.equal(cup.logits[inside.expand(-1, 8, -1, -1)], cup_views[inside.expand(-1, 8, -1, -1)])
    return float(inside.float().mean()), pred, p


def test_predict_pair_views_without_samples(nets):
    from wtpse_hip import validate as V
    data = make_inputs(61, 2, 64, 64)[0].to(DEV)
    _, pred, p = check_views_without_samples(nets, data)
    assert not torch.equal(p, pred)                                             # the views do not all agree
    with pytest.raises(ValueError):
        V.predict_pair_views(*nets, data, None)
    with pytest.raises(ValueError):
        V.predict_pair_views(*nets, data, "d4", n_samples=9)


def test_merged_cup_is_restricted_to_a_partial_merged_disc(disc_nets):
    """The same checks with the disc head's bias moved so that half the pixels lie inside od_pred: the cup's samples are kept inside
    the merged disc and masked outside it, and both sets are non-empty."""
    data = make_inputs(61, 2, 64, 64)[0].to(DEV)
    nets = set_disc_bias(disc_nets, [data], "median")
    inside = check_views_without_samples(nets, data)[0]
    assert 0.05 < inside < 0.95


def test_predict_pair_views_with_samples(nets):
    from wtpse_hip import validate as V
    data = make_inputs(61, 2, 64, 64)[0].to(DEV)
    K, Vn, seed, offset = 2, 2, 9, 4096
    N = K * 64 * 64
    p, p_oc, disc, cup = V.predict_pair_views(*nets, data, "hflip", n_samples=K, seed=seed, offset=offset)
    assert tuple(disc.logits.shape) == tuple(cup.logits.shape) == (2, 4, 64, 64) and disc.n_samples == cup.n_samples == 4
    det = []
    for v in range(Vn):
        q, q_oc, d, c = V.predict_pair_samples(*nets, torch_view(data, v), K, seed, offset + 2 * N * v, 1.0, True, image_stride=2 * Vn * N)
        det.append(q)
        for k in range(K):
            assert torch.equal(disc.logits[:, v * K + k], torch_unview(d.logits[:, k], v)), (v, k)
    assert torch.equal(p[:, 0], (torch_unview(det[0], 0) + torch_unview(det[1], 1))[:, 0] * torch.tensor(0.5, device=DEV))
    assert not torch.equal(disc.logits[:, 0], disc.logits[:, 1])                # the samples differ
    again = V.predict_pair_views(*nets, data, "hflip", n_samples=K, seed=seed, offset=offset)
    assert torch.equal(again[0], p) and torch.equal(again[1], p_oc)
    for a, b in ((again[2], disc), (again[3], cup)):
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("mean", "std", "votes", "logits", "logit"))
    # image_stride = None is the layout predict_pair_samples has always had
    a = V.predict_pair_samples(*nets, data, K, seed, offset, 1.0, True)
    b = V.predict_pair_samples(*nets, data, K, seed, offset, 1.0, True, image_stride=2 * N)
    assert torch.equal(a[2].logits, b[2].logits) and torch.equal(a[3].logits, b[3].logits)


# ---- the drivers ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("crops"))
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(content(h, w, "random" if i % 2 else "smooth")).save(os.path.join(root, "crop %02d.png" % i))
    return root


@pytest.fixture(scope="module")
def plain(nets, folder, tmp_path_factory):
    from wtpse_hip.segment import Segmenter
    out = str(tmp_path_factory.mktemp("plain"))
    summary = Segmenter(*nets, out_dir=out, batch_size=3).run(folder)
    return tree(out), summary


UNC_FILES = ["uncertainty.csv"] + sorted(os.path.join("uncertainty", "crop %02d.png" % i) for i in range(6))


def test_segmenter_identity_view_writes_the_same_masks(nets, folder, plain, tmp_path):
    from wtpse_hip import uncertainty as U
    from wtpse_hip.segment import Segmenter
    out = str(tmp_path / "id")
    summary = Segmenter(*nets, out_dir=out, batch_size=3, views="id").run(folder)
    got, want = tree(out), plain[0]
    for k, v in want.items():
        if k != "summary.json":
            assert got[k] == v, k                                               # mask/, overlay/, measurements.csv byte for byte
    assert sorted(set(got) - set(want)) == UNC_FILES
    assert summary["views"] == [0] and summary["n_samples"] == 1
    assert {k: v for k, v in summary.items() if k not in ("n_samples", "mean_vcdr_std", "views")} == plain[1]
    for r in U.read_csv(out):
        assert r["n_samples"] == 1 and r["disc_std_mean"] == 0.0 and r["cup_std_mean"] == 0.0 and r["disc_disagree_px"] == 0


def test_segmenter_d4(nets, folder, plain, tmp_path):
    from wtpse_hip import uncertainty as U
    from wtpse_hip.segment import Segmenter
    out = str(tmp_path / "d4")
    seg = Segmenter(*nets, out_dir=out, batch_size=3, views="d4")
    summary = seg.run(folder)
    got = tree(out)
    assert sorted(set(got) - set(plain[0])) == UNC_FILES and set(plain[0]) <= set(got)
    with open(os.path.join(out, "summary.json")) as f:
        assert json.load(f) == summary
    assert summary["views"] == list(range(8)) and summary["n_samples"] == 8 and summary["n"] == 6
    assert seg.sample_offsets == [0] * 6                                        # nothing is drawn without samples
    rows = U.read_csv(out)
    assert len(rows) == 6 and [r["name"] for r in rows] == ["crop %02d.png" % i for i in range(6)]
    for r, (h, w) in zip(rows, SIZES):
        assert r["n_samples"] == 8 and 0 <= r["n_defined"] <= 8
        assert 0.0 <= r["disc_std_mean"] <= 0.5 and 0.0 <= r["cup_std_mean"] <= 0.5
        png = Image.open(os.path.join(out, "uncertainty", r["name"]))
        assert png.mode == "RGB" and png.size == (w, h)
    print("d4 rows:", [(r["n_defined"], r["disc_disagree_px"], r["cup_disagree_px"], round(r["disc_std_mean"], 5)) for r in rows])
    assert any(r["disc_std_mean"] > 0.0 for r in rows)                          # the views do not all agree


def test_segmenter_views_with_samples(nets, folder, tmp_path, monkeypatch):
    from wtpse_hip import ops, uncertainty as U
    from wtpse_hip.segment import Segmenter
    K, Vn, S = 4, 2, 256
    N = K * S * S
    draws, real = [], ops.shape_samples

    def spy(emb, *a):
        draws.append([a[9] + b * a[14] for b in range(emb.shape[0])])           # a[9]: offset, a[14]: image_stride
        return real(emb, *a)

    monkeypatch.setattr(ops, "shape_samples", spy)
    out = str(tmp_path / "hflip_k4")
    seg = Segmenter(*nets, out_dir=out, batch_size=3, views="hflip", samples=K, seed=3)
    summary = seg.run(folder)
    assert summary["n_samples"] == 8 and summary["views"] == [0, 1]
    assert seg.sample_offsets == [i * 2 * Vn * N for i in range(6)]
    # image i, view v: the disc draws from 2 V N i + 2 N v, the cup N behind it — whatever the batch
    want = []
    for first in (0, 3):
        for v in range(Vn):
            disc = [2 * Vn * N * i + 2 * N * v for i in range(first, first + 3)]
            want += [disc, [o + N for o in disc]]
    assert draws == want
    rows = U.read_csv(out)
    assert len(rows) == 6 and all(r["n_samples"] == 8 and 0.0 <= r["disc_std_mean"] <= 0.5 and 0.0 <= r["cup_std_mean"] <= 0.5 for r in rows)


@pytest.fixture(scope="module")
def cal_trees(tmp_path_factory):
    """The labelled synthetic tree of test_calibration_gpu.py: two Domain3/test trees, one per label size."""
    rs = np.random.RandomState(12)
    roots = []
    for t, idx in enumerate((range(0, 4), range(4, 6))):
        root = str(tmp_path_factory.mktemp("fundus_views%d" % t))
        for sub in ("image", "mask"):
            os.makedirs(os.path.join(root, "Domain3", "test", "ROIs", sub))
        for i in idx:
            im, mk = _sample(rs, CAL_SIZES[i][0], CAL_SIZES[i][1], rgb_mask=False)
            name = "%s-%d-L_test.png" % ("GNS"[i % 3], i)
            im.save(os.path.join(root, "Domain3", "test", "ROIs", "image", name))
            mk.save(os.path.join(root, "Domain3", "test", "ROIs", "mask", name))
        roots.append(root)
    return roots


def test_calibration_run_with_views(disc_nets, cal_trees, tmp_path):
    """The filler networks predict no disc, and a cup row without a scored pixel has no spread to report; here the disc head's bias
    is raised until every pixel of every crop is inside od_pred (set_disc_bias "min": a margin of 2 in the logit, where the views
    and the samples move it by hundredths), so the cup is scored everywhere with and without views and n_scored is comparable."""
    from wtpse_hip import calibration as C
    from wtpse_hip.calibration_run import CalibrationRun
    feed = _feed(cal_trees)
    nets = set_disc_bias(disc_nets, [b[0] for b in feed], "min")
    tables = {}
    for name, views in (("plain", None), ("hflip", "hflip")):
        out = str(tmp_path / name)
        summary = CalibrationRun(*nets, out_dir=out, samples=2, scales=(0, 1), bins=16, seed=3, views=views).run(feed)
        assert summary.get("views") == ([0, 1] if views else None)
        tables[name] = C.read_csv(out, "calibration")
    spread = ("spread_wrong_mean", "spread_right_mean", "spread_auroc")
    for a, b in zip(tables["plain"], tables["hflip"]):
        print("scale %g %s: n_scored %d (plain) / %d (hflip); hflip spread columns %s"
              % (b["scale"], b["structure"], a["n_scored"], b["n_scored"], [b[k] for k in spread]))
    for a, b in zip(tables["plain"], tables["hflip"]):
        assert (a["scale"], a["structure"]) == (b["scale"], b["structure"])
        assert a["n_scored"] == b["n_scored"] > 0
        if b["scale"] == 0.0:
            assert all(math.isnan(a[k]) for k in spread)                        # without views scale 0 stays the deterministic row
            assert all(math.isfinite(b[k]) for k in spread), b
    rows = C.read_csv(str(tmp_path / "hflip"), "per_image")
    assert len(rows) == 12 and all(math.isfinite(r["disc_dice"]) for r in rows)
