"""Calibration against labels on the device (-m gpu): ops.calibration_hist against calibration.hist_host bit for bit — tail lanes, an
odd width with the CPU test's special pixels planted, a constant map (every lane of every wave on one key), many workgroups per image,
a pre-filled record, the argument checks — and calibration_run.CalibrationRun end to end on the synthetic tree and the seeded networks
of tests/test_test_run_gpu.py."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

from oracle.fundus_tree import _sample
from oracle.inputs import make_inputs
from test_calibration_cpu import expected_record, special_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(prob, spread, label, region, threshold=0.75):
    """[B,h,w] arrays -> (device record, host record), uint32 [B, REC]."""
    from wtpse_hip import calibration as C, ops
    args = [None if a is None else a[:, None] for a in (prob, spread, label, region)]
    rec = ops.calibration_hist(*[_dev(a) for a in args], threshold)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (prob.shape[0], C.REC) and ops.CAL_REC == C.REC and ops.CAL_BINS == C.BINS
    return rec.cpu().numpy().view(np.uint32), C.hist_host(prob, spread, label, region, threshold)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _random(seed, B, h, w):
    """Fundus-like and hostile at once: mostly saturated probabilities, a band of everything between, values beyond [0, 1], a few
    NaNs; a spread that is mostly 0; labels 0 / 1 / 2; a region that leaves out a border."""
    rng = np.random.default_rng(seed)
    prob = rng.uniform(-0.1, 1.1, (B, h, w)).astype(np.float32)
    kind = rng.random((B, h, w))
    prob[kind < 0.35] = 0.0
    prob[kind > 0.75] = 1.0
    prob[rng.random((B, h, w)) < 0.003] = np.nan
    spread = np.where(rng.random((B, h, w)) < 0.6, 0.0, rng.uniform(-0.05, 0.6, (B, h, w))).astype(np.float32)
    spread[rng.random((B, h, w)) < 0.002] = np.nan
    label = rng.integers(0, 3, (B, h, w)).astype(np.float32) * (rng.random((B, h, w)) < 0.5)
    region = (rng.random((B, h, w)) < 0.8).astype(np.uint8) * 7
    region[:, :, :max(1, w // 9)] = 0
    return prob, spread, label.astype(np.float32), region


def test_tail_lanes_8x12():
    """96 pixels: one and a half waves of one workgroup."""
    from wtpse_hip import calibration as C
    prob, spread, label, region = _random(1, 1, 8, 12)
    got, want = _run(prob, spread, label, region)
    _same(got, want, "8x12")
    assert C.split_record(got[0])[2].sum() == 96


def test_odd_width_with_the_special_pixels():
    from wtpse_hip import calibration as C
    B, h, w = 3, 37, 53
    prob, spread, label, region = _random(2, B, h, w)
    sp, ss, sl, sr, want_special, tail_special = special_case()
    for b, at in ((0, 0), (1, 700), (2, h * w - 15)):                # the 15 pixels at the start, in the middle, at the very end
        for a, s in ((prob, sp), (spread, ss), (label, sl), (region, sr)):
            a[b].reshape(-1)[at:at + 15] = s
    got, want = _run(prob, spread, label, region)
    _same(got, want, "37x53")
    for part in C.split_record(got)[:2]:
        assert (part.sum((1, 2)) == C.split_record(got)[2][:, 3]).all()
    assert (C.split_record(got)[2].sum(1) == h * w).all()
    # the special pixels alone, on the device
    got, want = _run(sp.reshape(1, 3, 5), ss.reshape(1, 3, 5), sl.reshape(1, 3, 5), sr.reshape(1, 3, 5))
    _same(got, want, "special")
    assert np.array_equal(got[0], expected_record(want_special, tail_special))
    # no region, no spread
    got, want = _run(prob, None, label, None)
    _same(got, want, "37x53 without region and spread")
    hs, tail = C.split_record(got)[1:]
    assert (hs[:, 1:].sum((1, 2)) == 0).all() and (tail[:, :2] == 0).all() and (tail[:, 2] == np.isnan(prob).sum((1, 2))).all()
    # another threshold reaches the kernel
    got, want = _run(prob, spread, label, region, 0.3)
    _same(got, want, "threshold 0.3")


def test_constant_map_every_lane_on_one_key():
    """prob = 0.25, spread = 0 everywhere: every wave is uniform in both keys, the worst contention there is.  Image 0 is all
    background, image 1 all object: per image one nonzero slot per histogram, holding h w."""
    from wtpse_hip import calibration as C
    B, h, w = 2, 256, 256
    prob = np.full((B, h, w), 0.25, np.float32)
    spread = np.zeros((B, h, w), np.float32)
    label = np.zeros((B, h, w), np.float32)
    label[1] = 1.0
    got, want = _run(prob, spread, label, None)
    _same(got, want, "constant")
    hp, hs, tail = C.split_record(got)
    for b in range(B):
        assert np.argwhere(hp[b]).tolist() == [[256, b]] and hp[b, 256, b] == h * w
        assert np.argwhere(hs[b]).tolist() == [[0, b]] and hs[b, 0, b] == h * w          # 0.25 is below the threshold: image 1 is all misses
        assert tail[b].tolist() == [0, 0, 0, h * w]


def test_many_workgroups_and_repeatability():
    from wtpse_hip import calibration as C, ops
    prob, spread, label, region = _random(4, 1, 600, 800)
    args = [_dev(a[:, None]) for a in (prob, spread, label, region)]
    first = ops.calibration_hist(*args)
    got = first.cpu().numpy().view(np.uint32)
    _same(got, C.hist_host(prob, spread, label, region), "600x800")
    hp, hs, tail = C.split_record(got[0])
    assert hp.sum() == hs.sum() == tail[3] and tail.sum() == 600 * 800 and tail[3] > 300000
    assert torch.equal(ops.calibration_hist(*args), first)


def test_record_is_zeroed_and_bad_arguments_do_not_launch():
    from wtpse_hip import calibration as C, ops
    from wtpse_hip.lib import lib
    prob, spread, label, region = _random(5, 2, 20, 33)
    p, s, l, r = (_dev(a[:, None]) for a in (prob, spread, label, region))
    rec = torch.full((2, C.REC), -559038737, dtype=torch.int32, device=DEV)
    st = ops.stream_ptr()
    L = lib()
    L.call("wtpse_calibration_hist", ops.ptr(p), ops.ptr(s), ops.ptr(l), ops.ptr(r), 0.75, ops.ptr(rec), 2, 20, 33, st)
    _same(rec.cpu().numpy().view(np.uint32), C.hist_host(prob, spread, label, region), "pre-filled")
    garbage = torch.full((2, C.REC), 12345, dtype=torch.int32, device=DEV)
    raw = L.raw("wtpse_calibration_hist")
    for B, h, w in ((2, 0, 33), (2, 20, 4097), (8192, 20, 33), (0, 20, 33), (2, 4097, 1)):
        assert raw(ops.ptr(p), ops.ptr(s), ops.ptr(l), ops.ptr(r), 0.75, ops.ptr(garbage), B, h, w, st) == -1, (B, h, w)
    for args in ((0, ops.ptr(l), ops.ptr(garbage)), (ops.ptr(p), 0, ops.ptr(garbage)), (ops.ptr(p), ops.ptr(l), 0)):
        assert raw(args[0], ops.ptr(s), args[1], ops.ptr(r), 0.75, args[2], 2, 20, 33, st) == -1
    torch.cuda.synchronize()
    assert bool((garbage == 12345).all())                            # nothing was launched, nothing was zeroed
    # the binding's own checks
    for kw in (dict(prob=p.cpu()), dict(label=l.to(torch.float64)), dict(spread=s[:, :, :, :32]), dict(region=r.float()),
               dict(region=r[:1]), dict(prob=p[:, 0])):
        a = dict(prob=p, spread=s, label=l, region=r)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.calibration_hist(a["prob"], a["spread"], a["label"], a["region"])


# ---- the run end to end -----------------------------------------------------------------------------------------------------------
SIZES = [(300, 280)] * 4 + [(212, 251)] * 2                          # (width, height) of the six crops: a batch of four, a batch of two
SAMPLES, SCALES, BINS = 4, (0.0, 1.0), 16


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """Two Domain3/test trees, one per label size (the images of one batch must share it)."""
    rs = np.random.RandomState(12)
    roots = []
    for t, idx in enumerate((range(0, 4), range(4, 6))):
        root = str(tmp_path_factory.mktemp("fundus_cal%d" % t))
        for sub in ("image", "mask"):
            os.makedirs(os.path.join(root, "Domain3", "test", "ROIs", sub))
        for i in idx:
            im, mk = _sample(rs, SIZES[i][0], SIZES[i][1], rgb_mask=False)
            name = "%s-%d-L_test.png" % ("GNS"[i % 3], i)
            im.save(os.path.join(root, "Domain3", "test", "ROIs", "image", name))
            mk.save(os.path.join(root, "Domain3", "test", "ROIs", "mask", name))
        roots.append(root)
    return roots


@pytest.fixture(scope="module")
def nets():
    """Seeded networks one training step away from the filler, as tests/test_test_run_gpu.py builds them."""
    from test_parity_gpu import build_nets, HP
    from wtpse_hip.step import TrainStep
    nets = build_nets(1)
    img, od, oc = make_inputs(41, 3, 64, 64)
    ts = TrainStep(nets[0], nets[1], nets[2], nets[3], HP)
    for n in nets:
        n.seed_noise(5)
    ts.step(img.to(DEV), od.to(DEV), oc.to(DEV))
    torch.cuda.synchronize()
    return nets


def _feed(trees):
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.test_run import FundusTestBatches
    return list(itertools.chain(*[FundusTestBatches(FundusTree(t, phase="test", splitid=(3,), state="prediction"), 4, DEV) for t in trees]))


@pytest.fixture(scope="module")
def run(trees, nets, tmp_path_factory):
    from wtpse_hip.calibration_run import CalibrationRun
    out = str(tmp_path_factory.mktemp("cal_run"))
    for n in nets:
        n.train()
    feed = _feed(trees)
    assert [b[0].shape[0] for b in feed] == [4, 2]
    r = CalibrationRun(*nets, out_dir=out, samples=SAMPLES, scales=SCALES, bins=BINS, seed=3)
    summary = r.run(feed)
    assert all(n.training for n in nets)                             # eval for the duration, restored
    return out, r, summary, feed


FILES = ("calibration.csv", "reliability.csv", "risk_coverage.csv", "per_image.csv", "summary.json")


def test_run_writes_the_documented_files(run):
    import json
    from wtpse_hip import calibration as C
    out, r, summary, feed = run
    for f, cols in (("calibration", C.CALIBRATION_COLUMNS), ("reliability", C.RELIABILITY_COLUMNS), ("risk_coverage", C.RISK_COLUMNS),
                    ("per_image", C.PER_IMAGE_COLUMNS)):
        with open(os.path.join(out, f + ".csv")) as fh:
            assert fh.readline().strip().split(",") == list(cols), f
    assert C.CALIBRATION_COLUMNS[:6] == ("scale", "structure", "n_scored", "n_excluded_neg", "n_excluded_pos", "n_invalid")
    with open(os.path.join(out, "summary.json")) as fh:
        assert json.load(fh) == summary
    assert summary["n"] == 6 and summary["scales"] == [0.0, 1.0] and summary["samples"] == SAMPLES and summary["bins"] == BINS
    assert set(summary["disc"]) == set(summary["cup"]) == {"lowest_nll", "lowest_ece"} and summary["disc"]["lowest_nll"] in (0.0, 1.0)
    table = C.read_csv(out, "calibration")
    assert [(t["scale"], t["structure"]) for t in table] == [(0.0, "disc"), (0.0, "cup"), (1.0, "disc"), (1.0, "cup")]
    pixels = sum(w * h for w, h in SIZES)
    for t in table:
        assert t["n_scored"] + t["n_excluded_neg"] + t["n_excluded_pos"] + t["n_invalid"] == pixels, t
        if t["structure"] == "disc":
            assert t["n_excluded_neg"] == t["n_excluded_pos"] == 0 and t["n_defined"] == 0 and math.isnan(t["vcdr_coverage"])
        if t["scale"] == 0.0:
            assert math.isnan(t["spread_auroc"]) and math.isnan(t["vcdr_coverage"]) and math.isnan(t["vcdr_spearman"]) and t["n_defined"] == 0
        print("scale %g %s: n_scored %d, n_excluded %d + %d, error_rate %r, nll %r" % (t["scale"], t["structure"], t["n_scored"],
                                                                                     t["n_excluded_neg"], t["n_excluded_pos"], t["error_rate"], t["nll"]))
        assert t["n_invalid"] == 0
        if t["n_scored"] == 0:                                       # (these networks may predict no disc at all: then no cup pixel is scored)
            assert all(math.isnan(t[k]) for k in ("error_rate", "ece", "mce", "brier", "nll", "auroc"))
        else:
            assert 0.0 <= t["error_rate"] <= 1.0 and t["nll"] > 0.0 and 0.0 <= t["ece"] <= t["mce"] <= 1.0 and 0.0 <= t["brier"] <= 1.0
    cup1 = table[3]
    assert 0 <= cup1["n_defined"] <= 6 and (cup1["n_defined"] == 0 or 0.0 <= cup1["vcdr_coverage"] <= 1.0)
    rel = C.read_csv(out, "reliability")
    assert len(rel) == 4 * BINS and sum(x["n"] for x in rel if x["scale"] == 1.0 and x["structure"] == "disc") == table[2]["n_scored"]
    risk = C.read_csv(out, "risk_coverage")
    assert {(x["scale"], x["structure"], x["level"]) for x in risk} == {(1.0, s, lv) for s in C.STRUCTURES for lv in ("pixel", "image")}
    assert len(risk) == 4 * 20
    last = [x for x in risk if x["structure"] == "disc" and x["level"] == "pixel"][-1]
    assert last["coverage"] == 1.0 and abs(last["risk"] - table[2]["error_rate"]) < 1e-12
    rows = C.read_csv(out, "per_image")
    assert [(x["scale"], x["index"]) for x in rows] == [(s, i) for s in SCALES for i in range(1, 7)]
    assert [x["name"] for x in rows[:6]] == sum((b[3] for b in feed), [])
    for x in rows[:6]:
        assert all(math.isnan(x["vcdr_" + k]) for k in ("mean", "std", "p05", "p95")) and math.isnan(x["vcdr_inside"]) and 0.0 < x["vcdr_label"] < 1.0
    for a, b in zip(rows[:6], rows[6:]):                             # the deterministic columns do not depend on the scale
        assert all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in ("disc_dice", "cup_dice", "vcdr_label", "vcdr_pred", "acdr_pred"))


def test_scale_zero_is_the_deterministic_prediction(run, nets):
    """At scale 0 every scored pixel sits in spread bin 0, and hist_p summed over the images is hist_host of torch.sigmoid of
    predict_pair's resized logits — the cup's under the region rule, rebuilt here from ops.roi's od_pred."""
    from wtpse_hip import calibration as C, ops, validate as V
    out, r, summary, feed = run
    hp, hs, tail = C.split_record(r.records[0.0])                    # [6, 2, ...]
    assert (hs[:, :, 1:].sum((2, 3)) == 0).all() and (hs[:, :, 0].sum(2) == tail[:, :, 3]).all()
    want = np.zeros((2, C.REC), np.int64)
    for n in nets:
        n.eval()
    first = 0
    for image, od, oc, _ in feed:
        size, B = tuple(od.shape[2:]), image.shape[0]
        pred, pred_oc = V.predict_pair(*nets, image, size)
        od_pred = ops.roi(image.contiguous(), V.predict_pair(*nets, image)[0])[1]
        region = (ops.resize_bilinear(od_pred, size) == 1.0).cpu().numpy()
        want[0] += C.hist_host(torch.sigmoid(pred).cpu().numpy(), None, od.cpu().numpy(), None, 0.75).astype(np.int64).sum(0)
        per_image = C.hist_host(torch.sigmoid(pred_oc).cpu().numpy(), None, oc.cpu().numpy(), region, 0.75)
        want[1] += per_image.astype(np.int64).sum(0)
        assert np.array_equal(r.records[0.0][first:first + B, 1], per_image)
        first += B
    for n in nets:
        n.train()
    got = r.records[0.0].astype(np.int64).sum(0)
    assert np.array_equal(got, want)
    assert np.array_equal(C.split_record(got)[0], C.split_record(want)[0])
    table = C.read_csv(out, "calibration")
    for j in range(2):
        assert table[j]["n_scored"] == want[j, -1] and table[j]["n_excluded_pos"] == want[j, -3]
        s = C.scores(C.split_record(want[j])[0], BINS)
        assert all(table[j][k] == s[k] or (s[k] != s[k] and table[j][k] != table[j][k]) for k in ("ece", "mce", "brier", "nll", "auroc"))
    # the sampled scale: the region is the deterministic one, so the same pixels are left out; both histograms hold the scored ones
    hp1, hs1, tail1 = C.split_record(r.records[1.0])
    assert np.array_equal(tail1[:, :, :2], tail[:, :, :2]) and (tail1.sum(2) == tail.sum(2)).all()
    assert (hp1.sum((2, 3)) == tail1[:, :, 3]).all() and (hs1.sum((2, 3)) == tail1[:, :, 3]).all()


def test_dice_columns_equal_the_test_run(run, nets, tmp_path):
    from wtpse_hip import calibration as C
    from wtpse_hip.test_run import TestRun, read_table
    out, r, summary, feed = run
    TestRun(*nets, out_dir=str(tmp_path)).run(feed)
    want, _ = read_table(str(tmp_path))
    rows = C.read_csv(out, "per_image")
    for s in range(len(SCALES)):
        for a, b in zip(rows[6 * s:6 * s + 6], want):
            assert (a["index"], a["name"]) == (b["index"], b["name"])
            assert a["disc_dice"] == b["disc_dice"] and a["cup_dice"] == b["cup_dice"]


def test_second_run_writes_the_same_bytes(run, nets, tmp_path):
    from wtpse_hip.calibration_run import CalibrationRun
    out, r, summary, feed = run
    again = CalibrationRun(*nets, out_dir=str(tmp_path), samples=SAMPLES, scales=SCALES, bins=BINS, seed=3)
    assert again.run(feed) == summary
    for f in FILES:
        with open(os.path.join(out, f), "rb") as fa, open(tmp_path / f, "rb") as fb:
            assert fa.read() == fb.read(), f
    assert sorted(os.listdir(tmp_path)) == sorted(FILES)


# ---- the run on stub predictions: a predicted disc with a cup inside, so that the cup's region, the sampled maps and the image-level
# ---- numbers all carry values (the seeded networks above predict no disc) --------------------------------------------------------
STUB_K, STUB_SCALES = 8, (0.0, 1.0, 2.0)
#              cy,  cx,   r, the label's cup: (offset in r, radius in r)
STUB_IMAGES = [(120, 130, 70, 0.05, 0.45), (140, 110, 60, 0.80, 0.45), (128, 128, 85, 0.00, 0.47), (118, 140, 64, 0.10, 0.75),
               (135, 120, 78, 0.00, 0.44)]
STUB_BATCHES = [((280, 300), (0, 1, 2)), ((200, 256), (3, 4))]       # label size (h, w), the images of the batch


def _soft_disc(S, cy, cx, r):
    """A logit map [S,S]: +-30 with a soft edge, in steps of 0.25 (none within 0.1 of ln 3, where sigmoid crosses 0.75)."""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    return (np.round(4.0 * np.clip(2.0 * (r - np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)), -30.0, 30.0)) / 4.0).astype(np.float32)


def _stub_run_class():
    from wtpse_hip import ops
    from wtpse_hip.calibration_run import CalibrationRun
    from wtpse_hip.uncertainty import ShapeSamples

    class StubRun(CalibrationRun):
        """CalibrationRun with the two network calls replaced: the image's first pixel names its row of STUB_IMAGES."""

        def _params(self, image):
            return [STUB_IMAGES[int(round(float(v)))] for v in image[:, 0, 0, 0].cpu()]

        def _logits(self, image, scale_d=None, scale_c=None):
            """-> (disc, cup) logits [B,K,S,S] (K = 1 for the deterministic pair): sample k scales the radii by 1 + scale g_k."""
            S = image.shape[2]
            g = np.linspace(-1.5, 1.5, STUB_K) * 0.04
            fd = [1.0] if scale_d is None else 1.0 + scale_d * g
            fc = [1.0] if scale_c is None else 1.0 - scale_c * g
            d = np.stack([[_soft_disc(S, cy, cx, r * f) for f in fd] for cy, cx, r, _, _ in self._params(image)])
            c = np.stack([[_soft_disc(S, cy + 5, cx - 4, 0.45 * r * f) for f in fc] for cy, cx, r, _, _ in self._params(image)])
            return _dev(d), _dev(c)

        def predict_pair(self, image):
            d, c = self._logits(image)
            return d, ops.relu_mask(c, ops.roi(image.contiguous(), d)[1])

        def predict_samples(self, image, scale, first):
            pred, pred_oc = self.predict_pair(image)
            od_pred = ops.roi(image.contiguous(), pred)[1]
            out = []
            for logits, logit, masked in zip(self._logits(image, scale, scale), (pred, pred_oc), (False, True)):
                if masked:                                           # as validate.predict_pair_samples leaves the cup outside od_pred
                    logits = logits * od_pred
                p = torch.sigmoid(logits)
                out.append(ShapeSamples(mean=p.mean(1, keepdim=True).contiguous(), std=p.std(1, unbiased=False, keepdim=True).contiguous(),
                                        votes=(p > 0.75).sum(1, keepdim=True).to(torch.uint8).contiguous(), logits=logits.contiguous(),
                                        logit=logit, n_samples=STUB_K, seed=self.seed, offset=0, scale=scale))
            return out

    return StubRun


def _stub_feed():
    feed = []
    for (h, w), idx in STUB_BATCHES:
        image = np.random.default_rng(h).uniform(-1, 1, (len(idx), 3, 256, 256)).astype(np.float32)
        od, oc = np.zeros((len(idx), 1, h, w), np.float32), np.zeros((len(idx), 1, h, w), np.float32)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        for j, i in enumerate(idx):
            image[j, 0, 0, 0] = i
            cy, cx, r, off, rel = STUB_IMAGES[i]
            cy, cx, ry, rx = cy * h / 256.0, cx * w / 256.0, r * h / 256.0, r * w / 256.0
            od[j, 0] = ((yy - cy - 2) / ry) ** 2 + ((xx - cx + 2) / rx) ** 2 <= 1.0
            oc[j, 0] = ((yy - cy - off * ry) / (rel * ry)) ** 2 + ((xx - cx - off * rx) / (rel * rx)) ** 2 <= 1.0
        feed.append((_dev(image), _dev(od), _dev(oc), ["stub%d.png" % i for i in idx]))
    return feed


@pytest.fixture(scope="module")
def stub_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cal_stub"))
    feed = _stub_feed()
    r = _stub_run_class()(*[torch.nn.Identity() for _ in range(4)], out_dir=out, samples=STUB_K, scales=STUB_SCALES, bins=BINS, seed=1)
    r.run(feed)
    return out, r, feed


def test_stub_run_scores_the_cup_inside_the_resized_disc(stub_run):
    """Every per-image record of every scale against hist_host of host copies of what the run must have fed the kernel: at scale 0
    the sigmoid of the resized pair, at a sampled scale the resized mean (prob) and std (spread) of each stage — disc first, cup
    second — the cup under the region rebuilt on the host: od_pred = (logit > ln 3), resized, == 1.0."""
    from wtpse_hip import calibration as C, ops
    out, r, feed = stub_run
    table = C.read_csv(out, "calibration")
    for t in table:
        print({k: t[k] for k in ("scale", "structure", "n_scored", "n_excluded_neg", "n_excluded_pos", "error_rate", "nll", "spread_auroc")})
        if t["structure"] == "cup":
            assert t["n_scored"] > 0 and t["n_excluded_neg"] > 0 and t["n_excluded_pos"] > 0
        assert t["n_scored"] + t["n_excluded_neg"] + t["n_excluded_pos"] + t["n_invalid"] == sum(h * w * len(i) for (h, w), i in STUB_BATCHES)
    host = lambda t, size: ops.resize_bilinear(t.contiguous(), size).cpu().numpy()
    first = 0
    for image, od, oc, _ in feed:
        size, B = tuple(od.shape[2:]), image.shape[0]
        pred, pred_oc = r.predict_pair(image)
        od_pred = _dev((pred.cpu().numpy() > math.log(3.0)).astype(np.float32))
        resized = host(od_pred, size)
        region = resized == 1.0
        assert ((resized > 0) & ~region).any() and region.any()      # a seam that `> 0` would let in
        lod, loc = od.cpu().numpy(), oc.cpu().numpy()
        for scale in STUB_SCALES:
            if scale == 0.0:
                maps = [torch.sigmoid(ops.resize_bilinear(t.contiguous(), size)).cpu().numpy() for t in (pred, pred_oc)] + [None, None]
            else:
                disc, cup = r.predict_samples(image, scale, first)
                maps = [host(t, size) for t in (disc.mean, cup.mean, disc.std, cup.std)]
                assert float(maps[2].max()) > 0.05 and float(maps[3].max()) > 0.05 and not np.array_equal(maps[0], maps[2])
            got = r.records[scale][first:first + B]
            _same(got[:, 0], C.hist_host(maps[0], maps[2], lod, None, 0.75), ("disc", scale, size))
            _same(got[:, 1], C.hist_host(maps[1], maps[3], loc, region, 0.75), ("cup", scale, size))
        first += B
    assert all(t["spread_auroc"] == t["spread_auroc"] and t["spread_wrong_mean"] >= 0.0 for t in table if t["scale"] != 0.0)


def test_stub_run_image_level_numbers_follow_from_the_rows(stub_run):
    """coverage, vcdr_inside, vcdr_spearman, n_defined and the image risk-coverage curve recomputed from per_image.csv."""
    from wtpse_hip import calibration as C
    out, r, feed = stub_run
    table, rows, risk = C.read_csv(out, "calibration"), C.read_csv(out, "per_image"), C.read_csv(out, "risk_coverage")
    n = len(STUB_IMAGES)
    assert len(rows) == n * len(STUB_SCALES)
    seen = set()
    for scale in STUB_SCALES[1:]:
        rs = [x for x in rows if x["scale"] == scale]
        cup = [t for t in table if t["scale"] == scale and t["structure"] == "cup"][0]
        assert [x["index"] for x in rs] == list(range(1, n + 1))
        for x in rs:
            assert x["vcdr_std"] > 0.0 and x["vcdr_p05"] < x["vcdr_mean"] < x["vcdr_p95"] and 0.2 < x["vcdr_pred"] < 0.7
            assert x["vcdr_inside"] == float(x["vcdr_p05"] <= x["vcdr_label"] <= x["vcdr_p95"])
            seen.add(x["vcdr_inside"])
        assert cup["n_defined"] == n
        for k in C.RATIOS:
            inside = [x[k + "_p05"] <= x[k + "_label"] <= x[k + "_p95"] for x in rs]
            assert cup[k + "_coverage"] == sum(inside) / n, (k, scale)
        assert cup["vcdr_coverage"] == sum(x["vcdr_inside"] for x in rs) / n
        err = [abs(x["vcdr_pred"] - x["vcdr_label"]) for x in rs]
        want = C.spearman([x["vcdr_std"] for x in rs], err)
        assert cup["vcdr_spearman"] == want and want == want
        order = sorted(range(n), key=lambda i: (rs[i]["vcdr_std"], i))
        for name in C.STRUCTURES:
            curve = [x for x in risk if x["scale"] == scale and x["structure"] == name and x["level"] == "image"]
            assert len(curve) == 20
            for k, x in enumerate(curve, 1):
                kept = order[:-(-k * n // 20)]
                assert abs(x["risk"] - (1.0 - sum(rs[i][name + "_dice"] for i in kept) / len(kept))) < 1e-14, (name, k)
    assert seen == {0.0, 1.0}                                        # image 3's label ratio lies outside every interval, others inside
    wide, narrow = ([x["vcdr_std"] for x in rows if x["scale"] == s] for s in (2.0, 1.0))
    assert all(a > b for a, b in zip(wide, narrow))                  # the larger scale spreads the ratios further
