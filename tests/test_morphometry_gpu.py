"""Optic-disc morphometry on the device (-m gpu): ops.onh_profile against morphometry.profile_host bit for bit, its repeatability and
argument checks, Segmenter.back / Segmenter.run / TestRun.batch with the switch on against the host's finishing of the host's records,
and the switch-off outputs unchanged beside them."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.inputs import make_inputs
from test_morphometry_cpu import raster_ellipse, same
from test_segment_cpu import content
from test_segment_gpu import BACK_SIZES, _back_expectation, _check_row, _pseudo_logits, _segmenter

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
def _pair(kind, h, w):
    """One (disc, cup) pair [h, w] uint8: 0 an off-centre ellipse disc with a cup shifted inside it, 1 a cup that sticks out of the disc,
    2 an empty disc with a cup, 3 an empty cup, 4 an all-ones disc (every lane of a wave in a handful of sectors, corners included)
    with a cup over its left part."""
    cy, cx, r = 0.45 * (h - 1), 0.56 * (w - 1), 0.5 * min(h, w)
    disc = raster_ellipse(h, w, cy, cx, 0.8 * r + 0.4, 0.6 * r + 0.4, 0.4) * 255
    cup = raster_ellipse(h, w, cy + 0.1 * r, cx - 0.15 * r, 0.4 * r + 0.4, 0.25 * r + 0.4, 1.2) * 3
    if kind == 1:
        cup = raster_ellipse(h, w, cy - 0.5 * r, cx + 0.6 * r, 0.5 * r + 0.4, 0.2 * r + 0.4, 2.5)
    elif kind == 2:
        disc = np.zeros_like(disc)
    elif kind == 3:
        cup = np.zeros_like(cup)
    elif kind == 4:
        disc = np.ones_like(disc)
        cup = np.zeros_like(cup)
        cup[:, :max(1, w // 3)] = 9
    return disc.astype(np.uint8), cup.astype(np.uint8)


#         B, h, w, N, first kind (image b holds kind (first + b) % 5)
CASES = [(1, 1, 1, 8, 4), (3, 37, 53, 24, 0), (2, 64, 64, 24, 3), (3, 70, 301, 360, 4), (2, 513, 70, 8, 2), (1, 1030, 1027, 24, 4),
         (1, 8, 4096, 24, 4), (130, 32, 32, 24, 0)]


def _case(B, h, w, first):
    pairs = [_pair((first + b) % 5, h, w) for b in range(B)]
    return np.stack([p[0] for p in pairs])[:, None], np.stack([p[1] for p in pairs])[:, None]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_%dx%d_N%d" % c[:4])
def test_onh_profile_matches_host_bitwise(case):
    from wtpse_hip import morphometry as M, ops
    B, h, w, N, first = case
    disc, cup = _case(B, h, w, first)
    d, c = _dev(disc), _dev(cup)
    geom = ops.mask_geometry(d)
    prof, mom = ops.onh_profile(d, c, geom, N)
    assert tuple(prof.shape) == (B, N, 4) and prof.dtype == torch.int32 and tuple(mom.shape) == (B, 2, 4) and mom.dtype == torch.int64
    want_p, want_m = M.profile_host(disc[:, 0], cup[:, 0], N)
    got_p, got_m = prof.cpu().numpy().view(np.uint32), mom.cpu().numpy()
    assert np.array_equal(got_m, want_m), (case, got_m[:2].tolist(), want_m[:2].tolist())
    bad = np.argwhere(got_p != want_p)
    assert len(bad) == 0, (case, len(bad), bad[:4].tolist(), got_p[tuple(bad[0])], want_p[tuple(bad[0])])
    assert int(want_p[:, :, 2].sum()) == int((disc != 0)[disc.reshape(B, -1).any(1)].sum())                    # every disc pixel counted
    # repeatability: the second run on the same input, bit for bit
    prof2, mom2 = ops.onh_profile(d, c, geom, N)
    assert torch.equal(prof2, prof) and torch.equal(mom2, mom)


def test_onh_profile_argument_checks(monkeypatch):
    from wtpse_hip import ops
    disc, cup = (_dev(a) for a in _case(2, 16, 16, 0))
    geom = ops.mask_geometry(disc)
    ops.onh_profile(disc, cup, geom, 8)
    launches, real = [], ops.lib().call
    monkeypatch.setattr(ops.lib(), "call", lambda *a: launches.append(a) or real(*a))
    wide = torch.zeros(2, 1, 16, 32, dtype=torch.uint8, device=DEV)
    bad = [dict(disc=disc.float()),                                                # wrong dtype
           dict(cup=cup.to(torch.int8)),
           dict(disc=wide[:, :, :, ::2]),                                          # non-contiguous
           dict(cup=wide),                                                         # shape mismatch
           dict(geom=geom[:1]), dict(geom=geom.to(torch.int32)), dict(geom=geom.t().contiguous().t()),
           dict(geom=geom.cpu()), dict(cup=cup.cpu()),                             # records / mask on another device
           dict(N=12), dict(N=368), dict(N=0), dict(N=16.5)]
    for kw in bad:
        args = dict(disc=disc, cup=cup, geom=geom, N=24)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.onh_profile(args["disc"], args["cup"], args["geom"], args["N"])
    assert launches == []
    ops.onh_profile(disc, cup, geom, 24)
    assert len(launches) == 1 and launches[0][0] == "wtpse_onh_profile"


def test_sector_table_is_cached_per_device_and_N():
    from wtpse_hip import morphometry as M, ops
    disc, cup = (_dev(a) for a in _case(1, 16, 16, 0))
    geom = ops.mask_geometry(disc)
    ops.onh_profile(disc, cup, geom, 16)
    t = ops._SECTOR_TABLES[(disc.device, 16)]
    ops.onh_profile(disc, cup, geom, 16)
    assert ops._SECTOR_TABLES[(disc.device, 16)] is t and np.array_equal(t.cpu().numpy(), M.sector_table(16))


# ---- Segmenter.back ---------------------------------------------------------------------------------------------------------------
def _check_morph(got, want):
    from wtpse_hip import morphometry as M
    for k in M.INT_COLUMNS + ("eye",):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in M.FLOAT_COLUMNS:
        assert same(got[k], want[k]), (k, got[k], want[k])
    assert len(got["rim"]) == len(want["rim"]) and all(same(a, b) for a, b in zip(got["rim"], want["rim"]))
    assert all(same(a, b) for a, b in zip(got["rim_rel"], want["rim_rel"]))


def _host_row(d, c, N, eye):
    from wtpse_hip import morphometry as M
    from wtpse_hip.segment import mask_geometry_host
    prof, mom = M.profile_host(d, c, N)
    return M.finish(mask_geometry_host(d), mask_geometry_host(c), mom[0], prof[0], d.shape[0], d.shape[1], eye)


def test_back_with_morphometry_on_injected_logits(tmp_path):
    from wtpse_hip import morphometry as M
    from wtpse_hip.segment import read_measurements
    image = _dev(np.random.default_rng(2).uniform(-1, 1, (3, 3, 256, 256)).astype(np.float32))
    names = ["left eye.png", "b.png", "c.png"]
    for sub, empty_disc, N, eye in (("all", None, 24, "right"), ("one_empty", 1, 64, None)):
        lod, loc = (_dev(a) for a in _pseudo_logits(empty_disc))
        plain = _segmenter(str(tmp_path / sub / "plain"))
        labels0, overlays0, rows0 = plain.back(image, lod, loc, BACK_SIZES)
        seg = _segmenter(str(tmp_path / sub / "morph"), morphometry=True, sectors=N, eye=eye)
        res = seg.back_result(image, lod, loc, BACK_SIZES)
        labels, overlays, rows, morph = res.labels, res.overlays, res.rows, res.morph
        assert res.spreads is None and plain.back_result(image, lod, loc, BACK_SIZES).morph is None
        assert len(seg.back(image, lod, loc, BACK_SIZES)) == 3                     # the tuple of `back` does not grow
        # what morphometry=False returns
        assert all(np.array_equal(a, b) for a, b in zip(labels, labels0)) and all(np.array_equal(a, b) for a, b in zip(overlays, overlays0))
        for a, b in zip(rows, rows0):
            _check_row(a, b)
        want = _back_expectation(image, lod, loc)
        for i, ((d, c, _), (h, w)) in enumerate(zip(want, BACK_SIZES)):
            _check_morph(morph[i], _host_row(d, c, N, eye))
            assert morph[i]["height"] == h and morph[i]["width"] == w and morph[i]["sectors"] == N
            if i == empty_disc:
                assert morph[i]["vcdr_ellipse"] != morph[i]["vcdr_ellipse"]
            else:
                assert 0.3 < morph[i]["vcdr_ellipse"] < 0.6 and morph[i]["rim_min"] > 0 and (eye is None) == (morph[i]["isnt"] != morph[i]["isnt"])
        for s, lab, ov, r, m in ((plain, labels0, overlays0, rows0, None), (seg, labels, overlays, rows, morph)):
            s.write(names, lab, ov, r, m)
        s0, s1 = plain.finish(), seg.finish()
        assert {k: v for k, v in s1.items() if k in s0} == s0
        assert set(s1) - set(s0) == {"sectors", "mean_vcdr_ellipse", "mean_rim_min_rel"} | ({"n_isnt_violations"} if eye else set())
        assert s1["sectors"] == N
        with open(tmp_path / sub / "plain" / "measurements.csv", "rb") as fa, open(tmp_path / sub / "morph" / "measurements.csv", "rb") as fb:
            assert fa.read() == fb.read()
        assert read_measurements(str(tmp_path / sub / "morph"))[1] == s1
        back = M.read_csv(str(tmp_path / sub / "morph"))
        assert [r["name"] for r in back] == names and [r["index"] for r in back] == [1, 2, 3]
        for a, b in zip(back, morph):
            assert all(same(a[k], b[k]) for k in M.FLOAT_COLUMNS) and all(same(x, y) for x, y in zip(a["rim"], b["rim"]))
        assert not os.path.exists(tmp_path / sub / "plain" / "morphometry.csv")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from test_parity_gpu import build_nets
    nets = build_nets(1)
    for n in nets:
        n.eval()
    return nets


def test_segmenter_run_with_morphometry_and_samples(nets, tmp_path):
    from wtpse_hip import morphometry as M
    from wtpse_hip.segment import Segmenter
    root = tmp_path / "crops"
    root.mkdir()
    for i, (h, w) in enumerate([(70, 90), (100, 64), (70, 90)]):
        Image.fromarray(content(h, w, "random" if i % 2 else "smooth")).save(root / ("crop %02d.png" % i))
    plain, out = str(tmp_path / "plain"), str(tmp_path / "morph")
    s0 = Segmenter(*nets, out_dir=plain, batch_size=2, samples=3, seed=3).run(str(root))
    s1 = Segmenter(*nets, out_dir=out, batch_size=2, samples=3, seed=3, morphometry=True, sectors=16, eye="left").run(str(root))
    for f in ("morphometry.csv", "rim_profile.csv", "morphometry_uncertainty.csv"):
        assert os.path.isfile(os.path.join(out, f)) and not os.path.exists(os.path.join(plain, f)), f
    for f in ("measurements.csv", "uncertainty.csv"):
        with open(os.path.join(plain, f), "rb") as fa, open(os.path.join(out, f), "rb") as fb:
            assert fa.read() == fb.read(), f
    rows = M.read_csv(out)
    assert len(rows) == 3 and [r["index"] for r in rows] == [1, 2, 3] and [r["name"] for r in rows] == ["crop %02d.png" % i for i in range(3)]
    assert all(r["sectors"] == 16 and len(r["rim"]) == 16 and r["eye"] == "left" for r in rows)
    assert [(r["height"], r["width"]) for r in rows] == [(70, 90), (100, 64), (70, 90)]
    unc = M.read_uncertainty_csv(out)
    assert len(unc) == 3 and all(r["n_samples"] == 3 and 0 <= r["n_defined"] <= 3 and len(r["rim_rel_std"]) == 16 for r in unc)
    with open(os.path.join(out, "summary.json")) as f:
        summary = json.load(f)
    assert summary == s1 and {k: v for k, v in s1.items() if k in s0} == s0
    assert set(s1) - set(s0) == {"sectors", "mean_vcdr_ellipse", "mean_rim_min_rel", "n_isnt_violations"} and s1["sectors"] == 16
    # the rows belong to the written masks: the cup's area is the label map's, the disc's at least what the map shows of it
    for r in rows:
        lm = np.array(Image.open(os.path.join(out, "mask", r["name"])))
        cup = (lm == 0).astype(np.uint8)
        assert int(cup.sum()) == r["cup_area"] and int((lm == 128).sum()) <= r["disc_area"]


def test_morphometry_test_run_batch(nets, tmp_path):
    from wtpse_hip import morphometry as M, ops, validate as V
    from wtpse_hip.test_run import TestRun
    B, h, w = 2, 90, 70
    image = make_inputs(61, B, 64, 64)[0].to(DEV)
    lod = np.stack([raster_ellipse(h, w, 44, 36, 30, 26, 0.3), raster_ellipse(h, w, 40, 30, 28, 22, 1.0)])[:, None].astype(np.float32)
    loc = np.stack([raster_ellipse(h, w, 47, 33, 14, 10, 0.8), raster_ellipse(h, w, 38, 32, 9, 12, 0.0)])[:, None].astype(np.float32)
    plain = TestRun(*nets, out_dir=str(tmp_path / "plain"))
    m0, orig0, over0 = plain.batch(image, _dev(lod), _dev(loc))
    run = TestRun(*nets, out_dir=str(tmp_path / "morph"), morphometry=True, sectors=24, eye="right")
    off = TestRun(*nets, out_dir=str(tmp_path / "off"))
    m1, orig1, over1 = run.batch(image, _dev(lod), _dev(loc))
    assert np.array_equal(orig0, orig1) and np.array_equal(over0, over1)
    assert all(all(same(a, b) for a, b in zip(m0[k], m1[k])) for k in V.METRIC_KEYS)
    m2 = off.batch(image, _dev(lod), _dev(loc))
    assert np.array_equal(m2[1], orig0) and np.array_equal(m2[2], over0) and off.morph_label == [] and off.morphometry is False
    assert len(run.morph_label) == len(run.morph_pred) == B
    # the switch leaves the host sides' metrics and pictures as they are too
    mh0 = TestRun(*nets, out_dir=str(tmp_path / "h0"), overlay="host", metrics="host").batch(image, _dev(lod), _dev(loc))
    mh1 = TestRun(*nets, out_dir=str(tmp_path / "h1"), overlay="host", metrics="host", morphometry=True).batch(image, _dev(lod), _dev(loc))
    assert np.array_equal(mh0[1], mh1[1]) and np.array_equal(mh0[2], mh1[2])
    assert all(all(same(a, b) for a, b in zip(mh0[0][k], mh1[0][k])) for k in V.METRIC_KEYS)
    pred, pred_oc = V.predict_pair(*nets, image, (h, w))
    masks = ops.postprocess_masks(torch.cat((pred, pred_oc), 0).contiguous()).cpu().numpy()
    for i in range(B):
        _check_morph(run.morph_label[i], _host_row(lod[i, 0], loc[i, 0], 24, "right"))
        _check_morph(run.morph_pred[i], _host_row(masks[i, 0], masks[B + i, 0], 24, "right"))
    assert abs(run.morph_label[0]["vcdr_ellipse"] - 0.46) < 0.05 and abs(run.morph_label[1]["hcdr_ellipse"] - 9 / 23.9) < 0.05
    # the table of a run
    means = run.run([(image, _dev(lod), _dev(loc), ["a.png", "b.png"])])
    assert means["n"] == B
    rows, last = M.read_errors_csv(str(tmp_path / "morph"))
    assert [r["name"] for r in rows] == ["a.png", "b.png"] and last["name"] == "mean"
    for i, r in enumerate(rows):
        for k in M.STAT_KEYS:
            assert same(r[k + "_label"], run.morph_label[i][k]) and same(r[k + "_pred"], run.morph_pred[i][k])
            assert same(r[k + "_abs_diff"], abs(run.morph_pred[i][k] - run.morph_label[i][k]))
    plain.run([(image, _dev(lod), _dev(loc), ["a.png", "b.png"])])
    assert not os.path.exists(tmp_path / "plain" / "morphometry_errors.csv")
    for f in ("per_image.csv", "summary.json"):
        with open(tmp_path / "plain" / f, "rb") as fa, open(tmp_path / "morph" / f, "rb") as fb:
            assert fa.read() == fb.read(), f


# ---- the one copy -------------------------------------------------------------------------------------------------------------------
def test_everything_comes_back_in_one_copy_per_size_group_or_batch(nets, tmp_path, monkeypatch):
    """Every optional output on: Segmenter.back_result copies once per size group, TestRun.batch once per batch."""
    from wtpse_hip.test_run import TestRun
    calls, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **kw: calls.append(tuple(self.shape)) or real(self, *a, **kw))
    rng = np.random.default_rng(2)
    image = _dev(rng.uniform(-1, 1, (3, 3, 256, 256)).astype(np.float32))
    spread = tuple(_dev(rng.uniform(0, 0.5, (3, 1, 256, 256)).astype(np.float32)) for _ in range(2))
    lod, loc = (_dev(a) for a in _pseudo_logits(None))
    seg = _segmenter(str(tmp_path / "seg"), morphometry=True, sectors=24, eye="right")
    res = seg.back_result(image, lod, loc, BACK_SIZES, spread)
    assert len(set(BACK_SIZES)) == 2 and len(calls) == 2, calls
    assert all(x is not None for x in res.overlays + res.spreads + res.morph) and res.spreads[1].shape == (2,) + BACK_SIZES[1]
    B, h, w = 2, 90, 70
    small = make_inputs(61, B, 64, 64)[0].to(DEV)
    lab_od = _dev(np.stack([raster_ellipse(h, w, 44, 36, 30, 26, 0.3), raster_ellipse(h, w, 40, 30, 28, 22, 1.0)])[:, None].astype(np.float32))
    lab_oc = _dev(np.stack([raster_ellipse(h, w, 47, 33, 14, 10, 0.8), raster_ellipse(h, w, 38, 32, 9, 12, 0.0)])[:, None].astype(np.float32))
    run = TestRun(*nets, out_dir=str(tmp_path / "run"), overlay="device", metrics="device", morphometry=True)
    del calls[:]
    m, original, over = run.batch(small, lab_od, lab_oc)
    assert len(calls) == 1, calls
    assert original.shape == over.shape == (B, h, w, 3) and len(m["disc_dice"]) == len(run.morph_pred) == len(run.morph_label) == B
