"""The gradability pass on the device (-m gpu): ops.gradability_record against gradability.record_host, entry for entry — small and odd
sizes, workgroup seams, every base alignment and row phase, the thresholds, sums beyond 32 bits, repeatability, stray writes and
the argument checks — and `locate --gradability` / `segment --gradability` end to end against the host composition, to the bit."""
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

from test_locate_cpu import synth_photo
from test_segment_gpu import nets  # noqa: F401  (the seeded networks, a module fixture here too)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _field(N, H, W, seed):
    """Random pictures with a random circular field: noise inside a circle whose centre lies in the middle third of the picture and
    whose radius is 0.3 .. 0.6 of its longer side (so it is cut by the borders), grey levels 0..5 outside it."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = rng.uniform(H / 3.0, 2.0 * H / 3.0), rng.uniform(W / 3.0, 2.0 * W / 3.0)
    inside = np.hypot(yy - cy, xx - cx) < rng.uniform(0.3, 0.6) * max(H, W) + 1.0
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    return np.where(inside[None, :, :, None], img, rng.integers(0, 6, (N, H, W, 1), dtype=np.uint8))


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, [(int(i), int(e), int(got[i, e]), int(want[i, e])) for i, e in bad[:8]])


# ---- the record ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (8, 8), (9, 9), (37, 53), (64, 199)], ids=str)
def test_record_matches_host(size, N):
    from wtpse_hip import gradability as GR, ops
    H, W = size
    img = _field(N, H, W, H * 131 + W + N)
    got = ops.gradability_record(_dev(img), 24, 250)
    assert tuple(got.shape) == (N, GR.GRAD_REC) and got.dtype == torch.int64
    _same(got, GR.record_host(img, 24, 250), size)
    if H > 1:
        one = ops.gradability_record(_dev(img[0]), 24, 250)        # a single [H,W,3] picture: one record
        assert tuple(one.shape) == (1, GR.GRAD_REC) and torch.equal(one[0], got[0])


def test_record_across_workgroup_seams():
    """A tile is 32 rows x 256 pixels and, while a launch has at most 2048 of them, every tile is a workgroup of its own: 599 x 601
    is 19 x 3 of them, the last row 23 rows tall, the last column 89 pixels wide.  The field is a circle of radius 270 about the
    centre: its edge crosses both column seams (x = 256, 512) and every row seam from y = 32 to y = 544, and the halo of 4 reaches
    across each of them.  Then the other path: 1100 pictures leave one workgroup a picture (2048 // 1100), which walks the three
    tiles of a 70 x 20 picture in turn and keeps one record for them."""
    from wtpse_hip import gradability as GR, ops
    H, W = 599, 601
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    inside = np.hypot(yy - 299.0, xx - 300.0) < 270.0
    assert inside[299, 255] and inside[299, 512] and not inside[32, 100] and inside[32, 300] and inside[544, 300] and not inside[544, 100]
    img = np.where(inside[None, :, :, None], rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8), rng.integers(0, 6, (1, H, W, 1), dtype=np.uint8))
    want = GR.record_host(img, 24, 250)
    _same(ops.gradability_record(_dev(img), 24, 250), want, "599 x 601")
    assert 0 < want[0, 267] < want[0, 262] < H * W and want[0, 263:267].tolist() == [30, 568, 31, 569]
    many = _field(1100, 70, 20, 8)
    many[1::2] = np.random.default_rng(9).integers(0, 256, many[1::2].shape, dtype=np.uint8)        # every other one: no two alike
    _same(ops.gradability_record(_dev(many), 24, 250), GR.record_host(many, 24, 250), "1100 x 70 x 20")


def test_record_at_every_base_alignment_and_row_phase():
    """The first byte at every offset 0..15 from a 16-byte boundary (a view into a larger byte buffer), at the widths 16..31: 3 W mod 16
    takes every value 0..15, so every row of every picture starts at its own phase."""
    from wtpse_hip import gradability as GR, ops
    H = 11
    assert sorted(3 * W % 16 for W in range(16, 32)) == list(range(16))
    for W in range(16, 32):
        img = _field(2, H, W, W)
        want = GR.record_host(img, 24, 250)
        for off in range(16):
            flat = torch.zeros(off + img.size, dtype=torch.uint8, device=DEV)
            flat[off:] = _dev(img).reshape(-1)
            view = flat[off:].view(2, H, W, 3)
            assert view.is_contiguous() and view.data_ptr() % 16 == (flat.data_ptr() + off) % 16
            _same(ops.gradability_record(view, 24, 250), want, (W, off))


@pytest.mark.parametrize("sat", [1, 250, 255])
@pytest.mark.parametrize("t", [0, 24, 255])
def test_record_thresholds_on_three_crops(t, sat):
    from wtpse_hip import gradability as GR, ops
    img = _field(3, 32, 32, 17)
    img[2, 5:9, 5:9] = 255                                         # something reaches 255 in every channel
    want = GR.record_host(img, t, sat)
    _same(ops.gradability_record(_dev(img), t, sat), want, (t, sat))
    assert (want[:, 262] == 1024).all() if t == 0 else (want[:, 262] < 1024).all() and want[2, 262] >= 16


def test_sums_beyond_32_bits_are_exact_and_repeatable():
    from wtpse_hip import gradability as GR, ops
    yy, xx = np.mgrid[0:160, 0:160]
    img = np.zeros((1, 160, 160, 3), np.uint8)
    img[..., 0] = 255
    img[0, ..., 1] = np.where((yy + xx) % 2 == 0, 255, 0)
    got = ops.gradability_record(_dev(img), 24, 250).cpu().numpy()
    _same(got, GR.record_host(img, 24, 250), "checkerboard")
    assert got[0, 267:270].tolist() == [158 * 158, 158 * 158 * 1020 ** 2, 0] and got[0, 268] > 2 ** 34         # 2.6e10
    assert got[0, 270:273].tolist() == [156 * 156, 0, 0]           # two steps away the board repeats
    pic = _dev(_field(2, 300, 300, 5))
    first = ops.gradability_record(pic, 24, 250)
    for _ in range(3):
        assert torch.equal(ops.gradability_record(pic, 24, 250), first)


def test_no_stray_write():
    from wtpse_hip import gradability as GR, ops
    from wtpse_hip.lib import lib
    N, H, W, pad = 2, 37, 53, 64
    img = _field(N, H, W, 21)
    for off in (0, 5):
        flat = torch.full((pad + off + img.size + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        flat[pad + off:pad + off + img.size] = _dev(img).reshape(-1)
        before = flat.clone()
        rec = torch.full((8 + N * GR.GRAD_REC + 8,), -559038737, dtype=torch.int64, device=DEV)
        status = lib().call("wtpse_gradability_record", flat.data_ptr() + pad + off, rec.data_ptr() + 64, N, H, W, 24, 250, ops.stream_ptr())
        torch.cuda.synchronize()
        assert not status
        assert torch.equal(flat, before)                           # the picture and the bytes around it
        assert bool((rec[:8] == -559038737).all()) and bool((rec[-8:] == -559038737).all())          # the guard words around rec
        _same(rec[8:-8].reshape(N, GR.GRAD_REC), GR.record_host(img, 24, 250), off)                   # pre-filled: initialised on the stream


def test_argument_checks():
    """Every refused argument returns -1 before any launch; every pointer below is real device memory of the right size (see
    tests/test_trainer_cpu.py::test_loss_log_argument_checks), so a missing check would show as a wrong status or a changed record,
    never as a launch on an address nobody owns."""
    from wtpse_hip import gradability as GR, ops
    from wtpse_hip.lib import lib
    img = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    garbage = torch.full((2 * GR.GRAD_REC + 1,), 12345, dtype=torch.int64, device=DEV)
    raw, st = lib().raw("wtpse_gradability_record"), ops.stream_ptr()
    ip, rp = img.data_ptr(), garbage.data_ptr()
    for N, H, W, t, sat in ((0, 8, 8, 24, 250), (65536, 8, 8, 24, 250), (2, 0, 8, 24, 250), (2, 8, 0, 24, 250), (2, 65537, 8, 24, 250),
                            (2, 8, 65537, 24, 250), (2, 8, 8, -1, 250), (2, 8, 8, 256, 250), (2, 8, 8, 24, 0), (2, 8, 8, 24, 256), (-1, 8, 8, 24, 250)):
        assert raw(ip, rp, N, H, W, t, sat, st) == -1, (N, H, W, t, sat)
    assert raw(0, rp, 2, 8, 8, 24, 250, st) == -1 and raw(ip, 0, 2, 8, 8, 24, 250, st) == -1
    assert raw(ip, rp + 4, 2, 8, 8, 24, 250, st) == -1             # rec must be 8-byte aligned
    torch.cuda.synchronize()
    assert bool((garbage == 12345).all())                          # nothing was launched, nothing was initialised
    # the binding's own checks
    assert ops.gradability_record(img, 0, 1).cpu().numpy()[:, 262].tolist() == [64, 64]
    wide = torch.zeros(2, 8, 8, 6, dtype=torch.uint8, device=DEV)
    for bad, t, sat in ((img.float(), 24, 250), (img, 256, 250), (img, -1, 250), (img, 24, 0), (img, 24, 256), (wide[..., ::2], 24, 250),
                        (img.cpu(), 24, 250), (img[0, 0], 24, 250), (wide[..., :4], 24, 250), (img[None], 24, 250)):
        with pytest.raises(ValueError):
            ops.gradability_record(bad, t, sat)
    with pytest.raises(ValueError):
        ops.gradability_record(np.zeros((1, 8, 8, 3), np.uint8))


# ---- the programs end to end ------------------------------------------------------------------------------------------------------
def _equal(a, b):
    return a == b or (a != a and b != b)


def _host_measures(judge, img, t, c):
    from wtpse_hip import gradability as GR
    from wtpse_hip.locate import cells_host
    return judge.measures(GR.record_host(img, t, judge.sat)[0], cells_host(img, c, t), c)


@pytest.fixture(scope="module")
def located(nets, tmp_path_factory):  # noqa: F811
    """Two 600 x 800 photographs, the second blurred before it was saved, located and segmented without and with the switch.  The
    threshold of the second run is the midpoint of the two focus ratios as the HOST forms them from the decoded files."""
    from wtpse_hip import gradability as GR, locate as L
    root = str(tmp_path_factory.mktemp("photographs"))
    Image.fromarray(synth_photo(600, 800, 1, (0.5, 0.72))[0]).save(os.path.join(root, "sharp.png"))
    Image.fromarray(synth_photo(600, 800, 7, (0.5, 0.72))[0]).filter(ImageFilter.GaussianBlur(2)).save(os.path.join(root, "blurred.png"))
    plain, out = str(tmp_path_factory.mktemp("plain")), str(tmp_path_factory.mktemp("graded"))
    L.WholeImageSegmenter(*nets, out_dir=plain, candidates=2, refine=1, batch_size=2).run(root)
    cell = {r["name"]: r["cell"] for r in L.read_roi_csv(plain)}
    files = {n: np.array(Image.open(os.path.join(root, n)).convert("RGB")) for n in ("blurred.png", "sharp.png")}
    host = {n: _host_measures(GR.Gradability(), im, 24, cell[n]) for n, im in files.items()}
    middle = (host["sharp.png"]["focus_ratio"] + host["blurred.png"]["focus_ratio"]) / 2.0
    judge = GR.Gradability(min_focus_ratio=middle)
    run = L.WholeImageSegmenter(*nets, out_dir=out, candidates=2, refine=1, batch_size=2, gradability=judge)
    summary = run.run(root)
    return root, plain, out, host, judge, summary


def test_locate_writes_the_table_and_changes_nothing_else(located):
    from wtpse_hip import gradability as GR, locate as L, tables as T
    root, plain, out, host, judge, summary = located
    rows = GR.read_csv(out)
    assert [r["name"] for r in rows] == ["blurred.png", "sharp.png"] and [r["index"] for r in rows] == [1, 2]
    assert tuple(rows[0]) == GR.columns(("photo_", "roi_")) and not os.path.exists(os.path.join(plain, "gradability.csv"))
    roi = L.read_roi_csv(out)
    for r, q in zip(rows, roi):
        assert q["located"] == 1 and q["name"] == r["name"]
        for k in GR.MEASURES:
            assert _equal(r["photo_" + k], host[r["name"]][k]), (r["name"], k, r["photo_" + k], host[r["name"]][k])
        crop = np.array(Image.open(os.path.join(out, "crop", r["name"])))
        want = _host_measures(judge, crop, 0, GR.crop_cell(*crop.shape[:2]))
        for k in GR.MEASURES:
            assert _equal(r["roi_" + k], want[k]), (r["name"], "roi", k, r["roi_" + k], want[k])
        assert r["roi_fov_area"] == q["roi_side"] ** 2 and r["photo_fov_area"] == q["fov_area"]
        assert r["photo_evenness_cv"] == r["photo_evenness_cv"] and r["roi_evenness_cv"] == r["roi_evenness_cv"]      # the tables had cells
    blurred, sharp = rows
    assert blurred["photo_focus_ratio"] < judge.min_focus_ratio < sharp["photo_focus_ratio"]
    assert (blurred["focus_rank"], sharp["focus_rank"]) == (25.0, 75.0)
    assert (blurred["ok_focus_ratio"], blurred["gradable"], sharp["ok_focus_ratio"], sharp["gradable"]) == (0, 0, 1, 1)
    assert all(r[f] == -1 for r in rows for f in GR.FLAGS if f not in ("ok_focus_ratio", "gradable"))
    assert summary["gradability"] == dict(judge.config(), n_judged=2, n_gradable=1) and T.read_json(os.path.join(out, "summary.json")) == summary
    # everything else is what a run without the switch writes
    for sub in ("crop", "mask", "full_mask"):
        assert sorted(os.listdir(os.path.join(out, sub))) == sorted(os.listdir(os.path.join(plain, sub))) == ["blurred.png", "sharp.png"]
    for f in ["roi.csv", "measurements.csv"] + [os.path.join(sub, n) for sub in ("crop", "mask", "full_mask") for n in ("blurred.png", "sharp.png")]:
        with open(os.path.join(plain, f), "rb") as fa, open(os.path.join(out, f), "rb") as fb:
            assert fa.read() == fb.read(), f
    there = T.read_json(os.path.join(plain, "summary.json"))
    assert {k: v for k, v in summary.items() if k != "gradability"} == there


def test_segment_on_the_crops_writes_the_roi_values(located, nets, tmp_path):  # noqa: F811
    from wtpse_hip import gradability as GR
    from wtpse_hip.segment import Segmenter
    _, plain, out, _, judge, _ = located
    crops = os.path.join(out, "crop")
    summary = Segmenter(*nets, out_dir=str(tmp_path / "on"), batch_size=2, gradability=GR.Gradability(max_dark=0.9)).run(crops)
    rows, want = GR.read_csv(str(tmp_path / "on")), GR.read_csv(out)
    assert tuple(rows[0]) == GR.columns() and [r["name"] for r in rows] == [r["name"] for r in want]
    for r, w in zip(rows, want):
        for k in GR.MEASURES:
            assert _equal(r[k], w["roi_" + k]), (r["name"], k)
        assert (r["ok_dark"], r["gradable"], r["ok_focus_ratio"]) == (1, 1, -1)
    assert sorted(r["focus_rank"] for r in rows) == [25.0, 75.0]
    assert summary["gradability"]["n_judged"] == 2 and summary["gradability"]["max_dark"] == 0.9
    # off: no table, the other files the same
    Segmenter(*nets, out_dir=str(tmp_path / "off"), batch_size=2).run(crops)
    assert not os.path.exists(tmp_path / "off" / "gradability.csv")
    for f in ["measurements.csv"] + [os.path.join("mask", n) for n in ("blurred.png", "sharp.png")]:
        with open(tmp_path / "off" / f, "rb") as fa, open(tmp_path / "on" / f, "rb") as fb:
            assert fa.read() == fb.read(), f
