"""wtpse_hip/segment.py on the device (-m gpu): the LANCZOS front against the live Pillow bit for bit, ops.label_map and
ops.mask_geometry against their host specifications, the ground-truth-free overlay against ops.overlay with an empty ground truth,
Segmenter.back on injected logits against the host post-processing, and the driver end to end: in process against an expectation
assembled from the existing pieces, and through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.filler import fill_state_dict
from oracle.fundus_tree import _sample
from oracle.inputs import make_inputs
from test_segment_cpu import content
from test_test_run_cpu import _disc
from test_test_run_gpu import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wt-pse-code_amd")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _segmenter(out_dir=None, **kw):
    from wtpse_hip.segment import Segmenter
    return Segmenter(None, None, None, None, out_dir=out_dir, **kw)          # front / back never touch the networks


def _host_front(img):
    """FundusTree's resize and FundusTestBatches.host_sample's normalisation: [h,w,3] uint8 -> [3,256,256] fp32."""
    a = np.array(Image.fromarray(img, "RGB").resize((256, 256), Image.LANCZOS)).astype(np.float32)
    a /= 127.5
    a -= 1.0
    return np.ascontiguousarray(a.transpose(2, 0, 1))


# ---- front ------------------------------------------------------------------------------------------------------------------
def test_front_matches_pillow_on_a_batch_of_two():
    imgs = [content(800, 800, "random"), content(800, 800, "smooth")]
    got = _segmenter().front(imgs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 256, 256) and got.is_contiguous()
    want = np.stack([_host_front(im) for im in imgs])
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())


@pytest.mark.parametrize("size", [(613, 517), (256, 256), (100, 120), (257, 255), (300, 256), (1634, 1634)], ids=lambda s: "%dx%d" % s)
def test_front_matches_pillow_at_every_size(size):
    img = content(size[0], size[1], "random")
    got = _segmenter().front([img]).cpu().numpy()
    want = _host_front(img)[None]
    assert np.array_equal(got, want), (size, int((got != want).sum()))


def test_front_keeps_the_order_of_a_mixed_batch():
    sizes = [(100, 120), (300, 256), (100, 120), (257, 255), (300, 256)]
    imgs = [content(h, w, "random" if i % 2 else "smooth") for i, (h, w) in enumerate(sizes)]
    imgs[2] = imgs[2][::-1].copy()                                          # the two 100 x 120 pictures differ
    got = _segmenter().front(imgs).cpu().numpy()
    want = np.stack([_host_front(im) for im in imgs])
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        _segmenter().front([imgs[0].astype(np.float32)])


def test_image_finish_argument_checks():
    from wtpse_hip import ops
    t = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    assert float(ops.image_finish(t).max()) == -1.0
    for bad in (t.cpu(), t.float(), torch.zeros(1, 8, 9, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 8, 8, 1, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            ops.image_finish(bad)


# ---- label map ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 64, 64), (1, 1, 37, 53), (3, 1, 1, 1), (3, 1, 70, 301)], ids=str)
def test_label_map_matches_host(shape):
    from wtpse_hip import ops
    from wtpse_hip.segment import label_map_host
    from wtpse_hip.test_run import label_thresholds_host
    rng = np.random.default_rng(shape[2] * 1000 + shape[3])
    disc = (rng.random(shape) < 0.5).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    cup = (rng.random(shape) < 0.3).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    got = ops.label_map(_dev(disc), _dev(cup))
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy(), label_map_host(disc, cup))
    od, oc = ops.label_thresholds(got)                                      # the read-back rule, on the device too
    assert np.array_equal(oc.cpu().numpy(), (cup != 0).astype(np.float32))
    assert np.array_equal(od.cpu().numpy(), ((disc != 0) | (cup != 0)).astype(np.float32))
    assert np.array_equal(label_thresholds_host(got.cpu().numpy())[1], (cup != 0).astype(np.uint8))
    with pytest.raises(ValueError):
        ops.label_map(_dev(disc), _dev(cup).float())
    with pytest.raises(ValueError):
        ops.label_map(_dev(disc).cpu(), _dev(cup))


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def _geometry_content(h, w, variant):
    """Three masks: `variant` picks which three of empty / full / corner pixels / a roughened disc / two separate blobs."""
    rng = np.random.default_rng(h * 4099 + w)
    empty, full = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    corners = empty.copy()
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 1
    rough = (_disc(h, w, 0.45 * h, 0.55 * w, 0.3 * min(h, w)) & (rng.random((h, w)) < 0.9)).astype(np.uint8) * 7
    blobs = (_disc(h, w, 0.25 * h, 0.2 * w, 0.15 * min(h, w)) | _disc(h, w, 0.8 * h, 0.75 * w, 0.1 * min(h, w))).astype(np.uint8)
    blobs[h // 2, w - 1] = 1
    return np.stack([(empty, rough, corners), (full, blobs, empty), (rough, corners, blobs)][variant])[:, None]


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 53), (64, 64), (70, 301), (513, 70), (1030, 1027)], ids=lambda s: "%dx%d" % s)
def test_mask_geometry_matches_host(size):
    from wtpse_hip import ops
    from wtpse_hip.segment import mask_geometry_host
    for variant in range(3):
        m = _geometry_content(size[0], size[1], variant)
        got = ops.mask_geometry(_dev(m))
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, 8)
        want = mask_geometry_host(m[:, 0])
        assert np.array_equal(got.cpu().numpy(), want), (size, variant, got.cpu().numpy().tolist(), want.tolist())


def test_mask_geometry_sums_beyond_32_bits():
    from wtpse_hip import ops
    n = 2100
    got = ops.mask_geometry(torch.ones(1, 1, n, n, dtype=torch.uint8, device=DEV)).cpu().numpy()[0].tolist()
    s = n * (n * (n - 1) // 2)
    assert s > 2 ** 32 and got == [n * n, 0, n - 1, 0, n - 1, s, s, 0]


def test_mask_geometry_is_repeatable_and_captures_in_a_graph():
    from wtpse_hip import ops
    a, b = _dev(_geometry_content(70, 301, 2)), _dev(_geometry_content(70, 301, 1))
    first = ops.mask_geometry(a).cpu()
    for _ in range(3):
        assert torch.equal(ops.mask_geometry(a).cpu(), first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.mask_geometry(a)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.mask_geometry(a)
    a.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.mask_geometry(b)) and not torch.equal(out.cpu(), first)


def test_mask_geometry_argument_checks():
    from wtpse_hip import ops
    m = torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=DEV)
    assert ops.mask_geometry(m).cpu().numpy().tolist() == [[0, 8, -1, 8, -1, 0, 0, 0]]
    for bad in (m.cpu(), m.float(), torch.zeros(1, 1, 0, 8, dtype=torch.uint8, device=DEV), torch.zeros(1, 1, 8, 0, dtype=torch.uint8, device=DEV),
                torch.zeros(1, 1, 1, 4097, dtype=torch.uint8, device=DEV), torch.zeros(1, 1, 4097, 1, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            ops.mask_geometry(bad)


# ---- overlay without a ground truth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 96, 80), (3, 19, 257), (3, 35, 258), (3, 5, 3), (9, 800, 800)], ids=str)
def test_overlay_without_ground_truth_equals_empty_ground_truth(case):
    from wtpse_hip import ops
    B, h, w = case
    img, pod, poc, _, _ = _batch(h * 1000 + w, B, h, w)
    img, pod, poc = _dev(img), _dev(pod[:, None]), _dev(poc[:, None])
    zero = torch.zeros_like(pod)
    want_o, want_v = ops.overlay(img, pod, poc, zero, zero)
    got_o, got_v = ops.overlay(img, pod, poc, None, None)
    assert got_o.dtype == got_v.dtype == torch.uint8 and tuple(got_o.shape) == tuple(got_v.shape) == (B, h, w, 3)
    assert torch.equal(got_o, want_o) and torch.equal(got_v, want_v)
    assert h < 19 or not torch.equal(got_o, got_v)                          # something was painted
    assert not bool(((got_v == torch.tensor([255, 0, 0], dtype=torch.uint8, device=DEV)).all(3) & (got_o != got_v).any(3)).any())   # never red


def test_overlay_without_ground_truth_argument_checks():
    from wtpse_hip import ops
    img, m = torch.zeros(1, 3, 8, 8, device=DEV), torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=DEV)
    ops.overlay(img, m, m, None, None)
    with pytest.raises(ValueError):
        ops.overlay(img, m, m, m, None)
    with pytest.raises(ValueError):
        ops.overlay(img, m, m.float(), None, None)
    one = torch.zeros(1, 1, 1, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="unsupported size"):
        ops.overlay(torch.zeros(1, 3, 1, 8, device=DEV), one, one, None, None)
    # the C entry with a ground truth keeps rejecting NULL
    L = ops.lib()
    o = torch.empty(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.query("wtpse_overlay_ws", 1, 8, 8), dtype=torch.float32, device=DEV)
    assert L.raw("wtpse_overlay")(img.data_ptr(), m.data_ptr(), m.data_ptr(), None, None, o.data_ptr(), o.data_ptr(), ws.data_ptr(), 1, 8, 8,
                                  ops.stream_ptr()) == -1


# ---- Segmenter.back on injected logits -------------------------------------------------------------------------------------------
BACK_SIZES = [(120, 100), (90, 131), (120, 100)]


def _pseudo_logits(empty_disc=None):
    """+-30 discs and cups at 256 x 256 for the three images; `empty_disc`: that image's disc logit is negative everywhere."""
    lod, loc = np.full((3, 1, 256, 256), -30.0, np.float32), np.full((3, 1, 256, 256), -30.0, np.float32)
    for i, (cy, cx, r) in enumerate(((120, 130, 70), (140, 110, 60), (128, 128, 85))):
        if i != empty_disc:
            lod[i, 0][_disc(256, 256, cy, cx, r) > 0] = 30.0
        loc[i, 0][_disc(256, 256, cy + 5, cx - 4, 0.45 * r) > 0] = 30.0
    return lod, loc


def _back_expectation(image, lod, loc):
    """Per image: the device-resized logits through validate.postprocess on the host -> (disc, cup, resized image)."""
    from wtpse_hip import ops, validate as V
    out = []
    for i, (h, w) in enumerate(BACK_SIZES):
        d = V.postprocess(ops.resize_bilinear(lod[i:i + 1].contiguous(), (h, w))[0])[0]
        c = V.postprocess(ops.resize_bilinear(loc[i:i + 1].contiguous(), (h, w))[0])[0]
        out.append((d, c, ops.resize_bilinear(image[i:i + 1].contiguous(), (h, w))[0].cpu().numpy()))
    return out


def _check_row(got, want):
    from wtpse_hip.segment import FLOAT_COLUMNS, INT_COLUMNS
    for k in INT_COLUMNS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in FLOAT_COLUMNS:
        assert (np.isnan(got[k]) and np.isnan(want[k])) or got[k] == want[k], (k, got[k], want[k])


def test_back_on_injected_logits(tmp_path):
    from wtpse_hip.segment import label_map_host, mask_geometry_host, measure, read_measurements
    from wtpse_hip.test_run import overlay_host
    image = _dev(np.random.default_rng(2).uniform(-1, 1, (3, 3, 256, 256)).astype(np.float32))
    names = ["left eye.png", "b.png", "c.png"]
    for sub, empty_disc in (("all", None), ("one_empty", 1)):
        lod, loc = (_dev(a) for a in _pseudo_logits(empty_disc))
        seg = _segmenter(str(tmp_path / sub))
        labels, overlays, rows = seg.back(image, lod, loc, BACK_SIZES)
        seg.write(names, labels, overlays, rows)
        summary = seg.finish()
        want = _back_expectation(image, lod, loc)
        got_rows, got_summary = read_measurements(str(tmp_path / sub))
        assert got_summary == summary and summary["n"] == 3 and [r["name"] for r in got_rows] == names
        assert [r["index"] for r in got_rows] == [1, 2, 3]
        want_rows = []
        for i, ((d, c, img), (h, w)) in enumerate(zip(want, BACK_SIZES)):
            assert c.any() and (d.any() or i == empty_disc)
            png = Image.open(tmp_path / sub / "mask" / names[i])
            assert png.mode == "L" and png.size == (w, h) and np.array_equal(np.array(png), label_map_host(d, c))
            want_rows.append(measure(mask_geometry_host(d), mask_geometry_host(c), h, w))
            _check_row(got_rows[i], want_rows[-1])
            zero = np.zeros((h, w), np.uint8)
            assert np.array_equal(np.array(Image.open(tmp_path / sub / "overlay" / names[i])), overlay_host(img, d, c, zero, zero)[1])
        defined = [r for i, r in enumerate(want_rows) if i != empty_disc]
        assert summary["n_empty_disc"] == (0 if empty_disc is None else 1) and summary["n_empty_cup"] == 0
        for k in ("vcdr", "hcdr", "acdr"):
            assert all(0.0 < r[k] < 1.0 for r in defined)
            assert summary["mean_" + k] == float(np.mean(np.array([r[k] for r in defined], np.float64)))
            if empty_disc is not None:
                assert np.isnan(got_rows[empty_disc][k])
    # overlay=False: no picture is produced or written
    seg = _segmenter(str(tmp_path / "bare"), overlay=False)
    labels, overlays, rows = seg.back(image, lod, loc, BACK_SIZES)
    seg.write(names, labels, overlays, rows)
    assert overlays == [None] * 3 and not os.path.exists(tmp_path / "bare" / "overlay") and len(os.listdir(tmp_path / "bare" / "mask")) == 3
    with pytest.raises(ValueError):
        seg.back(image, lod, loc, BACK_SIZES[:2])


# ---- the driver end to end -------------------------------------------------------------------------------------------------------
E2E = (("eye_04.png", 300, 280), ("Patient 7 (left).png", 222, 190), ("a.png", 300, 280), ("zz-top.png", 222, 190), ("m.png", 300, 280))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Five crops at two native sizes, alternating, under names that follow no dataset prefix."""
    root = str(tmp_path_factory.mktemp("unlabelled"))
    rs = np.random.RandomState(11)
    for name, w, h in E2E:
        _sample(rs, w, h, rgb_mask=False)[0].save(os.path.join(root, name))
    return root


@pytest.fixture(scope="module")
def nets():
    """Seeded networks one training step away from the filler: BatchNorm's running statistics have moved."""
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


@pytest.fixture(scope="module")
def run(folder, nets, tmp_path_factory):
    from wtpse_hip.segment import Segmenter, read_measurements
    out = str(tmp_path_factory.mktemp("segmented"))
    for n in nets:
        n.train()
    summary = Segmenter(*nets, out_dir=out, batch_size=2).run(folder)
    assert all(n.training for n in nets)                                    # eval for the duration, restored
    rows, read_summary = read_measurements(out)
    assert read_summary == summary
    return out, rows, summary


def test_end_to_end_matches_the_pieces(folder, nets, run):
    from wtpse_hip import ops, validate as V
    from wtpse_hip.segment import ImageFolder, label_map_host, mask_geometry_host, measure
    out, rows, summary = run
    feed = ImageFolder(folder)
    assert [os.path.basename(p) for p in feed.paths] == sorted(n for n, _, _ in E2E) and summary["n"] == 5 and len(rows) == 5
    for n in nets:
        n.eval()
    try:
        for first in range(0, 5, 2):
            idx = list(range(first, min(first + 2, 5)))
            decoded = [np.array(Image.open(feed.paths[i]).convert("RGB")) for i in idx]
            image = _dev(np.stack([_host_front(im) for im in decoded]))
            pred, pred_oc = V.predict_pair(*nets, image)
            groups = {}
            for j, im in enumerate(decoded):
                groups.setdefault(im.shape[:2], []).append(j)
            for (h, w), js in groups.items():
                sel = torch.tensor(js, device=DEV)
                masks = ops.postprocess_masks(torch.cat((ops.resize_bilinear(pred[sel], (h, w)), ops.resize_bilinear(pred_oc[sel], (h, w))), 0))
                masks = masks.cpu().numpy()
                for k, j in enumerate(js):
                    d, c = masks[k, 0], masks[len(js) + k, 0]
                    i = idx[j]
                    assert rows[i]["index"] == i + 1 and rows[i]["name"] == feed.names[i]
                    png = Image.open(os.path.join(out, "mask", feed.names[i]))
                    assert png.mode == "L" and png.size == (w, h) and np.array_equal(np.array(png), label_map_host(d, c)), feed.names[i]
                    _check_row(rows[i], measure(mask_geometry_host(d), mask_geometry_host(c), h, w))
                    over = np.array(Image.open(os.path.join(out, "overlay", feed.names[i])))
                    assert over.shape == (h, w, 3) and not (over == (255, 0, 0)).all(axis=2).any()
    finally:
        for n in nets:
            n.train()
    assert sorted(os.listdir(os.path.join(out, "mask"))) == sorted(feed.names) == sorted(os.listdir(os.path.join(out, "overlay")))


def test_written_masks_read_back_as_labels(folder, run, tmp_path):
    """O/mask as pseudo-labels: copied beside the images under the dataset layout, FundusTree reads them as labels."""
    import shutil
    from wtpse_hip.fundus_data import FundusTree
    out, rows, _ = run
    for sub in ("image", "mask"):
        os.makedirs(tmp_path / "Domain3" / "test" / "ROIs" / sub)
    name = E2E[0][0]
    shutil.copy(os.path.join(folder, name), tmp_path / "Domain3" / "test" / "ROIs" / "image" / "G-1.png")
    shutil.copy(os.path.join(out, "mask", name), tmp_path / "Domain3" / "test" / "ROIs" / "mask" / "G-1.png")
    tree = FundusTree(str(tmp_path), phase="test", splitid=(3,), state="prediction")
    mask = np.array(tree.pools[tree.keys()[0]][1][0])
    row = [r for r in rows if r["name"] == name][0]
    assert mask.shape == (row["height"], row["width"]) and int((mask <= 50).sum()) == row["cup_area"]
    assert set(np.unique(mask)) <= {0, 128, 255}


def test_command_line(folder, nets, run, tmp_path):
    """A checkpoint written by Validator, `python -m wtpse_hip.segment` in a fresh child process: the in-process run's files."""
    from wtpse_hip import validate as V
    from wtpse_hip.segment import read_measurements
    out, rows, summary = run
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    img, od, oc = make_inputs(41, 3, 64, 64)
    val = V.Validator("OD_OC", out_dir=str(ckdir), metrics="device")
    assert val(0, *nets, [(img.to(DEV), od.to(DEV), oc.to(DEV))])[0] == 1
    path = os.path.join(str(ckdir), "checkpoint_1.pth.tar")
    assert os.path.isfile(path)
    out_cli = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "wtpse_hip.segment", "--images", folder, "--checkpoint", path, "--out", out_cli,
           "--batch-size", "2"]
    res = subprocess.run(cmd, cwd=PKG, env=env, capture_output=True, text=True, timeout=660)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    import json
    assert json.loads(res.stdout.strip().splitlines()[-1]) == summary
    rows_c, summary_c = read_measurements(out_cli)
    assert summary_c == summary and len(rows_c) == len(rows) == 5
    for a, b in zip(rows_c, rows):
        assert a["index"] == b["index"] and a["name"] == b["name"]
        _check_row(a, b)
        for sub in ("mask", "overlay"):
            assert np.array_equal(np.array(Image.open(os.path.join(out_cli, sub, a["name"]))), np.array(Image.open(os.path.join(out, sub, a["name"]))))
