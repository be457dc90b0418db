"""wtpse_hip/test_run.py on the device (-m gpu): ops.overlay (csrc/overlay.hip) against its host specification overlay_host byte for
byte — the CPU cases of tests/test_test_run_cpu.py (themselves pinned to the marching-squares oracle there), full-size batches,
widths that are no multiple of 4 or of the tile — repeatability and graph capture, the label thresholds, and the driver end to end:
device against host, the means against validate_epoch, the checkpoint round trip and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.filler import fill_state_dict
from oracle.fundus_tree import _sample
from oracle.inputs import make_inputs
from test_test_run_cpu import CASES, _disc

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wt-pse-code_amd")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(img, pod, poc, god, goc):
    """[B,3,h,w] fp32 and four [B,h,w] uint8 arrays: device == host, both outputs, every byte."""
    from wtpse_hip import ops
    from wtpse_hip.test_run import overlay_host_batch
    ms = [np.ascontiguousarray(m[:, None]) for m in (pod, poc, god, goc)]
    got_o, got_v = ops.overlay(_dev(img), *[_dev(m) for m in ms])
    B, _, h, w = img.shape
    assert got_o.dtype == got_v.dtype == torch.uint8 and tuple(got_o.shape) == tuple(got_v.shape) == (B, h, w, 3)
    want_o, want_v = overlay_host_batch(img, *ms)
    got_o, got_v = got_o.cpu().numpy(), got_v.cpu().numpy()
    assert np.array_equal(got_o, want_o), ("original", img.shape, int((got_o != want_o).any(axis=3).sum()))
    assert np.array_equal(got_v, want_v), ("overlay", img.shape, int((got_v != want_v).any(axis=3).sum()))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_overlay_matches_host_on_the_cpu_cases(case):
    _, img, pod, poc, god, goc = case
    _check(img[None], pod[None], poc[None], god[None], goc[None])


def _batch(seed, B, h, w):
    """Fundus-like: a disc with a cup, both jittered per image and roughened with speckle, against a shifted ground truth; image 0
    has its ground truth on the top-left border, image 1 (when there is one) on the bottom-right border."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1.0, 1.0, (B, 3, h, w)).astype(np.float32)
    pod, poc, god, goc = (np.zeros((B, h, w), np.uint8) for _ in range(4))
    s = min(h, w)
    for i in range(B):
        cy, cx, r = h * rng.uniform(0.4, 0.6), w * rng.uniform(0.4, 0.6), s * rng.uniform(0.2, 0.35)
        pod[i] = _disc(h, w, cy, cx, r) & (rng.random((h, w)) < 0.97)
        poc[i] = _disc(h, w, cy + 2, cx - 3, 0.5 * r) | ((rng.random((h, w)) < 0.001) & (pod[i] > 0))
        gy, gx = (0.1 * s, 0.1 * s) if i == 0 else (h - 0.1 * s, w - 0.1 * s) if i == 1 else (cy + 3, cx + 2)
        god[i] = _disc(h, w, gy, gx, 0.9 * r)
        goc[i] = _disc(h, w, gy, gx, 0.4 * r)
    return img, pod, poc, god, goc


@pytest.mark.parametrize("size", [(512, 512), (800, 800)])
def test_overlay_matches_host_full_size_batches(size):
    _check(*_batch(size[0], 9, *size))


@pytest.mark.parametrize("size", [(19, 255), (19, 257), (35, 258), (17, 259), (70, 301), (33, 1023), (280, 302), (5, 3)])
def test_overlay_matches_host_on_ragged_widths(size):
    """Widths that are no multiple of 4 (byte-wise loads, misaligned output rows) and that end one to three pixels into a tile."""
    assert size[1] % 4
    _check(*_batch(size[0] * 1000 + size[1], 3, *size))


def test_overlay_argument_checks():
    from wtpse_hip import ops
    img, m = torch.zeros(1, 3, 8, 8, device=DEV), torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=DEV)
    ops.overlay(img, m, m, m, m)
    with pytest.raises(ValueError):
        ops.overlay(img.cpu(), m, m, m, m)
    with pytest.raises(ValueError):
        ops.overlay(img, m.float(), m, m, m)
    with pytest.raises(ValueError):
        ops.overlay(img, m, m, m, torch.zeros(1, 1, 8, 9, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.overlay(torch.zeros(1, 1, 8, 8, device=DEV), m, m, m, m)
    one = torch.zeros(1, 1, 1, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="unsupported size"):
        ops.overlay(torch.zeros(1, 3, 1, 8, device=DEV), one, one, one, one)


def test_overlay_is_repeatable_and_captures_in_a_graph():
    from wtpse_hip import ops
    a, b = _batch(5, 3, 96, 80), _batch(6, 3, 96, 80)
    ts = [_dev(a[0])] + [_dev(np.ascontiguousarray(m[:, None])) for m in a[1:]]
    first = [t.cpu() for t in ops.overlay(*ts)]
    for _ in range(3):
        assert all(torch.equal(t.cpu(), f) for t, f in zip(ops.overlay(*ts), first))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.overlay(*ts)                                        # warm the capture stream's workspace
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.overlay(*ts)
    for t, src in zip(ts, [b[0]] + [np.ascontiguousarray(m[:, None]) for m in b[1:]]):
        t.copy_(_dev(src))
    graph.replay()
    torch.cuda.synchronize()
    want = ops.overlay(*ts)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    assert not torch.equal(out[1].cpu(), first[1])


def test_label_thresholds_match_host():
    from wtpse_hip import ops
    from wtpse_hip.test_run import label_thresholds_host
    rng = np.random.default_rng(3)
    for shape in ((2, 1, 64, 64), (1, 1, 37, 53), (3, 1, 1, 1)):
        m = rng.integers(0, 256, shape).astype(np.uint8)
        m.reshape(-1)[:6] = (0, 50, 51, 200, 201, 255)[:m.size]
        od, oc = ops.label_thresholds(_dev(m))
        want_od, want_oc = label_thresholds_host(m)
        assert od.dtype == oc.dtype == torch.float32 and tuple(od.shape) == shape
        assert np.array_equal(od.cpu().numpy(), want_od.astype(np.float32)) and np.array_equal(oc.cpu().numpy(), want_oc.astype(np.float32))


# ---- the driver end to end --------------------------------------------------------------------------------------------------
NAMES = ("G-1-L_test.png", "N-2-R_test.png", "S-3-L_test.png")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Domain3/test with three 300 x 280 crops: one label size, so they batch (oracle/fundus_tree.py's own test split mixes sizes)."""
    root = str(tmp_path_factory.mktemp("fundus_run"))
    rs = np.random.RandomState(8)
    for sub in ("image", "mask"):
        os.makedirs(os.path.join(root, "Domain3", "test", "ROIs", sub))
    for n in NAMES:
        im, mk = _sample(rs, 300, 280, rgb_mask=False)
        im.save(os.path.join(root, "Domain3", "test", "ROIs", "image", n))
        mk.save(os.path.join(root, "Domain3", "test", "ROIs", "mask", n))
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


def _feed(tree, batch_size=2):
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.test_run import FundusTestBatches
    return FundusTestBatches(FundusTree(tree, phase="test", splitid=(3,), state="prediction"), batch_size, DEV)


def _pngs(out_dir, n):
    from PIL import Image
    return [[np.array(Image.open(os.path.join(out_dir, sub, "%d.png" % (i + 1)))) for i in range(n)] for sub in ("original_image", "overlay")]


def _same_rows(a, b, asd_rel=0.0):
    from wtpse_hip import validate as V
    assert [(r["index"], r["name"]) for r in a] == [(r["index"], r["name"]) for r in b]
    for ra, rb in zip(a, b):
        for k in V.METRIC_KEYS:
            if k.endswith("_asd") and asd_rel:
                assert abs(ra[k] - rb[k]) <= asd_rel * max(abs(rb[k]), 1e-300), (k, ra[k], rb[k])
            else:
                assert ra[k] == rb[k], (k, ra[k], rb[k])


@pytest.fixture(scope="module")
def device_run(tree, nets, tmp_path_factory):
    from wtpse_hip.test_run import TestRun, read_table
    out = str(tmp_path_factory.mktemp("run_device"))
    for n in nets:
        n.train()
    means = TestRun(*nets, out_dir=out, overlay="device", metrics="device").run(_feed(tree))
    assert all(n.training for n in nets)                         # eval for the duration, restored
    rows, summary = read_table(out)
    assert summary == means and means["n"] == 3
    return out, rows, means


def test_feed_yields_what_the_reference_loader_does(tree):
    from wtpse_hip.test_run import label_thresholds_host
    feed = _feed(tree)
    got = list(feed)
    assert [len(g[3]) for g in got] == [2, 1] and sorted(sum((g[3] for g in got), [])) == sorted(NAMES)
    for b, (image, od, oc, names) in enumerate(got):
        himg, hmask, hnames = feed.host_batch(b)
        assert names == hnames and image.is_cuda and tuple(image.shape) == (len(names), 3, 256, 256) and tuple(od.shape) == (len(names), 1, 280, 300)
        assert np.array_equal(image.cpu().numpy(), himg)
        want_od, want_oc = label_thresholds_host(hmask)
        assert np.array_equal(od.cpu().numpy(), want_od.astype(np.float32)) and np.array_equal(oc.cpu().numpy(), want_oc.astype(np.float32))
    assert all(len(t) == 3 for t in feed.triples())


def test_device_run_matches_host_run(tree, nets, device_run, tmp_path):
    from wtpse_hip.test_run import TestRun, read_table
    out_d, rows_d, means_d = device_run
    out_h = str(tmp_path)
    means_h = TestRun(*nets, out_dir=out_h, overlay="host", metrics="host").run(_feed(tree))
    rows_h, _ = read_table(out_h)
    _same_rows(rows_d, rows_h, asd_rel=1e-12)
    assert means_d["n"] == means_h["n"]
    for k in ("cup_dice", "disc_dice", "cup_hd", "disc_hd"):
        assert means_d[k] == means_h[k], k
    for k in ("cup_asd", "disc_asd"):
        assert abs(means_d[k] - means_h[k]) <= 1e-12 * max(abs(means_h[k]), 1e-300), k
    for pd_, ph in zip(_pngs(out_d, 3), _pngs(out_h, 3)):
        for a, b in zip(pd_, ph):
            assert a.shape == (280, 300, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    orig, over = _pngs(out_d, 3)
    assert any((o != v).any() for o, v in zip(orig, over))       # something was painted: the ground truth at least
    assert all(((v == (255, 0, 0)).all(axis=2)).any() for v in over)


def test_summary_equals_validate_epoch(tree, nets, device_run):
    from wtpse_hip import validate as V
    _, _, means = device_run
    assert V.validate_epoch(*nets, _feed(tree).triples(), metrics="device") == means
    host = V.validate_epoch(*nets, list(_feed(tree).triples()))
    assert all(host[k] == means[k] for k in ("n", "cup_dice", "disc_dice", "cup_hd", "disc_hd"))


def test_mixed_sides(tree, nets, device_run, tmp_path):
    """overlay and metrics choose their side independently."""
    from wtpse_hip.test_run import TestRun, read_table
    out_d, rows_d, _ = device_run
    out = str(tmp_path)
    TestRun(*nets, out_dir=out, overlay="device", metrics="host").run(_feed(tree, 3))
    _same_rows(read_table(out)[0], rows_d, asd_rel=1e-12)
    for pa, pb in zip(_pngs(out, 3), _pngs(out_d, 3)):
        assert all(np.array_equal(a, b) for a, b in zip(pa, pb))


def test_checkpoint_round_trip_and_command_line(tree, nets, device_run, tmp_path):
    """A checkpoint written by Validator -> load_checkpoint into fresh, differently filled networks -> the same table; and the
    same through `python -m wtpse_hip.test_run` in a fresh child process."""
    from wtpse_hip import validate as V
    from wtpse_hip.test_run import TestRun, build_networks, load_checkpoint, read_table
    out_d, rows_d, means_d = device_run
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    val = V.Validator("OD_OC", out_dir=str(ckdir), metrics="device")
    assert val(0, *nets, list(_feed(tree).triples()))[0] == 1
    path = os.path.join(str(ckdir), "checkpoint_1.pth.tar")
    assert os.path.isfile(path)
    fresh = build_networks(DEV)
    for i, n in enumerate(fresh):
        fill_state_dict(n, 4321 + i)
    load_checkpoint(path, *fresh)
    out = str(tmp_path / "fresh")
    assert TestRun(*fresh, out_dir=out).run(_feed(tree)) == means_d
    _same_rows(read_table(out)[0], rows_d)
    # the command line
    out_cli = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "wtpse_hip.test_run", "--data-dir", tree, "--datasetTest", "3", "--checkpoint", path,
           "--out", out_cli, "--batch-size", "2"]
    res = subprocess.run(cmd, cwd=PKG, env=env, capture_output=True, text=True, timeout=660)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows_c, means_c = read_table(out_cli)
    assert means_c == means_d
    _same_rows(rows_c, rows_d)
    for pa, pb in zip(_pngs(out_cli, 3), _pngs(out_d, 3)):
        assert all(np.array_equal(a, b) for a, b in zip(pa, pb))
