"""SURVEY.md §8f row 2, the back half (-m gpu): validation post-processing, Dice and ASD / HD95 on the device
(csrc/postprocess.hip; ops.postprocess_masks / ops.seg_metrics; validate.device_metrics and metrics="device") against the host
path (validate.postprocess / dice / hd95 / asd on scipy), the flood-fill oracle (oracle/postprocess_cpu.py) and the brute-force
surface-distance oracle (oracle/metrics_cpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import metrics_cpu as M
from oracle import postprocess_cpu as P
from oracle.inputs import make_inputs
from test_postprocess_cpu import _masks
from test_validate_cpu import CASES, _disc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _logits(masks):
    """uint8 masks [h,w] of one size -> [B,1,h,w] device logits of +-4."""
    m = torch.from_numpy(np.stack(masks).astype(np.float32))[:, None]
    return (m * 8.0 - 4.0).to(DEV)


def _spiral(n):
    """A one-pixel-wide square spiral from the top-left corner inwards: one component spanning every tile."""
    m = np.zeros((n, n), np.uint8)
    y = x = k = 0
    d = ((0, 1), (1, 0), (0, -1), (-1, 0))
    m[0, 0] = 1
    while True:
        for _ in range(2):
            dy, dx = d[k]
            ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= my < n and 0 <= mx < n and m[my, mx]):
                y, x = ny, nx
                m[y, x] = 1
                break
            k = (k + 1) % 4
        else:
            return m


def _disc_with_holes(n):
    m = _disc(n, n, n // 2, n // 2 + 3, n // 3)
    c = n // 2
    m[c - 20:c - 10, c - 20:c - 10] = 0                        # a square hole
    m[c + 5:c + 25, c + 5:c + 25] = 0                          # a hole with an island (a separate, smaller component)
    m[c + 12:c + 18, c + 12:c + 18] = 1
    m[c, : c // 2] = 0                                          # a slit to the border: not a hole
    m[:6, :6] = 1                                               # a far corner blob
    return m


def _extra_masks():
    rng = np.random.default_rng(23)
    out = [(rng.random((256, 256)) < p).astype(np.uint8) for p in (0.3, 0.41, 0.6)]
    sp = _spiral(256)
    out += [sp, 1 - sp, _disc_with_holes(512), _disc_with_holes(800)]
    out += [(rng.random(s) < 0.5).astype(np.uint8) for s in ((1, 300), (300, 1), (17, 130))]
    return out


def _check_postprocess(masks, oracle=True):
    from wtpse_hip import ops, validate as V
    x = _logits(masks)
    got = ops.postprocess_masks(x)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(x.shape)
    got = got.cpu().numpy()
    for i, m in enumerate(masks):
        host = V.postprocess(x[i])
        assert np.array_equal(got[i], host), ("host", i, m.shape, int((got[i] != host).sum()))
        if oracle:
            want = P.get_largest_fillhole(m).astype(np.uint8)
            assert np.array_equal(got[i, 0], want), ("oracle", i, m.shape)


def test_postprocess_matches_oracle_on_the_cpu_cases():
    for m in _masks():
        _check_postprocess([m])


def test_postprocess_matches_oracle_large_and_odd_shapes():
    for m in _extra_masks():
        _check_postprocess([m], oracle=m.size <= 300 * 300)
    # several images per launch, of one size: no image sees another's labels
    rng = np.random.default_rng(4)
    batch = [(rng.random((40, 70)) < p).astype(np.uint8) for p in (0.0, 0.35, 0.42, 0.5, 0.65, 1.0)]
    _check_postprocess(batch)


def test_threshold_matches_torch_sigmoid():
    """Every fp32 within 4096 ulp of ln 3 (sigmoid = 0.75): one 1x1 image each, so the decision is the threshold alone."""
    from wtpse_hip import ops
    c = np.array(np.log(3.0), np.float32).view(np.int32)
    x = torch.from_numpy(np.arange(int(c) - 4096, int(c) + 4097, dtype=np.int32).view(np.float32).copy()).to(DEV)
    got = ops.postprocess_masks(x.reshape(-1, 1, 1, 1).contiguous()).reshape(-1).cpu()
    want = (torch.sigmoid(x) > 0.75).cpu()
    assert torch.equal(got.bool(), want), int((got.bool() != want).sum())
    assert want.any() and not want.all()


def _records(pairs):
    """(mask, label) pairs of one size -> host records."""
    from wtpse_hip import ops
    m = torch.from_numpy(np.stack([a for a, _ in pairs]).astype(np.uint8))[:, None].to(DEV)
    lab = torch.from_numpy(np.stack([b for _, b in pairs]).astype(np.float32))[:, None].to(DEV)
    return ops.seg_metrics(m.contiguous(), lab.contiguous()).cpu().numpy()


def _check_metrics(pairs, brute=False):
    from wtpse_hip import validate as V
    rec = _records(pairs)
    for r, (a, b) in zip(rec, pairs):
        assert V._finish_dice(r) == V.dice(a, b)
        if not a.any():
            assert V._finish_surface(r) == (100.0, 100.0) == V.surface_metrics(a, b)
            continue
        if not b.any():
            with pytest.raises(RuntimeError):
                V.surface_metrics(a, b)
            with pytest.raises(RuntimeError):
                V._finish_surface(r)
            continue
        hd, asd = V._finish_surface(r)
        assert hd == V.hd95(a, b), (hd, V.hd95(a, b))
        ref = V.asd(a, b)
        assert abs(asd - ref) <= 1e-12 * max(abs(ref), 1e-300), (asd, ref)
        if brute:
            assert abs(hd - M.hd95(a.tolist(), b.tolist())) < 1e-12
            assert abs(asd - M.asd(a.tolist(), b.tolist())) < 1e-12


def test_metrics_match_host_on_the_cpu_cases():
    for a, b in CASES:
        _check_metrics([(a, b), (b, a), (a, a)], brute=True)


def test_metrics_match_host_on_random_and_postprocessed_masks():
    from wtpse_hip import ops
    rng = np.random.default_rng(9)
    for p in (0.3, 0.41, 0.6):
        a = (rng.random((256, 256)) < p).astype(np.uint8)
        b = (rng.random((256, 256)) < 0.5).astype(np.uint8)
        _check_metrics([(a, b)])
    small = [((rng.random((12, 14)) > 0.6).astype(np.uint8), (rng.random((12, 14)) > 0.5).astype(np.uint8)) for _ in range(8)]
    _check_metrics(small, brute=True)
    # post-processed predictions against disc labels, several sizes
    for h, w in ((256, 256), (80, 72), (1, 300), (17, 130)):
        g = torch.Generator().manual_seed(h * 1000 + w)
        x = torch.randn(4, 1, h, w, generator=g) * 2.0
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        x += 6.0 * (((yy - h / 2) ** 2 + (xx - w / 2) ** 2) < (min(h, w) / 3) ** 2).float() - 3.0
        post = ops.postprocess_masks(x.to(DEV)).cpu().numpy()[:, 0]
        labels = [_disc(h, w, h // 2 + k, w // 2 - k, max(1, min(h, w) // 3)) for k in range(4)]
        _check_metrics(list(zip(post, labels)))


def test_metrics_conventions():
    z, d = np.zeros((8, 8), np.uint8), _disc(8, 8, 4, 4, 2)
    _check_metrics([(z, d), (d, z), (z, z), (d, d)])


def _nets_and_batches(label_size, seed):
    from test_parity_gpu import build_nets
    img, od, oc = make_inputs(seed, 4, 64, 64)
    lod = (F.interpolate(od, size=label_size) > 0.5).float().to(DEV)
    loc = (F.interpolate(oc, size=label_size) > 0.5).float().to(DEV)
    return build_nets(1), [(img.to(DEV), lod, loc)]


def _same_means(h, d):
    assert set(h) == set(d) and h["n"] == d["n"]
    for k in ("cup_dice", "disc_dice", "cup_hd", "disc_hd"):
        assert h[k] == d[k], (k, h[k], d[k])
    for k in ("cup_asd", "disc_asd"):
        assert abs(h[k] - d[k]) <= 1e-12 * max(abs(h[k]), 1e-300), (k, h[k], d[k])


@pytest.mark.parametrize("label_size", [(80, 72), (64, 64)])
def test_validate_device_matches_host_end_to_end(label_size):
    from wtpse_hip import validate as V
    nets, batches = _nets_and_batches(label_size, 31)
    for n in nets:
        n.train()
    _same_means(V.validate_epoch(*nets, batches), V.validate_epoch(*nets, batches, metrics="device"))
    assert V.validate(*nets, batches) == V.validate(*nets, batches, metrics="device")
    assert all(n.training for n in nets)
    host, dev = V.Validator("OD_OC"), V.Validator("OD_OC", metrics="device")
    for epoch in range(2):
        rh, rd = host(epoch, *nets, batches), dev(epoch, *nets, batches)
        assert rh[0] == rd[0] and (rh[1], rh[2], rh[4], rh[5]) == (rd[1], rd[2], rd[4], rd[5])
        for k in (3, 6):
            assert abs(rh[k] - rd[k]) <= 1e-12 * max(abs(rh[k]), 1e-300)
        assert (host.best_epoch, host.best_mean_dice) == (dev.best_epoch, dev.best_mean_dice)
        _same_means(host.last, dev.last)
    assert set(host.checkpoint) == set(dev.checkpoint)


def test_device_metrics_refuses_host_tensors():
    from wtpse_hip import validate as V
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="device tensors"):
        V.device_metrics(x.to(DEV), x.to(DEV), x, x)


def _inputs(seed, B=3, h=96, w=80):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, h, w, generator=g) * 2.0
    x[:, :, h // 4: 3 * h // 4, w // 4: 3 * w // 4] += 3.0
    lab = torch.zeros(B, 1, h, w)
    lab[:, :, h // 5: 4 * h // 5, w // 3: 5 * w // 6] = 1.0
    return x.to(DEV), lab.to(DEV)


def test_records_are_repeatable_and_capture_in_a_graph():
    from wtpse_hip import ops
    x, lab = _inputs(1)
    run = lambda: ops.seg_metrics(ops.postprocess_masks(x), lab)
    first = run().cpu()
    for _ in range(3):
        assert torch.equal(run().cpu(), first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                   # warm the capture stream's workspaces
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        masks = ops.postprocess_masks(x)
        rec = ops.seg_metrics(masks, lab)
    x2, lab2 = _inputs(2)
    x.copy_(x2)
    lab.copy_(lab2)
    graph.replay()
    torch.cuda.synchronize()
    want_masks = ops.postprocess_masks(x2)
    assert torch.equal(masks, want_masks)
    assert torch.equal(rec.cpu(), ops.seg_metrics(want_masks, lab2).cpu())
    assert not torch.equal(rec.cpu(), first)
