"""wtpse_hip/tent.py on the host: the float64 specification of the entropy objective against torch float64 autograd of the literal
-s ln s - (1 - s) ln(1 - s) on masked means, its rule cases, the argument checks of TentStep and ops.entropy_loss, the checkpoint dict,
the two tables' round trip, the parser's defaults and the C-ABI surface.  Nothing here needs a GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

INF = float("inf")


def _case(seed, shape, scale, masked):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale
    m = (torch.rand(shape, generator=g) < 0.6).double() if masked else None
    return x, m


def _literal(x, m, margin, reweight):
    """The definition, literally, in torch float64 with autograd -> (H [B], loss, dloss/dx)."""
    x = x.clone().requires_grad_(True)
    B = x.shape[0]
    mm = torch.ones_like(x) if m is None else m
    s = torch.sigmoid(x * mm)
    h = -(s * torch.log(s) + (1 - s) * torch.log(1 - s))
    H = (mm * h).reshape(B, -1).sum(1) / mm.reshape(B, -1).sum(1)
    sel = (H < margin).double()
    w = torch.exp(margin - H).detach() if (reweight and math.isfinite(margin)) else torch.ones_like(H)
    loss = (sel * w * H).sum() / B
    loss.backward()
    return H.detach().numpy(), float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize("masked", [False, True], ids=["disc", "cup"])
@pytest.mark.parametrize("scale", [1.0, 8.0, 30.0])
@pytest.mark.parametrize("margin,reweight", [(INF, False), (0.45, False), (0.45, True)])
def test_host_formulas_against_the_literal_definition(scale, masked, margin, reweight):
    """|x| <= 30 (beyond it 1 - s rounds to 0 in float64 and the literal form is inf * 0): values within 1e-12 — the stable form
    differs from the literal one by 3e-15 on that range — gradients within 1e-9 relative (to the plane's largest)."""
    from wtpse_hip import tent
    x, m = _case(int(scale) + 7 * masked, (4, 1, 9, 13), scale, masked)
    x[1] *= 0.05                                     # one plane near z = 0: entropy near ln 2, above a margin of 0.45
    H_lit, loss_lit, g_lit = _literal(x, m, margin, reweight)
    xn, mn = x.numpy(), None if m is None else m.numpy()
    H, sel, w = tent.entropy_planes_host(xn, mn, margin, reweight)
    assert np.abs(H - H_lit).max() <= 1e-12
    assert list(sel) == [bool(h < margin) for h in H_lit]
    assert not sel[1] or margin == INF
    assert abs(tent.tent_loss_host(xn, mn, margin, reweight) - loss_lit) <= 1e-12
    g = tent.tent_grad_host(xn, mn, margin, reweight)
    assert g.shape == g_lit.shape
    for b in range(x.shape[0]):
        assert np.abs(g[b] - g_lit[b]).max() <= 1e-9 * max(np.abs(g_lit[b]).max(), 1e-300), b
        if not sel[b]:
            assert not g[b].any() and not np.signbit(g[b]).any()
    if m is not None:
        assert not g[mn == 0].any()
    # the fp32 restatement is the same function up to fp32 rounding
    H32, loss32, g32 = tent.entropy_fp32(xn, mn, margin, reweight)
    assert H32.dtype == np.float32 and g32.dtype == np.float32 and g32.shape == g.shape
    assert np.abs(H32 - H).max() <= 1e-5 and abs(float(loss32) - loss_lit) <= 1e-5
    assert np.abs(g32 - g).max() <= 1e-5 * np.abs(g).max() + 1e-12


def test_pixel_entropy_is_symmetric_bounded_and_stable():
    from wtpse_hip import tent
    z = np.array([0.0, 1.0, -1.0, 40.0, -40.0, 80.0, -80.0, 745.0, 1e4])
    h = tent.entropy_pixels_host(z)
    assert h[0] == math.log(2.0) and h[1] == h[2] and h[3] == h[4] and h[5] == h[6]
    assert (h >= 0).all() and (h <= math.log(2.0)).all() and np.isfinite(h).all() and h[-1] == 0.0
    assert h[5] > 0.0                                  # e = exp(-80) = 1.8e-35: finite in float64, the term |z| e survives
    assert tent.EATA_MARGIN == 0.4 * math.log(2.0)


def test_rule_cases_of_the_planes():
    from wtpse_hip import tent
    g = np.random.RandomState(3)
    x = g.randn(5, 1, 6, 7) * np.array([1.0, 8.0, 8.0, 2.0, 8.0]).reshape(5, 1, 1, 1)
    m = np.ones_like(x)
    m[2] = 0.0                                         # M_b = 0
    x[4, 0, 3, 3] = np.nan                             # a NaN plane
    H, sel, w = tent.entropy_planes_host(x, m, INF)
    assert H[2] == 0.0 and not sel[2]                  # never selected, whatever the margin
    assert math.isnan(H[4]) and not sel[4]             # fails `<`, also against +inf
    assert list(sel) == [True, True, False, True, False] and list(w) == [1.0] * 5
    # margin = inf is plain TENT: the loss is the mean over ALL planes of the selected entropies
    assert tent.tent_loss_host(x, m, INF) == math.fsum(H[[0, 1, 3]]) / 5
    gr = tent.tent_grad_host(x, m, INF)
    assert not gr[2].any() and not gr[4].any() and not np.isnan(gr).any() and gr[0].any()
    # a finite margin filters, reweight scales by exp(margin - H_b), a constant of the gradient
    mg = tent.EATA_MARGIN
    H2, sel2, w2 = tent.entropy_planes_host(x, m, mg, reweight=True)
    assert list(sel2) == [False, True, False, False, False] and H2[0] > mg > H2[1]
    assert w2[1] == np.exp(mg - H2[1]) and w2[1] > 1.0
    plain, weighted = tent.tent_grad_host(x, m, mg), tent.tent_grad_host(x, m, mg, reweight=True)
    assert np.allclose(weighted[1], w2[1] * plain[1], rtol=1e-15, atol=0) and not weighted[0].any()
    assert list(tent.entropy_planes_host(x, m, INF, reweight=True)[2]) == [1.0] * 5           # no weight without a finite margin
    # a plane's numbers do not depend on its neighbours (the mean runs over all B planes)
    alone = tent.tent_grad_host(x[1:2], m[1:2], mg)
    assert np.array_equal(alone[0] / 5, plain[1]) or np.allclose(alone[0] / 5, plain[1], rtol=4e-16, atol=0)
    # masked pixels add nothing: the masked mean equals the mean over the kept pixels alone
    keep = g.rand(6, 7) < 0.5
    mk = np.ones_like(x)
    mk[0, 0] = keep
    Hk = tent.entropy_planes_host(x, mk, INF)[0][0]
    assert abs(Hk - tent.entropy_pixels_host(x[0, 0][keep]).mean()) <= 1e-14
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="margin"):
            tent.entropy_planes_host(x, m, bad)
    with pytest.raises(ValueError):
        tent.entropy_planes_host(x, m[:2])
    with pytest.raises(ValueError):
        tent.entropy_planes_host(np.zeros(4))


def test_tent_step_and_entropy_loss_refuse_bad_arguments():
    from wtpse_hip import ops, tent
    ok = tent.check_arguments()
    assert ok == dict(lr=1e-3, betas=[0.9, 0.999], steps=1, margin=INF, reweight=False, stats="batch", eps=1e-8)
    for kw, word in ((dict(lr=0.0), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr="fast"), "lr"), (dict(betas=(0.9,)), "betas"),
                     (dict(betas=(0.9, 1.0)), "betas"), (dict(betas=(-0.1, 0.9)), "betas"), (dict(steps=-1), "steps"),
                     (dict(steps=1.5), "steps"), (dict(steps=True), "steps"), (dict(margin=0.0), "margin"),
                     (dict(margin=float("nan")), "margin"), (dict(stats="site"), "stats"), (dict(eps=0.0), "eps")):
        with pytest.raises(ValueError, match=word):
            tent.TentStep(None, None, None, None, **kw)
    with pytest.raises(ValueError, match="four networks"):
        tent.TentStep(None, None, None, None)
    # the networks live in device memory only: a host network is refused before anything is launched
    import algorithms
    import shape_networks
    from wtpse_hip.synth import default_hparams
    hp = default_hparams(True)
    seg = [algorithms.WT_PSE(3, 1, hp, "cpu", ts, per_domain_batch=1) for ts in (False, True)]
    shp = [shape_networks.ShapeVariationalDist_x(hp, "cpu", 1, 3, 1) for _ in range(2)]
    with pytest.raises(RuntimeError, match="device"):
        tent.TentStep(seg[0], shp[0], seg[1], shp[1])
    with pytest.raises(ValueError, match="WT_PSE"):
        tent.TentStep(shp[0], shp[0], seg[1], shp[1])
    # the BatchNorm modules a step moves: inc and the U-Net body, nothing of the teacher
    names = [n for n, _ in tent.affine_modules(seg[0])]
    assert len(names) == 3 + 4 * 3 + 2 + 3 * 3 and names[0] == "inc.bn1" and "up1.bn2" in names and "up1.bn1" not in names
    assert not any(n.startswith(("prior_dist", "wt_model")) for n in names)
    assert sum(1 for n, _ in seg[0].named_modules() if n.startswith("prior_dist") and n.endswith(("bn1", "bn2", "bn3", ".1", ".4"))) > 0
    # ops.entropy_loss: the checks come before the library is asked for anything
    x = torch.zeros(2, 1, 4, 4)
    with pytest.raises(ValueError, match="device memory"):
        ops.entropy_loss(x)
    with pytest.raises(ValueError):
        ops.adam_index(x, x, x, x, torch.zeros(3, dtype=torch.int32), x, 0.9, 0.999, 1e-8, 1)


def test_c_abi_of_the_two_entries():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    protos = build.parse_prototypes()
    assert protos["wtpse_entropy_loss"] == ["const float*", "const float*", "int", "int", "double", "int", "void*", "float*", "int*",
                                            "float*", "float*", "void*"]
    assert protos["wtpse_entropy_loss_ws"] == ["int", "int"]
    assert protos["wtpse_adam_index"] == ["float*", "const float*", "float*", "float*", "const int*", "int", "const float*", "double",
                                          "double", "double", "int", "const int*", "const int*", "void*"]
    L = lib()
    # the workspace: fp64 partials [B][blocks][2] + fp64 terms [B] + 8 B bytes; the block count depends on hw alone
    assert L.query("wtpse_entropy_loss_ws", 3, 33 * 65) == 3 * 1 * 16 + 3 * 16
    assert L.query("wtpse_entropy_loss_ws", 3, 96 * 96) == 3 * 3 * 16 + 3 * 16
    assert L.query("wtpse_entropy_loss_ws", 1, 96 * 96) - 16 == (L.query("wtpse_entropy_loss_ws", 7, 96 * 96) - 7 * 16) // 7
    assert L.query("wtpse_entropy_loss_ws", 2, 512 * 512) == 2 * 32 * 16 + 2 * 16
    for B, hw in ((0, 16), (65536, 16), (1, 0), (2, 1 << 30), (1, (1 << 30) + 1)):
        assert L.query("wtpse_entropy_loss_ws", B, hw) == -1, (B, hw)
    # refused before any launch: no logits, no workspace, a margin that is not a positive number, no index list, step 0.  The
    # pointers are placeholders that nothing dereferences; a validator that wrongly accepted one must never reach a device, so
    # this part runs on a host without a GPU only (as tests/test_conv_args_cpu.py)
    if torch.cuda.is_available():
        return
    raw = L.raw("wtpse_entropy_loss")
    assert raw(0, 0, 2, 16, INF, 0, 64, 0, 0, 64, 0, 0) == -1
    assert raw(64, 0, 2, 16, INF, 0, 0, 0, 0, 64, 0, 0) == -1
    assert raw(64, 0, 2, 16, 0.0, 0, 64, 0, 0, 64, 0, 0) == -1
    assert raw(64, 0, 2, 16, float("nan"), 0, 64, 0, 0, 64, 0, 0) == -1
    assert raw(64, 0, 2, 16, INF, 0, 68, 0, 0, 64, 0, 0) == -1             # workspace not 8-byte aligned
    raw = L.raw("wtpse_adam_index")
    assert raw(64, 64, 64, 64, 0, 4, 64, 0.9, 0.999, 1e-8, 1, 0, 0, 0) == -1
    assert raw(64, 64, 64, 64, 64, 0, 64, 0.9, 0.999, 1e-8, 1, 0, 0, 0) == -1
    assert raw(64, 64, 64, 64, 64, 4, 0, 0.9, 0.999, 1e-8, 1, 0, 0, 0) == -1
    assert raw(64, 64, 64, 64, 64, 4, 64, 0.9, 0.999, 1e-8, 0, 0, 0, 0) == -1


def test_checkpoint_dict():
    from wtpse_hip import tent
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    sds = [{"a.weight": torch.full((3,), float(i)), "a.running_mean": torch.zeros(3), "n": torch.tensor(i)} for i in range(4)]
    info = dict(tent.check_arguments(margin=0.3), images=5, source="checkpoint_1.pth.tar")
    ck = tent.tent_checkpoint(sds, info, clahe={"clip": 2.0})
    assert list(ck) == list(CHECKPOINT_KEYS) + ["tent", "clahe"] and ck["tent"] == info and ck["clahe"] == {"clip": 2.0}
    for key, sd in zip(CHECKPOINT_KEYS, sds):
        assert list(ck[key]) == list(sd)
        for k, v in sd.items():
            assert torch.equal(ck[key][k], v) and ck[key][k].data_ptr() != v.data_ptr()          # cloned, bit for bit
    assert "clahe" not in tent.tent_checkpoint(sds, info)
    with pytest.raises(ValueError):
        tent.tent_checkpoint(sds[:3], info)


def test_tables_round_trip(tmp_path):
    from wtpse_hip import tent
    from wtpse_hip.test_run import CHECKPOINT_KEYS
    rows = [dict(epoch=0, step=0, images=2, ent_od=0.1234567891234, sel_od=2, ent_oc=float("nan"), sel_oc=0),
            dict(epoch=1, step=1, images=1, ent_od=1e-30, sel_od=1, ent_oc=0.69, sel_oc=1)]
    mk = lambda w, b: {"inc.bn1.weight": torch.tensor(w), "inc.bn1.bias": torch.tensor(b), "inc.bn1.running_mean": torch.zeros(2),
                       "inc.conv1.weight": torch.ones(2)}
    source = {k: mk([1.0, 1.0], [0.0, 0.0]) for k in CHECKPOINT_KEYS}
    final = {k: mk([1.5, 0.75], [0.0, -0.125]) for k in CHECKPOINT_KEYS}
    drift = tent.drift_rows(source, final)
    assert [(r["network"], r["name"]) for r in drift] == [("model", "inc.bn1"), ("model_oc", "inc.bn1")]
    assert drift[0] == dict(network="model", name="inc.bn1", channels=2, gamma_max=0.5, gamma_mean=0.375, beta_max=0.125, beta_mean=0.0625)
    assert all(not any(r[k] for k in tent.DRIFT_COLUMNS[3:]) for r in tent.drift_rows(source, source))
    tent.write_tables(str(tmp_path), rows, drift)
    back_rows, back_drift = tent.read_tables(str(tmp_path))
    assert back_drift == drift and list(back_rows[0]) == list(tent.TENT_COLUMNS)
    assert back_rows[1] == rows[1] and math.isnan(back_rows[0]["ent_oc"]) and back_rows[0]["ent_od"] == rows[0]["ent_od"]
    assert open(str(tmp_path / "drift.csv")).readline().strip() == ",".join(tent.DRIFT_COLUMNS)


def test_parser_defaults():
    from wtpse_hip import tent
    a = tent.parser().parse_args(["--images", "d", "--checkpoint", "c", "--out", "o"])
    assert (a.lr, a.steps, a.epochs, a.margin, a.reweight, a.stats, a.batch_size, a.clahe) == (1e-3, 1, 1, INF, False, "batch", 9, "checkpoint")
    a = tent.parser().parse_args(["--images", "d", "--checkpoint", "c", "--out", "o", "--margin", "0.2773", "--reweight", "--stats", "frozen",
                                  "--steps", "0", "--epochs", "2", "--lr", "5e-4", "--batch-size", "2"])
    assert (a.lr, a.steps, a.epochs, a.margin, a.reweight, a.stats, a.batch_size) == (5e-4, 0, 2, 0.2773, True, "frozen", 2)
    with pytest.raises(SystemExit):
        tent.parser().parse_args(["--images", "d", "--checkpoint", "c", "--out", "o", "--stats", "site"])
    import inspect
    sig = inspect.signature(tent.TentStep.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[5:12]] == [
        ("lr", 1e-3), ("betas", (0.9, 0.999)), ("steps", 1), ("margin", INF), ("reweight", False), ("stats", "batch"), ("episodic", False)]
    assert sig.parameters["affine_only"].default is True
