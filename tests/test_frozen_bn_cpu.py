"""Frozen-BatchNorm training (the backward through an eval-mode BatchNorm), the parts that need no GPU: the host specification of
the fold against torch's autograd, what the fixture tests/golden/frozen_bn.npz (tools/make_golden_frozen.py: the reference's own
modules in .eval()) lists, the C ABI of the new entry points, and the flag's way through TrainRun's config."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ("wtpse_bn_eval_coeffs_stats", "wtpse_bn_bwd_frozen", "wtpse_bn_bwd_from_stats_frozen",
               "wtpse_bn_bwd_finalize_coef_frozen", "wtpse_bn_bwd_scale_coef", "wtpse_dgrad_bnb_coef_frozen")


@pytest.mark.parametrize("relu", [False, True])
def test_fold_spec_equals_eval_batchnorm_autograd(relu):
    """ops.bn_frozen_fold_spec (dy = s g, dbeta = sum g, dgamma = r sum g (y - m), dbias = s sum g) against autograd of
    conv-bias -> F.batch_norm(training=False) -> ReLU in fp64."""
    from wtpse_hip import ops
    gen = torch.Generator().manual_seed(11)
    B, C, H, W = 3, 5, 6, 4
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    y0 = rnd(B, C, H, W).requires_grad_(True)
    bias, gamma, beta = rnd(C).requires_grad_(True), (1.0 + 0.3 * rnd(C)).requires_grad_(True), rnd(C).requires_grad_(True)
    gamma.data[1] = -gamma.data[1]                      # a negative scale, too
    rm, rv, w = 0.2 * rnd(C), 0.6 + torch.rand(C, generator=gen, dtype=torch.float64), rnd(B, C, H, W)
    rm0, rv0 = rm.clone(), rv.clone()
    y = y0 + bias.view(1, -1, 1, 1)
    a = F.batch_norm(y, rm, rv, gamma, beta, False, 0.1, 1e-5)
    z = torch.relu(a) if relu else a
    (z * w).sum().backward()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    g = w * (a.detach() > 0) if relu else w
    dy, dgamma, dbeta, dbias, mean, invstd = ops.bn_frozen_fold_spec(g, y.detach(), gamma.detach(), rm, rv, 1e-5)
    for got, want, what in ((dy, y0.grad, "dy"), (dgamma, gamma.grad, "dgamma"), (dbeta, beta.grad, "dbeta"), (dbias, bias.grad, "dbias")):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), what
    assert torch.equal(mean, rm) and torch.allclose(invstd, 1 / torch.sqrt(rv + 1e-5), rtol=1e-15)
    assert float(bias.grad.abs().min()) > 0          # (behind batch statistics this gradient is exactly zero)


def _prebn_biases(net):
    """Names of the conv biases in front of a BatchNorm, from the module structure: convN / bnN siblings of the U-Net blocks and the
    conv -> bn pairs (i, i + 1) of a DoubleConv's Sequential."""
    names = {n for n, _ in net.named_parameters()}
    out = []
    for n in sorted(names):
        if not n.endswith(".bias"):
            continue
        stem, leaf = n[:-5].rsplit(".", 1)
        if leaf.startswith("conv") and "%s.bn%s.weight" % (stem, leaf[4:]) in names:
            out.append(n)
        elif leaf.isdigit() and "%s.%d.weight" % (stem, int(leaf) + 1) in names and \
                any(b == "%s.%d.running_mean" % (stem, int(leaf) + 1) for b, _ in net.named_buffers()):
            out.append(n)
    return out


def test_fixture_lists_every_prebn_bias(golden_dir):
    """Every parameter the reference's eval-mode graph reaches is in the fixture with a nonzero fp64 gradient — in particular all
    conv biases in front of a BatchNorm (51 in the segmentation network: 26 of its own U-Net and 25 of the teacher; 23 in the student),
    which carry none in train mode — and the three fp32 draws sit where fp32 sits."""
    import algorithms
    import shape_networks
    from oracle import wtpse_cpu as O
    g = np.load(os.path.join(golden_dir, "frozen_bn.npz"))
    hp = dict(O.DEFAULT_HPARAMS)
    main = algorithms.WT_PSE(n_channels=3, n_classes=1, hparams=hp, device="cpu", two_step=False, per_domain_batch=2, source_domain_num=3)
    shape = shape_networks.ShapeVariationalDist_x(hp, "cpu", n_classes=1, number_source_domain=3, batch_size=2)
    assert [tuple(int(v) for v in c[:3]) for c in g["cases"]] == [(6, 2, 64), (6, 2, 256)]
    for ci in range(2):
        for call, net, nbias in (("A", main, 51), ("B", shape, 23)):
            names = [str(n) for n in g["c%d_%s_names" % (ci, call)]]
            params = dict(net.named_parameters())
            want = sorted(n for n in params if not (call == "B" and n.startswith("logvar_prior.")))
            assert names == want
            biases = _prebn_biases(net)
            assert len(biases) == nbias and set(biases) <= set(names)
            n2 = g["c%d_%s_n2" % (ci, call)]
            yard2 = g["c%d_%s_yard2" % (ci, call)]
            assert n2.shape == (len(names), 2) and yard2.shape == (len(names), 3)
            for i, k in enumerate(names):
                assert int(n2[i, 0]) == params[k].numel(), k
                assert n2[i, 1] > 0, "%s: zero gradient in the reference's eval-mode backward" % k
            small = sum(int(n) for n, _ in n2 if n <= 4096)
            assert g["c%d_%s_fp_small" % (ci, call)].shape == (small,)
            assert g["c%d_%s_fp_proj" % (ci, call)].shape == (sum(1 for n, _ in n2 if n > 4096), 128)
            assert float((yard2.sum(0).max() / n2[:, 1].sum()) ** 0.5) < 1e-4        # all gradients: fp32 from fp64
            bufs = [str(n) for n in g["c%d_%s_buf_names" % (ci, call)]]
            assert bufs == sorted(n for n, _ in net.named_buffers())
    assert g["c1_logits"].shape == (6, 1, 64, 64) and g["c0_logits"].shape == (6, 1, 64, 64)
    assert os.path.getsize(os.path.join(golden_dir, "frozen_bn.npz")) < (1 << 20)


def test_header_declares_and_library_binds_the_new_entries():
    from wtpse_hip import build, lib
    protos = build.parse_prototypes()
    bound = lib.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos and protos[name][-1] == "void*", name         # (stream last: the entry gets a plan thunk)
        assert len(bound[name]) == len(protos[name])
    frozen, plain = protos["wtpse_dgrad_bnb_coef_frozen"], protos["wtpse_dgrad_bnb_coef"]
    assert len(frozen) == len(plain) + 1                                         # + dbias; nothing else moved
    build.build()
    dll = ctypes.CDLL(lib.LIB_PATH)
    dll.wtpse_plan_fn_name.restype = ctypes.c_char_p
    recordable = {dll.wtpse_plan_fn_name(i).decode() for i in range(dll.wtpse_plan_fn_count())}
    for name in NEW_ENTRIES:
        assert getattr(dll, name) is not None and name in recordable, name
    # arguments are checked before anything is launched
    fn = dll.wtpse_bn_bwd_scale_coef
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    assert fn(None, None, None, 1, 1, 1, None, None) == -1


def test_freeze_bn_flag_round_trips_through_the_config():
    from wtpse_hip.step import TrainStep
    from wtpse_hip.trainer import TrainRun
    assert inspect.signature(TrainStep.__init__).parameters["freeze_bn"].default is False
    assert inspect.signature(TrainRun.__init__).parameters["freeze_bn"].default is False
    run = TrainRun.__new__(TrainRun)
    run.base_lr, run.iter_per_epoch, run.max_epoch, run.stop_epoch = (1e-3,) * 4, 3, 2, -1
    run.interval_validate, run.lr_schedule, run.seed, run.checkpoint_every = 10, None, 5, 0
    run.graph, run.betas = "plan", (0.9, 0.99)
    for flag in (False, True):
        run.freeze_bn = flag
        cfg = run.config()
        assert cfg["freeze_bn"] is flag
        kw = TrainRun.config_kwargs(cfg)
        assert kw["freeze_bn"] is flag and kw["lr_schedule"] is None and kw["lr"] == (1e-3,) * 4
        assert set(kw) <= set(inspect.signature(TrainRun.__init__).parameters)
    old = {k: v for k, v in run.config().items() if k != "freeze_bn"}            # a checkpoint from before the flag
    assert TrainRun.config_kwargs(old)["freeze_bn"] is False
    with pytest.raises(ValueError, match="freeze_bn"):
        TrainStep(None, None, None, None, {"whitening": True}, dp=object(), freeze_bn=True)
