"""Case tables, seeded inputs and rescale helpers of the power-of-two equivariance tests (profiles/scale_equivariance.md is the table
in prose).  Imports neither the product nor the GPU: test_scale_equivariance_cpu.py proves on the host that the stock-fp32 oracle has
the property on exactly these inputs, test_scale_equivariance_gpu.py asks the same of the HIP path and compares BITS.

Why bits: multiplying by 2^k commutes with every fp32 and fp16 rounding (no overflow, nothing subnormal).  Every scale of the x2h
arithmetic (two fp16 terms per fp32 operand) is a power of two taken from a bound of the operand's own tensor — a gradient's amax table,
the Samuelson bound behind a train-mode BatchNorm, the stored data's amax behind an eval-mode one, the pack kernel's weight scale — so
rescaling a tensor by 2^k moves its scale by 2^-k and every term, product and sum keeps its significand: after the power of two is
undone NO bit of any result may change.  A fixed scale, a stale table, the wrong tensor's table or a missing one changes bits.

  section 1  gradient scale, whole calls: backward of 2^k x loss for calls A (WT_PSE.update + BCE + ins + dom) and B (the student's
             update: kd + ins + dom) against k = 0
  section 2  activation scale, blocks: a BatchNorm's gamma, beta x f and its consumer's weights / f (f = 2^k) in a ConvD and a ConvU
             block: function preserving, the tensor in between is f times larger
  section 4  entry points of ops.py that write into a caller's float tensor: no amax table may outlive the contents it was taken from"""
import contextlib
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import wtpse_cpu as O
from oracle.filler import filled_state
from oracle.inputs import make_inputs, make_noise

HP = dict(O.DEFAULT_HPARAMS)
TERMS = (2, 3, 1)                       # wtpse_x3_terms: x2h (the default), x3, the one-term bf16 mode
MODES = ("train", "eval")               # batch statistics / frozen (running) statistics

# ---------------------------------------------------------------------------------------------------------------- section 1
GRAD_KS = (-24, -7, 9, 20)
CALL_B, CALL_PB, CALL_H = 3, 1, 32
CALL_SEED_IN, CALL_SEED_NOISE, CALL_SEED_W = 77, 78, 1234      # weights: main CALL_SEED_W, student CALL_SEED_W + 3 (by key name)


@functools.lru_cache(maxsize=None)
def call_inputs():
    """-> (img, od, eps) of calls A and B; shared, never written."""
    img, od, _ = make_inputs(CALL_SEED_IN, CALL_B, CALL_H, CALL_H)
    return img, od, make_noise(CALL_SEED_NOISE, (CALL_B, 1, CALL_H, CALL_H))


def call_states():
    """-> (state dict of the main network, of the student): what fill_state_dict(net, CALL_SEED_W [+ 3]) gives the HIP modules."""
    from test_oracle_golden import main_template, shape_template
    return filled_state(main_template(), CALL_SEED_W), filled_state(shape_template(), CALL_SEED_W + 3)


@contextlib.contextmanager
def oracle_statistics(mode):
    """The oracle's BatchNorms on batch statistics ("train": as written) or on the running ones ("eval": frozen, what update() under
    .eval() runs on the device)."""
    if mode == "train":
        yield
        return
    real = O._bn
    O._bn = lambda sd, name, x, training: real(sd, name, x, False)
    try:
        yield
    finally:
        O._bn = real


def oracle_calls(k, mode, dtype=torch.float32):
    """Calls A and B on the oracle with the loss multiplied by 2^k.
    -> {"A.logits", "A.loss" [3], "B.loss" [5], "A.g.<name>", "B.g.<name>"}."""
    img, od, eps = (t.to(dtype) for t in call_inputs())
    cast = lambda sd: {n: (v.to(dtype) if v.is_floating_point() else v) for n, v in sd.items()}
    main, shape = (cast(sd) for sd in call_states())
    out = {}
    with oracle_statistics(mode):
        a = O.as_leaves(main)
        logits, _, _, ins, dom = O.wt_pse_update(a, HP, img, od, img, True, eps, 3, CALL_PB)
        seg = O.seg_loss_od(logits, od)
        ((seg + ins + dom) * 2.0 ** k).backward()
        out["A.logits"], out["A.loss"] = logits.detach(), torch.stack([seg, ins, dom]).detach()
        out.update({"A.g." + n: v.grad for n, v in a.items() if not O.is_buffer(n) and v.grad is not None})
        b = O.as_leaves(shape)
        kd, ins_t, ins_ij, ins_ii, dom_s = O.shape_update(b, cast(main), HP, img, od, img, True, None, None, CALL_PB)
        ((kd + ins_t + dom_s) * 2.0 ** k).backward()
        out["B.loss"] = torch.stack([kd, ins_t, ins_ij, ins_ii, dom_s]).detach()
        out.update({"B.g." + n: v.grad for n, v in b.items() if not O.is_buffer(n) and v.grad is not None})
    return out


# ---------------------------------------------------------------------------------------------------------------- section 2
BLOCK_KS = (-16, -5, 5, 13)
Block = namedtuple("Block", "kind args x prev dz seed_w seed_x seed_prev seed_dz")
BLOCKS = {
    # ConvDBlock(32, 64): max-pool, three conv + BatchNorm layers on 8 x 8 maps
    "convd": Block("convd", (32, 64), (3, 32, 16, 16), None, (3, 64, 8, 8), 4242, 901, None, 902),
    # ConvUBlock(64, first=False): conv1 128 -> 64 (3x3), x2 upsampling, conv2 64 -> 32 (1x1), conv3 cat(prev 32, y 32) -> 64 (3x3)
    "convu": Block("convu", (64, False), (3, 128, 8, 8), (3, 32, 16, 16), (3, 64, 16, 16), 4343, 911, 912, 913),
}
# (block, rescaled BatchNorm, consumer, first rescaled input column of the consumer or None = all).  The last one is the CONCAT pair:
# only the second half of conv3's input columns is rescaled, and both halves share one input scale and one weight pack scale in x2h
Pair = namedtuple("Pair", "block bn conv lo")
PAIRS = {
    "convd.bn1-conv2": Pair("convd", "bn1", "conv2", None),
    "convd.bn2-conv3": Pair("convd", "bn2", "conv3", None),
    "convu.bn1-conv2": Pair("convu", "bn1", "conv2", None),
    "convu.bn2-conv3": Pair("convu", "bn2", "conv3", 32),
}
BITWISE_PAIRS = ("convd.bn1-conv2", "convd.bn2-conv3", "convu.bn1-conv2")
CONCAT_PAIR = "convu.bn2-conv3"


def block_template(blk):
    from test_oracle_golden import convd_template, convu_template
    return convd_template("", *blk.args) if blk.kind == "convd" else convu_template("", *blk.args)


@functools.lru_cache(maxsize=None)
def block_inputs(name):
    """-> (x, prev or None, dz); shared, never written."""
    b = BLOCKS[name]
    return (make_noise(b.seed_x, b.x), make_noise(b.seed_prev, b.prev) if b.prev is not None else None, make_noise(b.seed_dz, b.dz))


def block_state(name):
    """What fill_state_dict(block, seed_w) gives the HIP block (values by key name)."""
    b = BLOCKS[name]
    return filled_state(block_template(b), b.seed_w)


def rescale_state(sd, pair, k):
    """Function-preserving rescaling by f = 2^k on a copy of the state dict: gamma, beta of `pair.bn` x f, the weights of `pair.conv`
    (its input columns from pair.lo on) / f — ReLU, max-pool and bilinear upsampling are positively homogeneous."""
    f = 2.0 ** k
    out = {n: v.clone() for n, v in sd.items()}
    out[pair.bn + ".weight"] *= f
    out[pair.bn + ".bias"] *= f
    w = out[pair.conv + ".weight"]
    if pair.lo is None:
        w *= 1.0 / f
    else:
        w[:, pair.lo:] *= 1.0 / f
    return out


def expected_factors(pair, k, names):
    """What the k = 0 result `name` is multiplied by, element-wise, under rescale_state(.., pair, k): d gamma and d beta of the rescaled
    BatchNorm / f, dW of the consumer x f (the rescaled columns), everything else — the block's output, dx, dprev, every other
    gradient — x 1.  -> {name: float or a tensor broadcasting against the result}."""
    f = 2.0 ** k
    out = {}
    for n in names:
        if n in ("g." + pair.bn + ".weight", "g." + pair.bn + ".bias"):
            out[n] = 1.0 / f
        elif n == "g." + pair.conv + ".weight":
            if pair.lo is None:
                out[n] = f
            else:
                cin = BLOCKS[pair.block].args[0]            # ConvU(planes): conv3 has `planes` input columns
                col = torch.ones(1, cin, 1, 1)
                col[:, pair.lo:] = f
                out[n] = col
        else:
            out[n] = 1.0
    return out


def oracle_block(name, sd, mode, dtype=torch.float32):
    """The block on the oracle (conv_d / conv_u), forward + backward of the seeded upstream gradient.
    -> {"y", "dx", "dprev" (ConvU), "g.<parameter>"}."""
    b = BLOCKS[name]
    x, prev, dz = block_inputs(name)
    leaves = O.as_leaves({"b." + n: (v.to(dtype) if v.is_floating_point() else v) for n, v in sd.items()})
    x = x.to(dtype).clone().requires_grad_(True)
    prev = prev.to(dtype).clone().requires_grad_(True) if prev is not None else None
    with oracle_statistics(mode):
        y = O.conv_d(leaves, "b.", x, False, True) if b.kind == "convd" else O.conv_u(leaves, "b.", x, prev, b.args[1], True)
        y.backward(dz.to(dtype))
    out = {"y": y.detach(), "dx": x.grad}
    if prev is not None:
        out["dprev"] = prev.grad
    out.update({"g." + n[2:]: v.grad for n, v in leaves.items() if not O.is_buffer(n) and v.grad is not None})
    return out


def pre_bn_bias(name):
    """The bias of a convolution in front of a BatchNorm: behind batch statistics its gradient is exactly zero (the HIP path never
    writes it, the reference carries rounding noise there)."""
    return name.startswith("g.conv") and name.endswith(".bias")


def concat_bound(err_k, err_0, k):
    """The criterion of the concat pair (x2h): a shared input scale costs the smaller half at most one bit per binade of imbalance,
    x 2 for rounding direction."""
    return err_k <= 2.0 * 2.0 ** abs(k) * err_0


# ---------------------------------------------------------------------------------------------------------------- restated
def scale_from_amax(amax):
    from exact_cases import scale_from_amax as s
    return s(amax)


def is_subnormal(t):
    """Non-zero elements of an fp32 tensor below the smallest normal 2^-126."""
    t = t.detach().float()
    return (t != 0) & (t.abs() < 2.0 ** -126)


# ---------------------------------------------------------------------------------------------------------------- section 4
# Entry points of ops.py that write into a float tensor the CALLER supplies.  (name, builder): builder(o, dev) makes valid arguments on
# the device and -> (call, [written tensors]); the GPU test attaches a table of a wrong value to each written tensor, calls, and
# expects no table or one that holds the tensor's abs().max().  Not listed: attn_fuse_bwd(accumulate) — it takes its accumulator as a
# raw device pointer (d_wb_ptr), so there is no tensor object that could carry a table; the weight-gradient and BatchNorm-backward
# targets (views of the flat gradient buffer made per launch: nothing can be attached to them between two launches).
def _r(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _wt_loss_bwd(o, dev):
    st = o.wt_loss_fwd(_r(3, 16, 8, 8, seed=1).to(dev), 3, 1, 0.0)
    dz = _r(3, 16, 8, 8, seed=2).to(dev)
    return (lambda: o.wt_loss_bwd(st, dz, True)), [dz]


def _maxpool2_bwd(o, dev):
    x, dout, dx = _r(2, 8, 8, 8, seed=3).to(dev), _r(2, 8, 4, 4, seed=4).to(dev), _r(2, 8, 8, 8, seed=5).to(dev)
    return (lambda: o.maxpool2_bwd(x, dout, dx, True)), [dx]


def _maxpool2_bwd_bnb(o, dev):
    x, dout, dx = _r(2, 8, 8, 8, seed=6).to(dev), _r(2, 8, 4, 4, seed=7).to(dev), _r(2, 8, 8, 8, seed=8).to(dev)
    pro = torch.stack([torch.ones(8), torch.zeros(8)], 1).contiguous().to(dev)
    mean = torch.zeros(8, device=dev)

    def call():
        assert o.maxpool2_bwd_bnb(x, dout, dx, pro, True, mean) is not None
    return call, [dx]


def _relu_mask(o, dev):
    dz, ref, out = _r(2, 8, 8, 8, seed=9).to(dev), _r(2, 8, 8, 8, seed=10).to(dev), _r(2, 8, 8, 8, seed=11).to(dev)
    return (lambda: o.relu_mask(dz, ref, out=out, accumulate=True)), [out]


def _axpy(o, dev):
    dst, src = _r(1000, seed=12).to(dev), _r(1000, seed=13).to(dev)
    return (lambda: o.axpy(dst, src, 3.0)), [dst]


def _zero(o, dev):
    t = _r(1000, seed=14).to(dev)
    return (lambda: o.zero_(t)), [t]


def _nan_scrub(o, dev):
    t = _r(1000, seed=15).to(dev)
    t[7] = float("nan")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    return (lambda: o.nan_scrub_(t, flag)), [t]


def _head_bwd(o, dev):
    B, H, W, nc = 2, 8, 8, 1
    D = lambda t: t.to(dev).contiguous()
    x = D(_r(B, 32, H, W, seed=16))
    w1, b1 = D(_r(32, 32, 1, 1, seed=17, scale=0.3)), D(_r(32, seed=18, scale=0.2))
    w2, b2 = D(_r(8, 32, 1, 1, seed=19, scale=0.3)), D(_r(8, seed=20, scale=0.2))
    w3, b3 = D(_r(nc, 8, 1, 1, seed=21, scale=0.5)), D(_r(nc, seed=22, scale=0.2))
    dy = D(_r(B, nc, H, W, seed=23))
    _, h1, h2 = o.head_fwd(x, None, False, w1, b1, w2, b2, w3, b3, True, want_h1=True)
    dpar = D(_r(1320 + 9 * nc, seed=24))
    return (lambda: o.head_bwd(dy, x, None, False, h1, h2, w1, w2, w3, dpar, accumulate=True, b1=b1)), [dpar]


def _loss_args(dev):
    x = _r(2, 1, 16, 16, seed=25).to(dev)
    t = (_r(2, 1, 16, 16, seed=26) > 0).float().to(dev)
    return x, t, torch.full((1,), 0.37, dtype=torch.float32, device=dev), _r(2, 1, 16, 16, seed=27, scale=1e-3).to(dev)


def _boundary_loss(o, dev):
    x, t, w, dx = _loss_args(dev)
    phi = o.signed_distance(t)
    return (lambda: o.boundary_loss(x, phi, w, dx=dx)), [dx]


def _overlap_loss(o, dev):
    x, t, w, dx = _loss_args(dev)
    cfg = namedtuple("Cfg", "fp fn focal smooth")(0.5, 0.5, 1.0, 1.0)
    return (lambda: o.overlap_loss(x, t, w, cfg, dx=dx)), [dx]


def _lovasz_loss(o, dev):
    x, t, w, dx = _loss_args(dev)
    return (lambda: o.lovasz_loss(x, t, w, dx=dx)), [dx]


def _adam_step(o, dev):
    p, g = _r(1000, seed=28).to(dev), _r(1000, seed=29).to(dev)
    m, v = torch.zeros(1000, device=dev), torch.zeros(1000, device=dev)
    return (lambda: o.adam_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1)), [p]


def _avg_merge(o, dev):
    acc, seg = _r(1000, seed=30).to(dev), _r(1000, seed=31).to(dev)
    return (lambda: o.avg_merge(acc, seg, 2, 3)), [acc]


def _shape_samples_mask(o, dev):
    ref = (_r(2, 1, 8, 8, seed=32) > 0).float().to(dev)
    mean, std = _r(2, 1, 8, 8, seed=33).to(dev), _r(2, 1, 8, 8, seed=34).abs().to(dev)
    votes = torch.ones(2, 1, 8, 8, dtype=torch.uint8, device=dev)
    logits = _r(2, 4, 8, 8, seed=35).to(dev)
    return (lambda: o.shape_samples_mask_(ref, mean, std, votes, logits)), [mean, std, logits]


INPLACE_ENTRY_POINTS = (
    ("wt_loss_bwd", _wt_loss_bwd), ("maxpool2_bwd", _maxpool2_bwd), ("maxpool2_bwd_bnb", _maxpool2_bwd_bnb),
    ("relu_mask(out=)", _relu_mask), ("axpy", _axpy), ("zero_", _zero), ("nan_scrub_", _nan_scrub),
    ("head_bwd(accumulate)", _head_bwd), ("boundary_loss(dx=)", _boundary_loss), ("overlap_loss(dx=)", _overlap_loss),
    ("lovasz_loss(dx=)", _lovasz_loss), ("adam_step", _adam_step), ("avg_merge", _avg_merge),
    ("shape_samples_mask_", _shape_samples_mask),
)
INPLACE_NOT_REACHABLE = ("attn_fuse_bwd(accumulate)",)      # raw pointer: see above
