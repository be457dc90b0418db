"""Case tables, seeded inputs, fp64 / stock-PyTorch references and a Python restatement of every launcher's branch predicate for
the bandwidth-bound kernels behind csrc/pointwise.hip, csrc/bn.hip and csrc/wt_loss.hip (profiles/dispatch_paths.md is the
table in prose).  Imports neither the product nor the GPU: test_dispatch_paths_cpu.py proves the tables on the host
(predicate == expected branch == the library's host query; the kink conditions of the references), test_dispatch_paths_gpu.py
runs them.  A case names the branch it is there for; a retune that moves a case onto another branch fails both files."""
import numpy as np
import torch
import torch.nn.functional as F

GUARD = 64                      # floats of sentinel on either side of every output
NAN_BITS = 0x7FC0BEEF           # the sentinel: a quiet NaN with a payload no kernel produces
PLANE_CAP = 32768               # PLANE_GRID: gridDim.y stops here and the kernels loop bc += gridDim.y


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def ceil_div(a, b):
    return (a + b - 1) // b


# =============================================================================================== predicates (pointwise.hip)
def plane_trips(planes):
    """Trips of the `for (bc = blockIdx.y; bc < BC; bc += gridDim.y)` loop that the first planes take."""
    return ceil_div(planes, min(planes, PLANE_CAP))


def pool_fwd_branch(H, W, aligned=True):          # wtpse_maxpool2_fwd: x | out
    return "vec" if W % 4 == 0 and aligned else "scalar"


def pool_bwd_branch(H, W, aligned=True):          # wtpse_maxpool2_bwd: x | dx | dout
    return "vec" if W % 4 == 0 and H % 2 == 0 and aligned else "scalar"


def up_fwd_branch(H, W, out_aligned=True):        # wtpse_upsample2x_fwd: out only (x is read with scalar loads)
    return "vec" if W % 2 == 0 and W >= 2 and out_aligned else "scalar"


def up_bwd_branch(H, W, aligned=True):            # wtpse_upsample2x_bwd: dout | dx
    return "vec" if W % 4 == 0 and aligned else "scalar"


def flat_branch(n, aligned=True):                 # wtpse_relu_mask / wtpse_axpy / vec_ok() of bn.hip
    return "vec" if n % 4 == 0 and aligned else "scalar"


def amax_branch(n, aligned=True):                 # amax_k: (16-byte body, scalar tail elements) or the misaligned form
    return ("body+tail" if n % 4 else "body") if aligned else "misaligned"


def reduce_blocks(n):                             # red_blocks(): 4096 elements per workgroup, at most 1024 workgroups
    return max(1, min(1024, ceil_div(n, 256 * 16)))


def loss_trips(n):
    """Grid-stride trips of the first thread of a loss kernel."""
    return ceil_div(n, reduce_blocks(n) * 256)


def reduce_rows_branch(rows, cols):               # wtpse_attn_fuse_bwd's fold of its (dw, db) partials
    return "tall" if rows >= 1024 else "rows"


def pool_stats_blocks(B, H, W):
    return B * ceil_div((H // 2) * (W // 4), 256)


def up_stats_blocks(B, H, W):
    return B * ceil_div((H + 1) * (W // 2), 256)


# =============================================================================================== predicates (bn.hip)
def bn_bwd_segs(B, C, HW):
    segs, cap = 1, 2048 // max(C, 1)
    while B * segs * 2 <= cap and HW % (segs * 2 * 2048) == 0 and HW // (segs * 2) >= 8192:
        segs *= 2
    return segs


def bn_bwd_nsplit(B, C, HW):
    return max(1, min(2048 // max(C, 1), B * bn_bwd_segs(B, C, HW)))


def bn_fold_width(nrows):                         # BN_LAUNCH_FOLD: threads of the kernels that fold `nrows` partial rows per channel
    return 1024 if nrows >= 2048 else 256


def bn_bwd_branch(B, C, HW, in_aligned=True, dy_aligned=True, halves=False):
    """wtpse_bn_bwd -> the launches it makes.  reduce: vec needs dz | y; apply and the one-launch form need dz | y | dy.
    halves: through wtpse_bn_bwd_reduce + wtpse_bn_bwd_apply (the synchronised-BatchNorm pair), which have no one-launch form."""
    vec_in = HW % 4 == 0 and in_aligned
    vec_all = vec_in and dy_aligned
    if B * HW <= 32768 and C >= 96 and vec_all and not halves:
        return {"path": "small"}
    segs, ns = bn_bwd_segs(B, C, HW), bn_bwd_nsplit(B, C, HW)
    SL = HW // segs
    return {"path": "three", "reduce": "vec" if vec_in else "scalar", "apply": "vec" if vec_all else "scalar", "segs": segs,
            "nsplit": ns, "units_per_split": ceil_div(B * segs, ns), "finalize": bn_fold_width(ns),
            # bn_bwd_reduce_k<true>: threads whose last float4 is taken by the `if (p < SL)` remainder instead of the paired loop
            "remainder": vec_in and any(_reduce_remainder(SL, t) for t in range(256))}


def _reduce_remainder(SL, t):
    p = 4 * t
    while p + 1024 < SL:
        p += 2048
    return p < SL


# =============================================================================================== predicates (wt_loss.hip)
def wt_split(B, HW):
    target = max(1, 768 // max(B, 1))
    chunk = max(2048, ceil_div(ceil_div(HW, target), 512) * 512)
    return ceil_div(HW, chunk), chunk


def wt_branch(B, HW, z_aligned=True, dz_aligned=True, S=None):
    s, chunk = wt_split(B, HW)
    S = s if S is None else S
    fwd = "vec" if HW % 4 == 0 and z_aligned else "scalar"
    bwd = "vec" if HW % 4 == 0 and z_aligned and dz_aligned else "scalar"
    NW = 16 if S >= 32 else 4
    single = False                                 # gram_finalize_k: does any wave's single-step remainder loop run?
    for q in range(NW):
        k = q
        while k + NW < S:
            k += 2 * NW
        single = single or k < S
    return {"S": S, "chunk": chunk, "last_chunk": HW - (s - 1) * chunk, "fwd": fwd, "bwd": bwd,
            "bwd_blocks": ceil_div(HW, 1024 if bwd == "vec" else 256), "finalize": NW, "finalize_pairs": S > NW,
            "finalize_single": single}


# =============================================================================================== case tables
# ---- pool / upsample: name -> (shape, expected branch, expected plane-loop trips)
POOL_FWD_CASES = {
    "plane_cap":   ((3, 10925, 2, 4), "vec", 2),       # B*C = 32775: the channel index wraps across the gridDim.y stride
    "plane_exact": ((2, 16384, 2, 4), "vec", 1),       # B*C = 32768 exactly
    "odd_h":       ((2, 3, 7, 8), "vec", 1),           # the last row is dropped
    "align":       ((2, 3, 8, 12), "vec", 1),
    "ties":        ((2, 3, 6, 8), "vec", 1),
    "odd_w":       ((2, 3, 6, 6), "scalar", 1),
}
POOL_BWD_CASES = {
    "plane_cap":   ((3, 10925, 2, 4), "vec", 2),
    "plane_exact": ((2, 16384, 2, 4), "vec", 1),
    "odd_h":       ((2, 3, 7, 8), "scalar", 1),        # W % 4 == 0 but H odd
    "even_h":      ((2, 3, 6, 8), "vec", 1),
    "align":       ((2, 3, 8, 12), "vec", 1),
    "ties":        ((2, 3, 6, 8), "vec", 1),
}
UP_FWD_CASES = {
    "plane_cap":   ((3, 10925, 1, 2), "vec", 2),
    "plane_exact": ((2, 16384, 1, 2), "vec", 1),
    "w2":          ((2, 3, 1, 2), "vec", 1),           # even W that is no multiple of 4, H = 1
    "w6":          ((2, 3, 1, 6), "vec", 1),
    "w10":         ((2, 3, 1, 10), "vec", 1),
    "w6_h3":       ((2, 3, 3, 6), "vec", 1),
    "w1":          ((2, 3, 1, 1), "scalar", 1),
    "w5":          ((2, 3, 1, 5), "scalar", 1),
    "align":       ((2, 3, 8, 12), "vec", 1),
}
UP_BWD_CASES = {                                       # shapes of dx; dout is twice as large
    "plane_cap":   ((3, 10925, 1, 4), "vec", 2),
    "plane_exact": ((2, 16384, 1, 4), "vec", 1),
    "w4":          ((2, 3, 3, 4), "vec", 1),           # the smallest vector case: both halo loads are guarded
    "w8_h1":       ((2, 3, 1, 8), "vec", 1),
    "w6":          ((2, 3, 3, 6), "scalar", 1),
    "align":       ((2, 3, 8, 12), "vec", 1),
}
UP_BWD_BN_CASES = {"w4": (2, 3, 3, 4), "w8": (2, 3, 2, 8)}
AMAX_SIZES = (1, 3, 4, 5, 1023, 1027)
FLAT_SIZES = (1, 3, 4, 1021, 1024, 1028)

# ---- losses
LOSS_SIZES = {1: 1, 255: 1, 257: 1, 4096: 1, 4097: 2, 1024 * 4096 + 257: 1024}     # n -> wtpse_reduce_blocks(n)
ADAM_SIZES = (1, 255, 257)
ATTN_CASES = {                                         # name -> (B, CE, HW, rows of partials, fold kernel)
    "rows_1023":   (1, 2, 1023 * 256, 1023, "rows"),
    "tall_1024":   (1, 2, 1024 * 256, 1024, "tall"),
    "tall_ragged": (1, 2, 1024 * 256 + 5, 1025, "tall"),
}
RANDN_SIZES = (1001, 1002, 1003)
SATURATED = [float(v) for v in range(0, 9)] + [20.0, 40.0, 90.0]

# ---- BatchNorm backward: name -> (shape, relu, expected subset of bn_bwd_branch())
BN_CASES = {
    "segs2":       ((1, 2, 128, 128), True, {"path": "three", "segs": 2, "nsplit": 2, "reduce": "vec"}),
    "segs4":       ((1, 2, 128, 256), False, {"path": "three", "segs": 4, "nsplit": 4}),
    "segs2_b3":    ((3, 2, 128, 128), True, {"path": "three", "segs": 2, "nsplit": 6}),
    # (wtpse_bn_bwd itself sends 1024 channels of 48 elements to the one-launch kernel: this case goes through the two halves)
    "two_units":   ((3, 1024, 4, 4), True, {"path": "three", "segs": 1, "nsplit": 2, "units_per_split": 2, "reduce": "vec"}),
    "wide":        ((2051, 1, 2, 2), True, {"path": "three", "nsplit": 2048, "finalize": 1024, "units_per_split": 2}),
    "small_96":    ((2, 96, 16, 16), True, {"path": "small"}),
    "three_95":    ((2, 95, 16, 16), True, {"path": "three", "reduce": "vec", "finalize": 256}),
}
BN_HALVES = ("two_units",)                                    # cases run through wtpse_bn_bwd_reduce + wtpse_bn_bwd_apply
BN_VEC_HW = (1020, 1024, 1028, 2044, 2048, 2052, 3076)        # (2, 3, 1, HW): the paired loop and its remainder
BN_SCALAR_HW = (1, 63, 1023)                                  # (5, 3, 1, HW): HW % 4 != 0
for _hw in BN_VEC_HW:
    BN_CASES["vec_%d" % _hw] = ((2, 3, 1, _hw), _hw % 8 == 4, {"path": "three", "reduce": "vec", "apply": "vec", "nsplit": 2,
                                                               "remainder": _hw not in (2048,)})
for _hw in BN_SCALAR_HW:
    BN_CASES["scalar_%d" % _hw] = ((5, 3, 1, _hw), _hw != 63, {"path": "three", "reduce": "scalar", "apply": "scalar"})

# ---- the finishers of the BatchNorm backward (csrc/bn_math.h: bn_bwd_store, bn_bwd_channel) on sums that are exact
BN_EXACT_SHAPE = (2, 96, 4, 4)                 # wtpse_bn_bwd: the one-launch kernel; cut to BN_EXACT_CUT channels: reduce, finalize<256>, apply
BN_EXACT_CUT = 95
BN_EXACT_ROWS = (3, 2051)                      # rows of host-built partials: bn_bwd_finalize_k<256> and <1024>
BN_EXACT_C = 3
BN_EXACT_TAIL = 6                              # exact_cases.TABLES["bnb"]: the smallest case (B * Cl * H * W) of the fp32 layout
BN_EXACT_FORMS = ("one_launch", "three", "finalize", "finalize_frozen", "tail", "tail_frozen")

# ---- WT loss: name -> (shape, per_domain, expected subset of wt_branch()); the seeds: WT_SEEDS
WT_CASES = {
    "hw2052":   ((3, 16, 36, 57), 1, {"S": 2, "last_chunk": 4, "fwd": "vec", "bwd": "vec", "bwd_blocks": 3, "finalize": 4}),
    "hw2049":   ((3, 16, 3, 683), 1, {"S": 2, "last_chunk": 1, "fwd": "scalar", "bwd": "scalar", "bwd_blocks": 9}),
    "hw5120":   ((6, 16, 64, 80), 2, {"S": 3, "fwd": "vec", "bwd": "vec", "bwd_blocks": 5}),
    "hw35":     ((3, 16, 5, 7), 1, {"S": 1, "fwd": "scalar", "bwd": "scalar", "bwd_blocks": 1}),
    "b770":     ((770, 16, 4, 4), 2, {"S": 1, "chunk": 2048, "fwd": "vec", "bwd": "vec"}),       # 768 / B clamps to 1; R = 6 < B
}
WT_FINALIZE_S = {31: (4, True, True), 32: (16, True, False), 33: (16, True, True), 47: (16, True, True), 64: (16, True, False)}
#                 S -> (waves NW, the paired loop runs, some wave runs the single-step remainder loop)
KINK_MARGIN = 1e-5


# seeds chosen on the host so that no fp64 Gram entry lies within KINK_MARGIN of a sign kink (test_dispatch_paths_cpu.py asserts it)
WT_SEEDS = {"hw2052": 1, "hw2049": 0, "hw5120": 4, "hw35": 0, "b770": 768}
WT_FINALIZE_SEEDS = {31: 0, 32: 0, 33: 0, 47: 1, 64: 2}


# =============================================================================================== references
def act64(x, pro, relu):
    v = x.double()
    if pro is not None:
        C = pro.shape[0]
        v = v * pro[:, 0].double().view(1, C, 1, 1) + pro[:, 1].double().view(1, C, 1, 1)
    return F.relu(v) if relu else v


def make_pro(C, seed):
    return torch.stack([rnd(C, seed=seed) * 0.5 + 1.0, rnd(C, seed=seed + 1) * 0.3], 1).contiguous()


def pool_input(name, shape, seed=31):
    x = rnd(*shape, seed=seed)
    if name == "ties":
        # windows that are all-equal (positive and negative) and all-negative: under ReLU the negative ones become all-zero,
        # and the first element wins (as ATen)
        x[0, 0, 0:2, 0:2] = 0.75
        x[0, 1, 2:4, 4:6] = -0.5
        x[1, 2, 4:6, 6:8] = -x[1, 2, 4:6, 6:8].abs() - 0.1
        x[1, 0, 0:2, 4:8] = 0.0
    return x


def pool_window_gap(x, pro, relu):
    """Smallest non-zero gap between the largest two values of a 2x2 window (fp64): an exact tie is decided the same way by every
    implementation, a gap of rounding size is not."""
    a = act64(x, pro, relu)
    B, C, H, W = a.shape
    a = a[:, :, :H // 2 * 2, :W // 2 * 2]
    w = a.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
    top = w.topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    gap = gap[gap > 0]
    return float(gap.min()) if gap.numel() else float("inf")


def pool_ref(x, pro, relu, dp, base, accumulate):
    """-> (pooled, dx) in fp64: dx = ((accumulate & 1 ? base : 0) + pool backward) * (accumulate & 2 ? [act(x) > 0] : 1)."""
    a = act64(x, pro, relu).requires_grad_(True)
    p = F.max_pool2d(a, 2)
    p.backward(dp.double())
    g = a.grad
    if accumulate & 1:
        g = g + base.double()
    if accumulate & 2:
        g = g * (a.detach() > 0)
    return p.detach(), g


def up_ref(x, pro, relu):
    return F.interpolate(act64(x, pro, relu), scale_factor=2, mode="bilinear", align_corners=False)


def up_bwd_ref(du, base=None):
    B, C, Ho, Wo = du.shape
    x = torch.zeros(B, C, Ho // 2, Wo // 2, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False).backward(du.double())
    return x.grad if base is None else x.grad + base.double()


# ---- BatchNorm
def bn_inputs(shape, relu, seed=100, channels=None):
    """Seeded operands of a train-mode BatchNorm backward on a random y, the statistics the forward would have saved (fp64 of the
    fp32 y, rounded once) and the fp64 autograd reference.  channels: keep the first `channels` channels of the same data."""
    B, C, H, W = shape
    y = rnd(B, C, H, W, seed=seed)
    dz = rnd(B, C, H, W, seed=seed + 1)
    gamma = rnd(C, seed=seed + 2) * 0.2 + 1
    beta = rnd(C, seed=seed + 3) * 0.2
    if channels is not None:
        y, dz, gamma, beta = y[:, :channels].contiguous(), dz[:, :channels].contiguous(), gamma[:channels].clone(), beta[:channels].clone()
        C = channels
    mean = y.double().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(y.double().var((0, 2, 3), unbiased=False) + 1e-5)
    ss = torch.stack([gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd], 1).float().contiguous()
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(y64, None, None, g64, b64, True, 0.1, 1e-5)
    on_kink = (z.detach().abs() < 2e-6) if relu else torch.zeros_like(z, dtype=torch.bool)
    (F.relu(z) if relu else z).backward(dz.double())
    gm = dz.double() * (z.detach() > 0) if relu else dz.double()          # the masked incoming gradient
    return {"y": y, "dz": dz, "gamma": gamma, "beta": beta, "mean": mean.float().contiguous(), "invstd": invstd.float().contiguous(),
            "ss": ss, "relu": relu, "dy": y64.grad, "dgamma": g64.grad, "dbeta": b64.grad, "on_kink": on_kink, "g_masked": gm,
            "shape": (B, C, H, W)}


def _ints(shape, seed, lim=3):
    return torch.randint(-lim, lim + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).double()


def bn_exact_channels(C, seed):
    """Per channel: gamma and invstd arbitrary fp32, the mean an integer or a half.  -> gamma, invstd, mean (fp32)"""
    return rnd(C, seed=seed) * 0.2 + 1, rnd(C, seed=seed + 1).abs() * 0.7 + 0.4, (_ints((C,), seed + 2, 4) * 0.5).float()


def bn_exact_inputs(channels=None, seed=700):
    """Operands of wtpse_bn_bwd on BN_EXACT_SHAPE whose sums are exact in EVERY kernel, whatever the order: dz = g and y - mean are
    integers |v| <= 3, the mean and the shift are halves and the scale is one of (1, 2, -1, 0.5), so the ReLU decision, the products
    g (y - mean) and all their fp32 sums are exact.  bn_bwd_reduce_k multiplies a THREAD's sum by invstd in fp32 before its butterfly
    (bn_bwd_small_k does the same in fp64): for that to be exact too, the products of an (image, channel) plane are non-zero in one
    float4 (one row: W = 4) only and add up to +-2^k there — chosen by rejection among seeded candidates; in the other rows g or
    y - mean is 0 element by element.  -> as bn_inputs, with the exact sums s1 = sum g [z > 0] and n2 = sum g [z > 0] (y - mean)."""
    B, C, H, W = BN_EXACT_SHAPE
    assert W == 4
    gamma, invstd, mean = bn_exact_channels(C, seed)
    sc = torch.tensor([1.0, 2.0, -1.0, 0.5], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=torch.Generator().manual_seed(seed + 3))]
    sf = _ints((C,), seed + 4) * 0.5
    ch = lambda v: v.view(1, C, 1, 1)
    g, d = _ints((B, C, H, W), seed + 5), _ints((B, C, H, W), seed + 6)
    coin = torch.randint(0, 2, (B, C, H, W), generator=torch.Generator().manual_seed(seed + 7)).bool()
    g, d = torch.where(coin, g, torch.zeros_like(g)), torch.where(coin, torch.zeros_like(d), d)          # g (y - mean) = 0 everywhere ...
    K = 64                                                                                               # ... but in one row per plane
    cg, cd = _ints((B, C, K, W), seed + 8), _ints((B, C, K, W), seed + 9)
    live = ((cd + mean.double().view(1, C, 1, 1)) * ch(sc) + ch(sf)) > 0
    n = (cg * live * cd).sum(3)
    pow2 = torch.log2(n.abs().clamp(min=1)) % 1 == 0
    score = 2 * ((n != 0) & pow2).long() + (n == 0).long()               # (a channel whose ReLU is never live has only zero sums)
    assert bool((score.max(2).values > 0).all()), "no candidate row with a power-of-two sum"
    pick = score.argmax(2)                                                                                # the first of the best
    row = torch.randint(0, H, (B, C), generator=torch.Generator().manual_seed(seed + 10))
    bi, ci = torch.meshgrid(torch.arange(B), torch.arange(C), indexing="ij")
    g[bi, ci, row], d[bi, ci, row] = cg[bi, ci, pick], cd[bi, ci, pick]
    y = d + ch(mean.double())
    gm = g * ((y * ch(sc) + ch(sf)) > 0)
    r = {"y": y.float(), "dz": g.float(), "gamma": gamma, "mean": mean, "invstd": invstd, "ss": torch.stack([sc, sf], 1).float().contiguous(),
         "relu": True, "g_masked": gm, "s1": gm.sum((0, 2, 3)), "n2": (gm * d).sum((0, 2, 3)), "shape": BN_EXACT_SHAPE,
         "on_kink": torch.zeros(B, C, H, W, dtype=torch.bool)}
    if channels is not None:
        r = {k: (v if k in ("relu", "shape") else (v[:, :channels] if v.dim() == 4 else v[:channels]).contiguous()) for k, v in r.items()}
        r["shape"] = (B, channels, H, W)
    return r


def bn_exact_rows(seed=720):
    """Host-built partial rows (sum g, sum g (y - mean)) for the finalize kernels: BN_EXACT_ROWS[1] rows of integers |v| <= 3 and the
    same sums in BN_EXACT_ROWS[0] rows (contiguous groups added up).  -> {rows: fp32 [rows, C, 2]}, s1, n2 (fp64 [C])"""
    few, many = BN_EXACT_ROWS
    rows = _ints((many, BN_EXACT_C, 2), seed)
    cut = [many * i // few for i in range(few + 1)]
    grouped = torch.stack([rows[cut[i]:cut[i + 1]].sum(0) for i in range(few)])
    return {many: rows.float().contiguous(), few: grouped.float().contiguous()}, rows[:, :, 0].sum(0), rows[:, :, 1].sum(0)


def bn_finish_ref(s1, n2, count, gamma, mean, invstd, frozen=False):
    """csrc/bn_math.h (bn_bwd_store, bn_bwd_channel) in numpy float64, in the order the functions write the expressions, from the
    exact sums s1 = sum g and n2 = sum g (y - mean); the fp32 operands enter as they are.  Nothing is rounded to fp32 here.
    k3_tol: k3 is a difference of two terms — 2^-23 (|k1 s1 / N| + |k2 mean|)."""
    f = lambda t: np.asarray(t.detach().cpu().double().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
    s1, n2, gamma, mean, invstd, count = f(s1), f(n2), f(gamma), f(mean), f(invstd), float(count)
    s2 = n2 * invstd
    k1 = gamma * invstd
    k2 = -gamma * invstd * invstd * s2 / count
    k3 = -k1 * s1 / count - k2 * mean
    out = {"dbeta": s1, "dgamma": s2, "k3_tol": 2.0 ** -23 * (np.abs(k1 * s1 / count) + np.abs(k2 * mean))}
    if frozen:
        k2, k3 = np.zeros_like(k2), np.zeros_like(k3)
        out["dbias"] = k1 * s1
    out.update(k1=k1, k2=k2, k3=k3)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def ulps_apart(got, ref64):
    """Largest distance, in fp32 steps, between `got` (fp32) and the fp64 reference rounded once to fp32."""
    key = lambda t: (lambda i: torch.where(i < 0, -(i & 0x7FFFFFFF), i))(t.detach().cpu().contiguous().view(torch.int32).long())
    return int((key(got.float()) - key(ref64.float())).abs().max())


def kink_cap(numel):
    return max(2, numel // 100000)


# ---- WT loss
def wt_feature(shape, seed):
    return rnd(*shape, seed=seed, scale=0.7)


def wt_gram64(z):
    B, C, H, W = z.shape
    f = z.double().reshape(B, C, -1)
    return torch.bmm(f, f.transpose(1, 2)) / (H * W - 1) + 1e-5 * torch.eye(C, dtype=torch.float64)


def wt_kink_distance(z):
    """Smallest distance of an fp64 Gram entry from a sign kink: |G_ij| (i < j) and |G_ii - 1|."""
    g = wt_gram64(z)
    iu = torch.triu_indices(16, 16, 1)
    return min(float(g[:, iu[0], iu[1]].abs().min()), float((g.diagonal(dim1=1, dim2=2) - 1).abs().min()))


def wt_margin_one_off(z):
    """A margin between the smallest and the second smallest per-image off-diagonal sum: it switches exactly one image's
    off-diagonal clamp off (the diagonal sums are an order of magnitude larger and stay on)."""
    g = wt_gram64(z)
    off = (g.abs() * torch.ones(16, 16, dtype=torch.float64).triu(1)).sum((1, 2)).sort().values
    return float(torch.tensor(0.5 * float(off[0] + off[1]), dtype=torch.float32))


def wt_ref(z, per_domain, margin, weights=(1.0, 1.0, 1.0), domain_num=3):
    """oracle.wtpse_cpu.whitening_loss in fp64 -> off, diag, dom, gram [B,16,16], v [B,120], dz (of w0 off + w1 diag + w2 dom)."""
    from oracle import wtpse_cpu as O
    zr = z.double().requires_grad_(True)
    off, dg, dom = O.whitening_loss(zr, domain_num, per_domain, float(margin))
    (weights[0] * off + weights[1] * dg + weights[2] * dom).backward()
    g = wt_gram64(z)
    iu = torch.triu_indices(16, 16, 1)
    return {"off": off.detach(), "diag": dg.detach(), "dom": dom.detach(), "gram": g, "v": g[:, iu[0], iu[1]], "dz": zr.grad}


def wt_partials(z, S):
    """The pixels of z in S groups (pixel p -> group p % S), each group's z z^T in fp64, rounded to fp32: [B * S, 256]."""
    B, C, H, W = z.shape
    f = z.double().reshape(B, C, -1)
    parts = [torch.bmm(f[:, :, s::S], f[:, :, s::S].transpose(1, 2)) for s in range(S)]
    return torch.stack(parts, 1).reshape(B * S, 256).float().contiguous()


def wt_combine_ref(losses, den, mode):
    """The two folds of wt_combine_k's header comment, in fp64.  -> (ins_total, ins_off, ins_diag, dom)."""
    l = losses.double()
    off, dom = l[:, 0].sum() / den, l[:, 2].sum() / den
    if mode == 0:
        diag = l[:, 1].sum() / den
        tot = (l[:, 0] + l[:, 1]).sum() / den
    else:
        diag = 2 * l[-1, 1] / den
        tot = off + diag
    return torch.stack([tot, off, diag, dom])


# ---- losses / Adam
def loss_inputs(n, seed=61):
    x = rnd(n, seed=seed) * 3
    t = (rnd(n, seed=seed + 1) > 0).float()
    m = (rnd(n, seed=seed + 2) > -0.5).float()
    if n < 8:
        t[0], m[0] = 1.0, 1.0                      # a positive, unmasked target: pos_weight is finite
    a, b = rnd(n, seed=seed + 3), rnd(n, seed=seed + 4)
    return x, t, m, a, b


def loss_refs(x, t, m, a, b, g=1.0, w=1.0):
    """fp64 values and gradients (upstream gradient g, loss weight w) of the caller's losses."""
    x64 = x.double().requires_grad_(True)
    bce = F.binary_cross_entropy(torch.sigmoid(x64), t.double())
    (g * w * bce).backward()
    sums = torch.stack([m.double().sum(), (m.double() * t.double()).sum()])
    pw = sums[0] / sums[1]
    if not torch.isfinite(pw):
        pw = torch.tensor(1.0, dtype=torch.float64)
    x2 = x.double().requires_grad_(True)
    bpw = F.binary_cross_entropy_with_logits(x2 * m.double(), t.double(), pos_weight=pw)
    (g * w * bpw).backward()
    a64 = a.double().requires_grad_(True)
    mse = F.mse_loss(a64, b.double())
    (g * w * mse).backward()
    return {"bce": bce.detach(), "dbce": x64.grad, "sums": sums, "pw": pw, "bpw": bpw.detach(), "dbpw": x2.grad,
            "mse": mse.detach(), "dmse": a64.grad}


def saturated_inputs():
    """Every logit of +-SATURATED with both target values.  9 < |x| < 18 is kept out: there 1 - sigmoid(x) has only a few bits in
    fp32 and one ulp of difference in the sigmoid moves the element's loss by percents — a property of the formula, not of an
    implementation."""
    xs = torch.tensor([s * v for v in SATURATED for s in (1.0, -1.0)], dtype=torch.float32)
    x = torch.cat([xs, xs])
    t = torch.cat([torch.zeros_like(xs), torch.ones_like(xs)])
    return x, t


def adam_ref(p, g, m, v, lr, b1, b2, eps, step):
    """One step of the fp64 Adam recurrence (torch.optim.Adam, no weight decay / amsgrad).  -> p, m, v"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    return p - lr / (1 - b1 ** step) * m / denom, m, v


def attn_ref(B, CE, HW, seed=51):
    z = rnd(B, 1, 1, HW, seed=seed)
    emb = rnd(B, CE, 1, HW, seed=seed + 1)
    dfuse = rnd(B, CE, 1, HW, seed=seed + 2)
    wb = torch.tensor([0.7, -0.2])
    z64, e64, wb64 = z.double().requires_grad_(True), emb.double().requires_grad_(True), wb.double().requires_grad_(True)
    att = torch.sigmoid(z64 * wb64[0] + wb64[1])
    (0.3 * e64 + att * e64).backward(dfuse.double())
    return {"z": z, "emb": emb, "dfuse": dfuse, "wb": wb, "att": att.detach().float(), "demb": e64.grad, "dz": z64.grad, "dwb": wb64.grad}
