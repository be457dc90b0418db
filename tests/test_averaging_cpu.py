"""Dense weight averaging without a GPU (wtpse_hip/averaging.py): the loss-valley policy against a brute-force restatement that
keeps every segment, the accuracy of the running-mean arithmetic against float64, and the two C-ABI prototypes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

from wtpse_hip.averaging import LossValley, avg_merge_spec, avg_step_spec  # noqa: E402

SHAPES = [(1, 1), (2, 2), (3, 6), (4, 2)]          # (Ns, Ne)
N = 5                                              # elements of a segment's one array


# ------------------------------------------------------------------------------------------------ the restatement
def brute_force(losses, segments, counts, Ns, Ne, ratio):
    """Every segment kept; s and t from the full loss list by their definitions; avg_merge_spec folded in index order.
    -> (array, info)."""
    n = len(losses)
    s = next((i for i in range(n - Ns + 1) if all(losses[i] <= losses[j] for j in range(i, i + Ns))), None)
    if s is None:
        return segments[-1].copy(), dict(converged=False, start=None, end=None, iterates=counts[-1], threshold=None)
    T = ratio * float(np.mean(np.asarray(losses[s:s + Ns], dtype=np.float64)))
    t = next((i for i in range(s + 1, n - Ne + 1) if min(losses[i:i + Ne]) > T), None)
    last = n if t is None else t
    acc, total = None, 0
    for i in range(s, last):
        acc = avg_merge_spec(acc, segments[i], total, counts[i])
        total += counts[i]
    return acc, dict(converged=True, start=s, end=t, iterates=total, threshold=T)


def drive(losses, segments, counts, Ns, Ne, ratio, reload_at=None):
    """The streaming policy over the same evaluations.  reload_at: after that many observations the state moves into a new object.
    -> (array, info, most segments ever held, the object)."""
    v = LossValley(Ns, Ne, ratio)
    most = 0
    for e, (l, seg, c) in enumerate(zip(losses, segments, counts)):
        if reload_at is not None and e == reload_at:
            state = v.state()
            v = LossValley(Ns, Ne, ratio)
            v.load_state(state)
        v.observe([seg.copy()], c, l, 10 * (e + 1))
        most = max(most, v.held)
    tensors, info = v.result()
    return tensors[0], info, most, v


def check(losses, counts, Ns, Ne, ratio=1.5, seed=0):
    rng = np.random.RandomState(seed)
    segments = [rng.standard_normal(N).astype(np.float32) for _ in losses]
    want, winfo = brute_force(list(losses), segments, list(counts), Ns, Ne, ratio)
    got, info, most, v = drive(losses, segments, counts, Ns, Ne, ratio)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (losses, counts, Ns, Ne, info, winfo)
    for k, val in winfo.items():
        assert info[k] == val, (k, info[k], val, losses)
    assert info["losses"] == [float(l) for l in losses][:info["evaluations"]]
    assert v.closed == (winfo["end"] is not None)
    assert most <= max(Ns, Ne), (most, Ns, Ne)
    # result() modifies nothing: asked twice, the same bits
    assert v.result()[0][0].tobytes() == got.tobytes()
    for at in sorted({1, len(losses) // 2, len(losses) - 1}):
        if 0 < at < len(losses):
            again, info2, _, _ = drive(losses, segments, counts, Ns, Ne, ratio, reload_at=at)
            assert again.tobytes() == want.tobytes() and info2 == info, ("reload at", at)
    return info


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("Ns,Ne", SHAPES)
def test_valley_against_brute_force_random(Ns, Ne):
    """A hundred seeded random loss sequences per (Ns, Ne): a noisy descent, a floor, a noisy rise of random lengths, random counts."""
    rng = np.random.RandomState(100 * Ns + Ne)
    seen = {"converged": 0, "closed": 0, "open": 0, "never": 0}
    for trial in range(100):
        n = int(rng.randint(1, 30))
        down, up = int(rng.randint(0, n + 1)), int(rng.randint(0, n + 1))
        base = np.concatenate([np.linspace(2.0, 1.0, down), np.ones(max(n - down - up, 0)), np.linspace(1.0, 3.0, up)])[:n]
        base = np.pad(base, (0, n - len(base)), constant_values=1.0)
        losses = [float(x) for x in base + rng.choice([0.0, 0.05, 0.4]) * rng.standard_normal(n)]
        if trial % 7 == 0:
            losses = [round(l, 1) for l in losses]            # ties
        counts = [int(c) for c in rng.randint(1, 9, size=n)]
        info = check(losses, counts, Ns, Ne, ratio=float(rng.choice([1.0, 1.2, 1.5])), seed=trial)
        seen["converged" if info["converged"] else "never"] += 1
        if info["converged"]:
            seen["closed" if info["end"] is not None else "open"] += 1
    # the draw reaches every outcome (with Ns = 1 evaluation 0 is always a start: "never" cannot occur)
    assert all(v > 0 for k, v in seen.items() if not (Ns == 1 and k == "never")), seen


def test_valley_edge_cases():
    # never converges: strictly falling losses, no index is the minimum of a window of 3 -> the last segment alone
    info = check([5.0, 4.0, 3.0, 2.0, 1.0], [2, 3, 4, 5, 6], 3, 6)
    assert info == dict(info, converged=False, start=None, end=None, iterates=6, threshold=None)
    # fewer evaluations than a window
    info = check([1.0, 2.0], [1, 1], 3, 6)
    assert not info["converged"] and info["iterates"] == 1
    # a start found at the last evaluation: the result is S_s .. the last segment
    info = check([3.0, 2.0, 1.0, 1.5, 1.25], [1, 2, 3, 4, 5], 3, 6)
    assert (info["start"], info["end"], info["iterates"]) == (2, None, 12)
    assert info["threshold"] == 1.5 * float(np.mean(np.array([1.0, 1.5, 1.25])))
    # an end found immediately after the start: t = s + 1, decided inside the converging window (Ne < Ns) -> S_s alone
    info = check([1.0, 9.0, 9.0, 9.0, 9.0], [7, 1, 1, 1, 1], 4, 2, ratio=1.0)
    assert (info["start"], info["end"], info["iterates"]) == (0, 1, 7)
    info = check([1.0, 5.0], [3, 4], 1, 1)
    assert (info["start"], info["end"], info["iterates"]) == (0, 1, 3)
    # ties: l_s <= l_j holds with equality, and a loss EQUAL to the threshold is not above it
    info = check([2.0, 2.0, 2.0, 3.0, 3.0, 3.0, 3.5, 3.5], [1] * 8, 3, 2)
    assert (info["start"], info["threshold"], info["end"], info["iterates"]) == (0, 3.0, 6, 6)
    # a run that ends with the valley open: one loss above the threshold, but never Ne in a row
    info = check([1.0, 1.0, 1.0, 9.0, 1.0, 9.0, 1.0], [2] * 7, 2, 2)
    assert (info["start"], info["end"], info["iterates"]) == (0, None, 14)
    # observations behind a closed valley are ignored
    v = LossValley(1, 1, 1.5)
    for e, l in enumerate([1.0, 5.0, 0.1, 0.1]):
        v.observe([np.full(N, l, np.float32)], 1, l, e)
    assert v.closed and v.result()[1]["evaluations"] == 2 and v.held == 0
    assert [r[3] for r in v.table()] == ["merged", "outside"]
    with pytest.raises(ValueError, match="nothing to average"):
        LossValley().result()
    with pytest.raises(ValueError, match="at least one"):
        LossValley().observe([np.zeros(N, np.float32)], 0, 1.0)
    assert LossValley().config() == {"n_converge": 3, "n_tolerance": 6, "tolerance_ratio": 1.5}     # the reference's config.yaml


def test_valley_table_and_state_are_plain():
    v = LossValley(2, 3, 1.5)
    for e, l in enumerate([2.0, 1.0, 1.0, 1.2, 1.1]):
        v.observe([np.full(N, e, np.float32)], 2, l, 2 * (e + 1))
    assert [r[3] for r in v.table()] == ["outside", "merged", "merged", "held", "held"]
    assert [r[:3] for r in v.table()][1] == [1, 4, 1.0]
    st = v.state()
    assert st["held_index"] == [3, 4] and st["n_final"] == 4 and st["start"] == 1 and not st["closed"]
    other = LossValley(2, 2, 1.5)
    with pytest.raises(ValueError, match="saved valley"):
        other.load_state(st)


# the distance measured below on the CPU against float64 (seed 0: 3.352e-06, recorded in profiles/averaging.md — weights up to
# |4|, one ulp there is 4.8e-07, a thousand rounded folds); asserted at 4x to cover other seeds
MEASURED_MAX_ERR = 3.352e-6


def test_avg_step_spec_accuracy():
    """1000 iterates of a random walk with 1e-3-sized steps around O(1) weights, folded by avg_step_spec, against the float64 mean of
    the same fp32 iterates.  The bound is the measured distance times four (the measurement: this test, printed)."""
    rng = np.random.RandomState(0)
    p = rng.standard_normal(4096).astype(np.float32)
    a = np.full_like(p, np.float32(np.nan))              # whatever the buffer held is ignored: k == 1 copies
    total = np.zeros(p.shape, np.float64)
    for k in range(1, 1001):
        p = (p + np.float32(1e-3) * rng.standard_normal(p.shape).astype(np.float32)).astype(np.float32)
        a = avg_step_spec(a, p, k)
        total += p.astype(np.float64)
    err = float(np.max(np.abs(a.astype(np.float64) - total / 1000.0)))
    print("avg_step_spec: max |fp32 running mean - float64 mean| over 4096 weights x 1000 iterates = %.3e" % err)
    assert a.dtype == np.float32
    assert err <= 4 * MEASURED_MAX_ERR, err


def test_specs_are_separately_rounded():
    """Operands chosen so that a fused multiply-add, or a reciprocal in place of the division, would give other bits."""
    a, p = np.float32(1.0), np.float32(1.0 + 3 * 2.0 ** -23)
    got = avg_step_spec(np.array([a]), np.array([p]), 3)[0]
    assert got == np.float32(a + np.float32(np.float32(p - a) / np.float32(3)))
    acc, seg = np.array([np.float32(1.0)]), np.array([np.float32(1.0 + 2.0 ** -12)])
    w = np.float32(5.0 / 8.0)
    got = avg_merge_spec(acc, seg, 3, 5)[0]
    assert got == np.float32(acc[0] + np.float32(np.float32(seg[0] - acc[0]) * w))
    assert avg_merge_spec(acc, seg, 0, 7)[0] == seg[0] and avg_step_spec(acc, seg, 1)[0] == seg[0]
    # the weight is formed in double and rounded once
    third = avg_merge_spec(np.zeros(1, np.float32), np.ones(1, np.float32), 2, 1)[0]
    assert third == np.float32(1.0 / 3.0)


def test_header_declares_the_two_entry_points():
    """Both prototypes parse, every argument type has a PlanArg slot, and both are recordable (they end with a stream)."""
    from wtpse_hip import build
    from wtpse_hip.lib import PlanArg
    protos = build.parse_prototypes()
    assert protos["wtpse_avg_step"] == ["float*", "const float*", "long long"] * 4 + ["int*", "const int*", "const int*", "void*"]
    assert protos["wtpse_avg_merge"] == ["float*", "const float*", "long long", "long long", "long long", "void*"]
    fields = {name for name, _ in PlanArg._fields_}
    for name in ("wtpse_avg_step", "wtpse_avg_merge"):
        for t in protos[name]:
            assert build.C_TYPES["void*" if "*" in t else t][1] in fields, (name, t)
        assert len(protos[name]) - 1 <= 40           # csrc/plan.hip: argument slots of one recorded call
