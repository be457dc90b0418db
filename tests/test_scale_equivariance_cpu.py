"""Host half of the power-of-two equivariance tests (tests/scale_cases.py): the stock-fp32 oracle has the property, bit for bit, on
every (case, k) the GPU file runs — so a difference on the device is a property of the kernels or of their wiring, not of the inputs —
the restated scale rule maps 2^k a to 2^-k S(a), no gradient of the smallest k is subnormal, and the tables are consistent."""
import inspect

import pytest
import torch

import scale_cases as S


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("mode", S.MODES)
def test_oracle_calls_are_equivariant_in_the_gradient_scale(mode):
    """Section 1 on the host: backward of 2^k x loss for calls A and B; the forward does not depend on k, every gradient tensor is the
    k = 0 one x 2^k, and at k = -24 nothing is subnormal (so nothing is flushed on the device either)."""
    base = S.oracle_calls(0, mode)
    grads = [n for n in base if ".g." in n]
    assert len(grads) > 200 and {n[0] for n in grads} == {"A", "B"}
    for k in S.GRAD_KS:
        run = S.oracle_calls(k, mode)
        assert sorted(run) == sorted(base)
        bad = [n for n in base if not _same(run[n], base[n] * 2.0 ** k if ".g." in n else base[n])]
        assert not bad, "k = %d, %s: %d of %d tensors differ: %s" % (k, mode, len(bad), len(base), bad[:6])
        if k == min(S.GRAD_KS):
            sub = [n for n in grads if bool(S.is_subnormal(run[n]).any())]
            assert not sub, "subnormal gradient elements at k = %d: %s" % (k, sub[:6])
            assert all(bool((run[n] != 0).any()) for n in grads if bool((base[n] != 0).any()))


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("pair", sorted(S.PAIRS))
def test_oracle_blocks_are_equivariant_in_the_activation_scale(pair, mode):
    """Section 2 on the host, the concat pair included (stock fp32 shares no scale between the halves): output, dx, dprev unchanged,
    d gamma / d beta of the rescaled BatchNorm / f, the consumer's dW x f on the rescaled columns, every other gradient unchanged."""
    p = S.PAIRS[pair]
    sd = S.block_state(p.block)
    base = S.oracle_block(p.block, sd, mode)
    assert {"y", "dx", "g." + p.bn + ".weight", "g." + p.bn + ".bias", "g." + p.conv + ".weight"} <= set(base)
    assert ("dprev" in base) == (S.BLOCKS[p.block].prev is not None)
    for k in S.BLOCK_KS:
        run = S.oracle_block(p.block, S.rescale_state(sd, p, k), mode)
        fac = S.expected_factors(p, k, base)
        assert sorted(run) == sorted(base)
        # (the bias in front of a train-mode BatchNorm: the exact gradient is 0, the reference carries rounding noise there, and
        # noise is not equivariant — the HIP path never writes it)
        bad = [n for n in base if not (mode == "train" and S.pre_bn_bias(n)) and not _same(run[n], base[n] * fac[n])]
        assert not bad, "%s, k = %d, %s: %s" % (pair, k, mode, bad)
        assert not any(bool(S.is_subnormal(v).any()) for v in run.values())


def test_scale_rule_follows_a_power_of_two():
    """x3_scale_from_amax (restated in exact_cases.py): S(2^k a) = 2^-k S(a) for every k the GPU file uses, and a S(a) in [2^14, 2^15)."""
    g = torch.Generator().manual_seed(7)
    values = [1.0, 1.5, 2.0 - 2.0 ** -23, 2.0 ** -9, 3e-4, 17.25, 65504.0, 1e5] + [float(v) for v in torch.rand(16, generator=g) * 8 + 1e-3]
    for a in values:
        s = S.scale_from_amax(a)
        assert 2.0 ** 14 <= a * s < 2.0 ** 15
        for k in sorted(set(S.GRAD_KS) | set(S.BLOCK_KS) | {12, -12}):
            assert S.scale_from_amax(a * 2.0 ** k) == s * 2.0 ** -k, (a, k)


def test_tables_are_consistent():
    assert set(S.BITWISE_PAIRS) | {S.CONCAT_PAIR} == set(S.PAIRS) and S.CONCAT_PAIR not in S.BITWISE_PAIRS
    for name, p in S.PAIRS.items():
        sd = S.block_state(p.block)
        assert {p.bn + ".weight", p.bn + ".bias", p.conv + ".weight"} <= set(sd), name
        w = sd[p.conv + ".weight"]
        assert (p.lo is None) == (name != S.CONCAT_PAIR) and (p.lo is None or 0 < p.lo < w.shape[1])
        assert w.shape[1] - (p.lo or 0) == sd[p.bn + ".weight"].numel()          # the rescaled columns are the BatchNorm's channels
        r = S.rescale_state(sd, p, 5)
        changed = sorted(n for n in sd if not torch.equal(sd[n], r[n]))
        assert changed == sorted([p.bn + ".weight", p.bn + ".bias", p.conv + ".weight"])
    for b in S.BLOCKS.values():
        x, prev, dz = S.block_inputs(b.kind)
        assert tuple(x.shape) == b.x and tuple(dz.shape) == b.dz and (prev is None) == (b.prev is None)
    names = [n for n, _ in S.INPLACE_ENTRY_POINTS]
    assert len(set(names)) == len(names) and not set(names) & set(S.INPLACE_NOT_REACHABLE)
    for n, build in S.INPLACE_ENTRY_POINTS:
        assert list(inspect.signature(build).parameters) == ["o", "dev"], n
    assert all(abs(k) <= 24 for k in S.GRAD_KS) and 0 not in S.GRAD_KS and 0 not in S.BLOCK_KS
