"""Every dispatch branch of csrc/dwt.hip (-m gpu) at fp32-grade bounds.

The cases, their inputs, the float64 oracle, the fp32 yardstick and the branch each case is there for live in dwt_cases.py;
test_dwt_paths_cpu.py proves on the host that each case takes that branch and that the bound rejects wrong transforms.  Here
every call goes through ops.lib().call("wtpse_dwt2_fwd" / "wtpse_dwt2_inv") on buffers between guards (test_dispatch_paths_gpu's
out / dev / guards_ok): the outputs pre-filled with the NaN sentinel, `tmp` at exactly its contract size, the input guarded too.
A measured figure is printed before it is asserted (profiles/dwt_paths.md records them)."""
import numpy as np
import pytest
import torch

import dwt_cases as C
from test_dispatch_paths_gpu import L, P, S, dev, guards_ok, out

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF
BOTH = ["haar", "db2"]


def bits(t):
    return t.contiguous().view(torch.int32)


def untouched(t):
    return bool((bits(t) == NAN_BITS).all())


def tmp_for(shape, off=0):
    B, Ch, H, W = shape
    return out((2 * B * Ch * (H // 2) * (W // 2),), off)        # exactly the contract size of include/wtpse_hip.h


def forward(x, wavelet, levels, offs=(0, 0, 0)):
    """wtpse_dwt2_fwd on guarded buffers -> the coefficient tensor (on the device, still inside its guards)."""
    x = torch.from_numpy(np.ascontiguousarray(x))
    B, Ch, H, W = x.shape
    xd, coef, tmp = dev(x, offs[0]), out(x.shape, offs[1]), tmp_for(x.shape, offs[2])
    L().call("wtpse_dwt2_fwd", P(xd), P(coef), P(tmp), B * Ch, H, W, C.WAVELETS[wavelet], levels, S())
    guards_ok(coef, tmp, xd)
    assert torch.equal(bits(xd).cpu(), bits(x)), "the input changed"
    assert not bool((bits(coef) == NAN_BITS).any()), "a coefficient was not written"
    assert bool(torch.isfinite(coef).all())
    return coef


def inverse(coef, wavelet, levels, offs=(0, 0, 0)):
    """wtpse_dwt2_inv on guarded buffers; coef: numpy float32 or a device tensor."""
    c = torch.from_numpy(np.ascontiguousarray(coef)) if isinstance(coef, np.ndarray) else coef
    B, Ch, H, W = c.shape
    cd, x, tmp = dev(c, offs[1]), out(c.shape, offs[0]), tmp_for(c.shape, offs[2])
    before = bits(cd).clone()
    L().call("wtpse_dwt2_inv", P(cd), P(x), P(tmp), B * Ch, H, W, C.WAVELETS[wavelet], levels, S())
    guards_ok(x, tmp, cd)
    assert torch.equal(bits(cd), before), "the coefficients changed"
    assert not bool((bits(x) == NAN_BITS).any()), "a pixel was not written"
    assert bool(torch.isfinite(x).all())
    return x


def check_forward(coef, r, levels, path, what):
    rows = C.band_ratios(coef.cpu().numpy(), r["ref"], r["yard"], levels)
    lv, nm, ratio, err, yb, top, _ = C.worst(rows)
    print("DWT-RATIO fwd %s: worst err_band / max(yard_band, 2^-24 max|ref_band|) = %.2f (level %d %s: err %.3g, yard %.3g, max %.3g)"
          % (what, ratio, lv, nm, err, yb, top))
    thick = [t for t in rows if t[6] >= C.THIN_BAND]
    if thick and len(thick) < len(rows):
        print("DWT-RATIO fwd %s, bands of >= %d coefficients: %.2f" % (what, C.THIN_BAND, C.worst(thick)[2]))
    assert not C.over_bound(rows, path), (what, C.over_bound(rows, path))


@pytest.mark.parametrize("wavelet", BOTH)
@pytest.mark.parametrize("name", list(C.CASES))
def test_forward_paths(name, wavelet):
    c = C.CASES[name]
    br = C.case_branch(name)
    assert C.matches(br, c["expect"]) is None
    r = C.reference(name, wavelet)
    coef = forward(r["x"], wavelet, c["levels"], c["offs"])
    check_forward(coef, r, c["levels"], br["path"], "%s %s %s" % (br["path"], wavelet, name))


@pytest.mark.parametrize("wavelet", BOTH)
@pytest.mark.parametrize("name", list(C.CASES))
def test_inverse_paths(name, wavelet):
    """The inverse is always the generic kernel: the 256 / 512 cases give it gridDim.y = 2 and 4, 144 x 16 the half-empty block."""
    c = C.CASES[name]
    assert C.case_branch(name, "inv")["path"] == "generic"
    r = C.reference(name, wavelet)
    x = inverse(r["coef32"], wavelet, c["levels"], c["offs"])
    ratio, err, yd = C.image_ratio(x.cpu().numpy(), r["x"], r["inv_yard"])
    print("DWT-RATIO inv generic %s %s: err / max(yard, 2^-24 max|x|) = %.2f (err %.3g, yard %.3g)" % (wavelet, name, ratio, err, yd))
    assert ratio <= C.K, (name, wavelet, ratio)
    y = inverse(forward(r["x"], wavelet, c["levels"], c["offs"]), wavelet, c["levels"])
    ratio, err, yd = C.image_ratio(y.cpu().numpy(), r["x"], r["trip_yard"])
    print("DWT-RATIO trip %s %s %s: err / max(yard, 2^-24 max|x|) = %.2f (err %.3g, yard %.3g)"
          % (C.case_branch(name)["path"], wavelet, name, ratio, err, yd))
    assert ratio <= C.K, (name, wavelet, "round trip", ratio)


@pytest.mark.parametrize("wavelet", BOTH)
def test_alignment_fallback_agrees_with_the_streaming_path(wavelet):
    """x, then coef, then tmp 8 bytes past a 16-byte boundary: the generic kernels, within the bound of the oracle (test_forward_paths)
    and within twice the bound of the aligned run of the same input.  The two paths round differently: no bitwise comparison."""
    a = C.CASES["256_L3_aligned"]
    assert C.case_branch("256_L3_aligned")["path"] == "fast256"
    r = C.reference("256_L3_aligned", wavelet)
    fast = forward(r["x"], wavelet, a["levels"]).cpu().numpy()
    for name in C.ALIGNMENT_CASES:
        c = C.CASES[name]
        assert C.case_branch(name)["path"] == "generic" and C.case_branch(name)["why"].startswith("align:")
        slow = forward(r["x"], wavelet, c["levels"], c["offs"])
        check_forward(slow, r, c["levels"], "generic", "generic %s %s" % (wavelet, name))
        rows = C.band_ratios(slow.cpu().numpy(), r["ref"], r["yard"], c["levels"], against=fast)
        lv, nm, ratio = C.worst(rows)[:3]
        print("DWT-RATIO generic against fast256, %s %s: %.2f (level %d %s)" % (wavelet, name, ratio, lv, nm))
        assert ratio <= 2 * max(C.K_FWD["generic"], C.K_FWD["fast256"]), (name, wavelet, ratio)


@pytest.mark.parametrize("wavelet", BOTH)
@pytest.mark.parametrize("name", C.INDEPENDENCE_CASES)
def test_a_plane_does_not_depend_on_its_neighbours(name, wavelet):
    """Plane p of the batched call is, bitwise, the one-plane call on that plane alone: first, middle, last; forward and inverse."""
    c = C.CASES[name]
    r = C.reference(name, wavelet)
    H, W = c["shape"][2:]
    x = r["x"].reshape(1, -1, H, W)
    c32 = r["coef32"].reshape(1, -1, H, W)
    n = x.shape[1]
    fwd, inv = forward(x, wavelet, c["levels"]), inverse(c32, wavelet, c["levels"])
    for p in (0, n // 2, n - 1):
        assert torch.equal(bits(forward(x[:, p:p + 1], wavelet, c["levels"])), bits(fwd[:, p:p + 1])), (name, wavelet, p, "forward")
        assert torch.equal(bits(inverse(c32[:, p:p + 1], wavelet, c["levels"])), bits(inv[:, p:p + 1])), (name, wavelet, p, "inverse")


@pytest.mark.parametrize("name", C.REPEAT_CASES)
def test_forward_is_repeatable(name):
    c = C.CASES[name]
    assert [C.case_branch(n)["path"] for n in C.REPEAT_CASES] == ["generic", "fast256", "fast512"]
    for wavelet in BOTH:
        x = C.reference(name, wavelet)["x"]
        assert torch.equal(bits(forward(x, wavelet, c["levels"])), bits(forward(x, wavelet, c["levels"]))), (name, wavelet)


@pytest.mark.parametrize("n", C.RAMP_SIZES)
def test_ramp_details_vanish(n):
    """db2, one level, x = a r + b c + c0: the detail coefficients at least two pairs from the periodic seam are rounding alone —
    within K x what the fp32 restatement leaves there (test_dwt_paths_cpu.py).  64 x 64: generic; 256 x 256: the streaming path."""
    assert C.fwd_branch(1, n, n, 1)["path"] == ("fast256" if n == 256 else "generic")
    coef = forward(C.ramp_input(n), "db2", 1).cpu().numpy()
    got, yard = float(np.abs(C.ramp_interior(coef)).max()), C.ramp_yardstick(n)
    print("DWT-RATIO ramp %d: max|detail| %.3g, fp32 restatement %.3g, ratio %.2f" % (n, got, yard, got / yard))
    assert got <= C.K * yard, (n, got, yard)


def test_refusals_leave_the_outputs_alone():
    """Every WTPSE_REQUIRE of the two entry points returns before a launch: WtpseError, and the sentinel-filled outputs and `tmp`
    still hold nothing but the sentinel.  A pointer at an odd float offset is refused, never launched."""
    from wtpse_hip.lib import WtpseError
    shape = (1, 2, 32, 64)
    x = torch.from_numpy(np.ascontiguousarray(C.case_input("planes")[:1, :2]))
    assert tuple(x.shape) == shape
    ok = dict(planes=2, H=32, W=64, wavelet=1, levels=2)
    bad = [dict(H=34), dict(W=66), dict(levels=0), dict(levels=13), dict(wavelet=2), dict(planes=0), dict(planes=65536),
           dict(same=True), dict(null=0), dict(null=1), dict(null=2), dict(offs=(1, 0, 0)), dict(offs=(0, 1, 0)), dict(offs=(0, 0, 1))]
    for entry in ("wtpse_dwt2_fwd", "wtpse_dwt2_inv"):
        for b in bad:
            a = dict(ok, **{k: v for k, v in b.items() if k in ok})
            offs = b.get("offs", (0, 0, 0))
            assert not C.accepted(offs=offs, same=b.get("same", False), null="null" in b, **a), b
            src, dst, tmp = dev(x, offs[0]), out(shape, offs[1]), tmp_for(shape, offs[2])
            ptrs = [P(src), P(src) if b.get("same") else P(dst), P(tmp)]
            if "null" in b:
                ptrs[b["null"]] = 0
            with pytest.raises(WtpseError):
                L().call(entry, ptrs[0], ptrs[1], ptrs[2], a["planes"], a["H"], a["W"], a["wavelet"], a["levels"], S())
            torch.cuda.synchronize()
            guards_ok(src, dst, tmp)
            assert untouched(dst) and untouched(tmp), (entry, b)
            assert torch.equal(bits(src).cpu(), bits(x)), (entry, b)
        # and the same call with nothing wrong goes through
        src, dst, tmp = dev(x), out(shape), tmp_for(shape)
        L().call(entry, P(src), P(dst), P(tmp), ok["planes"], ok["H"], ok["W"], ok["wavelet"], ok["levels"], S())
        guards_ok(src, dst, tmp)
        assert bool(torch.isfinite(dst).all())
