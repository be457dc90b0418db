"""wtpse_hip/views.py on the host: the eight view codes and their inverses, the named sets of `parse`, merge_host (the specification
of wtpse_views_merge) on a hand-made 2 x 2 case with every output written out, the refusals of the two C entry points (no launch is
made without a GPU) and the limits of Segmenter(views=...)."""
import ctypes
import math

import numpy as np
import pytest

from wtpse_hip import views as VW

ASYM = np.arange(9, dtype=np.float32).reshape(3, 3)          # no symmetry of the square leaves it alone


def test_unview_inverts_view_and_the_inverse_code():
    x = np.random.default_rng(1).standard_normal((2, 3, 5, 5)).astype(np.float32)
    for c in range(8):
        assert np.array_equal(VW.unview_host(VW.view_host(x, c), c), x)
        assert np.array_equal(VW.view_host(VW.unview_host(x, c), c), x)
        assert np.array_equal(VW.view_host(x, VW.inverse(c)), VW.unview_host(x, c))
    assert [VW.inverse(c) for c in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]


def test_the_eight_views_are_distinct_and_defined_by_numpy():
    seen = {VW.view_host(ASYM, c).tobytes() for c in range(8)}
    assert len(seen) == 8
    assert np.array_equal(VW.view_host(ASYM, 0), ASYM)
    assert np.array_equal(VW.view_host(ASYM, 1), ASYM[:, ::-1])
    assert np.array_equal(VW.view_host(ASYM, 2), ASYM[::-1])
    assert np.array_equal(VW.view_host(ASYM, 3), ASYM[::-1, ::-1])
    assert np.array_equal(VW.view_host(ASYM, 4), ASYM.T)
    assert np.array_equal(VW.view_host(ASYM, 5), ASYM.T[:, ::-1]) and np.array_equal(VW.view_host(ASYM, 5), np.rot90(ASYM, -1))
    assert np.array_equal(VW.view_host(ASYM, 6), ASYM.T[::-1]) and np.array_equal(VW.view_host(ASYM, 6), np.rot90(ASYM, 1))
    assert np.array_equal(VW.view_host(ASYM, 7), ASYM.T[::-1, ::-1])
    for c in range(8):
        rows = [sorted(r) for r in VW.view_host(ASYM, c).tolist()]
        is_row = all(r in [sorted(q) for q in ASYM.tolist()] for r in rows)
        assert is_row == (c < 4)                             # codes 0..3 leave a row's content a row, 4..7 make it a column
    for bad in (8, -1, 1.0, True, "1"):
        with pytest.raises(ValueError):
            VW.view_host(ASYM, bad)


def test_parse():
    assert VW.parse(None) is None and VW.parse("none") is None and VW.parse(" None ") is None
    assert VW.parse("id") == (0,) and VW.parse("hflip") == (0, 1) and VW.parse("flips") == (0, 1, 2, 3)
    assert VW.parse("d4") == tuple(range(8)) and VW.parse("D4") == tuple(range(8))
    assert VW.parse("0,5, 3") == (0, 5, 3) and VW.parse((0, 6)) == (0, 6) and VW.parse([0]) == (0,) and VW.parse("0") == (0,)
    assert VW.parse(np.array([0, 7])) == (0, 7)
    for bad in ("", "all", "1,0", "1", "0,0", "0,8", "0,-1", "0,1.5", "0,,1", (1, 0), (0, 1, 1), (), (0, 8), 3, (0, 1.0),
                "0,1,2,3,4,5,6,7,0"):
        with pytest.raises(ValueError):
            VW.parse(bad)


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_merge_host_hand_made_case():
    l0 = np.array([[0.0, 2.0], [-1.0, 3.0]], np.float32)                      # view 0: the picture's own frame
    u1 = np.array([[1.0, 2.0], [4.0, -3.0]], np.float32)                      # view 1's map as it should come back
    in1 = np.array([[4.0, 1.0], [-3.0, 2.0]], np.float32)                     # ... and as code 5 presents it: u1.T, columns reversed
    assert np.array_equal(VW.view_host(u1, 5), in1)
    res = VW.merge_host(np.stack((l0, in1)).reshape(2, 1, 1, 2, 2), (0, 5))
    assert res["logits"].shape == (1, 2, 2, 2) and res["logits"].dtype == np.float32
    assert np.array_equal(res["logits"][0, 0], l0) and np.array_equal(res["logits"][0, 1], u1)
    assert res["mean_logit"].dtype == np.float32 and res["mean_logit"].tolist() == [[[0.5, 2.0], [1.5, 0.0]]]
    assert res["votes"].dtype == np.uint8 and res["votes"].tolist() == [[[0, 2], [1, 1]]]     # ln 3 = 1.0986: 2, 3 and 4 vote
    for (i, j) in ((0, 0), (0, 1), (1, 0), (1, 1)):
        p0, p1 = _sig(float(l0[i, j])), _sig(float(u1[i, j]))
        assert res["mean"][0, i, j] == pytest.approx((p0 + p1) / 2, abs=1e-15)
        assert res["std"][0, i, j] == pytest.approx(abs(p0 - p1) / 2, abs=1e-15)
    assert res["std"][0, 0, 1] == 0.0 and res["mean"].dtype == np.float64
    # a threshold of its own
    assert VW.merge_host(np.stack((l0, in1)).reshape(2, 1, 1, 2, 2), (0, 5), threshold=0.5)["votes"].tolist() == [[[1, 2], [1, 1]]]


def test_merge_host_equal_samples_and_single_map():
    r = np.random.default_rng(2)
    x = (2.0 * r.standard_normal((2, 6, 6))).astype(np.float32)
    K = 3
    # the same map under every view, K times each: every un-viewed sample is x, the spread is exactly 0
    logits = np.stack([np.repeat(VW.view_host(x, c)[:, None], K, 1) for c in range(8)])
    res = VW.merge_host(logits, range(8))
    assert all(np.array_equal(res["logits"][:, s], x) for s in range(8 * K))
    assert np.all(res["std"] == 0.0)
    assert np.all((res["votes"] == 0) | (res["votes"] == 8 * K)) and (res["votes"] == 0).any() and (res["votes"] == 8 * K).any()
    # V = K = 1: the mean logit is the input, bit for bit (a negative zero included)
    x[0, 0, 0] = -0.0
    one = VW.merge_host(x.reshape(1, 2, 1, 6, 6), (0,))
    assert one["mean_logit"].tobytes() == x.tobytes() and np.all(one["std"] == 0.0)
    # the float32 sum is sequential in order of s: not the pairwise sum, not the float64 mean rounded
    big = np.array([1e8, 1.0, -1e8, 1.0], np.float32).reshape(4, 1, 1, 1, 1) * np.ones((1, 1, 1, 4, 4), np.float32)
    assert np.all(VW.merge_host(big, (0, 1, 2, 3))["mean_logit"] == np.float32(0.25))
    with pytest.raises(ValueError):
        VW.merge_host(np.zeros((2, 1, 1, 4, 4), np.float32), (0,))
    with pytest.raises(ValueError):
        VW.merge_host(np.zeros((1, 1, 1, 4, 6), np.float32), (0,))
    with pytest.raises(ValueError):
        VW.merge_host(np.zeros((5, 1, 13, 4, 4), np.float32), (0, 1, 2, 3, 4))


def test_argument_checks_come_before_any_launch():
    from wtpse_hip import build
    from wtpse_hip.lib import lib
    build.build()
    gen, merge = lib().raw("wtpse_dihedral_views"), lib().raw("wtpse_views_merge")
    P = 4096                                               # never dereferenced: every call below is refused on its arguments
    good = (ctypes.c_int * 9)(0, 1, 2, 3, 4, 5, 6, 7, 0)
    bad = (ctypes.c_int * 9)(0, 1, 8, 3, 4, 5, 6, 7, 0)
    neg = (ctypes.c_int * 9)(0, -1, 2, 3, 4, 5, 6, 7, 0)
    A = ctypes.addressof

    def g(x=P, out=P, codes=A(good), V=8, N=6, S=20):
        return gen(x, out, codes, V, N, S, 0)

    def m(logits=P, codes=A(good), V=8, B=2, K=3, S=20, logits_out=P, mean=P, std=P, votes=P, mean_logit=P):
        return merge(logits, codes, V, B, K, S, 0.75, logits_out, mean, std, votes, mean_logit, 0)

    assert g(x=0) == -1 and g(out=0) == -1 and g(codes=0) == -1
    assert g(codes=A(bad)) == -1 and g(codes=A(neg)) == -1
    assert g(V=9) == -1 and g(V=0) == -1 and g(N=0) == -1
    assert g(S=18) == -1 and g(S=0) == -1
    assert g(x=P + 4) == -1 and g(out=P + 8) == -1
    assert m(logits=0) == -1 and m(codes=0) == -1 and m(mean=0) == -1 and m(std=0) == -1 and m(votes=0) == -1
    assert m(codes=A(bad)) == -1 and m(codes=A(neg)) == -1
    assert m(V=9) == -1 and m(V=0) == -1 and m(K=0) == -1 and m(B=0) == -1
    assert m(V=5, K=13) == -1 and m(V=8, K=9) == -1 and m(V=1, K=65) == -1
    assert m(S=18) == -1 and m(S=0) == -1
    for k in ("logits", "logits_out", "mean", "std", "mean_logit"):
        assert m(**{k: P + 4}) == -1, k
    assert m(votes=P + 2) == -1


def test_segmenter_limits(tmp_path):
    from wtpse_hip.segment import Segmenter
    mk = lambda **kw: Segmenter(None, None, None, None, out_dir=str(tmp_path), **kw)
    assert mk().views is None and mk(views="none").views is None and mk().n_maps == 0 and mk(samples=4).n_maps == 4
    assert mk(views="d4").views == tuple(range(8)) and mk(views="d4").n_maps == 8
    assert mk(views="d4", samples=8).n_maps == 64 and mk(views=(0, 5), samples=3).n_maps == 6 and mk(views="id").n_maps == 1
    with pytest.raises(ValueError):
        mk(views="d4", samples=9)                          # 72 maps
    with pytest.raises(ValueError):
        mk(views="hflip", samples=33)
    with pytest.raises(ValueError):
        mk(views="d4", batch_size=512)                     # 2 * 512 * 8 records in one set of post-processing launches
    with pytest.raises(ValueError):
        mk(views="hflip", samples=8, batch_size=256)
    assert mk(views="d4", batch_size=511).batch_size == 511
    with pytest.raises(ValueError):
        mk(views="1,0")
    with pytest.raises(ValueError):
        mk(views="quarter")


def test_calibration_run_limits(tmp_path):
    from wtpse_hip.calibration_run import CalibrationRun, parse_args
    mk = lambda **kw: CalibrationRun(None, None, None, None, out_dir=str(tmp_path), **kw)
    assert mk().views is None and mk(views="hflip", samples=32).views == (0, 1)
    with pytest.raises(ValueError):
        mk(views="hflip", samples=33)
    base = ["--data-dir", "d", "--datasetTest", "1", "--checkpoint", "c", "--out", "o"]
    assert parse_args(base).views is None and parse_args(base + ["--views", "flips"]).views == (0, 1, 2, 3)
    with pytest.raises(SystemExit):
        parse_args(base + ["--views", "d4"])               # 8 x the default 16 samples
    with pytest.raises(SystemExit):
        parse_args(base + ["--views", "2,0"])
