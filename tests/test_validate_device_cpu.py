"""Host-side finishing of the device metrics (wtpse_hip/validate.py): HD95 from the two order statistics of the pooled squared
surface distances equals numpy.percentile(distances, 95) bit for bit, with the ranks taken from the restated virtual index."""
import numpy as np
import pytest

from wtpse_hip import validate as V


def test_hd95_from_order_stats_equals_np_percentile():
    rng = np.random.default_rng(11)
    for n in range(1, 5001):
        hi = int(rng.choice([2, 50, 5000, 1 << 20]))
        d2 = np.sort(rng.integers(0, hi, n))
        dist = np.sqrt(d2.astype(np.float64))                   # what distance_transform_edt returns at the surface pixels
        lo_rank, hi_rank, _ = V.percentile95_position(n)
        assert 0 <= lo_rank <= hi_rank <= n - 1 and hi_rank - lo_rank <= 1
        got = V.hd95_from_order_stats(n, int(d2[lo_rank]), int(d2[hi_rank]))
        want = float(np.percentile(dist, 95))
        assert got == want, (n, got, want)


@pytest.mark.parametrize("n", [1, 2, 19, 20, 21, 40, 100, 4096])
def test_percentile_ranks_bracket_the_virtual_index(n):
    lo, hi, gamma = V.percentile95_position(n)
    a = np.arange(n, dtype=np.float64)                          # percentile of 0..n-1 is the virtual index itself
    assert float(np.percentile(a, 95)) == V.hd95_from_order_stats(n, lo * lo, hi * hi)
    assert 0.0 <= gamma or lo == hi


def test_record_finishing_conventions():
    empty_pred = np.array([0, 0, 5, 0, 4, 0, 0, 0], np.int64)
    assert V._finish_surface(empty_pred) == (100.0, 100.0)
    with pytest.raises(RuntimeError, match="second supplied array"):
        V._finish_surface(np.array([0, 5, 0, 4, 0, 0, 0, 0], np.int64))
    assert V._finish_dice(np.array([3, 5, 4, 0, 0, 0, 0, 0], np.int64)) == (2 * 3.0 + 1.0) / (1.0 + 5.0 + 4.0)
    with pytest.raises(ValueError):
        V.Validator(metrics="gpu")
