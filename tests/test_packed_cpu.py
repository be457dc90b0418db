"""packed.fetch on CPU tensors (torch.cat and .cpu() work there): every array equals its source in dtype, shape and value wherever it
starts in the packed bytes, and the number of .cpu() calls is the number of copies the docstrings promise."""
import numpy as np
import pytest
import torch

from wtpse_hip.packed import fetch


@pytest.fixture
def cpu_calls(monkeypatch):
    calls, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **kw: calls.append(tuple(self.shape)) or real(self, *a, **kw))
    return calls


def _sources():
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, 7).astype(np.uint8),                              # odd length: everything behind it is misaligned
            rng.integers(-2 ** 62, 2 ** 62, (2, 8)).astype(np.int64),
            rng.standard_normal((2, 1, 3, 5)).astype(np.float32),
            rng.integers(0, 2 ** 32, (3, 4)).astype(np.uint32)]


def _address(a):
    return a.__array_interface__["data"][0]


def _check(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (g.dtype, g.shape, w.dtype, w.shape)


def test_misaligned_pieces_come_back_whole(cpu_calls):
    src = _sources()
    got = fetch([torch.from_numpy(a) for a in src])
    _check(got, src)
    assert len(cpu_calls) == 1 and cpu_calls[0] == (7 + 128 + 120 + 48,)
    # offsets 7, 135 and 255 are no multiples of 8 / 4 / 4: copies, aligned, not views into the fetched bytes
    assert all(g.flags.aligned for g in got) and all(_address(g) - _address(got[0]) != off for g, off in zip(got[1:], (7, 135, 255)))


def test_aligned_pieces_are_views_of_one_buffer(cpu_calls):
    src = [np.arange(16, dtype=np.int64).reshape(2, 8), np.arange(8, dtype=np.uint8), np.arange(6, dtype=np.float32).reshape(1, 2, 3)]
    got = fetch([torch.from_numpy(a) for a in src])
    _check(got, src)
    assert len(cpu_calls) == 1
    assert [_address(g) - _address(got[0]) for g in got] == [0, 128, 136]


def test_zero_element_tensor_in_the_middle(cpu_calls):
    src = _sources()
    src.insert(2, np.zeros((3, 0, 2), np.float32))
    src.insert(4, np.zeros((0,), np.int64))
    _check(fetch([torch.from_numpy(a) for a in src]), src)
    assert len(cpu_calls) == 1
    _check(fetch([torch.zeros(0, 4), torch.zeros(2, 0, dtype=torch.int64)]), [np.zeros((0, 4), np.float32), np.zeros((2, 0), np.int64)])
    assert len(cpu_calls) == 1                                                     # nothing to copy: no copy


def test_non_contiguous_input(cpu_calls):
    base = torch.arange(7 * 6, dtype=torch.int32).reshape(7, 6)
    parts = [torch.arange(3, dtype=torch.uint8), base[:, ::2], base.t(), torch.arange(24, dtype=torch.float64).reshape(2, 3, 4).permute(2, 0, 1)]
    assert not any(p.is_contiguous() for p in parts[1:])
    got = fetch(parts)
    _check(got, [p.numpy() for p in parts])
    assert all(g.flags.c_contiguous for g in got) and len(cpu_calls) == 1


def test_single_tensor_skips_the_cat(cpu_calls, monkeypatch):
    cats, real = [], torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **kw: cats.append(1) or real(*a, **kw))
    src = _sources()[2]
    _check(fetch([torch.from_numpy(src)]), [src])
    assert cats == [] and len(cpu_calls) == 1
    _check(fetch([torch.from_numpy(src)[:, :, ::2]]), [src[:, :, ::2]])
    assert cats == [] and len(cpu_calls) == 2
    fetch([torch.from_numpy(a) for a in _sources()])
    assert cats == [1]


def test_empty_list_copies_nothing(cpu_calls):
    assert fetch([]) == [] and fetch(iter(())) == []
    assert cpu_calls == []


def test_scalars_and_bools():
    got = fetch([torch.tensor(True), torch.tensor([1.5], dtype=torch.float64), torch.tensor(-3, dtype=torch.int16)])
    assert got[0].dtype == np.bool_ and got[0].shape == () and bool(got[0]) is True
    assert got[1].dtype == np.float64 and got[1].tolist() == [1.5] and got[2].dtype == np.int16 and int(got[2]) == -3
