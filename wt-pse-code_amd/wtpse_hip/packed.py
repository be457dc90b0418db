"""The one copy: what a batch or a size group leaves on the device comes back in a single device -> host transfer.  `fetch` is the only
place that packs the pieces and knows their byte offsets; its callers hand it tensors and take arrays."""
import numpy as np
import torch

_NUMPY = {}


def _numpy_dtype(dtype):
    if dtype not in _NUMPY:
        _NUMPY[dtype] = torch.empty(0, dtype=dtype).numpy().dtype
    return _NUMPY[dtype]


def fetch(tensors):
    """Tensors of one device, any dtypes and shapes -> numpy arrays of the same dtypes, shapes and order, out of ONE torch.cat of their
    bytes and ONE .cpu() (a single tensor skips the cat; an empty list returns [] and copies nothing).  A non-contiguous tensor is made
    contiguous first.  An array is a view of the fetched bytes where its offset is a multiple of its item size and a copy where it is
    not."""
    tensors = [t.contiguous() for t in tensors]
    if not tensors:
        return []
    flat = [t.reshape(-1).view(torch.uint8) for t in tensors if t.numel()]           # (a tensor without elements adds no bytes)
    if not flat:
        return [np.empty(tuple(t.shape), _numpy_dtype(t.dtype)) for t in tensors]
    host = (torch.cat(flat) if len(flat) > 1 else flat[0]).cpu().numpy()
    out, off = [], 0
    for t in tensors:
        dtype, nbytes = _numpy_dtype(t.dtype), t.numel() * t.element_size()
        piece = host[off:off + nbytes]
        if off % dtype.itemsize:
            piece = piece.copy()
        out.append(piece.view(dtype).reshape(tuple(t.shape)))
        off += nbytes
    return out
