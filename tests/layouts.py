"""Awkward memory layouts of one column, for the ingest tests (host and GPU):
each builder returns a view whose logical content is the given 1-D numpy
array `a` but whose storage is not a fresh contiguous 16-byte-aligned
buffer.  The storage around the view is filled with `a` reversed (plus an
offset for floats): values of the column's own range, so a reader that
ignores the strides stays in bounds and in range and gets wrong numbers."""
import numpy as np
import torch

LAYOUTS = ("contiguous", "base8", "column", "step2")


def _junk(a: np.ndarray) -> np.ndarray:
    j = a[::-1].copy()
    return j + 1000.0 if a.dtype.kind == "f" else j


def _storage(a: np.ndarray, layout: str) -> np.ndarray:
    n, j = len(a), _junk(a)
    if layout == "base8":          # buf[1:] of an n + 1 buffer
        return np.concatenate([j[:1], a])
    if layout == "column":         # table[:, 1] of a [n, 3] table
        return np.ascontiguousarray(np.stack([j, a, j], axis=1))
    if layout == "step2":          # x[::2] of a 2n buffer
        return np.ascontiguousarray(np.stack([a, j], axis=1)).reshape(-1).copy()
    if layout == "col2d":          # an [n, 1] column
        return a.copy().reshape(n, 1)
    if layout == "contiguous":
        return a.copy()
    raise ValueError(layout)


def _view(s, layout: str):
    if layout == "base8":
        return s[1:]
    if layout == "column":
        return s[:, 1]
    if layout == "step2":
        return s[::2]
    return s


def numpy_view(a: np.ndarray, layout: str) -> np.ndarray:
    return _view(_storage(a, layout), layout)


def torch_view(a: np.ndarray, layout: str, device="cpu") -> torch.Tensor:
    """The same view as a torch tensor whose storage lives on `device` (the
    whole storage is moved, so the layout survives the copy)."""
    return _view(torch.from_numpy(_storage(a, layout)).to(device), layout)


def expanded(x, n: int, lib: str, dtype):
    """n copies of one element, stride 0."""
    if lib == "torch":
        return torch.tensor([x], dtype=getattr(torch, dtype)).expand(n)
    return np.broadcast_to(np.array([x], dtype=dtype), (n,))
