"""Rotary position embedding (RoPE): the table, the fused-kernel path and the tensor-op form.

The convention is the half-split ("rotate-half") one: element j < d/2 of a head row pairs with
element j + d/2, and at position p

    out[j]       = x[j]       * cos[p][j] - x[j + d/2] * sin[p][j]
    out[j + d/2] = x[j + d/2] * cos[p][j] + x[j]       * sin[p][j]

with the angle p * theta ** (-2j / d). Token t of batch row b sits at
min(max(pos0[b], 0) + t, n_positions - 1) (pos0 None: 0), on both paths.
"""
from __future__ import annotations

import numpy as np

from .tensor_functions import Rope, tensor_from_numpy

__all__ = ["RotaryTable", "apply_rope"]

datatype = np.float32


class RotaryTable:
    """The cos / sin tables [n_positions, head_dim / 2] of a rotary embedding: the angles
    p * theta ** (-2j / head_dim) computed in float64 on the host, rounded once to fp32
    (cos_host, sin_host) and uploaded once to the backend (cos, sin: constant tensors, made on
    first use). The kernel and the tensor-op form both read these values, so they agree on
    every angle to the bit."""

    def __init__(self, n_positions: int, head_dim: int, theta: float = 10000.0, backend=None):
        n_positions, head_dim = int(n_positions), int(head_dim)
        if n_positions <= 0:
            raise ValueError(f"RotaryTable: n_positions must be positive, got {n_positions}")
        if head_dim <= 0 or head_dim % 2:
            raise ValueError(f"RotaryTable: head_dim must be even and positive, got {head_dim}")
        if not float(theta) > 0.0:
            raise ValueError(f"RotaryTable: theta must be positive, got {theta}")
        self.n_positions = n_positions
        self.head_dim = head_dim
        self.theta = float(theta)
        self.backend = backend
        j = np.arange(head_dim // 2, dtype=np.float64)
        p = np.arange(n_positions, dtype=np.float64)
        angle = p[:, None] * (self.theta ** (-2.0 * j / head_dim))[None, :]
        self.cos_host = np.cos(angle).astype(datatype)
        self.sin_host = np.sin(angle).astype(datatype)
        self._dev = None
        self._consts: dict = {}  # the tensor-op form's constants, by value

    def _tables(self):
        if self._dev is None:
            if self.backend is None:
                raise ValueError("a TensorBackend is required (RotaryTable(..., backend=...))")
            self._dev = (tensor_from_numpy(self.cos_host, backend=self.backend),
                         tensor_from_numpy(self.sin_host, backend=self.backend))
        return self._dev

    @property
    def cos(self):
        return self._tables()[0]

    @property
    def sin(self):
        return self._tables()[1]

    def positions(self, pos0, batch_size: int, seq_len: int) -> np.ndarray:
        """The table rows of a [batch_size, seq_len] block of tokens as host int64 [1 or B, T]:
        min(max(pos0[b], 0) + t, n_positions - 1), the formula mt_rope applies on the device."""
        t = np.arange(seq_len, dtype=np.int64)[None, :]
        if pos0 is None:
            start = np.zeros((1, 1), dtype=np.int64)
        else:
            start = np.maximum(_host_vector(pos0, batch_size), 0)[:, None]
        return np.minimum(start + t, self.n_positions - 1)

    # ---- the tensor-op form's constants ---------------------------------------------------
    def _const(self, key, backend, make):
        key = (id(backend),) + key
        c = self._consts.get(key)
        if c is None:
            if len(self._consts) > 64:
                self._consts.clear()
            c = self._consts[key] = tensor_from_numpy(make(), backend=backend)
        return c

    def half_swap(self, backend):
        """P [d, d]: (x @ P)[j] = -x[j + d/2], (x @ P)[j + d/2] = x[j]."""
        d, h = self.head_dim, self.head_dim // 2

        def make():
            p = np.zeros((d, d), dtype=datatype)
            p[np.arange(h) + h, np.arange(h)] = -1.0
            p[np.arange(h), np.arange(h) + h] = 1.0
            return p
        return self._const(("P",), backend, make)

    def widened(self, pos: np.ndarray, backend):
        """(C, S) [1 or B, 1, T, d]: the cos / sin rows of the positions pos [1 or B, T], each
        repeated over both halves of a head row."""
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        key = (pos.shape, pos.tobytes())
        wide = lambda tab: np.concatenate([tab[pos], tab[pos]], axis=-1)[:, None]  # noqa: E731
        return (self._const(("C",) + key, backend, lambda: wide(self.cos_host)),
                self._const(("S",) + key, backend, lambda: wide(self.sin_host)))


def _host_vector(pos0, batch_size: int) -> np.ndarray:
    from .tensor import Tensor
    if isinstance(pos0, Tensor):
        a = pos0.to_numpy()
    elif hasattr(pos0, "detach"):  # a torch tensor (a KVCache's device lengths)
        a = pos0.detach().cpu().numpy()
    else:
        a = np.asarray(pos0)
    a = a.reshape(-1)
    if a.size != batch_size:
        raise ValueError(f"pos0 has {a.size} entries for a batch of {batch_size}")
    n = a.astype(np.int64)
    if (n != a).any():
        raise ValueError(f"pos0 must hold whole numbers, got {a.tolist()}")
    return n


def _pos_tensor(pos0, batch_size: int, backend):
    """pos0 as the constant [B] tensor the Rope Function carries (the way FlashAttention carries
    kv_len)."""
    from .tensor import Tensor
    from .tensor_data import TensorData
    if isinstance(pos0, Tensor):
        if pos0.size != batch_size:
            raise ValueError(f"pos0 has {pos0.size} entries for a batch of {batch_size}")
        return pos0
    if hasattr(pos0, "detach"):  # a torch device vector: converted on the device
        import torch
        if pos0.numel() != batch_size:
            raise ValueError(f"pos0 has {pos0.numel()} entries for a batch of {batch_size}")
        return Tensor(TensorData(pos0.reshape(-1).to(torch.float32), (batch_size,)), backend=backend)
    return tensor_from_numpy(_host_vector(pos0, batch_size).astype(datatype), backend=backend)


def apply_rope(x, table: RotaryTable, pos0=None, fused=None):
    """x [B, H, T, d] rotated by `table` (Tensor.rope). fused None: the kernel when x's backend
    has it (TensorBackend.rope), the tensor-op form otherwise; True / False choose (True on a
    backend without the kernel is an error). Both paths are differentiable in x.

    The tensor-op form is x * C + (x @ P) * S with P the constant signed half-swap matrix and
    C / S the table rows of every token's position widened to d columns: multiplies, adds and a
    matmul, so autodiff has its backward already. The positions are then taken on the host
    (pos0 None, host numbers, or a tensor that is read back)."""
    if x.dims != 4 or x.shape[3] != table.head_dim:
        raise ValueError(f"rope takes [B, H, T, {table.head_dim}] (the table's head_dim), got {tuple(x.shape)}")
    batch_size, _, seq_len, _ = x.shape
    kernel = getattr(x.backend, "rope", None)
    if fused is None:
        fused = kernel is not None
    if fused:
        if kernel is None:
            raise NotImplementedError("this backend has no rope kernel")
        args = (x, table.cos, table.sin)
        if pos0 is not None:
            args += (_pos_tensor(pos0, batch_size, x.backend),)
        return Rope.apply(*args)
    backend = x.backend
    C, S = table.widened(table.positions(pos0, batch_size, seq_len), backend)
    return x * C + (x @ table.half_swap(backend)) * S
