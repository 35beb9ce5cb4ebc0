"""``KVCache``: the projected keys and values of every layer, kept on the device for generation.

A decode step then needs the new tokens' Q/K/V and one read of each layer's cache
(``mt_flash_attn_decode``) instead of a full causal forward over the prefix. Per layer the cache
holds K and V as ``[B, n_positions, Hkv, d]`` storage (the layout ``MultiHeadAttention`` projects
into), seen by the kernels as ``[B, Hkv, n_positions, d]`` through strides; rows at or past
``length[b]`` are uninitialised and never read. ``Hkv = n_kv_head`` is the model's key / value
heads: ``n_head`` unless the model uses grouped-query attention. A filled cache also takes any
number of new tokens per row in one step (``mt_flash_attn_extend``: the next turn of a
conversation, a chunk of a long prompt; ``extend_counts`` builds that step's count vectors).
"""
from __future__ import annotations

import numpy as np

from .tensor import Tensor
from .tensor_data import TensorData

__all__ = ["KVCache", "LayerKV"]


class LayerKV:
    """One layer's K / V cache tensors ([B, n_kv_head, n_positions, d] views) and the owning cache."""

    def __init__(self, cache: "KVCache", k: Tensor, v: Tensor):
        self.cache = cache
        self.k = k
        self.v = v


class KVCache:
    def __init__(self, n_layer: int, batch_size: int, n_head: int, n_positions: int, head_dim: int, backend,
                 n_kv_head=None):
        if getattr(backend, "flash_attention_decode", None) is None or getattr(backend, "kv_cache_append", None) is None:
            raise ValueError("KVCache needs a backend with the decode kernels (HipKernelOps)")
        if head_dim % 4 != 0 or head_dim > 256:
            raise ValueError(f"KVCache: head_dim {head_dim} is not supported by the decode kernel "
                             "(fp32 rows must be a multiple of 16 bytes: head_dim % 4 == 0, head_dim <= 256)")
        if min(n_layer, batch_size, n_head, n_positions) <= 0:
            raise ValueError("KVCache: sizes must be positive")
        if n_kv_head is None:
            n_kv_head = n_head
        if n_kv_head <= 0 or n_head % n_kv_head:
            raise ValueError(f"KVCache: n_kv_head = {n_kv_head} does not divide n_head = {n_head}")
        import torch
        self.n_layer, self.batch_size, self.n_head = n_layer, batch_size, n_head  # n_head: the query heads
        self.n_kv_head = n_kv_head
        self.n_positions, self.head_dim, self.backend = n_positions, head_dim, backend
        shape = (batch_size, n_kv_head, n_positions, head_dim)
        strides = (n_positions * n_kv_head * head_dim, head_dim, n_kv_head * head_dim, 1)
        numel = batch_size * n_positions * n_kv_head * head_dim

        def buf():
            return Tensor(TensorData(torch.empty(numel, dtype=torch.float32, device="cuda"), shape, strides),
                          backend=backend)
        self.layers = [LayerKV(self, buf(), buf()) for _ in range(n_layer)]
        # tokens held per batch row: the device vector the kernels read and its host mirror
        self.length = torch.zeros(batch_size, dtype=torch.int32, device="cuda")
        self.length_host = np.zeros(batch_size, dtype=np.int64)
        self._visible = None

    def layer(self, i: int) -> LayerKV:
        return self.layers[i]

    @property
    def empty(self) -> bool:
        return not self.length_host.any()

    def reset(self) -> None:
        self.length.zero_()
        self.length_host[:] = 0
        self._visible = None

    def set_length(self, lengths) -> None:
        """Set the per-row token counts (host values, copied to the device)."""
        import torch
        a = np.asarray(lengths, dtype=np.int64).reshape(self.batch_size)
        if (a < 0).any() or (a > self.n_positions).any():
            raise ValueError(f"KVCache: lengths must be in [0, {self.n_positions}]")
        self.length_host[:] = a
        self.length.copy_(torch.from_numpy(a.astype(np.int32)))
        self._visible = None

    def visible(self, n_new: int):
        """Device int32 [B]: the keys each row sees once n_new tokens are appended at its
        current length (one vector per step, shared by the layers)."""
        if self._visible is None or self._visible[0] != n_new:
            self._visible = (n_new, self.length + n_new)
        return self._visible[1]

    def extend_counts(self, new_len):
        """Device int32 [B] vectors (visible, q_len) of an extend step that appends new_len[b]
        real tokens to row b (host counts; the batch is right-padded): the keys each row holds
        once they are appended, and the counts themselves. Built once per step and shared by the
        layers, like visible()."""
        import torch
        a = np.ascontiguousarray(np.asarray(new_len, dtype=np.int32).reshape(self.batch_size))
        key = ("extend", a.tobytes())
        if self._visible is None or self._visible[0] != key:
            q_len = torch.from_numpy(a).to("cuda")
            self._visible = (key, self.length + q_len, q_len)
        return self._visible[1], self._visible[2]

    def clamp_to_last_slot(self) -> None:
        """Rows that filled the cache step back to its last slot, on the device (stream-ordered,
        capturable) and in the host mirror: what a one-token step does first, so that a finished
        row that filled its cache re-writes its last slot (its output is discarded)."""
        self.length.clamp_(max=self.n_positions - 1)
        np.minimum(self.length_host, self.n_positions - 1, out=self.length_host)
        self._visible = None

    def mirror_step(self) -> None:
        """The host mirror of one replayed one-token step (clamp_to_last_slot, then one token
        appended): the captured step does the same on the device, nothing is copied."""
        np.minimum(self.length_host, self.n_positions - 1, out=self.length_host)
        self.length_host += 1
        self._visible = None

    def advance(self, n_new) -> None:
        """Count n_new appended tokens (an int, or one count per batch row)."""
        a = np.broadcast_to(np.asarray(n_new, dtype=np.int64), (self.batch_size,))
        if np.ndim(n_new) == 0 and int(self.length_host.max()) + int(n_new) <= self.n_positions:
            self.length.add_(int(n_new))  # stream-ordered, no host-to-device copy
            self.length_host += int(n_new)
            self._visible = None
        else:
            self.set_length(np.minimum(self.length_host + a, self.n_positions))
