"""``KVCache``: the projected keys and values of every layer, kept on the device for generation.

A decode step then needs the new tokens' Q/K/V and one read of each layer's cache
(``mt_flash_attn_decode``) instead of a full causal forward over the prefix. Per layer the cache
holds K and V as ``[B, n_positions, Hkv, d]`` storage (the layout ``MultiHeadAttention`` projects
into), seen by the kernels as ``[B, Hkv, n_positions, d]`` through strides; rows at or past
``length[b]`` are uninitialised and never read. ``Hkv = n_kv_head`` is the model's key / value
heads: ``n_head`` unless the model uses grouped-query attention. A filled cache also takes any
number of new tokens per row in one step (``mt_flash_attn_extend``: the next turn of a
conversation, a chunk of a long prompt; ``extend_counts`` builds that step's count vectors).

``kv_dtype="bf16"`` / ``"fp8"`` stores K and V quantised (torch.bfloat16, or torch.uint8 holding
OCP e4m3 codes with one fp32 scale per cached row): the new rows are quantised as they are appended
(``mt_kv_cache_append_quant``), a decode step reads the quantised rows directly
(``mt_flash_attn_decode_kvq``) and an extend step dequantises the visible rows into one fp32
scratch pair shared by the layers (``mt_kv_cache_dequant``) for the fp32 extend kernel.
"""
from __future__ import annotations

import numpy as np

from .tensor import Tensor
from .tensor_data import TensorData

__all__ = ["KVCache", "LayerKV"]


class LayerKV:
    """One layer's K / V cache tensors ([B, n_kv_head, n_positions, d] views) and the owning cache."""

    def __init__(self, cache: "KVCache", k, v, k_scale=None, v_scale=None):
        self.cache = cache
        # fp32 cache: minitorch Tensors. Quantised cache: torch tensors (bfloat16, or uint8 e4m3
        # codes with the fp32 row scales k_scale / v_scale [B, n_kv_head, n_positions])
        self.k = k
        self.v = v
        self.k_scale = k_scale
        self.v_scale = v_scale


class KVCache:
    KV_DTYPES = (None, "fp32", "bf16", "fp8")

    def __init__(self, n_layer: int, batch_size: int, n_head: int, n_positions: int, head_dim: int, backend,
                 n_kv_head=None, kv_dtype=None):
        """kv_dtype: None / "fp32" (fp32 storage), "bf16", or "fp8" (e4m3 codes and one fp32
        scale per cached row)."""
        if kv_dtype not in self.KV_DTYPES:
            raise ValueError(f"KVCache: kv_dtype must be one of {self.KV_DTYPES}, got {kv_dtype!r}")
        self.kv_dtype = "fp32" if kv_dtype is None else kv_dtype
        self.quantised = self.kv_dtype != "fp32"
        if self.quantised:
            if any(getattr(backend, f, None) is None
                   for f in ("kv_cache_append_quant", "flash_attention_decode_kvq", "kv_cache_dequant")):
                raise ValueError("KVCache(kv_dtype=...) needs a backend with the quantised-cache kernels (HipKernelOps)")
            if head_dim % 8 != 0:
                raise ValueError(f"KVCache: a quantised cache needs head_dim % 8 == 0, got {head_dim}")
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

        self._shape, self._strides, self._numel = shape, strides, numel

        def buf():
            return Tensor(TensorData(torch.empty(numel, dtype=torch.float32, device="cuda"), shape, strides),
                          backend=backend)

        def qbuf():
            t = torch.empty(numel, dtype=torch.bfloat16 if self.kv_dtype == "bf16" else torch.uint8, device="cuda")
            return torch.as_strided(t, shape, strides)

        def sbuf():
            if self.kv_dtype != "fp8":
                return None
            return torch.empty((batch_size, n_kv_head, n_positions), dtype=torch.float32, device="cuda")
        if self.quantised:
            self.layers = [LayerKV(self, qbuf(), qbuf(), sbuf(), sbuf()) for _ in range(n_layer)]
        else:
            self.layers = [LayerKV(self, buf(), buf()) for _ in range(n_layer)]
        self._scratch = None      # quantised: the fp32 K / V pair of one layer's size for extend steps
        self._workspaces = {}     # quantised: the decode workspace per number of new tokens
        # tokens held per batch row: the device vector the kernels read and its host mirror
        self.length = torch.zeros(batch_size, dtype=torch.int32, device="cuda")
        self.length_host = np.zeros(batch_size, dtype=np.int64)
        self._visible = None

    def layer(self, i: int) -> LayerKV:
        return self.layers[i]

    @property
    def nbytes(self) -> int:
        """Device bytes of K, V and (fp8) the row scales over all layers."""
        esize = {"fp32": 4, "bf16": 2, "fp8": 1}[self.kv_dtype]
        per_layer = 2 * self._numel * esize
        if self.kv_dtype == "fp8":
            per_layer += 2 * self.batch_size * self.n_kv_head * self.n_positions * 4
        return self.n_layer * per_layer

    def scratch(self):
        """The fp32 (K, V) scratch of a quantised cache, one layer's size and layout, shared by the
        layers: an extend step dequantises the visible rows into it. Allocated at the first use."""
        import torch
        if self._scratch is None:
            self._scratch = tuple(
                Tensor(TensorData(torch.empty(self._numel, dtype=torch.float32, device="cuda"), self._shape,
                                  self._strides), backend=self.backend) for _ in range(2))
        return self._scratch

    def decode_workspace(self, n_new: int):
        """The split-KV workspace of a decode step of n_new tokens on a quantised cache (None when
        the plan has one split), shared by the layers and kept, so that a captured step allocates
        nothing."""
        import torch
        from . import _hip
        if n_new not in self._workspaces:
            code = _hip.MT_KV_BF16 if self.kv_dtype == "bf16" else _hip.MT_KV_FP8
            need = _hip.decode_kvq_workspace_bytes(code, self.batch_size, self.n_head, n_new, self.n_positions,
                                                   self.head_dim, self.n_kv_head)
            self._workspaces[n_new] = torch.empty(need // 4, dtype=torch.float32, device="cuda") if need else None
        return self._workspaces[n_new]

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
