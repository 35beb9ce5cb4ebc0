"""Transformer modules (reference ``minitorch/modules_transfomer.py``).

``MultiHeadAttention(use_flash_attention=True)`` is the north-star caller: its
``self_attention`` hands the permuted ``[B, H, N, d]`` projections straight to
``q.flash_attention[_causal](k, v)`` (reference :154-175). The plain branch is the
unfused ``softmax(QKᵀ/√d) V`` composition (reference :177-193) and the fused-softmax
branch uses the HIP attention softmax (with the causal mask applied inside the kernel).

Fixes vs the reference: the ``use_flash_attention`` / ``use_fused_kernel`` flags reach
MultiHeadAttention from TransformerLayer and DecoderLM by keyword (reference :309-311,
:409-420 pass them positionally into the wrong slots); position embeddings are sized by
``n_positions`` (reference :408 uses ``n_vocab``).
"""
from __future__ import annotations

import weakref

import numpy as np

from .module import Module
from .modules_basic import Dropout, Embedding, FusedLayerNorm, LayerNorm1d, Linear
from .nn import GELU, softmax
from .rotary import RotaryTable, apply_rope
from .tensor_functions import tensor, tensor_from_numpy

# Small host-built index tensors the model makes on every forward (the [B] key-padding lengths
# of the flash path, the [1, T] position ids): cached by value, so a training loop that feeds
# the same shapes does not copy host memory to the device in every layer (each synchronous
# host-to-device copy also waits for the work already queued on the stream)
_INDEX_CACHE: dict = {}


def _kv_tensor(kv_len, batch_size: int, backend):
    from .tensor import Tensor
    if isinstance(kv_len, Tensor):  # already a device tensor (e.g. a graph-captured step's fixed input)
        if kv_len.size != batch_size:
            raise ValueError(f"kv_len has {kv_len.size} entries for a batch of {batch_size}")
        return kv_len
    a = np.ascontiguousarray(np.asarray(kv_len, dtype=datatype).reshape(batch_size))
    key = ("kv", id(backend), a.tobytes())
    t = _INDEX_CACHE.get(key)
    if t is None:
        if len(_INDEX_CACHE) > 64:
            _INDEX_CACHE.clear()
        t = _INDEX_CACHE[key] = tensor_from_numpy(a, backend=backend)
    return t


def _new_token_counts(kv_len, batch_size: int, seq_len: int) -> np.ndarray:
    """The per-row counts of real new tokens of an extend step as host int64 [B], each in
    [0, seq_len]."""
    from .tensor import Tensor
    a = kv_len.to_numpy() if isinstance(kv_len, Tensor) else kv_len
    a = np.asarray(a).reshape(-1)
    if a.size != batch_size:
        raise ValueError(f"kv_len has {a.size} entries for a batch of {batch_size}")
    n = a.astype(np.int64)
    if (n != a).any() or (n < 0).any() or (n > seq_len).any():
        raise ValueError(f"kv_len must hold whole numbers in [0, {seq_len}] (the new tokens per row), got {a.tolist()}")
    return n


def _positions(seq_len: int, backend):
    key = ("pos", id(backend), seq_len)
    t = _INDEX_CACHE.get(key)
    if t is None:
        if len(_INDEX_CACHE) > 64:
            _INDEX_CACHE.clear()
        t = _INDEX_CACHE[key] = tensor([[float(i) for i in range(seq_len)]], backend=backend)
    return t

def _group_ones(group: int, backend):
    key = ("ones", id(backend), group)
    t = _INDEX_CACHE.get(key)
    if t is None:
        if len(_INDEX_CACHE) > 64:
            _INDEX_CACHE.clear()
        t = _INDEX_CACHE[key] = tensor_from_numpy(np.ones((1, 1, group, 1, 1), dtype=datatype), backend=backend)
    return t

datatype = np.float32


class MultiHeadAttention(Module):
    def __init__(self, n_embd: int, n_head: int, causal: bool = False, p_dropout: float = 0.1,
                 bias: bool = True, backend=None, use_fused_kernel: bool = False,
                 use_flash_attention: bool = False, n_kv_head=None, rope=None):
        """n_kv_head: grouped-query attention. The n_head query heads share n_kv_head key / value
        heads in groups of n_head // n_kv_head (query head h uses kv head h // group; 1 is
        multi-query attention). None: n_head, every head its own K and V.
        rope: a RotaryTable (rotary position embedding), or None. Q and K are rotated by their
        tokens' positions right after the projection, so every attention branch and the KV cache
        see rotated tensors: by the rope kernel when use_fused_kernel is set and the backend has
        it, by the tensor-op form otherwise (rotary.apply_rope). With a cache the rotation is
        always the kernel's, one launch for Q and K, in place, at the cache's device lengths."""
        super().__init__()
        if n_kv_head is None:
            n_kv_head = n_head
        if n_kv_head <= 0 or n_head % n_kv_head:
            raise ValueError(f"n_kv_head = {n_kv_head} does not divide n_head = {n_head}")
        self.backend = backend
        self.n_embd = n_embd
        self.n_head = n_head
        self.n_kv_head = n_kv_head
        self.causal = causal
        self.attn_hidden_dim = n_embd // n_head
        self.q_projection = Linear(n_embd, n_embd, bias, backend)
        self.k_projection = Linear(n_embd, n_kv_head * self.attn_hidden_dim, bias, backend)
        self.v_projection = Linear(n_embd, n_kv_head * self.attn_hidden_dim, bias, backend)
        self.out_projection = Linear(n_embd, n_embd, bias, backend)
        self.dropout = Dropout(p_dropout)
        self.use_fused_kernel = use_fused_kernel
        self.use_flash_attention = use_flash_attention
        if rope is not None and rope.head_dim != self.attn_hidden_dim:
            raise ValueError(f"the RotaryTable was built for head_dim = {rope.head_dim}, the heads have "
                             f"{self.attn_hidden_dim}")
        self.rope = rope

    def create_causal_mask(self, bs, nh, seq_len):
        """Additive -FLT_MAX·triu(1) mask (reference :63-71), [1, 1, T, T] broadcast."""
        mask = -np.finfo(datatype).max * np.triu(np.ones((1, 1, seq_len, seq_len), dtype=datatype), 1)
        return tensor_from_numpy(mask, backend=self.backend)

    def project_to_query_key_value(self, x):
        batch_size, seq_len, n_embd = x.shape
        flat = x.view(batch_size * seq_len, n_embd)
        shp = (batch_size, seq_len, self.n_head, self.attn_hidden_dim)
        kv_shp = (batch_size, seq_len, self.n_kv_head, self.attn_hidden_dim)
        q = self.q_projection(flat).view(*shp).permute(0, 2, 1, 3)
        k4 = self.k_projection(flat).view(*kv_shp)
        kT = k4.permute(0, 2, 3, 1)
        k = k4.permute(0, 2, 1, 3)
        v = self.v_projection(flat).view(*kv_shp).permute(0, 2, 1, 3)
        return q, k, kT, v

    def _repeat_kv(self, x):
        """[B, n_kv_head, a, b] -> [B, n_head, a, b], head h a copy of kv head h // group (the
        order the decode kernel uses): a broadcast multiply by ones, whose backward sums the
        group's gradients. There is no fused grouped-query training kernel."""
        group = self.n_head // self.n_kv_head
        if group == 1:
            return x
        batch_size, n_kv, a, b = x.shape
        rep = x.contiguous().view(batch_size, n_kv, 1, a, b) * _group_ones(group, self.backend)
        return rep.contiguous().view(batch_size, self.n_head, a, b)

    def create_padding_mask(self, kv_len, seq_len):
        """The reference's key-padding contract (src/softmax_kernel.cu:26-33: attn_mask
        [B, to_len], 0 for tokens, -inf for padding) as an additive [B, 1, 1, T] mask."""
        kv = np.asarray(kv_len).reshape(-1, 1, 1, 1)
        mask = np.where(np.arange(seq_len)[None, None, None, :] < kv, 0.0, -np.inf).astype(datatype)
        return tensor_from_numpy(mask, backend=self.backend)

    def self_attention(self, q, kT, v, kv_len=None):
        """``kT`` is the [B,H,d,N] transpose, or the [B,H,N,d] keys on the flash path.
        ``kv_len``: optional per-batch-row count of valid (non-padding) keys: the flash path
        masks keys >= kv_len[b] in the kernel (mt_flash_attn_*_varlen); the other branches add
        the equivalent [B, to_len] padding mask. With n_kv_head < n_head, kT and v hold
        n_kv_head heads and are repeated to n_head first."""
        batch_size, num_head, queries_len, q_dim = q.shape
        kT, v = self._repeat_kv(kT), self._repeat_kv(v)
        scale = self.attn_hidden_dim ** 0.5
        if self.use_flash_attention:
            kv = None if kv_len is None else _kv_tensor(kv_len, batch_size, self.backend)
            result = (q.flash_attention_causal(kT, v, kv_len=kv) if self.causal
                      else q.flash_attention(kT, v, kv_len=kv))
        elif self.use_fused_kernel:
            scores = (q @ kT) / scale
            if kv_len is None:
                result = (scores.attn_softmax(None, mask_future=True) if self.causal
                          else scores.attn_softmax(None)) @ v
            else:
                mask = self.create_padding_mask(kv_len, queries_len)
                if self.causal:
                    mask = mask + self.create_causal_mask(batch_size, num_head, queries_len)
                result = scores.attn_softmax(mask) @ v
        else:
            scores = (q @ kT) / scale
            if self.causal:
                scores = scores + self.create_causal_mask(batch_size, num_head, queries_len)
            if kv_len is not None:
                scores = scores + self.create_padding_mask(kv_len, queries_len)
            result = softmax(scores, dim=3) @ v
        result = result.permute(0, 2, 1, 3).contiguous()
        return result.view(batch_size, queries_len, self.n_embd)

    def forward(self, x, kv_len=None, cache=None):
        """cache: None (training / full forward), or this layer's slice of a KVCache (a
        LayerKV; a one-layer KVCache is taken as its layer 0). With a cache the K / V rows of
        x's tokens are appended at the cache's current lengths; an empty cache is a prefill
        (today's causal flash attention over the prompt, kv_len = the prompt lengths of a
        right-padded batch), otherwise x holds at most 8 new tokens per row and attends the
        cache (Tensor.flash_attention_decode; the cache holds n_kv_head heads). A filled cache
        with kv_len given is an extend step: x is a right-padded batch of any length whose row b
        holds kv_len[b] real new tokens (Tensor.flash_attention_extend). The caller advances the
        cache's lengths once every layer has run (DecoderLM.forward does)."""
        batch_size, seq_len, n_embd = x.shape
        q, k, kT, v = self.project_to_query_key_value(x)
        if cache is None:
            if self.rope is not None:
                # training / a full forward: token t sits at position t; differentiable
                fused = bool(self.use_fused_kernel) and getattr(q.backend, "rope", None) is not None
                q = apply_rope(q, self.rope, None, fused=fused)
                k = apply_rope(k, self.rope, None, fused=fused)
                kT = k.permute(0, 1, 3, 2)
            attn = self.self_attention(q, k if self.use_flash_attention else kT, v, kv_len)
        else:
            attn = self._cached_attention(q, k, v, kv_len, cache)
        return self.out_projection(attn.view(batch_size * seq_len, n_embd)).view(batch_size, seq_len, n_embd)

    def _cached_attention(self, q, k, v, kv_len, cache):
        from .kv_cache import KVCache
        if not self.use_flash_attention:
            raise ValueError("a KV cache needs use_flash_attention=True")
        if not self.causal:
            raise ValueError("a KV cache needs causal attention")
        lkv = cache.layer(0) if isinstance(cache, KVCache) else cache
        kvc = lkv.cache
        batch_size, num_head, seq_len, q_dim = q.shape
        if (batch_size, num_head, self.n_kv_head, q_dim) != (kvc.batch_size, kvc.n_head, kvc.n_kv_head, kvc.head_dim):
            raise ValueError(f"the KV cache was built for (B, H, Hkv, d) = ({kvc.batch_size}, {kvc.n_head}, "
                             f"{kvc.n_kv_head}, {kvc.head_dim}), got ({batch_size}, {num_head}, "
                             f"{self.n_kv_head}, {q_dim})")
        prefill = kvc.empty
        if not prefill and kv_len is not None:
            return self._extend_attention(q, k, v, kv_len, lkv)
        if not prefill and seq_len > 8:
            raise ValueError(f"a decode step takes at most 8 new tokens per row, got {seq_len}")
        if int(kvc.length_host.max()) + seq_len > kvc.n_positions:
            raise ValueError(f"{seq_len} new tokens do not fit the KV cache ({kvc.n_positions} positions, "
                             f"{int(kvc.length_host.max())} held)")
        q, k = self._rotate_cached(q, k, None if prefill else kvc.length)
        if kvc.paged:
            return self._paged_attention(q, k, v, kv_len, lkv, prefill)
        if kvc.quantised:
            # the rows are quantised as they land; a prefill still attends the fresh fp32 K / V
            q.backend.kv_cache_append_quant(k, v, lkv.k, lkv.v, kvc.length, lkv.k_scale, lkv.v_scale)
        else:
            q.backend.kv_cache_append(k, v, lkv.k, lkv.v, kvc.length)
        if prefill:
            return self.self_attention(q, k, v, kv_len)
        if kvc.quantised:
            result = q.backend.flash_attention_decode_kvq(q, lkv.k, lkv.v, lkv.k_scale, lkv.v_scale,
                                                          kvc.visible(seq_len), True, kvc.decode_workspace(seq_len))
        else:
            result = q.flash_attention_decode(lkv.k, lkv.v, kvc.visible(seq_len))
        result = result.permute(0, 2, 1, 3).contiguous()
        return result.view(batch_size, seq_len, self.n_embd)

    def _rotate_cached(self, q, k, pos0):
        """Q and K of a cached step rotated in one two-tensor launch, in place in the projections'
        own buffers (inference: nothing differentiates through a cache). pos0: the cache's device
        lengths (a decode or extend step: row b's tokens continue at length[b], read by the kernel,
        so a captured step replays), or None for a prefill. Padding slots that pass the last
        position take it (mt_rope's clamp); their outputs are discarded."""
        if self.rope is None:
            return q, k
        if getattr(q.backend, "rope", None) is None:
            raise NotImplementedError("a rotary model with a KV cache needs a backend with the rope kernel "
                                      "(HipKernelOps)")
        return q.backend.rope(q, self.rope.cos, self.rope.sin, pos0=pos0, x2=k, inplace=True)

    def _paged_attention(self, q, k, v, kv_len, lkv, prefill):
        """A prefill or a decode step on a PagedKVCache: the pages are reserved from the host
        mirror's counts, the new rows appended through the block table, and a decode step reads the
        pages directly (mt_flash_attn_decode_paged; the workspace is the cache's, so a captured
        step allocates nothing). A prefill attends the fresh K / V as the contiguous cache does;
        of a right-padded prompt batch only the kv_len[b] real rows land (a paged cache has no
        stale tail to take the padding)."""
        kvc = lkv.cache
        batch_size, _, seq_len, _ = q.shape
        new_len, count = seq_len, None
        if prefill and kv_len is not None:
            new_len = _new_token_counts(kv_len, batch_size, seq_len)
            count = kvc.extend_counts(new_len)[1]
        kvc.reserve(kvc.length_host + new_len)
        q.backend.kv_cache_append_paged(k, v, lkv.k, lkv.v, kvc.block_table, kvc.length, count)
        if prefill:
            return self.self_attention(q, k, v, kv_len)
        result = q.backend.flash_attention_decode_paged(q, lkv.k, lkv.v, kvc.block_table, kvc.visible(seq_len),
                                                        True, kvc.decode_workspace(seq_len))
        result = result.permute(0, 2, 1, 3).contiguous()
        return result.view(batch_size, seq_len, self.n_embd)

    def _extend_attention(self, q, k, v, kv_len, lkv):
        """An extend step on a filled cache: kv_len[b] of the seq_len tokens of row b are real
        (a right-padded batch, any seq_len >= 1). All seq_len projected K / V rows are appended
        at the cache's lengths (the padding rows land in the stale tail, which is never read, or
        are dropped past the capacity), then the queries attend the cache
        (Tensor.flash_attention_extend; a paged or a quantised cache is read in place by the extend
        kernel's own entry points, with the bits a contiguous fp32 copy of the same rows would give)."""
        kvc = lkv.cache
        batch_size, _, seq_len, _ = q.shape
        new_len = _new_token_counts(kv_len, batch_size, seq_len)
        if (kvc.length_host + new_len > kvc.n_positions).any() or seq_len > kvc.n_positions:
            raise ValueError(f"the new tokens do not fit the KV cache ({kvc.n_positions} positions, "
                             f"{int(kvc.length_host.max())} held)")
        q, k = self._rotate_cached(q, k, kvc.length)
        visible, q_len = kvc.extend_counts(new_len)
        if kvc.paged:
            # only the real rows land (count = q_len: there is no stale tail for the padding); the
            # extend kernel reads the pages through the table
            kvc.reserve(kvc.length_host + new_len)
            q.backend.kv_cache_append_paged(k, v, lkv.k, lkv.v, kvc.block_table, kvc.length, q_len)
            result = q.backend.flash_attention_extend_paged(q, lkv.k, lkv.v, kvc.block_table, visible, q_len, True)
        elif kvc.quantised:
            # the extend kernel widens the quantised rows as it stages them
            q.backend.kv_cache_append_quant(k, v, lkv.k, lkv.v, kvc.length, lkv.k_scale, lkv.v_scale)
            result = q.backend.flash_attention_extend_kvq(q, lkv.k, lkv.v, lkv.k_scale, lkv.v_scale, visible,
                                                          q_len, True)
        else:
            q.backend.kv_cache_append(k, v, lkv.k, lkv.v, kvc.length)
            result = q.flash_attention_extend(lkv.k, lkv.v, visible, q_len)
        result = result.permute(0, 2, 1, 3).contiguous()
        return result.view(batch_size, seq_len, self.n_embd)


class FeedForward(Module):
    def __init__(self, n_embd: int, middle_dim: int = 256, p_dropout: float = 0.1, bias: bool = True,
                 backend=None):
        super().__init__()
        self.linear_in = Linear(n_embd, middle_dim, bias=bias, backend=backend)
        self.linear_out = Linear(middle_dim, n_embd, bias=bias, backend=backend)
        self.dropout = Dropout(p_dropout)

    def forward(self, x):
        batch_size, seq_len, n_embd = x.shape
        flat = x.view(batch_size * seq_len, n_embd)
        be = x.backend
        if (getattr(be, "bias_gelu_fw", None) is not None and self.linear_in.bias is not None
                and x._tensor.on_device):
            # linear_in's bias add and the GELU as one kernel each way (BiasGelu)
            from .tensor_functions import BiasGelu
            h = BiasGelu.apply(flat @ self.linear_in.weights.value, self.linear_in.bias.value)
        else:
            h = GELU(self.linear_in(flat))
        return self.dropout(self.linear_out(h)).view(batch_size, seq_len, n_embd)


class TransformerLayer(Module):
    """Pre-LN transformer block (reference :279-362)."""

    def __init__(self, n_embd: int, n_head: int, p_dropout: float = 0.1, ln_eps: float = 1e-8,
                 bias: bool = True, backend=None, use_fused_kernel: bool = False,
                 use_flash_attention: bool = False, causal: bool = True, n_kv_head=None, rope=None):
        super().__init__()
        self.attention = MultiHeadAttention(n_embd, n_head, causal=causal, p_dropout=p_dropout,
                                            bias=bias, backend=backend,
                                            use_fused_kernel=use_fused_kernel,
                                            use_flash_attention=use_flash_attention, n_kv_head=n_kv_head,
                                            rope=rope)
        self.ff = FeedForward(n_embd, 256, p_dropout, bias, backend)
        self.use_fused_kernel = use_fused_kernel
        if use_fused_kernel:
            self.ln_1 = FusedLayerNorm(n_embd, backend)
            self.ln_2 = FusedLayerNorm(n_embd, backend)
        else:
            self.ln_1 = LayerNorm1d(n_embd, ln_eps, backend)
            self.ln_2 = LayerNorm1d(n_embd, ln_eps, backend)

    def forward(self, x, kv_len=None, cache=None):
        batch_size, seq_len, x_dim = x.shape
        a = self.ln_1(x.view(batch_size * seq_len, x_dim)).view(batch_size, seq_len, x_dim)
        a = (self.attention(a, kv_len) if cache is None else self.attention(a, kv_len, cache)) + x
        h = self.ln_2(a.view(batch_size * seq_len, x_dim)).view(batch_size, seq_len, x_dim)
        return self.ff(h) + a


class DecoderLM(Module):
    """Decoder-only pre-LN LM with 4 TransformerLayers (reference :365-470)."""

    # generate(graph=True) keeps device memory on the model: per batch size one KVCache and
    # up to MAX_DECODE_GRAPHS captured steps (one per temperature / top_k / eos_id / top_p / min_p), for the
    # MAX_DECODE_BATCH_SIZES most recently used batch sizes; drop_decode_graphs() frees it all
    MAX_DECODE_GRAPHS = 4
    MAX_DECODE_BATCH_SIZES = 4

    def __init__(self, n_vocab: int, n_embd: int, n_head: int, n_positions: int,
                 p_dropout: float = 0.1, ln_eps: float = 1e-5, bias: bool = True, backend=None,
                 use_fused_kernel: bool = False, use_flash_attention: bool = False, n_layer: int = 4,
                 n_kv_head=None, pos_encoding: str = "learned", rope_theta: float = 10000.0):
        """pos_encoding: "learned" adds a learned position_embeddings row to every token's
        embedding (the reference's model); "rope" has no position parameter: one RotaryTable
        (n_positions rows, base rope_theta), shared by all layers, rotates every layer's Q and K
        (MultiHeadAttention(rope=...)) and the token embeddings are fed alone."""
        super().__init__()
        if pos_encoding not in ("learned", "rope"):
            raise ValueError(f'pos_encoding must be "learned" or "rope", got {pos_encoding!r}')
        self.backend = backend
        self.n_embd = n_embd
        self.n_vocab = n_vocab
        self.n_layer = n_layer
        self.pos_encoding = pos_encoding
        self.token_embeddings = Embedding(n_vocab, n_embd, backend)
        self.rope = None
        if pos_encoding == "rope":
            self.rope = RotaryTable(n_positions, n_embd // n_head, rope_theta, backend=backend)
        else:
            self.position_embeddings = Embedding(n_positions, n_embd, backend)
        for i in range(n_layer):
            setattr(self, f"t_layer_{i + 1}", TransformerLayer(
                n_embd, n_head, p_dropout, ln_eps, bias, backend,
                use_fused_kernel=use_fused_kernel, use_flash_attention=use_flash_attention,
                n_kv_head=n_kv_head, rope=self.rope))
        self.dropout = Dropout(p_dropout)
        self.lm_head = Linear(n_embd, n_vocab, bias, backend)
        self.use_fused_kernel = use_fused_kernel
        self.use_flash_attention = use_flash_attention
        self.n_positions = n_positions
        self.n_head = n_head
        self.n_kv_head = n_head if n_kv_head is None else n_kv_head
        self.ln = FusedLayerNorm(n_embd, backend) if use_fused_kernel else LayerNorm1d(n_embd, ln_eps, backend)
        self.graph_captures = 0  # hipGraph captures of the decode step (generate(graph=True))
        self.spec_stats = None   # the last generate(speculate=...) call's counters

    def forward(self, idx, kv_len=None, cache=None):
        """kv_len: optional valid-token count per batch row of a right-padded batch (keys past
        it are masked in every layer's self-attention; with the causal mask and right padding
        this changes only the outputs at padding positions).
        cache: a KVCache (generation). The tokens of idx continue each row at cache.length[b]:
        an empty cache is prefilled with the prompt (kv_len = the prompt lengths), afterwards
        idx holds at most 8 new tokens per row. The cache's lengths advance by kv_len (prefill)
        or by the number of tokens fed. A filled cache with kv_len given is an extend step
        (_forward_extend): idx is a right-padded batch of any length, row b holding kv_len[b]
        (0 <= kv_len[b] <= T) real new tokens; the cache advances by kv_len."""
        if cache is not None:
            return self._forward_cached(idx, kv_len, cache)
        batch_size, seq_len = idx.shape
        if self.rope is not None:  # rotary: the positions enter in every layer's attention
            h = self.token_embeddings(idx)
        else:
            pos = _positions(seq_len, self.backend)
            h = self.token_embeddings(idx) + self.position_embeddings(pos).view(1, seq_len, self.n_embd)
        h = self.dropout(h)
        for i in range(self.n_layer):
            h = getattr(self, f"t_layer_{i + 1}")(h, kv_len)
        h = self.ln(h.view(batch_size * seq_len, self.n_embd))
        return self.lm_head(h).view(batch_size, seq_len, self.n_vocab)

    def new_cache(self, batch_size: int, kv_dtype=None, page_size=None, n_pages=None):
        """A KVCache for this model and a batch of batch_size rows. kv_dtype: None / "fp32", or
        "bf16" / "fp8" for a quantised cache (KVCache). page_size (a power of two >= 16): a
        PagedKVCache of that page size whose pool holds n_pages pages (None: every row can fill
        up); fp32 pages only."""
        from .kv_cache import KVCache, PagedKVCache
        if page_size is not None:
            return PagedKVCache(self.n_layer, batch_size, self.n_head, self.n_positions, self.n_embd // self.n_head,
                                self.backend, n_kv_head=self.n_kv_head, page_size=page_size, n_pages=n_pages,
                                kv_dtype=kv_dtype)
        if n_pages is not None:
            raise ValueError("new_cache(n_pages=...) needs page_size")
        return KVCache(self.n_layer, batch_size, self.n_head, self.n_positions, self.n_embd // self.n_head,
                       self.backend, n_kv_head=self.n_kv_head, kv_dtype=kv_dtype)

    def _forward_cached(self, idx, kv_len, cache):
        if not self.use_flash_attention:
            raise ValueError("a KV cache needs use_flash_attention=True")
        batch_size, seq_len = idx.shape
        if cache.n_layer != self.n_layer or cache.batch_size != batch_size:
            raise ValueError(f"the KV cache was built for {cache.n_layer} layers and a batch of "
                             f"{cache.batch_size}, got {self.n_layer} and {batch_size}")
        prefill = cache.empty
        if not prefill and kv_len is not None:
            return self._forward_extend(idx, kv_len, cache)
        if not prefill and seq_len > 8:
            raise ValueError(f"a decode step takes at most 8 new tokens per row, got {seq_len}")
        pos = cache.length_host[:, None] + np.arange(seq_len)[None, :]
        if int(pos.max()) >= min(self.n_positions, cache.n_positions):
            raise ValueError(f"position {int(pos.max())} is past n_positions = {self.n_positions}")
        if self.rope is not None:
            h = self.token_embeddings(idx)
        else:
            pos = tensor_from_numpy(np.ascontiguousarray(pos, dtype=datatype), backend=self.backend)
            h = self.token_embeddings(idx) + self.position_embeddings(pos)
        h = self.dropout(h)
        for i in range(self.n_layer):
            h = getattr(self, f"t_layer_{i + 1}")(h, kv_len, cache.layer(i))
        h = self.ln(h.view(batch_size * seq_len, self.n_embd))
        out = self.lm_head(h).view(batch_size, seq_len, self.n_vocab)
        if prefill and kv_len is not None:
            from .tensor import Tensor
            held = kv_len.to_numpy() if isinstance(kv_len, Tensor) else kv_len
            cache.advance(np.asarray(held, dtype=np.int64).reshape(batch_size))
        else:
            cache.advance(seq_len)
        return out

    def _forward_extend(self, idx, kv_len, cache):
        """An extend step: a filled cache and kv_len[b] real new tokens in row b of the
        right-padded idx [B, T], any T >= 1 (continuing a conversation, a chunk of a long prompt,
        draft tokens to verify). Row b's tokens take the positions cache.length[b] + i; the cache
        advances by kv_len. The logits at padding slots are unspecified but finite."""
        batch_size, seq_len = idx.shape
        new_len = _new_token_counts(kv_len, batch_size, seq_len)
        limit = min(self.n_positions, cache.n_positions)
        if (cache.length_host + new_len > limit).any():
            b = int(np.argmax(cache.length_host + new_len))
            raise ValueError(f"row {b} holds {int(cache.length_host[b])} tokens and gets {int(new_len[b])} more: "
                             f"past n_positions = {limit}")
        # padding slots only can pass the last position: they take it (their outputs are discarded)
        pos = np.minimum(cache.length_host[:, None] + np.arange(seq_len)[None, :], self.n_positions - 1)
        if self.rope is not None:
            h = self.token_embeddings(idx)
        else:
            pos = tensor_from_numpy(np.ascontiguousarray(pos, dtype=datatype), backend=self.backend)
            h = self.token_embeddings(idx) + self.position_embeddings(pos)
        h = self.dropout(h)
        for i in range(self.n_layer):
            h = getattr(self, f"t_layer_{i + 1}")(h, new_len, cache.layer(i))
        h = self.ln(h.view(batch_size * seq_len, self.n_embd))
        out = self.lm_head(h).view(batch_size, seq_len, self.n_vocab)
        cache.advance(new_len)
        return out

    def _prefill_logits(self, idx, lens, cache, prefill_chunk):
        """Prefill the right-padded prompts idx [B, T] (lens[b] tokens each) into the empty cache
        and return (logits, rows) for the choice of every prompt's first new token: rows[b] is
        the position in logits [B, ., V] that decides row b (None: the only one). prefill_chunk
        None is one forward over the whole batch; an int C feeds C columns at a time (the first
        chunk as a prefill of the empty cache, the others as extend steps), so the activations
        are bounded by C, and gathers the deciding logits rows into one [B, 1, V] device tensor."""
        if prefill_chunk is None:
            return self.forward(tensor_from_numpy(idx, backend=self.backend), kv_len=lens.astype(datatype),
                                cache=cache), lens - 1
        import torch
        from .hip_kernel_ops import _torch_view, _wrap
        B, T = idx.shape
        first = torch.empty((B, 1, self.n_vocab), dtype=torch.float32, device="cuda")
        for s in range(0, T, prefill_chunk):
            width = min(prefill_chunk, T - s)
            held = np.clip(lens - s, 0, width)
            logits = self.forward(tensor_from_numpy(np.ascontiguousarray(idx[:, s:s + width]), backend=self.backend),
                                  kv_len=held.astype(datatype), cache=cache)
            rows = [b for b in range(B) if s <= lens[b] - 1 < s + width]  # the prompts that end in this chunk
            if rows:
                view = _torch_view(logits)
                r = torch.as_tensor(rows, device=view.device)
                c = torch.as_tensor([int(lens[b]) - 1 - s for b in rows], device=view.device)
                first[r, 0] = view[r, c]
        return _wrap(first.reshape(-1), (B, 1, self.n_vocab), self.backend), None

    def generate(self, prompts, max_new_tokens: int, eos_id=None, use_cache: bool = True,
                 temperature: float = 0.0, top_k: int = 0, seed=None, graph: bool = False, sync_every: int = 8,
                 prefill_chunk=None, kv_dtype=None, page_size=None, speculate=None, ngram: int = 3,
                 top_p=None, min_p=None):
        """Decoding of a list of token-id lists, as the reference's generate
        (project/run_machine_translation.py:271-328); returns the new ids per prompt (without
        the eos that stopped a row). A row also stops once it holds more than n_positions tokens.
        use_cache=False is the reference's loop, one prompt at a time with a full forward over
        the whole prefix per token. use_cache=True right-pads the prompts into one batch,
        prefills a KVCache once and then runs one decode step per token for the whole batch
        (finished rows keep stepping; their outputs are discarded). The model is in eval()
        for the call.

        temperature == 0 (default) is greedy (argmax) decoding. temperature > 0 samples from
        softmax(logits / temperature) over the top_k largest logits (0: all of them), on the
        device (mt_select_token; a backend without the kernel raises): step t of the call draws
        with seed + t and the uniform draw of batch row b (use_cache=False runs every prompt as
        row 0 of its own batch, so its draws differ from the batched legs'). seed=None takes one
        seed from NumPy's global generator (np.random.seed reproduces a run, as for dropout).

        top_p (in (0, 1]; None or 1: off) and min_p (in [0, 1]; None or 0: off) cut the sampled set
        further, in the usual order after temperature and top_k (mt_select_token_p): top_p keeps
        the most probable tokens up to a total probability of top_p (the nucleus; ties at its edge
        enter by index, the most probable token always stays), min_p those of at least min_p
        times the largest probability; the draw is from what both keep, renormalised. Greedy
        decoding ignores them, as it ignores top_k. Every path chooses by the same kernel, so the
        ids of a call do not depend on graph, speculate or the cache kind; a captured graph holds
        both by value, beside temperature and top_k. Unset, nothing changes.

        graph=True (needs use_cache=True and the select_token kernel): the prompt is prefilled
        and the first token chosen eagerly; every further token is one replay of a captured
        hipGraph of the whole step (positions from the cache's device lengths, the token chosen
        and recorded on the device), with no copy to or from the host. The host reads the `done`
        flags every sync_every replays to stop early once every row is finished, and the token
        history once at the end; the returned ids do not depend on sync_every. The graph stays on
        the model, with the KVCache of its batch size, for the next call with the same batch
        size, temperature, top_k, eos_id (held by value in the captured launches) and parameter
        storage (held by address: Parameter.update re-captures); graph_captures counts the
        captures. At most MAX_DECODE_GRAPHS graphs per batch size and MAX_DECODE_BATCH_SIZES
        batch sizes are kept (least recently used go first); drop_decode_graphs() frees them.

        prefill_chunk=C (needs use_cache=True): the padded prompt batch is prefilled C columns at
        a time, the first chunk into the empty cache and the others as extend steps on it
        (Tensor.flash_attention_extend), so the prefill's activations, the [B, C, V] logits among
        them, are bounded by C instead of the longest prompt. The tokens are those of
        prefill_chunk=None; a sampled draw still depends on (seed, b) alone.

        kv_dtype="bf16" / "fp8" (needs use_cache=True): the KV cache is stored quantised (KVCache);
        None / "fp32" is the fp32 cache. The prompt's own attention runs on the fresh fp32 K / V,
        every later step reads the quantised rows, so the ids may differ from the fp32 cache's.
        With prefill_chunk the later chunks already see the quantised prefix, so the ids may also
        differ from those of the one-shot prefill.

        page_size=P (a power of two >= 16; needs use_cache=True, fp32 storage): the KV cache is a
        PagedKVCache whose pool holds the pages the batch can fill,
        sum_b ceil(min(len_b + max_new_tokens, n_positions) / P), instead of B * n_positions rows.
        Every row is reserved to that length before the first step, so the block table is fixed
        while a graph is captured and replays (graph=True budgets at least 3 tokens per row, the
        steps a capture runs). The ids are those of the contiguous cache.

        speculate=k (1..7; needs use_cache=True and the spec_draft / spec_accept kernels; None or 0:
        off, nothing changes): speculative decoding with prompt-lookup drafts. Every step drafts up
        to k tokens per row as the continuation of the latest earlier occurrence of the row's last
        n-gram (the longest n <= ngram, 1..8, that occurs; mt_spec_draft), feeds the last token and
        the drafts through one (k + 1)-token decode step, chooses on the device the token the
        non-speculative path would choose at each of the k + 1 places (token number t of a row
        draws with seed + t and the row's uniform, as above) and keeps the drafts that equal them
        plus one more token (mt_spec_accept), so a step emits 1 to k + 1 tokens per row and the
        ids are those of the same call without speculate, greedy or sampled. The rejected drafts'
        K / V rows stay past the cache's length and are overwritten by the next step. Nothing goes
        through the host inside a step: graph=True replays it from one captured graph (kept per
        batch size, cache kind, k and ngram), graph=False calls it directly; the `done` flags are
        read every sync_every steps. Afterwards spec_stats holds dict(steps, tokens, drafted,
        accepted): the steps run while any row was live, the ids chosen (a stopping eos and every
        row's first token, chosen by the prefill, included), the drafts made and those accepted."""
        prompts = [[int(t) for t in p] for p in prompts]
        if not prompts or any(len(p) == 0 for p in prompts):
            raise ValueError("generate needs at least one prompt and no empty prompt")
        if max(len(p) for p in prompts) > self.n_positions:
            raise ValueError(f"a prompt of {max(len(p) for p in prompts)} tokens is longer than "
                             f"n_positions = {self.n_positions}")
        temperature = float(temperature)
        if not temperature >= 0.0:
            raise ValueError(f"temperature must be >= 0, got {temperature}")
        top_p = 1.0 if top_p is None else float(top_p)
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_p must be None or in (0, 1], got {top_p}")
        min_p = 0.0 if min_p is None else float(min_p)
        if not 0.0 <= min_p <= 1.0:
            raise ValueError(f"min_p must be None or in [0, 1], got {min_p}")
        if kv_dtype == "fp32":
            kv_dtype = None
        if kv_dtype is not None:
            if kv_dtype not in ("bf16", "fp8"):
                raise ValueError(f'kv_dtype must be None, "fp32", "bf16" or "fp8", got {kv_dtype!r}')
            if not use_cache:
                raise ValueError("generate(kv_dtype=...) stores a quantised KV cache: it needs use_cache=True")
        if page_size is not None:
            if int(page_size) != page_size or page_size < 16 or page_size & (int(page_size) - 1):
                raise ValueError(f"page_size must be a power of two >= 16, got {page_size}")
            if not use_cache:
                raise ValueError("generate(page_size=...) pages a KV cache: it needs use_cache=True")
            if kv_dtype is not None:
                raise ValueError("generate(page_size=...) stores fp32 pages: a quantised paged cache "
                                 "(kv_dtype) is not supported")
            page_size = int(page_size)
        if graph and not use_cache:
            raise ValueError("generate(graph=True) replays the cached decode step: it needs use_cache=True")
        if prefill_chunk is not None:
            if not use_cache:
                raise ValueError("generate(prefill_chunk=...) prefills a KV cache: it needs use_cache=True")
            if int(prefill_chunk) != prefill_chunk or prefill_chunk < 1:
                raise ValueError(f"prefill_chunk must be a whole number >= 1, got {prefill_chunk}")
            prefill_chunk = int(prefill_chunk)
        if speculate:  # None / 0: off
            if int(speculate) != speculate or not 1 <= speculate <= 7:
                raise ValueError(f"speculate must be None, 0 or a whole number in 1..7 (a decode step takes "
                                 f"k + 1 <= 8 tokens), got {speculate}")
            if int(ngram) != ngram or not 1 <= ngram <= 8:
                raise ValueError(f"ngram must be a whole number in 1..8, got {ngram}")
            if not use_cache:
                raise ValueError("generate(speculate=...) verifies drafts against a KV cache: it needs use_cache=True")
            if any(getattr(self.backend, f, None) is None for f in ("spec_draft", "spec_accept", "select_token")):
                raise ValueError("generate(speculate=...) drafts and verifies tokens on the device: it needs a "
                                 "backend with the spec_draft / spec_accept and select_token kernels (HipKernelOps)")
            speculate, ngram = int(speculate), int(ngram)
        sampler = None
        if temperature > 0.0 or graph or speculate:
            if getattr(self.backend, "select_token", None) is None:
                raise ValueError("sampling and graph=True choose tokens on the device: they need a backend "
                                 "with the select_token kernel (HipKernelOps)")
            if temperature == 0.0:
                seed = 0  # greedy: never read, and NumPy's generator is left where it was
            elif seed is None:
                seed = int(np.random.randint(0, 2**63 - 1, dtype=np.int64))
            sampler = (temperature, int(top_k), int(seed), top_p, min_p)
        was_training = self.training
        self.eval()
        try:
            if speculate:
                return self._generate_spec(prompts, max_new_tokens, eos_id, sampler, max(1, int(sync_every)),
                                           prefill_chunk, kv_dtype, page_size, speculate, ngram, bool(graph))
            if graph:
                return self._generate_graph(prompts, max_new_tokens, eos_id, sampler, max(1, int(sync_every)),
                                            prefill_chunk, kv_dtype, page_size)
            if temperature == 0.0:
                sampler = None
            if use_cache:
                return self._generate_cached(prompts, max_new_tokens, eos_id, sampler, prefill_chunk, kv_dtype,
                                             page_size)
            return [self._generate_plain(p, max_new_tokens, eos_id, sampler) for p in prompts]
        finally:
            if was_training:
                self.train()

    def _generate_plain(self, prompt, max_new_tokens, eos_id, sampler=None):
        tokens, new = list(prompt), []
        while len(new) < max_new_tokens and len(tokens) <= self.n_positions:
            idx = tensor_from_numpy(np.asarray([tokens], dtype=datatype), backend=self.backend)
            if sampler is None:
                logits = self.forward(idx).to_numpy()
                nxt = int(np.argmax(logits[0, len(tokens) - 1]))
            else:
                nxt = int(self.backend.select_token(self.forward(idx), sampler[0], sampler[1], sampler[2] + len(new),
                                                    top_p=sampler[3], min_p=sampler[4])[1].cpu().numpy()[0])
            if eos_id is not None and nxt == eos_id:
                break
            tokens.append(nxt)
            new.append(nxt)
        return new

    # steps _generate_graph may run on a fresh cache beyond the prompt whatever max_new_tokens: the
    # two warm-up steps of the capture and the captured step itself (their appends are undone by the
    # restore, but each reserves its token's page first)
    GRAPH_CAPTURE_STEPS = 3

    def _paged_budget(self, lens, max_new_tokens, page_size, graph=False):
        """(tokens per row, pages) a paged generate call can fill: row b holds at most
        min(len_b + max_new_tokens, n_positions) tokens. graph=True: at least GRAPH_CAPTURE_STEPS
        tokens past the prompt, so that capturing the step never needs a page the pool lacks (and
        the table never changes inside a capture)."""
        new = max(int(max_new_tokens), self.GRAPH_CAPTURE_STEPS if graph else 0)
        final = np.minimum(lens + new, self.n_positions)
        return final, int((-(-final // page_size)).sum())

    def _generate_cached(self, prompts, max_new_tokens, eos_id, sampler=None, prefill_chunk=None, kv_dtype=None,
                         page_size=None):
        B = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int64)
        T = int(lens.max())
        if page_size is None:
            cache = self.new_cache(B, kv_dtype)
        else:
            final, n_pages = self._paged_budget(lens, max_new_tokens, page_size)
            cache = self.new_cache(B, page_size=page_size, n_pages=n_pages)
            cache.reserve(final)  # the table is final before the first step
        idx = np.zeros((B, T), dtype=datatype)
        for b, p in enumerate(prompts):
            idx[b, :len(p)] = p
        new = [[] for _ in range(B)]
        done = np.zeros(B, dtype=bool)
        if max_new_tokens <= 0:
            return new

        def choose(logits, rows, t):
            # rows: the position per batch row whose logits decide (None: the only one)
            if sampler is None:
                host = logits.to_numpy()
                return np.argmax(host[np.arange(B), rows] if rows is not None else host[:, 0], axis=-1)
            return self.backend.select_token(logits, sampler[0], sampler[1], sampler[2] + t, rows=rows,
                                             top_p=sampler[3], min_p=sampler[4])[1].cpu().numpy()
        nxt = choose(*self._prefill_logits(idx, lens, cache, prefill_chunk), 0)
        t = 0
        while True:
            for b in range(B):
                if done[b]:
                    continue
                if eos_id is not None and int(nxt[b]) == eos_id:
                    done[b] = True
                    continue
                new[b].append(int(nxt[b]))
                # the row holds len(prompt) + len(new) tokens; past n_positions it cannot be fed
                if len(new[b]) >= max_new_tokens or lens[b] + len(new[b]) > self.n_positions:
                    done[b] = True
            if done.all():
                return new
            # a finished row that filled its cache re-writes its last slot (its output is discarded)
            if int(cache.length_host.max()) >= cache.n_positions:
                cache.set_length(np.minimum(cache.length_host, cache.n_positions - 1))
            step = tensor_from_numpy(nxt.astype(datatype).reshape(B, 1), backend=self.backend)
            t += 1
            nxt = choose(self.forward(step, cache=cache), None, t)

    # ---- the decode step that never touches the host, and its graph -----------------------
    def _device_step(self, st: "_DecodeState") -> None:
        """One new token per row with nothing from the host: positions from the cache's device
        lengths (rows that filled the cache step back to its last slot first), the token ids
        from the buffer the previous select_token wrote; append, decode attention and the
        cache's advance as in _forward_cached; then select_token writes the next ids, ORs
        `done` and stores into history[b, step], and the step counter and the seed advance by
        one on the device. Capturable: no to_numpy(), no tensor_from_numpy, no host constant."""
        import torch
        from .tensor import Tensor
        from .tensor_data import TensorData
        cache, B = st.cache, st.cache.batch_size
        cache.clamp_to_last_slot()
        if self.rope is not None:  # the layers read cache.length on the device themselves
            h = self.token_embeddings(st.ids)
        else:
            pos = Tensor(TensorData(cache.length.to(torch.float32), (B, 1)), backend=self.backend)
            h = self.token_embeddings(st.ids) + self.position_embeddings(pos)
        h = self.dropout(h)
        for i in range(self.n_layer):
            h = getattr(self, f"t_layer_{i + 1}")(h, None, cache.layer(i))
        h = self.ln(h.view(B, self.n_embd))
        logits = self.lm_head(h)
        cache.advance(1)
        self.backend.select_token(logits, st.temperature, st.top_k, seed_dev=st.seed, eos_id=st.eos_id,
                                  out=st.ids_dev, out_i32=st.ids_i32, done=st.done, history=st.history,
                                  step_dev=st.step, top_p=st.top_p, min_p=st.min_p)
        st.step.add_(1)
        st.seed.add_(1)

    def drop_decode_graphs(self) -> None:
        """Free the KV caches and captured graphs generate(graph=True) keeps on the model (the
        next such call captures again)."""
        self.__dict__.pop("_decode_graphs", None)

    def _generate_graph(self, prompts, max_new_tokens, eos_id, sampler, sync_every, prefill_chunk=None,
                        kv_dtype=None, page_size=None):
        from .graphs import StepGraph
        if not self.use_flash_attention:
            raise ValueError("a KV cache needs use_flash_attention=True")
        B = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int64)
        new = [[] for _ in range(B)]
        if max_new_tokens <= 0:
            return new
        temperature, top_k, seed, top_p, min_p = sampler
        graphs = self.__dict__.setdefault("_decode_graphs", {})
        slot = B if kv_dtype is None else (B, kv_dtype)  # a quantised cache has buffers and graphs of its own
        if page_size is not None:
            # a paged cache too, per page size and pool size (the captured launches hold the pools)
            final, n_pages = self._paged_budget(lens, max_new_tokens, page_size, graph=True)
            slot = (B, "paged", page_size, n_pages)
        entry = graphs.pop(slot, None)
        if entry is None:
            # per batch size: the buffers (one KVCache) and the graphs captured over them; the
            # last MAX_DECODE_BATCH_SIZES batch sizes are kept
            while len(graphs) >= self.MAX_DECODE_BATCH_SIZES:
                graphs.pop(next(iter(graphs)))
            entry = {"state": _DecodeState(self, B, kv_dtype, page_size, n_pages if page_size else None),
                     "graphs": {}}
        graphs[slot] = entry  # most recently used last
        st = entry["state"]
        st.begin(temperature, top_k, eos_id, seed, top_p, min_p)
        if page_size is not None:
            st.cache.reserve(final)  # the table is final before the first step: nothing changes while a graph replays
        # eager: the prefill (the prompt length varies) and the first token
        T = int(lens.max())
        idx = np.zeros((B, T), dtype=datatype)
        for b, p in enumerate(prompts):
            idx[b, :len(p)] = p
        logits, rows = self._prefill_logits(idx, lens, st.cache, prefill_chunk)
        self.backend.select_token(logits, temperature, top_k, rows=rows, seed_dev=st.seed, eos_id=st.eos_id,
                                  out=st.ids_dev, out_i32=st.ids_i32, done=st.done, history=st.history,
                                  step_dev=st.step, top_p=top_p, min_p=min_p)
        st.step.add_(1)
        st.seed.add_(1)
        # tokens row b can still return: max_new_tokens, or until it holds more than n_positions
        limit = np.minimum(max_new_tokens, self.n_positions - lens + 1)
        total = int(limit.max())
        steps = 1
        step_graph = None
        if total > 1:
            # the captured launches hold the sampling arguments by value (one graph per set of
            # them, the last MAX_DECODE_GRAPHS kept) and the parameters by address
            args = (temperature, top_k, st.eos_id, top_p, min_p)
            params = tuple(p.value._tensor.data_ptr() for p in self.parameters())
            held = entry["graphs"].pop(args, None)
            if held is not None and held[1] == params:
                step_graph = held[0]
            else:
                held = None  # a stale graph's memory goes first
                while len(entry["graphs"]) >= self.MAX_DECODE_GRAPHS:
                    entry["graphs"].pop(next(iter(entry["graphs"])))
                saved = st.snapshot()
                # the graph must die with the model, by reference count: a model <-> step-function
                # cycle would leave the hipGraph to the cyclic collector, which may run inside
                # somebody else's stream capture, where destroying a graph is not allowed
                me = weakref.ref(self)
                step_graph = StepGraph(lambda: me()._device_step(st), warmup=2)  # warm-ups: real steps
                st.restore(saved)
                self.graph_captures = (self.graph_captures or 0) + 1
            entry["graphs"][args] = (step_graph, params)  # most recently used last
        while steps < total:
            step_graph.replay()
            st.cache.mirror_step()
            steps += 1
            if eos_id is not None and (steps - 1) % sync_every == 0:
                fin = st.done.cpu().numpy().astype(bool) | (steps >= limit)
                if fin.all():
                    break
        hist = st.history[:, :steps].cpu().numpy()
        for b in range(B):
            for tok in hist[b]:
                if eos_id is not None and int(tok) == eos_id:
                    break
                new[b].append(int(tok))
                if len(new[b]) >= max_new_tokens or lens[b] + len(new[b]) > self.n_positions:
                    break
        return new

    # ---- speculative decoding: prompt-lookup drafts verified in one (k + 1)-token step ----------
    def _spec_step(self, st: "_SpecState", ngram: int) -> None:
        """One speculative step with nothing from the host (capturable, in the style of
        _device_step): the drafts from the rows' own tokens (spec_draft), the last token and the k
        drafts fed at the positions cache.length + i through the layers' cached decode path (the
        append at cache.length, then the decode kernel on k + 1 query rows), ln and lm_head, then
        spec_accept, which chooses the k + 1 tokens, keeps the accepted run, and advances count,
        held, done and cache.length itself (cache.advance is not called: the rows advance by
        different amounts, known on the device only). The rejected drafts' K / V rows stay past
        cache.length: never read, overwritten by the next step's append."""
        import torch
        from .tensor import Tensor
        from .tensor_data import TensorData
        cache, B, n = st.cache, st.cache.batch_size, st.k + 1
        # a live row holds at most n_positions - 1 cached tokens (its limit forbids more): only a
        # finished row can sit higher, and steps back so that its k + 1 discarded rows fit
        cache.length.clamp_(max=cache.n_positions - n)
        cache._visible = None
        self.backend.spec_draft(st.tokens, st.held, st.k, ngram, feed_f32=st.feed_f32, feed_i32=st.feed_i32,
                                n_draft=st.n_draft)
        if self.rope is not None:  # the layers read cache.length on the device themselves
            h = self.token_embeddings(st.feed)
        else:
            # only discarded slots (past a row's limit) can pass the last position: they take it
            pos = (cache.length[:, None] + st.arange[None, :]).clamp_(max=self.n_positions - 1)
            pos = Tensor(TensorData(pos.to(torch.float32).reshape(-1), (B, n)), backend=self.backend)
            h = self.token_embeddings(st.feed) + self.position_embeddings(pos)
        h = self.dropout(h)
        for i in range(self.n_layer):
            h = getattr(self, f"t_layer_{i + 1}")(h, None, cache.layer(i))
        h = self.ln(h.view(B * n, self.n_embd))
        logits = self.lm_head(h).view(B, n, self.n_vocab)
        self.backend.spec_accept(logits, st.feed_i32, st.n_draft, st.limit, st.count, st.held, st.done, st.tokens,
                                 st.history, scratch=st.scratch, cache_len=cache.length, drafted=st.drafted,
                                 accepted=st.accepted, steps=st.steps, temperature=st.temperature, top_k=st.top_k,
                                 top_p=st.top_p, min_p=st.min_p, seed_dev=st.seed, eos_id=st.eos_id)

    def _generate_spec(self, prompts, max_new_tokens, eos_id, sampler, sync_every, prefill_chunk, kv_dtype,
                       page_size, k, ngram, graph):
        import torch
        from .graphs import StepGraph
        if not self.use_flash_attention:
            raise ValueError("a KV cache needs use_flash_attention=True")
        B = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int64)
        new = [[] for _ in range(B)]
        self.spec_stats = dict(steps=0, tokens=0, drafted=0, accepted=0)
        if max_new_tokens <= 0:
            return new
        temperature, top_k, seed, top_p, min_p = sampler
        final = n_pages = None
        if page_size is not None:
            # the k + 1 rows a step appends are reserved up front too, a finished row's included, so
            # that the table is final before the first step (as the graph path reserves its own)
            final = self._paged_budget(lens, max_new_tokens, page_size, graph=graph)[0]
            final = np.minimum(final + k + 1, -(-(self.n_positions + k) // page_size) * page_size)
            n_pages = int((-(-final // page_size)).sum())
        entry = None
        if graph:
            graphs = self.__dict__.setdefault("_decode_graphs", {})
            slot = ("spec", B, k, kv_dtype, page_size, n_pages)  # the buffers depend on k (the cache's rows)
            entry = graphs.pop(slot, None)
            if entry is None:
                while len(graphs) >= self.MAX_DECODE_BATCH_SIZES:
                    graphs.pop(next(iter(graphs)))
                entry = {"state": _SpecState(self, B, k, kv_dtype, page_size, n_pages), "graphs": {}}
            graphs[slot] = entry  # most recently used last
            st = entry["state"]
        else:
            st = _SpecState(self, B, k, kv_dtype, page_size, n_pages)
        st.begin(temperature, top_k, eos_id, seed, top_p, min_p)
        if page_size is not None:
            st.cache.reserve(final)
        # eager, as without speculation: the prefill and the first token (token number 0: the base seed)
        T = int(lens.max())
        idx = np.zeros((B, T), dtype=datatype)
        for b, p in enumerate(prompts):
            idx[b, :len(p)] = p
        logits, rows = self._prefill_logits(idx, lens, st.cache, prefill_chunk)
        self.backend.select_token(logits, temperature, top_k, rows=rows, seed_dev=st.seed, eos_id=st.eos_id,
                                  out=st.ids_dev, out_i32=st.ids_i32, done=st.done, history=st.history,
                                  step_dev=st.step, top_p=top_p, min_p=min_p)
        # tokens row b can still return: max_new_tokens, or until it holds more than n_positions
        limit = np.minimum(max_new_tokens, self.n_positions - lens + 1)
        st.start(idx, lens, limit)
        # the steps advance the device lengths only; the host mirror stays where the layers' checks
        # of it hold for every step (k + 1 rows fit) and is re-synchronised after the loop
        cache = st.cache
        np.minimum(cache.length_host, self.n_positions - 1, out=cache.length_host)
        cache._visible = None
        total = int(limit.max()) - 1  # every live row emits at least one token per step
        if total > 0:
            me = weakref.ref(self)  # no model <-> step-function cycle (see _generate_graph)
            step = lambda: me()._spec_step(st, ngram)  # noqa: E731
            if graph:
                args = (temperature, top_k, st.eos_id, k, ngram, top_p, min_p)
                params = tuple(p.value._tensor.data_ptr() for p in self.parameters())
                held = entry["graphs"].pop(args, None)
                if held is not None and held[1] == params:
                    step_graph = held[0]
                else:
                    held = None  # a stale graph's memory goes first
                    while len(entry["graphs"]) >= self.MAX_DECODE_GRAPHS:
                        entry["graphs"].pop(next(iter(entry["graphs"])))
                    saved = st.snapshot()
                    step_graph = StepGraph(step, warmup=2)  # warm-ups: real steps
                    st.restore(saved)
                    self.graph_captures = (self.graph_captures or 0) + 1
                entry["graphs"][args] = (step_graph, params)  # most recently used last
                step = step_graph.replay
            for n in range(1, total + 1):
                step()
                if n % sync_every == 0 and n < total and bool(st.done.cpu().numpy().all()):
                    break
        count = st.count.cpu().numpy()
        hist = st.history[:, :int(count.max())].cpu().numpy()
        stats = torch.stack((st.steps, st.drafted, st.accepted)).cpu().numpy()
        cache.length_host[:] = cache.length.cpu().numpy()
        cache._visible = None
        self.spec_stats = dict(steps=int(stats[0].max()), tokens=int(count.sum()), drafted=int(stats[1].sum()),
                               accepted=int(stats[2].sum()))
        for b in range(B):
            for tok in hist[b, :count[b]]:
                if eos_id is not None and int(tok) == eos_id:
                    break
                new[b].append(int(tok))
                if len(new[b]) >= max_new_tokens or lens[b] + len(new[b]) > self.n_positions:
                    break
        return new


class _DecodeState:
    """The device buffers of DecoderLM's captured decode step, for one batch size: the KVCache,
    the token ids the next step feeds (fp32, what mt_embedding_fw reads, and int32), the `done`
    flags, the token history [B, n_positions] (no row returns more tokens than that), the step
    counter and the seed slot."""

    def __init__(self, lm: DecoderLM, batch_size: int, kv_dtype=None, page_size=None, n_pages=None, cache=None):
        import torch
        from .tensor import Tensor
        from .tensor_data import TensorData
        self.cache = lm.new_cache(batch_size, kv_dtype, page_size, n_pages) if cache is None else cache
        self.ids_dev = torch.zeros(batch_size, dtype=torch.float32, device="cuda")
        self.ids = Tensor(TensorData(self.ids_dev, (batch_size, 1)), backend=lm.backend)
        self.ids_i32 = torch.zeros(batch_size, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(batch_size, dtype=torch.int32, device="cuda")
        self.history = torch.zeros((batch_size, lm.n_positions), dtype=torch.int32, device="cuda")
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.seed = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.temperature, self.top_k, self.eos_id = 0.0, 0, None
        self.top_p, self.min_p = 1.0, 0.0

    def begin(self, temperature, top_k, eos_id, seed: int, top_p: float = 1.0, min_p: float = 0.0) -> None:
        """A new call: an empty cache, no row done, step 0, the call's seed."""
        self.temperature, self.top_k = temperature, top_k
        self.top_p, self.min_p = top_p, min_p
        self.eos_id = None if eos_id is None else int(eos_id)
        self.cache.reset()
        self.done.zero_()
        self.step.zero_()
        seed &= 0xFFFFFFFFFFFFFFFF
        self.seed.fill_(seed - (1 << 64) if seed >> 63 else seed)  # the uint64's bits as int64

    def snapshot(self):
        c = self.cache
        return (c.length.clone(), c.length_host.copy(), self.ids_dev.clone(), self.ids_i32.clone(),
                self.done.clone(), self.step.clone(), self.seed.clone())

    def restore(self, saved) -> None:
        c = self.cache
        length, length_host, ids, ids_i32, done, step, seed = saved
        c.length.copy_(length)
        c.length_host[:] = length_host
        c._visible = None
        self.ids_dev.copy_(ids)
        self.ids_i32.copy_(ids_i32)
        self.done.copy_(done)
        self.step.copy_(step)
        self.seed.copy_(seed)


class _SpecState(_DecodeState):
    """_DecodeState for DecoderLM's speculative step with k drafts: a cache of n_positions + k rows
    (the k + 1 rows a step appends fit whatever the row holds; an emitted token never sits at a
    position >= n_positions, its limit forbids it), the rows' tokens [B, S] (prompt and everything
    emitted, S = n_positions + 1), the per-row counters the accept kernel advances (count, held,
    limit; drafted, accepted, steps), the fed tokens [B, k + 1] (fp32, what mt_embedding_fw reads,
    and int32), the draft counts and the scratch of chosen ids. `seed` holds the call's base seed
    throughout: token number t draws with seed + t."""

    def __init__(self, lm: DecoderLM, batch_size: int, k: int, kv_dtype=None, page_size=None, n_pages=None):
        import torch
        from .kv_cache import KVCache, PagedKVCache
        from .tensor import Tensor
        from .tensor_data import TensorData
        args = (lm.n_layer, batch_size, lm.n_head, lm.n_positions + k, lm.n_embd // lm.n_head, lm.backend)
        if page_size is not None:
            cache = PagedKVCache(*args, n_kv_head=lm.n_kv_head, page_size=page_size, n_pages=n_pages)
        else:
            cache = KVCache(*args, n_kv_head=lm.n_kv_head, kv_dtype=kv_dtype)
        super().__init__(lm, batch_size, cache=cache)
        B, n = batch_size, k + 1
        self.k = k
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
        self.tokens = i32(B, max(lm.n_positions + 1, k + 2))
        self.count, self.held, self.limit, self.n_draft = i32(B), i32(B), i32(B), i32(B)
        self.drafted, self.accepted, self.steps = i32(B), i32(B), i32(B)
        self.feed_i32, self.scratch = i32(B, n), i32(B, n)
        self.feed_f32 = torch.zeros(B * n, dtype=torch.float32, device="cuda")
        self.feed = Tensor(TensorData(self.feed_f32, (B, n)), backend=lm.backend)
        self.arange = torch.arange(n, dtype=torch.int32, device="cuda")

    def start(self, idx, lens, limit) -> None:
        """After the prefill and the first token (in ids_i32; done holds its eos flag): the rows'
        tokens are the prompts idx [B, T] (lens[b] each) and that token, count = 1, held = lens + 1;
        a row whose limit is 1 is done; the counters start at 0."""
        import torch
        B, T = idx.shape
        host = np.zeros(tuple(self.tokens.shape), dtype=np.int32)
        host[:, :T] = idx
        self.tokens.copy_(torch.from_numpy(host))
        at = torch.from_numpy(np.asarray(lens, dtype=np.int64)).to("cuda")
        self.tokens[torch.arange(B, device="cuda"), at] = self.ids_i32
        self.count.fill_(1)
        self.held.copy_(torch.from_numpy(np.asarray(lens + 1, dtype=np.int32)))
        self.limit.copy_(torch.from_numpy(np.asarray(limit, dtype=np.int32)))
        self.done |= (self.limit <= 1).to(torch.int32)
        for t in (self.drafted, self.accepted, self.steps):
            t.zero_()

    def snapshot(self):
        return super().snapshot(), tuple(t.clone() for t in (self.count, self.held, self.drafted, self.accepted,
                                                             self.steps))

    def restore(self, saved) -> None:
        # the tokens and the history a warm-up step wrote lie at or past held / count: the replayed
        # steps write the same values there again
        base, mine = saved
        super().restore(base)
        for t, s in zip((self.count, self.held, self.drafted, self.accepted, self.steps), mine):
            t.copy_(s)
