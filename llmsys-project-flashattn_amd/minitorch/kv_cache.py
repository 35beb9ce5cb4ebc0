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
(``mt_flash_attn_decode_kvq``) and so does an extend step (``mt_flash_attn_extend_kvq``, which
widens the rows as it stages them): no fp32 copy of the cache exists.

``PagedKVCache`` keeps the rows in pages of a pool instead, addressed through a block table
(``PageAllocator`` is its host-side free list with reference counts): memory follows the tokens
held, finished rows give their pages back, and rows can share the pages of a common prefix.
"""
from __future__ import annotations

import numpy as np

from .tensor import Tensor
from .tensor_data import TensorData

__all__ = ["KVCache", "LayerKV", "PagedKVCache", "PageAllocator", "PoolExhausted"]


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
    paged = False  # PagedKVCache: True

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
                   for f in ("kv_cache_append_quant", "flash_attention_decode_kvq", "flash_attention_extend_kvq")):
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

        self._numel = numel

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


class PoolExhausted(RuntimeError):
    """The page pool has fewer free pages than a request needs; nothing was changed."""


class PageAllocator:
    """The pages of one pool: a free list and a reference count per page. Host code only (no torch,
    no device). A page is held by every block-table entry that names it: ``alloc`` hands out pages
    with one reference, ``retain`` adds one, ``release`` drops one and returns the page to the
    free list with the last."""

    def __init__(self, n_pages: int):
        if int(n_pages) != n_pages or n_pages <= 0:
            raise ValueError(f"PageAllocator: n_pages must be a whole number >= 1, got {n_pages}")
        self.n_pages = int(n_pages)
        self._free = list(range(self.n_pages - 1, -1, -1))  # a stack: page 0 goes first
        self._refs = [0] * self.n_pages

    @property
    def n_free(self) -> int:
        return len(self._free)

    def refcount(self, page: int) -> int:
        return self._refs[self._check(page)]

    def _check(self, page) -> int:
        p = int(page)
        if p != page or not 0 <= p < self.n_pages:
            raise ValueError(f"PageAllocator: {page!r} is not a page of this pool (0..{self.n_pages - 1})")
        return p

    def alloc(self, n: int = 1) -> list:
        """n free pages, each with one reference. Raises PoolExhausted, before anything is changed,
        when fewer than n are free."""
        if n < 0:
            raise ValueError(f"PageAllocator: cannot allocate {n} pages")
        if n > len(self._free):
            raise PoolExhausted(f"the page pool is exhausted: {n} pages wanted, {len(self._free)} of "
                                f"{self.n_pages} free")
        pages = [self._free.pop() for _ in range(n)]
        for p in pages:
            self._refs[p] = 1
        return pages

    def retain(self, page: int) -> None:
        p = self._check(page)
        if self._refs[p] <= 0:
            raise ValueError(f"PageAllocator: page {p} is free, it cannot be retained")
        self._refs[p] += 1

    def release(self, page: int) -> None:
        p = self._check(page)
        if self._refs[p] <= 0:
            raise ValueError(f"PageAllocator: page {p} is already free (released twice?)")
        self._refs[p] -= 1
        if self._refs[p] == 0:
            self._free.append(p)


class PagedKVCache:
    """A KV cache whose rows live in pages of ``page_size`` tokens taken from one pool per layer
    and per K / V, addressed through one block table shared by the layers: memory follows the
    tokens actually held, a finished row gives its pages back (``free_row``) and rows may share
    the pages of a common prefix (``share_prefix``).

    Per layer the pools are ``[n_pages, page_size, Hkv, d]`` fp32 storage, seen by the kernels as
    ``[n_pages, Hkv, page_size, d]`` through strides. ``block_table`` is a device int32 ``[B, W]``
    at a fixed address, ``W = ceil(n_positions / page_size)``: logical token j of row b is row
    ``j % page_size`` of page ``block_table[b, j // page_size]``; an unallocated entry is -1. The
    host keeps the table's mirror and the allocator; the device copy is refreshed only when a page
    is taken or given back. One write rule: a row never appends into a page whose reference count
    exceeds 1; ``reserve`` and ``set_length`` give the row a private copy of such a page first.

    It exposes what the model uses of ``KVCache``. A decode step appends through the table
    (``mt_kv_cache_append_paged``) and reads the pages directly (``mt_flash_attn_decode_paged``);
    an extend step does the same (``mt_flash_attn_extend_paged``): the pools and the table are all
    the device memory the cache holds."""

    paged = True
    quantised = False
    kv_dtype = "fp32"

    def __init__(self, n_layer: int, batch_size: int, n_head: int, n_positions: int, head_dim: int, backend,
                 n_kv_head=None, page_size: int = 16, n_pages=None, kv_dtype=None):
        if kv_dtype not in (None, "fp32"):
            raise ValueError(f"PagedKVCache stores fp32 pages: kv_dtype={kv_dtype!r} is not supported "
                             "(a quantised paged cache is out of scope)")
        if any(getattr(backend, f, None) is None
               for f in ("kv_cache_append_paged", "flash_attention_decode_paged", "flash_attention_extend_paged")):
            raise ValueError("PagedKVCache needs a backend with the paged-cache kernels (HipKernelOps)")
        if int(page_size) != page_size or page_size < 16 or page_size & (page_size - 1):
            raise ValueError(f"PagedKVCache: page_size must be a power of two >= 16, got {page_size}")
        if head_dim % 4 != 0 or head_dim > 256:
            raise ValueError(f"PagedKVCache: head_dim {head_dim} is not supported by the decode kernel "
                             "(fp32 rows must be a multiple of 16 bytes: head_dim % 4 == 0, head_dim <= 256)")
        if min(n_layer, batch_size, n_head, n_positions) <= 0:
            raise ValueError("PagedKVCache: sizes must be positive")
        if n_kv_head is None:
            n_kv_head = n_head
        if n_kv_head <= 0 or n_head % n_kv_head:
            raise ValueError(f"PagedKVCache: n_kv_head = {n_kv_head} does not divide n_head = {n_head}")
        import torch
        self.n_layer, self.batch_size, self.n_head = n_layer, batch_size, n_head
        self.n_kv_head = n_kv_head
        self.n_positions, self.head_dim, self.backend = n_positions, head_dim, backend
        self.page_size = P = int(page_size)
        self.width = W = (n_positions + P - 1) // P
        if n_pages is None:
            n_pages = batch_size * W
        self.allocator = PageAllocator(n_pages)
        self.n_pages = self.allocator.n_pages
        page = P * n_kv_head * head_dim
        shape = (self.n_pages, n_kv_head, P, head_dim)
        strides = (page, head_dim, n_kv_head * head_dim, 1)

        def pool():
            return torch.as_strided(torch.empty(self.n_pages * page, dtype=torch.float32, device="cuda"),
                                    shape, strides)
        self.layers = [LayerKV(self, pool(), pool()) for _ in range(n_layer)]
        self.table_host = np.full((batch_size, W), -1, dtype=np.int32)
        self.block_table = torch.full((batch_size, W), -1, dtype=torch.int32, device="cuda")
        self._shared = False      # share_prefix was used: a page may have more than one reference
        self._reserved = None     # (lengths, new_lengths) of the last reserve, while the table is as it left it
        self._workspaces = {}     # the decode workspace per number of new tokens
        self.length = torch.zeros(batch_size, dtype=torch.int32, device="cuda")
        self.length_host = np.zeros(batch_size, dtype=np.int64)
        self._visible = None

    # what the model uses of KVCache, unchanged (they touch length / length_host / _visible only)
    layer = KVCache.layer
    empty = KVCache.empty
    visible = KVCache.visible
    extend_counts = KVCache.extend_counts
    clamp_to_last_slot = KVCache.clamp_to_last_slot
    mirror_step = KVCache.mirror_step
    advance = KVCache.advance

    @property
    def pages_free(self) -> int:
        return self.allocator.n_free

    @property
    def nbytes(self) -> int:
        """Device bytes of the K and V pools over all layers and of the block table."""
        pools = self.n_layer * 2 * self.n_pages * self.page_size * self.n_kv_head * self.head_dim * 4
        return pools + self.table_host.size * 4

    def refcount(self, page: int) -> int:
        return self.allocator.refcount(page)

    def decode_workspace(self, n_new: int):
        """The split-KV workspace of a decode step of n_new tokens (None when the plan has one
        split), shared by the layers and kept, so that a captured step allocates nothing."""
        import torch
        from . import _hip
        if n_new not in self._workspaces:
            need = _hip.decode_paged_workspace_bytes(_hip.MT_F32, self.batch_size, self.n_head, n_new, self.width,
                                                     self.page_size, self.head_dim, self.n_kv_head)
            self._workspaces[n_new] = torch.empty(need // 4, dtype=torch.float32, device="cuda") if need else None
        return self._workspaces[n_new]

    # ---- pages ---------------------------------------------------------------------------------
    def _push_table(self) -> None:
        import torch
        self.block_table.copy_(torch.from_numpy(self.table_host))

    def _push_length(self) -> None:
        import torch
        self.length.copy_(torch.from_numpy(self.length_host.astype(np.int32)))
        self._visible = None

    def _make_room(self, exist, wfirst, wlast) -> None:
        """Per row b: the table entries below ceil(exist[b] / P) get a page where they have none, and
        the entries in [wfirst[b], wlast[b]) that name a shared page get a private copy of it. All
        or nothing: PoolExhausted is raised before the table, the counts or the pools change."""
        import torch
        P = self.page_size
        fresh, copies, drops = [], [], {}
        for b in range(self.batch_size):
            for idx in range(-(-int(exist[b]) // P)):
                pg = int(self.table_host[b, idx])
                if pg < 0:
                    fresh.append((b, idx))
                elif wfirst[b] <= idx < wlast[b] and self.allocator.refcount(pg) - drops.get(pg, 0) > 1:
                    copies.append((b, idx, pg))
                    drops[pg] = drops.get(pg, 0) + 1
        if not fresh and not copies:
            return
        pages = self.allocator.alloc(len(fresh) + len(copies))  # raises before anything is changed
        self._reserved = None
        for (b, idx), pg in zip(fresh, pages):
            self.table_host[b, idx] = pg
        if copies:
            new = pages[len(fresh):]
            dst = torch.as_tensor(new, device="cuda")
            src = torch.as_tensor([pg for _, _, pg in copies], device="cuda")
            for lkv in self.layers:
                lkv.k[dst] = lkv.k[src]
                lkv.v[dst] = lkv.v[src]
            for (b, idx, old), pg in zip(copies, new):
                self.table_host[b, idx] = pg
                self.allocator.release(old)
        self._push_table()

    def reserve(self, new_lengths) -> None:
        """Make room for row b to grow to new_lengths[b] tokens (host counts): its missing pages are
        taken from the pool, and a shared page the new tokens would land in is replaced by a
        private copy. The device table is copied only when a page was taken. Raises PoolExhausted,
        leaving the cache as it was, when the pool cannot give the pages."""
        new = np.minimum(np.asarray(new_lengths, dtype=np.int64).reshape(self.batch_size),
                         self.width * self.page_size)
        cur = self.length_host
        # one step calls this once per layer: only the first call can find anything to do
        if self._reserved is not None and np.array_equal(self._reserved[0], cur) and \
                np.array_equal(self._reserved[1], new):
            return
        P = self.page_size
        grow = new > cur
        need = np.where(grow, -(-new // P), 0)
        # the usual step has nothing to do: every page is there already and nothing is shared (a
        # row's pages are a prefix of its table row)
        if self._shared or not ((self.table_host >= 0).sum(axis=1) >= need).all():
            self._make_room(np.where(grow, new, 0), cur // P, need)
        # what the decode kernel cannot detect (it clamps a table entry, it does not refuse it): every
        # row's pages are a prefix of its table row and cover the tokens it holds and is about to get
        held = self.table_host >= 0
        if (held[:, 1:] > held[:, :-1]).any() or (held.sum(axis=1) < -(-np.maximum(cur, new) // P)).any():
            raise RuntimeError("PagedKVCache: the block table does not cover the rows' tokens "
                               f"(lengths {cur.tolist()}, reserved to {new.tolist()})")
        self._reserved = (cur.copy(), new.copy())

    def set_length(self, lengths) -> None:
        """Set the per-row token counts (host values, copied to the device). The pages a row needs
        to hold its count are taken where missing; a row set to end inside a shared page gets a
        private copy of that page (the next append lands there). Pages past the count stay with
        the row (free_row gives them back)."""
        a = np.asarray(lengths, dtype=np.int64).reshape(self.batch_size)
        if (a < 0).any() or (a > self.n_positions).any():
            raise ValueError(f"PagedKVCache: lengths must be in [0, {self.n_positions}]")
        P = self.page_size
        self._make_room(a, a // P, a // P + (a % P != 0))
        self.length_host[:] = a
        self._push_length()

    def _drop_row(self, b: int) -> None:
        for pg in self.table_host[b]:
            if pg >= 0:
                self.allocator.release(int(pg))
        self.table_host[b] = -1
        self.length_host[b] = 0
        self._reserved = None

    def free_row(self, b: int) -> None:
        """Give row b's pages back (a shared page loses one reference) and set its length to 0: the
        next extend step can put a new prompt there."""
        if not 0 <= b < self.batch_size:
            raise ValueError(f"PagedKVCache: row {b} is not in a batch of {self.batch_size}")
        self._drop_row(b)
        self._push_table()
        self._push_length()

    def reset(self) -> None:
        had = bool((self.table_host >= 0).any())
        for b in range(self.batch_size):
            self._drop_row(b)
        if had:
            self._push_table()
        self._shared = False
        self.length.zero_()
        self._visible = None

    def share_prefix(self, src: int, dst_rows, n_tokens: int) -> None:
        """The rows dst_rows take the first n_tokens tokens of row src: the n_tokens // P full pages
        by reference, the rows of a partial last page copied into a fresh page per destination row,
        in every layer. What the destination rows held is given back first; their lengths become
        n_tokens. Raises PoolExhausted before anything is changed."""
        P = self.page_size
        dst_rows = [int(r) for r in dst_rows]
        if not 0 <= src < self.batch_size or any(not 0 <= r < self.batch_size or r == src for r in dst_rows):
            raise ValueError(f"PagedKVCache.share_prefix: bad rows src={src}, dst={dst_rows}")
        if len(set(dst_rows)) != len(dst_rows):
            raise ValueError(f"PagedKVCache.share_prefix: a destination row is named twice: {dst_rows}")
        if not 0 < n_tokens <= int(self.length_host[src]):
            raise ValueError(f"PagedKVCache.share_prefix: row {src} holds {int(self.length_host[src])} tokens, "
                             f"cannot share {n_tokens}")
        full, part = n_tokens // P, n_tokens % P
        held = {}
        for r in dst_rows:
            for pg in self.table_host[r]:
                if pg >= 0:
                    held[int(pg)] = held.get(int(pg), 0) + 1
        freed = sum(1 for pg, c in held.items() if self.allocator.refcount(pg) == c)
        need = len(dst_rows) if part else 0
        if need > self.allocator.n_free + freed:
            raise PoolExhausted(f"the page pool is exhausted: share_prefix needs {need} pages, "
                                f"{self.allocator.n_free + freed} would be free")
        self._shared = True
        self._reserved = None
        for r in dst_rows:
            self._drop_row(r)
        for r in dst_rows:
            for idx in range(full):
                pg = int(self.table_host[src, idx])
                self.allocator.retain(pg)
                self.table_host[r, idx] = pg
            if part:
                pg = self.allocator.alloc(1)[0]
                old = int(self.table_host[src, full])
                for lkv in self.layers:
                    lkv.k[pg, :, :part] = lkv.k[old, :, :part]
                    lkv.v[pg, :, :part] = lkv.v[old, :, :part]
                self.table_host[r, full] = pg
            self.length_host[r] = n_tokens
        self._push_table()
        self._push_length()
