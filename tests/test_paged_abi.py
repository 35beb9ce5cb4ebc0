"""The C ABI of the paged KV cache (include/minitorch_hip.h: mt_flash_attn_decode_paged and its
split / workspace queries, mt_kv_cache_append_paged, mt_kv_cache_gather_paged): symbols, argument
validation before any device call (this runs without a GPU; nothing is launched), and the plan,
which is the plain decode plan at Nk = W * P."""
import ctypes

import pytest

MT_F32, MT_BF16, MT_BF16_F32OUT = 0, 1, 2
SYMS = ("mt_flash_attn_decode_paged", "mt_flash_attn_decode_paged_splits",
        "mt_flash_attn_decode_paged_workspace_bytes", "mt_kv_cache_append_paged", "mt_kv_cache_gather_paged")


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def bufs():
    """Host memory standing in for device pointers: aligned, never dereferenced (every call below
    must be refused first)."""
    raw = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(raw) + 255) // 256 * 256
    return raw, base


def _s3(*v):
    return (ctypes.c_int64 * 3)(*v)


def _decode(lib, dtype, sizes, q=None, k=None, v=None, o=None, strides=(None,) * 4, table=None, ws=None, wsb=0):
    """sizes: (B, H, Hkv, Nq, W, P, n_pages, d)"""
    return lib.mt_flash_attn_decode_paged(dtype, 1, q, k, v, o, None, None, *sizes, *strides, table, None, ws, wsb,
                                          None)


def _plan_sizes(sizes):
    B, H, Hkv, Nq, W, P, _, d = sizes
    return B, H, Hkv, Nq, W, P, d


def test_symbols_and_bindings(lib):
    from minitorch import _hip
    for name in SYMS:
        assert hasattr(lib, name), name
        assert name in _hip.exported_symbols(), name
    assert lib.mt_abi_version() == 3
    for fn in ("flash_decode_paged", "kv_cache_append_paged", "kv_cache_gather_paged", "decode_paged_splits",
               "decode_paged_workspace_bytes"):
        assert callable(getattr(_hip, fn))
    from minitorch.hip_kernel_ops import HipKernelOps
    for fn in ("flash_attention_decode_paged", "kv_cache_append_paged", "kv_cache_gather_paged"):
        assert callable(getattr(HipKernelOps, fn))


# both element sizes at every d that is a whole number of their 16-B chunks (a bf16 row of d = 20 is not)
@pytest.mark.parametrize("dtype,d", [(MT_F32, d) for d in (16, 20, 64, 128, 256)] +
                         [(MT_BF16, d) for d in (16, 64, 128, 256)])
@pytest.mark.parametrize("nq", [1, 4, 8])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (8, 1)])
@pytest.mark.parametrize("B,W,P", [(2, 32, 16), (2, 8, 64), (8, 256, 16), (1, 128, 128), (13, 69, 16)])
def test_plan_is_the_plain_decode_plan(lib, dtype, d, nq, H, Hkv, B, W, P):
    """The splits, span, tile and workspace are mt_flash_attn_decode_gqa's at Nk = W * P: a
    function of the sizes only."""
    span, tile, span0, tile0 = (ctypes.c_int64(0) for _ in range(4))
    n = lib.mt_flash_attn_decode_paged_splits(dtype, B, H, Hkv, nq, W, P, d, ctypes.byref(span), ctypes.byref(tile))
    n0 = lib.mt_flash_attn_decode_gqa_splits(dtype, B, H, Hkv, nq, W * P, d, ctypes.byref(span0), ctypes.byref(tile0))
    assert n >= 1 and (n, span.value, tile.value) == (n0, span0.value, tile0.value)
    want = lib.mt_flash_attn_decode_gqa_workspace_bytes(dtype, B, H, Hkv, nq, W * P, d)
    assert want == (0 if n == 1 else B * H * nq * n * (d + 2) * 4)
    assert lib.mt_flash_attn_decode_paged_workspace_bytes(dtype, B, H, Hkv, nq, W, P, d) == want
    assert lib.mt_flash_attn_decode_paged_splits(dtype, B, H, Hkv, nq, W, P, d, None, None) == n
    # the wave-wide load never straddles a page: it covers at most 16 keys, tile / 4 of them
    assert tile.value // 4 <= 16 <= P


@pytest.mark.parametrize("dtype,sizes,msg", [
    (MT_F32, (2, 4, 4, 1, 32, 24, 64, 64), b"power of two"),
    (MT_F32, (2, 4, 4, 1, 32, 8, 64, 64), b"power of two"),
    (MT_F32, (2, 4, 4, 1, 32, 0, 64, 64), b"power of two"),
    (MT_BF16, (2, 4, 4, 1, 32, 48, 64, 64), b"power of two"),
    (MT_F32, (2, 4, 4, 1, 0, 16, 64, 64), b"block table needs at least one column"),
    (MT_F32, (2, 4, 4, 1, -3, 16, 64, 64), b"block table needs at least one column"),
    (MT_F32, (2, 4, 4, 1, 32, 16, 0, 64), b"pool needs at least one page"),
    (MT_F32, (2, 4, 4, 1, 32, 16, -1, 64), b"pool needs at least one page"),
    (3, (2, 4, 4, 1, 32, 16, 64, 64), b"unsupported dtype"),
    (MT_F32, (2, 4, 4, 0, 32, 16, 64, 64), b"query rows"),
    (MT_F32, (2, 4, 4, 9, 32, 16, 64, 64), b"query rows"),
    (MT_F32, (2, 6, 4, 1, 32, 16, 64, 64), b"kv heads must divide"),
    (MT_BF16, (2, 4, 3, 1, 32, 16, 64, 64), b"kv heads must divide"),
    (MT_F32, (2, 4, 0, 1, 32, 16, 64, 64), b"kv heads must divide"),
    (MT_F32, (2, 4, 4, 1, 32, 16, 64, 260), b"d <= 256"),
    (MT_F32, (2, 4, 4, 1, 32, 16, 64, 18), b"16-B rows"),
    (MT_BF16, (2, 4, 4, 1, 32, 16, 64, 20), b"16-B rows"),
    (MT_BF16_F32OUT, (2, 4, 4, 1, 32, 16, 64, 20), b"16-B rows"),
    (MT_F32, (0, 4, 4, 1, 32, 16, 64, 64), b"bad sizes"),
])
def test_decode_rejects_sizes_before_any_device_call(lib, dtype, sizes, msg):
    assert _decode(lib, dtype, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    if sizes[6] > 0:  # the plan queries take no pool size
        assert lib.mt_flash_attn_decode_paged_splits(dtype, *_plan_sizes(sizes), None, None) <= 0
        assert lib.mt_flash_attn_decode_paged_workspace_bytes(dtype, *_plan_sizes(sizes)) < 0


def test_null_table_is_refused(lib, bufs):
    _, p = bufs
    sizes = (1, 2, 2, 1, 1, 16, 4, 64)  # one split: no workspace
    assert lib.mt_flash_attn_decode_paged_workspace_bytes(MT_F32, *_plan_sizes(sizes)) == 0
    assert _decode(lib, MT_F32, sizes, q=p, k=p, v=p, o=p, table=None) != 0
    assert b"block_table is NULL" in lib.mt_last_error()
    assert lib.mt_kv_cache_append_paged(MT_F32, p, p, p, p, 1, 2, 1, 1, 16, 4, 64, None, None, None, None,
                                        None, p, None, None) != 0
    assert b"block_table is NULL" in lib.mt_last_error()
    assert lib.mt_kv_cache_gather_paged(MT_F32, p, p, p, p, 1, 2, 1, 16, 4, 64, None, None, None, None,
                                        None, None, None) != 0
    assert b"block_table is NULL" in lib.mt_last_error()


@pytest.mark.parametrize("dtype", [MT_F32, MT_BF16])
@pytest.mark.parametrize("d", [16, 64, 256])
def test_workspace_one_byte_short_is_refused(lib, bufs, dtype, d):
    _, p = bufs
    sizes = (2, 4, 1, 3, 32, 16, 64, d)
    need = lib.mt_flash_attn_decode_paged_workspace_bytes(dtype, *_plan_sizes(sizes))
    assert need > 0
    assert _decode(lib, dtype, sizes, table=p, ws=p, wsb=need - 1) != 0
    assert b"workspace too small" in lib.mt_last_error()
    assert _decode(lib, dtype, sizes, table=p, ws=None, wsb=need) != 0
    assert b"workspace too small" in lib.mt_last_error()
    # with a large enough size the next check (NULL tensors) answers, still without a device call
    assert _decode(lib, dtype, sizes, table=p, ws=p, wsb=need) != 0
    assert b"q is NULL" in lib.mt_last_error()


@pytest.mark.parametrize("dtype,esz", [(MT_F32, 4), (MT_BF16, 2)])
def test_misaligned_pointers_and_strides_are_refused(lib, bufs, dtype, esz):
    _, p = bufs
    sizes = (1, 2, 2, 1, 1, 16, 4, 64)  # one split: no workspace
    ok = dict(q=p, k=p, v=p, o=p, table=p)
    for what, arg in (("q", "q"), ("k_pool", "k"), ("v_pool", "v"), ("o", "o")):
        assert _decode(lib, dtype, sizes, **{**ok, arg: p + 8}) != 0
        assert what.encode() in lib.mt_last_error() and b"aligned" in lib.mt_last_error(), lib.mt_last_error()
    # a pool row stride that is not a whole number of 16-B chunks
    bad = _s3(2 * 16 * 64, 16 * 64, 64 + 8 // esz)
    assert _decode(lib, dtype, sizes, **ok, strides=(None, bad, None, None)) != 0
    assert b"k_pool stride" in lib.mt_last_error()
    assert _decode(lib, dtype, sizes, **ok, strides=(None, None, bad, None)) != 0
    assert b"v_pool stride" in lib.mt_last_error()
    assert lib.mt_kv_cache_append_paged(dtype, p, p, p + 8, p, 1, 2, 1, 1, 16, 4, 64, None, None, None, None,
                                        p, p, None, None) != 0
    assert b"k_pool is not 16-B aligned" in lib.mt_last_error()
    assert lib.mt_kv_cache_append_paged(dtype, p, p, p, p, 1, 2, 1, 1, 16, 4, 64, bad, None, None, None,
                                        p, p, None, None) != 0
    assert b"k_new stride" in lib.mt_last_error()
    assert lib.mt_kv_cache_gather_paged(dtype, p, p, p, p + 8, 1, 2, 1, 16, 4, 64, None, None, None, None,
                                        p, None, None) != 0
    assert b"v_out is not 16-B aligned" in lib.mt_last_error()


@pytest.mark.parametrize("dtype,sizes,msg", [
    (5, (2, 2, 1, 8, 16, 32, 64), b"unsupported dtype"),
    (MT_F32, (2, 2, 1, 8, 24, 32, 64), b"power of two"),
    (MT_F32, (2, 2, 1, 8, 8, 32, 64), b"power of two"),
    (MT_F32, (2, 2, 1, 0, 16, 32, 64), b"block table needs at least one column"),
    (MT_F32, (2, 2, 1, 8, 16, 0, 64), b"pool needs at least one page"),
    (MT_F32, (2, 2, 1, 8, 16, 32, 18), b"16-B rows"),
    (MT_BF16, (2, 2, 1, 8, 16, 32, 20), b"16-B rows"),
    (MT_F32, (2, 2, 0, 8, 16, 32, 64), b"bad sizes"),
    (MT_F32, (2, 0, 1, 8, 16, 32, 64), b"bad sizes"),
    (MT_F32, (2, 2, 1, 8, 16, 32, 64), b"block_table is NULL"),
])
def test_append_rejects_before_any_device_call(lib, dtype, sizes, msg):
    """sizes: (B, Hkv, Nq, W, P, n_pages, d)"""
    assert lib.mt_kv_cache_append_paged(dtype, None, None, None, None, *sizes, None, None, None, None,
                                        None, None, None, None) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


def test_append_needs_pos(lib, bufs):
    _, p = bufs
    assert lib.mt_kv_cache_append_paged(MT_F32, p, p, p, p, 2, 2, 1, 8, 16, 32, 64, None, None, None, None,
                                        p, None, None, None) != 0
    assert b"pos is NULL" in lib.mt_last_error()


@pytest.mark.parametrize("dtype,sizes,msg", [
    (7, (2, 2, 8, 16, 32, 64), b"unsupported dtype"),
    (MT_F32, (2, 2, 8, 20, 32, 64), b"power of two"),
    (MT_F32, (2, 2, 0, 16, 32, 64), b"block table needs at least one column"),
    (MT_F32, (2, 2, 8, 16, 0, 64), b"pool needs at least one page"),
    (MT_BF16, (2, 2, 8, 16, 32, 12), b"16-B rows"),
    (MT_F32, (0, 2, 8, 16, 32, 64), b"bad sizes"),
    (MT_F32, (2, 2, 8, 16, 32, 64), b"block_table is NULL"),
])
def test_gather_rejects_before_any_device_call(lib, dtype, sizes, msg):
    """sizes: (B, Hkv, W, P, n_pages, d)"""
    assert lib.mt_kv_cache_gather_paged(dtype, None, None, None, None, *sizes, None, None, None, None,
                                        None, None, None) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


def test_cpu_backend_constructs_without_the_paged_ops():
    import minitorch
    from cpu_backend import NumpyOps
    backend = minitorch.TensorBackend(NumpyOps)
    assert backend.kv_cache_append_paged is None
    assert backend.flash_attention_decode_paged is None
    assert backend.kv_cache_gather_paged is None
    with pytest.raises(ValueError, match="paged-cache kernels"):
        minitorch.PagedKVCache(1, 1, 2, 32, 16, backend)
