"""The C ABI of the extend step on a paged and on a quantised cache (include/minitorch_hip.h:
mt_flash_attn_extend_paged, mt_flash_attn_extend_kvq and their plan queries): symbols and bindings,
the plans (mt_flash_attn_extend_plan's at Nk = W * P, respectively for MT_F32), and every refusal
with its message before any device call (this runs without a GPU; nothing is launched)."""
import ctypes

import pytest

MT_F32, MT_BF16, MT_BF16_F32OUT = 0, 1, 2
KV_BF16, KV_FP8 = 1, 2
CAP = 1100
SYMS = ("mt_flash_attn_extend_paged_plan", "mt_flash_attn_extend_paged", "mt_flash_attn_extend_kvq_plan",
        "mt_flash_attn_extend_kvq")


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


def _paged(lib, dtype, sizes, q=None, k=None, v=None, o=None, strides=(None,) * 4, table=None):
    """sizes: (B, H, Hkv, Nq, W, P, n_pages, d)"""
    return lib.mt_flash_attn_extend_paged(dtype, 1, q, k, v, o, None, None, *sizes, *strides, table, None, None, None)


def _kvq(lib, kv, sizes, q=None, k=None, v=None, ks=None, vs=None, o=None, strides=(None,) * 4):
    """sizes: (B, H, Hkv, Nq, Nk, d)"""
    return lib.mt_flash_attn_extend_kvq(kv, 1, q, k, v, ks, vs, o, None, None, *sizes, *strides, None, None, None)


def _paged_plan_sizes(sizes):
    B, H, Hkv, Nq, W, P, _, d = sizes
    return B, H, Hkv, Nq, W, P, d


def test_symbols_and_bindings(lib):
    from minitorch import _hip
    for name in SYMS:
        assert hasattr(lib, name), name
        assert name in _hip.exported_symbols(), name
    for fn in ("flash_extend_paged", "flash_extend_kvq", "extend_paged_plan", "extend_kvq_plan"):
        assert callable(getattr(_hip, fn))
    from minitorch.hip_kernel_ops import HipKernelOps
    for fn in ("flash_attention_extend_paged", "flash_attention_extend_kvq"):
        assert callable(getattr(HipKernelOps, fn))


# ---- plans ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [(MT_F32, d) for d in (16, 20, 64, 128, 256)] +
                         [(MT_BF16, d) for d in (16, 64, 128, 256)] + [(MT_BF16_F32OUT, 64)])
@pytest.mark.parametrize("nq", [1, 4, 8, 168])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (8, 1)])
@pytest.mark.parametrize("B,W,P", [(2, 32, 16), (2, 8, 64), (8, 256, 16), (1, 128, 128), (13, 69, 16)])
def test_paged_plan_is_the_plain_extend_plan(lib, dtype, d, nq, H, Hkv, B, W, P):
    bq, bk, bq0, bk0 = (ctypes.c_int64(0) for _ in range(4))
    kid = lib.mt_flash_attn_extend_paged_plan(dtype, B, H, Hkv, nq, W, P, d, ctypes.byref(bq), ctypes.byref(bk))
    kid0 = lib.mt_flash_attn_extend_plan(dtype, B, H, Hkv, nq, W * P, d, ctypes.byref(bq0), ctypes.byref(bk0))
    assert kid >= 0 and (kid, bq.value, bk.value) == (kid0, bq0.value, bk0.value)
    assert lib.mt_flash_attn_extend_paged_plan(dtype, B, H, Hkv, nq, W, P, d, None, None) == kid


@pytest.mark.parametrize("kv", [KV_BF16, KV_FP8])
@pytest.mark.parametrize("nq", [1, 3, 8, 40])
@pytest.mark.parametrize("d", [8, 40, 64, 128, 256])
@pytest.mark.parametrize("B,H,Hkv,Nk", [(13, 2, 2, CAP), (2, 8, 2, CAP), (8, 16, 16, 4096), (1, 16, 4, 16384),
                                        (64, 8, 8, 40)])
def test_kvq_plan_is_the_fp32_extend_plan(lib, kv, nq, d, B, H, Hkv, Nk):
    bq, bk, bq0, bk0 = (ctypes.c_int64(0) for _ in range(4))
    kid = lib.mt_flash_attn_extend_kvq_plan(kv, B, H, Hkv, nq, Nk, d, ctypes.byref(bq), ctypes.byref(bk))
    kid0 = lib.mt_flash_attn_extend_plan(MT_F32, B, H, Hkv, nq, Nk, d, ctypes.byref(bq0), ctypes.byref(bk0))
    assert 0 <= kid <= 3 and (kid, bq.value, bk.value) == (kid0, bq0.value, bk0.value)
    assert lib.mt_flash_attn_extend_kvq_plan(kv, B, H, Hkv, nq, Nk, d, None, None) == kid


# ---- refusals: the paged entry point ------------------------------------------------------------------
@pytest.mark.parametrize("dtype,sizes,msg", [
    (MT_F32, (2, 4, 4, 9, 32, 24, 64, 64), b"power of two"),
    (MT_F32, (2, 4, 4, 9, 32, 8, 64, 64), b"power of two"),
    (MT_F32, (2, 4, 4, 9, 32, 0, 64, 64), b"power of two"),
    (MT_BF16, (2, 4, 4, 9, 32, 48, 64, 64), b"power of two"),
    (MT_F32, (2, 4, 4, 9, 0, 16, 64, 64), b"block table needs at least one column"),
    (MT_F32, (2, 4, 4, 9, -3, 16, 64, 64), b"block table needs at least one column"),
    (MT_F32, (2, 4, 4, 9, 32, 16, 0, 64), b"pool needs at least one page"),
    (MT_F32, (2, 4, 4, 9, 32, 16, -1, 64), b"pool needs at least one page"),
    (3, (2, 4, 4, 9, 32, 16, 64, 64), b"unsupported dtype"),
    (MT_F32, (2, 4, 4, 0, 32, 16, 64, 64), b"at least one query row"),
    (MT_F32, (2, 4, 4, 513, 32, 16, 64, 64), b"at most Nk query rows"),
    (MT_F32, (2, 6, 4, 9, 32, 16, 64, 64), b"kv heads must divide"),
    (MT_BF16, (2, 4, 3, 9, 32, 16, 64, 64), b"kv heads must divide"),
    (MT_F32, (2, 4, 0, 9, 32, 16, 64, 64), b"kv heads must divide"),
    (MT_F32, (2, 4, 4, 9, 32, 16, 64, 260), b"d <= 256"),
    (MT_F32, (2, 4, 4, 9, 32, 16, 64, 18), b"16-B rows"),
    (MT_BF16, (2, 4, 4, 9, 32, 16, 64, 20), b"16-B rows"),
    (MT_BF16_F32OUT, (2, 4, 4, 9, 32, 16, 64, 20), b"16-B rows"),
    (MT_F32, (0, 4, 4, 9, 32, 16, 64, 64), b"bad sizes"),
])
def test_paged_rejects_sizes_before_any_device_call(lib, dtype, sizes, msg):
    assert _paged(lib, dtype, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    if sizes[6] > 0:  # the plan query takes no pool size
        assert lib.mt_flash_attn_extend_paged_plan(dtype, *_paged_plan_sizes(sizes), None, None) < 0
        assert msg in lib.mt_last_error(), lib.mt_last_error()


def test_paged_nq_up_to_the_capacity_is_a_size_the_plan_takes(lib):
    assert lib.mt_flash_attn_extend_paged_plan(MT_F32, 2, 4, 4, 512, 32, 16, 64, None, None) >= 0


def test_paged_null_table_and_null_tensors_are_refused(lib, bufs):
    _, p = bufs
    sizes = (1, 2, 2, 9, 2, 16, 4, 64)
    assert _paged(lib, MT_F32, sizes, q=p, k=p, v=p, o=p, table=None) != 0
    assert b"block_table is NULL" in lib.mt_last_error()
    assert _paged(lib, MT_F32, sizes, q=p, k=p, v=p, o=p, table=p + 2) != 0
    assert b"block_table is not 4-B aligned" in lib.mt_last_error()
    for arg, what in (("q", b"q is NULL"), ("k", b"k_pool is NULL"), ("v", b"v_pool is NULL"), ("o", b"o is NULL")):
        assert _paged(lib, MT_F32, sizes, **{**dict(q=p, k=p, v=p, o=p, table=p), arg: None}) != 0
        assert what in lib.mt_last_error(), lib.mt_last_error()


@pytest.mark.parametrize("dtype,esz", [(MT_F32, 4), (MT_BF16, 2)])
def test_paged_misaligned_pointers_and_strides_are_refused(lib, bufs, dtype, esz):
    _, p = bufs
    sizes = (1, 2, 2, 9, 2, 16, 4, 64)
    ok = dict(q=p, k=p, v=p, o=p, table=p)
    for what, arg in (("q", "q"), ("k_pool", "k"), ("v_pool", "v"), ("o", "o")):
        assert _paged(lib, dtype, sizes, **{**ok, arg: p + 8}) != 0
        assert what.encode() in lib.mt_last_error() and b"aligned" in lib.mt_last_error(), lib.mt_last_error()
    bad = _s3(2 * 16 * 64, 16 * 64, 64 + 8 // esz)  # a row stride that is not a whole number of 16-B chunks
    for i, what in enumerate((b"q stride", b"k_pool stride", b"v_pool stride", b"o stride")):
        strides = [None] * 4
        strides[i] = bad
        assert _paged(lib, dtype, sizes, **ok, strides=tuple(strides)) != 0
        assert what in lib.mt_last_error(), lib.mt_last_error()


# ---- refusals: the quantised entry point ----------------------------------------------------------------
@pytest.mark.parametrize("kv,sizes,msg", [
    (0, (2, 2, 2, 9, CAP, 64), b"unsupported kv_dtype"),
    (3, (2, 2, 2, 9, CAP, 64), b"unsupported kv_dtype"),
    (-1, (2, 2, 2, 9, CAP, 64), b"unsupported kv_dtype"),
    (KV_BF16, (2, 2, 2, 9, CAP, 20), b"multiple of 8"),
    (KV_FP8, (2, 2, 2, 9, CAP, 36), b"multiple of 8"),
    (KV_FP8, (2, 2, 2, 9, CAP, 18), b"16-B rows"),
    (KV_BF16, (2, 2, 2, 9, CAP, 264), b"d <= 256"),
    (KV_BF16, (2, 2, 2, 0, CAP, 64), b"at least one query row"),
    (KV_FP8, (2, 2, 2, CAP + 1, CAP, 64), b"at most Nk query rows"),
    (KV_BF16, (2, 6, 4, 9, CAP, 64), b"kv heads must divide"),
    (KV_FP8, (2, 4, 0, 9, CAP, 64), b"kv heads must divide"),
    (KV_BF16, (0, 2, 2, 9, CAP, 64), b"bad sizes"),
    (KV_FP8, (2, 2, 2, 9, 0, 64), b"bad sizes"),
])
def test_kvq_rejects_sizes_before_any_device_call(lib, kv, sizes, msg):
    assert _kvq(lib, kv, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    assert lib.mt_flash_attn_extend_kvq_plan(kv, *sizes, None, None) < 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


def test_kvq_fp8_needs_both_scales(lib, bufs):
    _, p = bufs
    sizes = (1, 2, 2, 9, 16, 64)
    for ks, vs in ((None, p), (p, None), (None, None)):
        assert _kvq(lib, KV_FP8, sizes, q=p, k=p, v=p, ks=ks, vs=vs, o=p) != 0
        assert b"a scale pointer is NULL" in lib.mt_last_error()
    assert _kvq(lib, KV_FP8, sizes, q=p, k=p, v=p, ks=p + 2, vs=p, o=p) != 0
    assert b"k_scale / v_scale is not 4-B aligned" in lib.mt_last_error()
    # bf16 ignores the scales: the next check (NULL tensors) answers, still without a device call
    assert _kvq(lib, KV_BF16, sizes, q=None, k=p, v=p, o=p) != 0
    assert b"q is NULL" in lib.mt_last_error()


@pytest.mark.parametrize("kv,row", [(KV_BF16, 16), (KV_FP8, 8)])
def test_kvq_misaligned_pointers_and_strides_are_refused(lib, bufs, kv, row):
    _, p = bufs
    sizes = (1, 2, 2, 9, 16, 64)
    ok = dict(q=p, k=p, v=p, ks=p, vs=p, o=p)
    for what, arg, off in (("q", "q", 8), ("k_cache", "k", row // 2), ("v_cache", "v", row // 2), ("o", "o", 8)):
        assert _kvq(lib, kv, sizes, **{**ok, arg: p + off}) != 0
        assert what.encode() in lib.mt_last_error() and b"aligned" in lib.mt_last_error(), lib.mt_last_error()
        assert _kvq(lib, kv, sizes, **{**ok, arg: None}) != 0
        assert (what + " is NULL").encode() in lib.mt_last_error(), lib.mt_last_error()
    esz = 2 if kv == KV_BF16 else 1
    bad = _s3(2 * 16 * 64, 16 * 64, 64 + row // 2 // esz)  # a cache row stride of half a chunk more
    for i, what in ((1, b"k_cache stride"), (2, b"v_cache stride")):
        strides = [None] * 4
        strides[i] = bad
        assert _kvq(lib, kv, sizes, **ok, strides=tuple(strides)) != 0
        assert what in lib.mt_last_error(), lib.mt_last_error()
    badq = _s3(2 * 9 * 64, 9 * 64, 66)  # an fp32 row stride of 8 bytes more
    for i, what in ((0, b"q stride"), (3, b"o stride")):
        strides = [None] * 4
        strides[i] = badq
        assert _kvq(lib, kv, sizes, **ok, strides=tuple(strides)) != 0
        assert what in lib.mt_last_error(), lib.mt_last_error()


# ---- the CPU backend ------------------------------------------------------------------------------
def test_cpu_backend_constructs_without_the_ops():
    import minitorch
    from cpu_backend import NumpyOps
    backend = minitorch.TensorBackend(NumpyOps)
    assert backend.flash_attention_extend_paged is None
    assert backend.flash_attention_extend_kvq is None
    with pytest.raises(ValueError, match="paged-cache kernels"):
        minitorch.PagedKVCache(1, 1, 2, 32, 16, backend)
    with pytest.raises(ValueError, match="quantised-cache kernels"):
        minitorch.KVCache(1, 1, 2, 32, 16, backend, kv_dtype="bf16")


def test_the_caches_have_no_scratch():
    from minitorch.kv_cache import KVCache, PagedKVCache
    for cls in (KVCache, PagedKVCache):
        assert not hasattr(cls, "scratch")
