"""The C ABI of the quantised KV cache (include/minitorch_hip.h: mt_flash_attn_decode_kvq and its
split / workspace queries, mt_kv_cache_append_quant, mt_kv_cache_dequant): symbols, argument
validation before any device call (this runs without a GPU; nothing is launched), and the plan,
which is the bf16 decode plan at the same sizes for both formats."""
import ctypes

import pytest

MT_BF16 = 1
KV_BF16, KV_FP8 = 1, 2
CAP = 1104
SYMS = ("mt_flash_attn_decode_kvq", "mt_flash_attn_decode_kvq_splits", "mt_flash_attn_decode_kvq_workspace_bytes",
        "mt_kv_cache_append_quant", "mt_kv_cache_dequant")


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


def _decode(lib, kv, sizes, q=None, k=None, v=None, ks=None, vs=None, o=None, strides=(None,) * 4, ws=None, wsb=0):
    return lib.mt_flash_attn_decode_kvq(kv, 1, q, k, v, ks, vs, o, None, None, *sizes, *strides, None, ws, wsb, None)


def _s3(*v):
    return (ctypes.c_int64 * 3)(*v)


def test_symbols_and_bindings(lib):
    from minitorch import _hip
    for name in SYMS:
        assert hasattr(lib, name), name
        assert name in _hip.exported_symbols(), name
    assert lib.mt_abi_version() == 3
    assert (_hip.MT_KV_BF16, _hip.MT_KV_FP8) == (KV_BF16, KV_FP8)
    for fn in ("kv_cache_append_quant", "flash_decode_kvq", "kv_cache_dequant", "decode_kvq_workspace_bytes"):
        assert callable(getattr(_hip, fn))


@pytest.mark.parametrize("kv,sizes,msg", [
    (0, (2, 2, 2, 1, CAP, 64), b"unsupported kv_dtype"),
    (3, (2, 2, 2, 1, CAP, 64), b"unsupported kv_dtype"),
    (-1, (2, 2, 2, 1, CAP, 64), b"unsupported kv_dtype"),
    (KV_BF16, (2, 2, 2, 1, CAP, 20), b"multiple of 8"),
    (KV_FP8, (2, 2, 2, 1, CAP, 12), b"multiple of 8"),
    (KV_BF16, (2, 2, 2, 1, CAP, 264), b"d <= 256"),
    (KV_FP8, (2, 2, 2, 1, CAP, 264), b"d <= 256"),
    (KV_FP8, (2, 2, 2, 0, CAP, 64), b"query rows"),
    (KV_BF16, (2, 2, 2, 9, CAP, 64), b"query rows"),
    (KV_FP8, (2, 6, 4, 1, CAP, 64), b"kv heads must divide"),
    (KV_BF16, (2, 2, 3, 1, CAP, 64), b"kv heads must divide"),
    (KV_BF16, (2, 2, 0, 1, CAP, 64), b"kv heads must divide"),
    (KV_FP8, (0, 2, 2, 1, CAP, 64), b"bad sizes"),
    (KV_FP8, (2, 2, 2, 1, 0, 64), b"bad sizes"),
])
def test_decode_rejects_sizes_before_any_device_call(lib, kv, sizes, msg):
    assert _decode(lib, kv, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    assert lib.mt_flash_attn_decode_kvq_splits(kv, *sizes, None, None) <= 0
    assert lib.mt_flash_attn_decode_kvq_workspace_bytes(kv, *sizes) < 0


def test_fp8_needs_both_scales(lib, bufs):
    _, p = bufs
    sizes = (2, 2, 2, 1, CAP, 64)
    for ks, vs in ((None, None), (p, None), (None, p)):
        assert _decode(lib, KV_FP8, sizes, ks=ks, vs=vs) != 0
        assert b"scale pointer is NULL" in lib.mt_last_error()
        assert lib.mt_kv_cache_append_quant(KV_FP8, None, None, None, None, ks, vs, 2, 2, 1, CAP, 64,
                                            None, None, None, None, None, None) != 0
        assert b"scale pointer is NULL" in lib.mt_last_error()
        assert lib.mt_kv_cache_dequant(KV_FP8, None, None, ks, vs, None, None, 2, 2, CAP, 64,
                                       None, None, None, None, None, None) != 0
        assert b"scale pointer is NULL" in lib.mt_last_error()
    # bf16 takes NULL scales: the next check (the workspace) answers
    assert _decode(lib, KV_BF16, sizes) != 0
    assert b"workspace too small" in lib.mt_last_error()


@pytest.mark.parametrize("kv", [KV_BF16, KV_FP8])
@pytest.mark.parametrize("d", [8, 64, 256])
def test_workspace_one_byte_short_is_refused(lib, bufs, kv, d):
    _, p = bufs
    sizes = (13, 2, 2, 5, CAP, d)
    need = lib.mt_flash_attn_decode_kvq_workspace_bytes(kv, *sizes)
    assert need > 0
    assert _decode(lib, kv, sizes, ks=p, vs=p, ws=p, wsb=need - 1) != 0
    assert b"workspace too small" in lib.mt_last_error()
    assert _decode(lib, kv, sizes, ks=p, vs=p, ws=None, wsb=need) != 0
    assert b"workspace too small" in lib.mt_last_error()
    # with a large enough size the next check (NULL tensors) answers, still without a device call
    assert _decode(lib, kv, sizes, ks=p, vs=p, ws=p, wsb=need) != 0
    assert b"q is NULL" in lib.mt_last_error()


@pytest.mark.parametrize("kv,row", [(KV_BF16, 16), (KV_FP8, 8)])
def test_misaligned_pointers_and_strides_are_refused(lib, bufs, kv, row):
    _, p = bufs
    sizes = (1, 2, 2, 1, 8, 64)  # one split: no workspace
    assert lib.mt_flash_attn_decode_kvq_workspace_bytes(kv, *sizes) == 0
    esz = 2 if kv == KV_BF16 else 1
    ok = dict(q=p, k=p, v=p, ks=p, vs=p, o=p)
    for what, arg in (("q", "q"), ("k_cache", "k"), ("v_cache", "v"), ("o", "o")):
        by = 16 if arg in ("q", "o") else row
        assert _decode(lib, kv, sizes, **{**ok, arg: p + by // 2}) != 0
        assert what.encode() in lib.mt_last_error() and b"aligned" in lib.mt_last_error(), lib.mt_last_error()
    # a cache row stride that is not a whole number of chunks (d + 4 elements)
    bad = _s3(2 * 8 * 68, 8 * 68, 64 + row // esz // 2)
    assert _decode(lib, kv, sizes, **ok, strides=(None, bad, None, None)) != 0
    assert b"k_cache stride" in lib.mt_last_error()
    assert _decode(lib, kv, sizes, **ok, strides=(None, None, bad, None)) != 0
    assert b"v_cache stride" in lib.mt_last_error()
    # fp8 rows start on 8 bytes, bf16 rows on 16: an 8-B offset passes one and not the other
    rc = lib.mt_kv_cache_dequant(kv, p + 8, p, p, p, None, None, 1, 2, 8, 64, None, None, None, None, None, None)
    assert rc != 0
    assert (b"k_cache is not 16-B aligned" if kv == KV_BF16 else b"k_out is NULL") in lib.mt_last_error()


@pytest.mark.parametrize("kv,sizes,msg", [
    (5, (2, 2, 1, CAP, 64), b"unsupported kv_dtype"),
    (KV_BF16, (2, 2, 1, CAP, 20), b"multiple of 8"),
    (KV_BF16, (2, 2, 1, CAP, 264), b"d <= 256"),
    (KV_BF16, (2, 2, 0, CAP, 64), b"bad sizes"),
    (KV_BF16, (2, 0, 1, CAP, 64), b"bad sizes"),
    (KV_BF16, (2, 2, 1, CAP, 64), b"pos is NULL"),
])
def test_append_rejects_before_any_device_call(lib, kv, sizes, msg):
    assert lib.mt_kv_cache_append_quant(kv, None, None, None, None, None, None, *sizes,
                                        None, None, None, None, None, None) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


@pytest.mark.parametrize("kv,sizes,msg", [
    (0, (2, 2, CAP, 64), b"unsupported kv_dtype"),
    (KV_FP8, (2, 2, CAP, 36), b"multiple of 8"),
    (KV_BF16, (2, 2, CAP, 512), b"d <= 256"),
    (KV_BF16, (2, 2, 0, 64), b"bad sizes"),
    (KV_BF16, (2, 2, CAP, 64), b"k_cache is NULL"),
])
def test_dequant_rejects_before_any_device_call(lib, kv, sizes, msg):
    assert lib.mt_kv_cache_dequant(kv, None, None, None, None, None, None, *sizes,
                                   None, None, None, None, None, None) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


@pytest.mark.parametrize("kv", [KV_BF16, KV_FP8])
@pytest.mark.parametrize("nq", [1, 3, 8])
@pytest.mark.parametrize("d", [8, 40, 64, 128, 256])
@pytest.mark.parametrize("B,H,Hkv,Nk", [(13, 2, 2, CAP), (2, 8, 2, CAP), (8, 16, 16, 4096), (1, 16, 4, 16384),
                                        (64, 8, 8, 40)])
def test_plan_is_the_bf16_decode_plan(lib, kv, nq, d, B, H, Hkv, Nk):
    """Both formats are read in chunks of 8 elements, a bf16 row's chunks: the splits, span, tile
    and workspace are mt_flash_attn_decode_gqa's for MT_BF16 at the same sizes, a function of the
    sizes only."""
    span, tile, span0, tile0 = (ctypes.c_int64(0) for _ in range(4))
    n = lib.mt_flash_attn_decode_kvq_splits(kv, B, H, Hkv, nq, Nk, d, ctypes.byref(span), ctypes.byref(tile))
    n0 = lib.mt_flash_attn_decode_gqa_splits(MT_BF16, B, H, Hkv, nq, Nk, d, ctypes.byref(span0), ctypes.byref(tile0))
    assert n >= 1 and (n, span.value, tile.value) == (n0, span0.value, tile0.value)
    assert span.value * n >= Nk > span.value * (n - 1) and span.value % tile.value == 0
    want = 0 if n == 1 else B * H * nq * n * (d + 2) * 4
    assert lib.mt_flash_attn_decode_kvq_workspace_bytes(kv, B, H, Hkv, nq, Nk, d) == want
    assert lib.mt_flash_attn_decode_kvq_splits(kv, B, H, Hkv, nq, Nk, d, None, None) == n


def test_cpu_backend_constructs_without_the_quantised_ops():
    import minitorch
    from cpu_backend import NumpyOps
    backend = minitorch.TensorBackend(NumpyOps)
    assert backend.kv_cache_append_quant is None
    assert backend.flash_attention_decode_kvq is None
    assert backend.kv_cache_dequant is None
