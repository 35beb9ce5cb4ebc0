"""The C ABI of the KV-cache decode path (include/minitorch_hip.h): symbols, argument validation
before any device call (so this runs without a GPU, nothing is launched), the split policy and
the workspace size."""
import ctypes

import pytest

MT_F32, MT_BF16, MT_BF16_F32OUT = 0, 1, 2
CAP = 1104
CASES = [(MT_F32, 16), (MT_F32, 32), (MT_F32, 64), (MT_F32, 128), (MT_BF16, 64), (MT_BF16, 128),
         (MT_BF16_F32OUT, 64)]


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


def _decode(lib, dtype, sizes, ws=None, ws_bytes=0):
    """mt_flash_attn_decode with NULL tensors: only legal for calls the library must refuse first."""
    return lib.mt_flash_attn_decode(dtype, 1, None, None, None, None, None, None, *sizes,
                                    None, None, None, None, None, ws, ws_bytes, None)


def test_symbols_exist(lib):
    for name in ("mt_flash_attn_decode_splits", "mt_flash_attn_decode_workspace_bytes",
                 "mt_flash_attn_decode", "mt_kv_cache_append"):
        assert hasattr(lib, name), name
    assert lib.mt_abi_version() == 3


@pytest.mark.parametrize("dtype,sizes,msg", [
    (MT_F32, (2, 2, 0, CAP, 64), b"query rows"),       # Nq = 0
    (MT_BF16, (2, 2, 9, CAP, 64), b"query rows"),      # Nq = 9
    (MT_BF16, (2, 2, 1, CAP, 20), b"16-B rows"),       # bf16 d = 20: 40-B rows
    (MT_BF16_F32OUT, (2, 2, 1, CAP, 20), b"16-B rows"),
    (MT_F32, (2, 2, 1, CAP, 6), b"16-B rows"),         # fp32 d = 6: 24-B rows
    (MT_F32, (2, 2, 1, CAP, 264), b"d <= 256"),
    (MT_BF16, (2, 2, 1, CAP, 264), b"d <= 256"),
    (3, (2, 2, 1, CAP, 64), b"unsupported dtype"),
    (-1, (2, 2, 1, CAP, 64), b"unsupported dtype"),
    (MT_F32, (0, 2, 1, CAP, 64), b"bad sizes"),
    (MT_F32, (2, 2, 1, 0, 64), b"bad sizes"),
])
def test_decode_rejects_before_any_device_call(lib, dtype, sizes, msg):
    assert _decode(lib, dtype, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    assert lib.mt_flash_attn_decode_splits(dtype, *sizes, None, None) <= 0
    assert lib.mt_flash_attn_decode_workspace_bytes(dtype, *sizes) < 0


@pytest.mark.parametrize("dtype,d", CASES)
def test_workspace_one_byte_short_is_refused(lib, dtype, d):
    sizes = (13, 2, 5, CAP, d)
    need = lib.mt_flash_attn_decode_workspace_bytes(dtype, *sizes)
    assert need > 0
    buf = ctypes.create_string_buffer(64)  # a non-NULL pointer; the size check comes before any use
    assert _decode(lib, dtype, sizes, ctypes.addressof(buf), need - 1) != 0
    assert b"workspace too small" in lib.mt_last_error()
    assert _decode(lib, dtype, sizes, None, need) != 0
    assert b"workspace too small" in lib.mt_last_error()
    # with a large enough size the next check (NULL tensors) answers, still without a device call
    assert _decode(lib, dtype, sizes, ctypes.addressof(buf), need) != 0
    assert b"is NULL" in lib.mt_last_error()


@pytest.mark.parametrize("nq", [1, 5, 8])
@pytest.mark.parametrize("dtype,d", CASES)
def test_split_policy_and_workspace_size(lib, dtype, d, nq):
    span, tile = ctypes.c_int64(0), ctypes.c_int64(0)
    B, H = 13, 2
    n = lib.mt_flash_attn_decode_splits(dtype, B, H, nq, CAP, d, ctypes.byref(span), ctypes.byref(tile))
    assert n >= 3, "a small B*H must still be split over the keys"
    assert span.value * n >= CAP > span.value * (n - 1)
    assert tile.value >= 1 and span.value % tile.value == 0
    # documented layout: per (b, h, query, split) d fp32 of O and the (m, l) pair
    assert lib.mt_flash_attn_decode_workspace_bytes(dtype, B, H, nq, CAP, d) == B * H * nq * n * (d + 2) * 4
    # the policy never depends on anything but the sizes: same answer on a second call
    assert lib.mt_flash_attn_decode_splits(dtype, B, H, nq, CAP, d, None, None) == n


def test_many_heads_take_one_split_and_no_workspace(lib):
    span = ctypes.c_int64(0)
    assert lib.mt_flash_attn_decode_splits(MT_F32, 64, 8, 1, 40, 32, ctypes.byref(span), None) == 1
    assert span.value >= 40
    assert lib.mt_flash_attn_decode_workspace_bytes(MT_F32, 64, 8, 1, 40, 32) == 0


def test_long_cache_small_batch_fills_the_chip(lib):
    """(1,16,16384,128) bf16: at least two workgroups per CU (256 CUs) from 16 heads."""
    n = lib.mt_flash_attn_decode_splits(MT_BF16, 1, 16, 1, 16384, 128, None, None)
    assert 16 * n >= 512


@pytest.mark.parametrize("dtype,sizes,msg", [
    (MT_F32, (2, 2, 1, CAP, 6), b"16-B rows"),
    (MT_BF16, (2, 2, 1, CAP, 20), b"16-B rows"),
    (7, (2, 2, 1, CAP, 64), b"unsupported dtype"),
    (MT_F32, (2, 2, 0, CAP, 64), b"bad sizes"),
    (MT_F32, (2, 2, 1, CAP, 64), b"pos is NULL"),
])
def test_append_rejects_before_any_device_call(lib, dtype, sizes, msg):
    assert lib.mt_kv_cache_append(dtype, None, None, None, None, *sizes, None, None, None, None,
                                  None, None) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


def test_cpu_backend_still_constructs_without_decode():
    import minitorch
    from cpu_backend import NumpyOps
    backend = minitorch.TensorBackend(NumpyOps)
    assert backend.flash_attention_decode is None
    assert backend.kv_cache_append is None
