"""The C ABI of grouped-query training attention (include/minitorch_hip.h: mt_flash_attn_fwd_gqa,
mt_flash_attn_bwd_gqa and its workspace query): symbols, binding, and the refusals before any
device call (NULL or never-dereferenced tensors, so this runs without a GPU), in the manner of
tests/test_gqa_abi.py."""
import ctypes

import pytest

MT_F32, MT_BF16 = 0, 1
NAMES = ("mt_flash_attn_fwd_gqa", "mt_flash_attn_bwd_gqa_workspace_bytes", "mt_flash_attn_bwd_gqa")
PTR = 4096  # a 16-B aligned address that a refused call never reads


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


def _fwd(lib, dtype, sizes, ptrs=(PTR,) * 4, strides=(None,) * 4):
    return lib.mt_flash_attn_fwd_gqa(dtype, 1, *ptrs, None, None, *sizes, *strides, None, None)


def _bwd(lib, dtype, sizes, ptrs=(PTR,) * 10, strides=None, ws=PTR, ws_bytes=1 << 40):
    return lib.mt_flash_attn_bwd_gqa(dtype, 1, *ptrs, *sizes, strides, None, ws, ws_bytes, None)


def test_symbols_exported_and_bound(lib):
    from minitorch import _hip
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _hip._PROTOS, name
        assert name in _hip.exported_symbols(), name
    assert lib.mt_abi_version() == 3


@pytest.mark.parametrize("dtype,sizes,msg", [  # sizes: (B, H, Hkv, N, d)
    (MT_F32, (2, 4, 0, 64, 64), b"kv heads"),      # Hkv = 0
    (MT_F32, (2, 4, -2, 64, 64), b"kv heads"),
    (MT_F32, (2, 4, 8, 64, 64), b"kv heads"),      # Hkv > H
    (MT_F32, (2, 6, 4, 64, 64), b"kv heads"),      # H % Hkv != 0
    (MT_BF16, (2, 4, 2, 64, 64), b"unsupported dtype"),
    (5, (2, 4, 2, 64, 64), b"unsupported dtype"),
    (MT_F32, (2, 4, 2, 64, 132), b"d <= 128"),
    (MT_F32, (2, 4, 2, 64, 30), b"16-B rows"),
    (MT_F32, (0, 4, 2, 64, 64), b"bad sizes"),
])
def test_bad_sizes_are_refused_before_any_device_call(lib, dtype, sizes, msg):
    assert _fwd(lib, dtype, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    assert _bwd(lib, dtype, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    if dtype == MT_F32:
        assert lib.mt_flash_attn_bwd_gqa_workspace_bytes(*sizes) < 0


def test_misaligned_tensors_are_refused(lib):
    sizes = (2, 4, 2, 64, 64)
    for i in range(4):  # a NULL tensor, then a base off 16 bytes
        assert _fwd(lib, MT_F32, sizes, ptrs=tuple(None if j == i else PTR for j in range(4))) != 0
        assert b"is NULL" in lib.mt_last_error()
        assert _fwd(lib, MT_F32, sizes, ptrs=tuple(PTR + 8 if j == i else PTR for j in range(4))) != 0
        assert b"not 16-B aligned" in lib.mt_last_error()
    odd = (ctypes.c_int64 * 3)(4 * 64 * 66, 64 * 66, 66)  # rows 66 floats apart: off 16 bytes
    assert _fwd(lib, MT_F32, sizes, strides=(None, odd, None, None)) != 0
    assert b"k stride" in lib.mt_last_error()
    for i in (0, 1, 2, 3, 4, 7, 8, 9):  # every tensor but m, l
        assert _bwd(lib, MT_F32, sizes, ptrs=tuple(PTR + 4 if j == i else PTR for j in range(10))) != 0
        assert b"not 16-B aligned" in lib.mt_last_error()
    dense_q, dense_k = (4 * 64 * 64, 64 * 64, 64), (2 * 64 * 64, 64 * 64, 64)
    t = [dense_q, dense_k, dense_k, dense_q, dense_q, dense_q, dense_k, (2 * 64 * 64, 64 * 64, 66)]
    assert _bwd(lib, MT_F32, sizes, strides=(ctypes.c_int64 * 24)(*[x for s in t for x in s])) != 0
    assert b"dv stride" in lib.mt_last_error()


def test_workspace_one_byte_short_is_refused(lib):
    sizes = (3, 6, 2, 130, 64)
    need = lib.mt_flash_attn_bwd_gqa_workspace_bytes(*sizes)
    assert need >= 2 * 3 * 6 * 130 * 4  # delta and the log2-LSE per query row
    assert need == lib.mt_flash_attn_bwd_gqa_workspace_bytes(*sizes)
    assert _bwd(lib, MT_F32, sizes, ws_bytes=need - 1) != 0
    assert b"workspace too small" in lib.mt_last_error()
    assert _bwd(lib, MT_F32, sizes, ws=None, ws_bytes=need) != 0
    assert b"workspace is NULL" in lib.mt_last_error()
    # Hkv == H asks what the plain backward asks
    assert lib.mt_flash_attn_bwd_gqa_workspace_bytes(3, 6, 6, 130, 64) == lib.mt_flash_attn_bwd_workspace_bytes(3, 6, 130, 64)
