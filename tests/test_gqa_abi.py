"""The C ABI of grouped-query decode attention (include/minitorch_hip.h: mt_flash_attn_decode_gqa
and its split / workspace queries): symbols, binding, refusals before any device call (NULL
tensors, so this runs without a GPU), and the plan: Hkv = H answers what the plain entry points
answer, the workspace stays per (b, query head, query, split)."""
import ctypes

import pytest

MT_F32, MT_BF16, MT_BF16_F32OUT = 0, 1, 2
CAP = 1104
CASES = [(MT_F32, 16), (MT_F32, 32), (MT_F32, 64), (MT_F32, 128), (MT_BF16, 64), (MT_BF16, 128),
         (MT_BF16_F32OUT, 64)]
NAMES = ("mt_flash_attn_decode_gqa_splits", "mt_flash_attn_decode_gqa_workspace_bytes", "mt_flash_attn_decode_gqa")


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


def _decode(lib, dtype, sizes, ws=None, ws_bytes=0):
    """mt_flash_attn_decode_gqa with NULL tensors: only legal for calls the library must refuse first."""
    return lib.mt_flash_attn_decode_gqa(dtype, 1, None, None, None, None, None, None, *sizes,
                                        None, None, None, None, None, ws, ws_bytes, None)


def test_symbols_exported_and_bound(lib):
    from minitorch import _hip
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _hip._PROTOS, name
        assert name in _hip.exported_symbols(), name
    assert lib.mt_abi_version() == 3


@pytest.mark.parametrize("dtype,sizes,msg", [
    (MT_F32, (2, 4, 0, 1, CAP, 64), b"kv heads"),      # Hkv = 0
    (MT_F32, (2, 4, -2, 1, CAP, 64), b"kv heads"),
    (MT_BF16, (2, 4, 8, 1, CAP, 64), b"kv heads"),     # Hkv > H
    (MT_F32, (2, 6, 4, 1, CAP, 64), b"kv heads"),      # H % Hkv != 0
    (MT_BF16, (2, 4, 2, 9, CAP, 64), b"query rows"),   # Nq = 9
    (MT_F32, (2, 4, 2, 0, CAP, 64), b"query rows"),
    (MT_BF16, (2, 4, 2, 1, CAP, 20), b"16-B rows"),
    (MT_F32, (2, 4, 2, 1, CAP, 264), b"d <= 256"),
    (5, (2, 4, 2, 1, CAP, 64), b"unsupported dtype"),
    (MT_F32, (0, 4, 2, 1, CAP, 64), b"bad sizes"),
])
def test_gqa_rejects_before_any_device_call(lib, dtype, sizes, msg):
    assert _decode(lib, dtype, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    assert lib.mt_flash_attn_decode_gqa_splits(dtype, *sizes, None, None) <= 0
    assert lib.mt_flash_attn_decode_gqa_workspace_bytes(dtype, *sizes) < 0


def test_binding_rejects_with_the_library_message():
    from minitorch import _hip
    with pytest.raises(ValueError, match="kv heads"):
        _hip.decode_splits(MT_F32, 2, 6, 1, CAP, 64, Hkv=4)
    with pytest.raises(ValueError, match="kv heads"):
        _hip.decode_workspace_bytes(MT_F32, 2, 6, 1, CAP, 64, Hkv=4)


def _plan(lib, fn, dtype, *sizes):
    span, tile = ctypes.c_int64(0), ctypes.c_int64(0)
    n = fn(dtype, *sizes, ctypes.byref(span), ctypes.byref(tile))
    return n, span.value, tile.value


@pytest.mark.parametrize("nq", [1, 5, 8])
@pytest.mark.parametrize("dtype,d", CASES)
def test_hkv_equal_h_is_the_plain_plan(lib, dtype, d, nq):
    from minitorch import _hip
    for B, H, Nk in ((13, 2, CAP), (64, 8, 40), (1, 16, 16384)):
        plain = _plan(lib, lib.mt_flash_attn_decode_splits, dtype, B, H, nq, Nk, d)
        gqa = _plan(lib, lib.mt_flash_attn_decode_gqa_splits, dtype, B, H, H, nq, Nk, d)
        assert gqa == plain
        want = lib.mt_flash_attn_decode_workspace_bytes(dtype, B, H, nq, Nk, d)
        assert lib.mt_flash_attn_decode_gqa_workspace_bytes(dtype, B, H, H, nq, Nk, d) == want
        # the binding: Hkv=None is Hkv=H
        assert _hip.decode_splits(dtype, B, H, nq, Nk, d) == plain == _hip.decode_splits(dtype, B, H, nq, Nk, d, Hkv=H)
        assert _hip.decode_workspace_bytes(dtype, B, H, nq, Nk, d) == want


@pytest.mark.parametrize("H,Hkv,nq", [(4, 1, 1), (4, 2, 4), (8, 1, 1), (6, 2, 3), (16, 1, 1), (4, 2, 5), (16, 2, 8)])
@pytest.mark.parametrize("dtype,d", CASES)
def test_gqa_plan_and_workspace_size(lib, dtype, d, H, Hkv, nq):
    B = 18
    n, span, tile = _plan(lib, lib.mt_flash_attn_decode_gqa_splits, dtype, B, H, Hkv, nq, CAP, d)
    assert n >= 3, "a small grid must still be split over the keys"
    assert span * n >= CAP > span * (n - 1)
    assert tile >= 1 and span % tile == 0
    # per (b, query head, query, split): d fp32 of O and the (m, l) pair, whatever the grouping
    assert lib.mt_flash_attn_decode_gqa_workspace_bytes(dtype, B, H, Hkv, nq, CAP, d) == B * H * nq * n * (d + 2) * 4
    # a function of the sizes only: the same answer on a second call
    assert _plan(lib, lib.mt_flash_attn_decode_gqa_splits, dtype, B, H, Hkv, nq, CAP, d) == (n, span, tile)
    # the span is sized by the query heads: the plain plan of (B, H), whatever Hkv
    assert (n, span, tile) == _plan(lib, lib.mt_flash_attn_decode_splits, dtype, B, H, nq, CAP, d)


def test_few_kv_heads_do_not_multiply_the_splits(lib):
    """(1,16,16384,128) bf16: two kv heads give 2 workgroups per split; the split count stays the
    plain plan's (every split is one more row per query for the combine's serial merge)."""
    plain = _plan(lib, lib.mt_flash_attn_decode_splits, MT_BF16, 1, 16, 1, 16384, 128)
    for Hkv in (16, 4, 2, 1):
        assert _plan(lib, lib.mt_flash_attn_decode_gqa_splits, MT_BF16, 1, 16, Hkv, 1, 16384, 128) == plain


def test_gqa_workspace_one_byte_short_is_refused(lib):
    sizes = (13, 4, 2, 2, CAP, 64)
    need = lib.mt_flash_attn_decode_gqa_workspace_bytes(MT_F32, *sizes)
    assert need > 0
    buf = ctypes.create_string_buffer(64)
    assert _decode(lib, MT_F32, sizes, ctypes.addressof(buf), need - 1) != 0
    assert b"workspace too small" in lib.mt_last_error()
    assert _decode(lib, MT_F32, sizes, ctypes.addressof(buf), need) != 0
    assert b"is NULL" in lib.mt_last_error()
