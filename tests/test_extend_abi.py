"""The C ABI of the extend step (include/minitorch_hip.h: mt_flash_attn_extend and its plan
query): symbols, argument validation before any device call (so this runs without a GPU, nothing
is launched) and the plan."""
import ctypes

import pytest

MT_F32, MT_BF16, MT_BF16_F32OUT = 0, 1, 2
CAP = 448
CASES = [(MT_F32, 16), (MT_F32, 32), (MT_F32, 64), (MT_F32, 68), (MT_F32, 128), (MT_F32, 256), (MT_BF16, 64),
         (MT_BF16, 128), (MT_BF16, 256), (MT_BF16_F32OUT, 64)]


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


def _extend(lib, dtype, sizes, ptrs=(None, None, None, None), strides=(None, None, None, None)):
    """mt_flash_attn_extend with NULL or dummy tensors: only legal for calls the library must
    refuse first. sizes = (B, H, Hkv, Nq, Nk, d)."""
    q, k, v, o = ptrs
    return lib.mt_flash_attn_extend(dtype, 1, q, k, v, o, None, None, *sizes, *strides, None, None, None)


def test_symbols_exist(lib):
    for name in ("mt_flash_attn_extend", "mt_flash_attn_extend_plan"):
        assert hasattr(lib, name), name
    assert lib.mt_abi_version() == 3


def test_python_binding_lists_the_symbols():
    from minitorch import _hip
    assert {"mt_flash_attn_extend", "mt_flash_attn_extend_plan"} <= set(_hip.exported_symbols())


@pytest.mark.parametrize("dtype,sizes,msg", [
    (MT_F32, (2, 2, 2, 0, CAP, 64), b"at least one query row"),     # Nq = 0
    (MT_F32, (2, 2, 2, -3, CAP, 64), b"at least one query row"),
    (MT_BF16, (2, 2, 2, CAP + 1, CAP, 64), b"at most Nk query rows"),  # Nq > Nk
    (MT_F32, (2, 2, 2, 9, 8, 64), b"at most Nk query rows"),
    (MT_BF16, (2, 2, 2, 9, CAP, 20), b"16-B rows"),                 # bf16 d = 20: 40-B rows
    (MT_BF16_F32OUT, (2, 2, 2, 9, CAP, 20), b"16-B rows"),
    (MT_F32, (2, 2, 2, 9, CAP, 6), b"16-B rows"),                   # fp32 d = 6: 24-B rows
    (MT_F32, (2, 2, 2, 9, CAP, 264), b"d <= 256"),
    (MT_BF16, (2, 2, 2, 9, CAP, 264), b"d <= 256"),
    (3, (2, 2, 2, 9, CAP, 64), b"unsupported dtype"),
    (-1, (2, 2, 2, 9, CAP, 64), b"unsupported dtype"),
    (MT_F32, (0, 2, 2, 9, CAP, 64), b"bad sizes"),
    (MT_F32, (2, 0, 1, 9, CAP, 64), b"bad sizes"),
    (MT_F32, (2, 2, 2, 9, 0, 64), b"bad sizes"),
    (MT_F32, (2, 2, 2, 9, CAP, 0), b"bad sizes"),
    (MT_F32, (2, 4, 0, 9, CAP, 64), b"kv heads must divide"),       # a bad Hkv
    (MT_F32, (2, 4, -1, 9, CAP, 64), b"kv heads must divide"),
    (MT_F32, (2, 4, 3, 9, CAP, 64), b"kv heads must divide"),
    (MT_BF16, (2, 4, 8, 9, CAP, 64), b"kv heads must divide"),
    (MT_F32, (2, 2, 2, 9, (1 << 30) + 1, 64), b"sizes out of range"),
    (MT_F32, (1 << 20, 1 << 10, 1, 9, CAP, 64), b"sizes out of range"),
])
def test_extend_rejects_before_any_device_call(lib, dtype, sizes, msg):
    assert _extend(lib, dtype, sizes) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()
    assert lib.mt_flash_attn_extend_plan(dtype, *sizes, None, None) < 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


def test_null_and_misaligned_tensors_are_refused(lib):
    sizes = (2, 4, 2, 9, CAP, 64)
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15  # 16-B aligned, never dereferenced: refused first
    for i, name in enumerate((b"q", b"k_cache", b"v_cache", b"o")):
        ptrs = [base] * 4
        ptrs[i] = None
        assert _extend(lib, MT_F32, sizes, ptrs) != 0
        assert name + b" is NULL" in lib.mt_last_error(), lib.mt_last_error()
        ptrs[i] = base + 4
        assert _extend(lib, MT_F32, sizes, ptrs) != 0
        assert name + b" is not 16-B aligned" in lib.mt_last_error(), lib.mt_last_error()
        strides = [None] * 4
        strides[i] = (ctypes.c_int64 * 3)(9 * 4 * 64 + 2, 64, 4 * 64)  # a batch stride of 8 B mod 16
        assert _extend(lib, MT_F32, sizes, [base] * 4, strides) != 0
        assert name + b" stride 0" in lib.mt_last_error(), lib.mt_last_error()
    # a bf16 output has 8 elements per 16 B: a stride of 4 mod 8 is refused
    strides = [None, None, None, (ctypes.c_int64 * 3)(9 * 4 * 64 + 4, 64, 4 * 64)]
    assert _extend(lib, MT_BF16, sizes, [base] * 4, strides) != 0
    assert b"o stride 0" in lib.mt_last_error()


@pytest.mark.parametrize("dtype,d", CASES)
def test_plan_depends_on_its_arguments_only(lib, dtype, d):
    bq, bk = ctypes.c_int64(0), ctypes.c_int64(0)
    sizes = (13, 4, 2, 168, CAP, d)
    kid = lib.mt_flash_attn_extend_plan(dtype, *sizes, ctypes.byref(bq), ctypes.byref(bk))
    assert kid >= 0
    assert bq.value >= 32 and bq.value % 32 == 0
    assert bk.value >= 16
    # a failing call in between leaves no trace; NULL outputs are allowed
    assert lib.mt_flash_attn_extend_plan(dtype, 0, 4, 2, 168, CAP, d, None, None) < 0
    bq2, bk2 = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.mt_flash_attn_extend_plan(dtype, *sizes, ctypes.byref(bq2), ctypes.byref(bk2)) == kid
    assert (bq2.value, bk2.value) == (bq.value, bk.value)
    assert lib.mt_flash_attn_extend_plan(dtype, *sizes, None, None) == kid
    # bf16 with an fp32 output runs the bf16 kernel
    if dtype == MT_BF16:
        assert lib.mt_flash_attn_extend_plan(MT_BF16_F32OUT, *sizes, None, None) == kid


def test_fp32_small_head_dims_take_the_three_piece_kernels(lib):
    """fp32 d <= 64 must not run on the fp32 MFMA (1/16 of the bf16 rate): ids 0 and 1 are the
    instantiations with three bf16 pieces per operand (csrc/fa_extend.hip extend_plan)."""
    ids = {d: lib.mt_flash_attn_extend_plan(MT_F32, 8, 16, 16, 512, 4096, d, None, None) for d in (16, 32, 48, 64, 68)}
    assert ids[16] == ids[32] == 0 and ids[48] == ids[64] == 1 and ids[68] == 2


def test_extend_plan_through_the_binding():
    from minitorch import _hip
    kid, bq, bk = _hip.extend_plan(MT_F32, 2, 4, 168, CAP, 64, Hkv=2)
    assert kid >= 0 and bq >= 32 and bk >= 16
    with pytest.raises(ValueError, match="at most Nk"):
        _hip.extend_plan(MT_F32, 2, 4, CAP + 1, CAP, 64)


def test_cpu_backend_still_constructs_without_extend():
    import minitorch
    from cpu_backend import NumpyOps
    backend = minitorch.TensorBackend(NumpyOps)
    assert backend.flash_attention_extend is None
