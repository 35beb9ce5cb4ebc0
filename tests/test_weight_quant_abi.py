"""Argument validation of the weight-only quantised linear's entry points (CPU: every refusal
precedes the first device call, so dummy pointers are enough and nothing is launched)."""
import ctypes

import pytest

P = 4096  # dummy "device" addresses, 16-byte aligned and far apart
BF16, FP8, INT4 = 1, 2, 3


def _rows(lib, **kw):
    a = dict(fmt=INT4, G=1, x=P, ldx=256, M=8, K=256, norm=0, gamma=None, beta=None, eps=1e-5, W=[16 * P],
             scales=[24 * P], N=[256], bias=None, residual=None, out=[32 * P], gelu=0, glu=0)
    a.update(kw)
    G = len(a["N"] or [0])
    vec = lambda v: None if v is None else (ctypes.c_void_p * G)(*v)  # noqa: E731
    return lib.mt_linear_rows_wq(a["fmt"], a["G"], a["x"], a["ldx"], a["M"], a["K"], a["norm"], a["gamma"], a["beta"],
                                 a["eps"], vec(a["W"]), vec(a["scales"]),
                                 None if a["N"] is None else (ctypes.c_int64 * G)(*a["N"]), vec(a["bias"]),
                                 vec(a["residual"]), vec(a["out"]), a["gelu"], a["glu"], None)


def _quant(lib, **kw):
    a = dict(fmt=FP8, W=P, ldw=256, K=256, N=256, glu=0, codes=16 * P, scales=24 * P)
    a.update(kw)
    return lib.mt_weight_quant(a["fmt"], a["W"], a["ldw"], a["K"], a["N"], a["glu"], a["codes"], a["scales"], None)


def _dequant(lib, **kw):
    a = dict(fmt=FP8, codes=16 * P, scales=24 * P, K=256, N=256, glu=0, out=P, codes_out=None)
    a.update(kw)
    return lib.mt_weight_dequant(a["fmt"], a["codes"], a["scales"], a["K"], a["N"], a["glu"], a["out"], a["codes_out"],
                                 None)


def _bytes(lib, **kw):
    a = dict(fmt=FP8, K=256, N=256, glu=0)
    a.update(kw)
    cb, sb = ctypes.c_int64(), ctypes.c_int64()
    return lib.mt_weight_quant_bytes(a["fmt"], a["K"], a["N"], a["glu"], ctypes.byref(cb), ctypes.byref(sb))


@pytest.mark.parametrize("call,kw,msg", [
    (_rows, dict(fmt=0), b"fmt=0"),
    (_rows, dict(fmt=4), b"fmt=4"),
    (_rows, dict(K=64, ldx=64), b"K=64"),
    (_rows, dict(K=192, ldx=192), b"K=192"),
    (_rows, dict(K=1152, ldx=1152), b"K=1152"),
    (_rows, dict(W=[None]), b"codes[0] is NULL"),
    (_rows, dict(W=[16 * P + 8]), b"codes[0] is misaligned"),
    (_rows, dict(scales=None), b"scales array is NULL"),
    (_rows, dict(scales=[None]), b"scales[0] is NULL"),
    (_rows, dict(scales=[24 * P + 2]), b"scales[0] is misaligned"),
    (_rows, dict(fmt=FP8, scales=[None]), b"scales[0] is NULL"),
    # what mt_linear_rows_ex refuses
    (_rows, dict(G=0), b"G=0"),
    (_rows, dict(G=4), b"G=4"),
    (_rows, dict(M=0), b"M=0"),
    (_rows, dict(M=65), b"M=65"),
    (_rows, dict(ldx=252), b"ldx"),
    (_rows, dict(x=None), b"x is NULL"),
    (_rows, dict(x=P + 4), b"x is misaligned"),
    (_rows, dict(W=None), b"array is NULL"),
    (_rows, dict(N=None), b"array is NULL"),
    (_rows, dict(out=[None]), b"out[0] is NULL"),
    (_rows, dict(N=[0]), b"N[0]=0"),
    (_rows, dict(norm=3), b"norm=3"),
    (_rows, dict(norm=1, gamma=2 * P), b"gamma and beta"),
    (_rows, dict(norm=2, gamma=2 * P, beta=3 * P), b"has no beta"),
    (_rows, dict(norm=2, gamma=2 * P, eps=-1.0), b"eps"),
    (_rows, dict(gelu=2), b"gelu_mask"),
    (_rows, dict(glu=2), b"glu_mask"),
    (_rows, dict(gelu=1, glu=1), b"share a group"),
    (_rows, dict(out=[P + 1024]), b"out[0] overlaps x"),
    (_rows, dict(residual=[32 * P + 64]), b"out[0] overlaps residual[0]"),
    (_quant, dict(fmt=5), b"fmt=5"),
    (_quant, dict(K=100), b"K=100"),
    (_quant, dict(K=2048), b"K=2048"),
    (_quant, dict(N=0), b"N=0"),
    (_quant, dict(W=None), b"W is NULL"),
    (_quant, dict(ldw=255), b"ldw=255"),
    (_quant, dict(glu=1, ldw=256), b"ldw=256"),
    (_quant, dict(codes=None), b"codes[0] is NULL"),
    (_quant, dict(codes=16 * P + 4), b"codes[0] is misaligned"),
    (_quant, dict(scales=None), b"scales[0] is NULL"),
    (_dequant, dict(fmt=-1), b"fmt=-1"),
    (_dequant, dict(K=130), b"K=130"),
    (_dequant, dict(codes=None), b"codes[0] is NULL"),
    (_dequant, dict(fmt=INT4, scales=None), b"scales[0] is NULL"),
    (_dequant, dict(out=None), b"W_out is NULL"),
    (_bytes, dict(fmt=0), b"fmt=0"),
    (_bytes, dict(K=96), b"K=96"),
])
def test_refusals(call, kw, msg):
    from minitorch import _hip
    lib = _hip.lib()
    assert call(lib, **kw) != 0
    err = lib.mt_last_error()
    assert err.startswith(b"mt_") and msg in err, err


def test_symbols_bytes_and_abi_version():
    import minitorch
    from minitorch import _hip
    assert _hip.lib().mt_abi_version() == 3
    for name in ("mt_weight_quant_bytes", "mt_weight_quant", "mt_weight_dequant", "mt_linear_rows_wq"):
        assert name in _hip.exported_symbols() and hasattr(_hip.lib(), name)
    assert minitorch.QuantizedWeight is _hip.QuantizedWeight
    # whole tiles of 64 columns (32 of a gated weight's N), K rows each; scales per column (and 32 rows)
    assert _hip.weight_quant_bytes(_hip.MT_W_BF16, 128, 63, False) == (64 * 128 * 2, 0)
    assert _hip.weight_quant_bytes(_hip.MT_W_FP8, 256, 200, False) == (256 * 256, 200 * 4)
    assert _hip.weight_quant_bytes(_hip.MT_W_INT4, 1024, 40, True) == (2 * 64 * 1024 // 2, 32 * 80 * 4)
    with pytest.raises(ValueError, match="K=96"):
        _hip.weight_quant_bytes(_hip.MT_W_INT4, 96, 64)
