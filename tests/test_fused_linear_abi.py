"""mt_linear_rows' argument validation (CPU: every refusal precedes the first device call, so
dummy pointers are enough and nothing is launched) and the model flag's construction rule."""
import ctypes

import pytest

P = 4096  # dummy "device" addresses, 16-byte aligned and far apart


def _call(lib, **kw):
    a = dict(G=1, x=P, ldx=256, M=8, K=256, gamma=None, beta=None, W=[16 * P], N=[256], bias=None, residual=None,
             out=[32 * P], gelu=0)
    a.update(kw)
    G = len(a["N"] or [0])
    vec = lambda v: None if v is None else (ctypes.c_void_p * G)(*v)  # noqa: E731
    return lib.mt_linear_rows(a["G"], a["x"], a["ldx"], a["M"], a["K"], a["gamma"], a["beta"], vec(a["W"]),
                              None if a["N"] is None else (ctypes.c_int64 * G)(*a["N"]), vec(a["bias"]),
                              vec(a["residual"]), vec(a["out"]), a["gelu"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(G=0), b"G=0"),
    (dict(G=4), b"G=4"),
    (dict(M=0), b"M=0"),
    (dict(M=65), b"M=65"),
    (dict(K=0), b"K=0"),
    (dict(K=258), b"K=258"),
    (dict(K=1028, ldx=1028), b"K=1028"),
    (dict(ldx=252), b"ldx"),
    (dict(ldx=258), b"ldx"),
    (dict(x=None), b"x is NULL"),
    (dict(W=None), b"array is NULL"),
    (dict(N=None), b"array is NULL"),
    (dict(out=None), b"array is NULL"),
    (dict(W=[None]), b"W[0] is NULL"),
    (dict(out=[None]), b"out[0] is NULL"),
    (dict(N=[0]), b"N[0]=0"),
    (dict(gamma=2 * P), b"gamma and beta"),
    (dict(beta=2 * P), b"gamma and beta"),
    (dict(x=P + 4), b"x is misaligned"),
    (dict(gamma=2 * P + 8, beta=3 * P), b"gamma / beta are misaligned"),
    (dict(W=[16 * P + 2]), b"group 0 is misaligned"),
    (dict(gelu=2), b"gelu_mask"),
    (dict(out=[P + 1024]), b"out[0] overlaps x"),             # inside x's 8 x 256 floats
    (dict(residual=[32 * P + 64]), b"out[0] overlaps residual[0]"),
    (dict(G=2, W=[16 * P, 17 * P], N=[256, 64], out=[32 * P, 32 * P + 4096]), b"out[1] overlaps out[0]"),
])
def test_refusals(kw, msg):
    from minitorch import _hip
    lib = _hip.lib()
    assert _call(lib, **kw) != 0
    err = lib.mt_last_error()
    assert err.startswith(b"mt_linear_rows") and msg in err, err


def test_abi_version_and_binding():
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    assert _hip.lib().mt_abi_version() == 3
    assert "mt_linear_rows" in _hip.exported_symbols()
    assert callable(_hip.fused_linear) and isinstance(_hip.fused_linear_calls, int)
    assert minitorch.TensorBackend(NumpyOps).fused_linear is None
    assert minitorch.TensorBackend(minitorch.HipKernelOps).fused_linear is not None
    cpu = minitorch.TensorBackend(NumpyOps)
    kw = dict(n_vocab=11, n_embd=8, n_head=2, n_positions=8, backend=cpu, n_layer=1)
    with pytest.raises(ValueError, match="use_fused_kernel"):
        minitorch.DecoderLM(fused_step=True, **kw)
    with pytest.raises(NotImplementedError, match="fused skinny linear"):
        minitorch.tensor_from_numpy(__import__("numpy").zeros((2, 8), "float32"), cpu).fused_linear(None)
