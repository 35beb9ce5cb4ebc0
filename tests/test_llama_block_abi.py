"""The Llama-shaped block's C entry points: exported and bound, and their argument validation (CPU:
every refusal precedes the first device call, so dummy pointers are enough and nothing is
launched), as tests/test_fused_linear_abi.py does for mt_linear_rows."""
import ctypes

import pytest

P = 4096  # dummy "device" addresses, 16-byte aligned and far apart
NEW = ("mt_linear_rows_ex", "mt_rmsnorm_fw", "mt_rmsnorm_bw_workspace_bytes", "mt_rmsnorm_bw", "mt_swiglu_fw",
       "mt_swiglu_bw")


def _linear(lib, **kw):
    a = dict(G=1, norm=2, gamma=2 * P, beta=None, eps=1e-5, W=[16 * P], N=[256], gelu=0, glu=1)
    a.update(kw)
    G = len(a["N"])
    vec = lambda v: (ctypes.c_void_p * G)(*v)  # noqa: E731
    return lib.mt_linear_rows_ex(a["G"], P, 256, 8, 256, a["norm"], a["gamma"], a["beta"], a["eps"], vec(a["W"]),
                                 (ctypes.c_int64 * G)(*a["N"]), None, None, vec([32 * P + 64 * P * g for g in range(G)]),
                                 a["gelu"], a["glu"], None)


@pytest.mark.parametrize("call,name,msg", [
    (lambda L: _linear(L, norm=3), b"mt_linear_rows_ex", b"norm=3"),
    (lambda L: _linear(L, norm=-1), b"mt_linear_rows_ex", b"norm=-1"),
    (lambda L: _linear(L, beta=3 * P), b"mt_linear_rows_ex", b"no beta"),
    (lambda L: _linear(L, gelu=1, glu=1), b"mt_linear_rows_ex", b"share a group"),
    (lambda L: _linear(L, glu=2), b"mt_linear_rows_ex", b"glu_mask=2"),
    (lambda L: _linear(L, G=2, W=[16 * P, 20 * P], N=[64, 64], glu=4), b"mt_linear_rows_ex", b"glu_mask=4"),
    (lambda L: _linear(L, eps=-1.0), b"mt_linear_rows_ex", b"eps"),
    (lambda L: L.mt_rmsnorm_fw(P, None, 2 * P, 3 * P, 4, 8, 1e-5, None), b"mt_rmsnorm_fw", b"NULL"),
    (lambda L: L.mt_rmsnorm_fw(P, 5 * P, 2 * P, 3 * P, 4, 0, 1e-5, None), b"mt_rmsnorm_fw", b"hidden=0"),
    (lambda L: L.mt_rmsnorm_fw(P, 5 * P, 2 * P, 3 * P, 4, 8, -1e-5, None), b"mt_rmsnorm_fw", b"eps"),
    (lambda L: L.mt_rmsnorm_bw(P, 2 * P, 3 * P, 4 * P, 5 * P, None, 4, 8, 6 * P, None), b"mt_rmsnorm_bw", b"NULL"),
    (lambda L: L.mt_rmsnorm_bw(P, 2 * P, 3 * P, 4 * P, 5 * P, 7 * P, 4, -8, 6 * P, None), b"mt_rmsnorm_bw", b"hidden=-8"),
    (lambda L: L.mt_swiglu_fw(P, None, 4, 8, None), b"mt_swiglu_fw", b"NULL"),
    (lambda L: L.mt_swiglu_fw(P, 2 * P, 4, 0, None), b"mt_swiglu_fw", b"F=0"),
    (lambda L: L.mt_swiglu_bw(P, 2 * P, None, 4, 8, None), b"mt_swiglu_bw", b"NULL"),
    (lambda L: L.mt_swiglu_bw(P, 2 * P, 3 * P, 4, -1, None), b"mt_swiglu_bw", b"F=-1"),
])
def test_refusals(call, name, msg):
    from minitorch import _hip
    lib = _hip.lib()
    assert call(lib) != 0
    err = lib.mt_last_error()
    assert err.startswith(name + b":") and msg in err, err


def test_abi_version_and_binding():
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    lib = _hip.lib()
    assert lib.mt_abi_version() == 3
    assert all(s in _hip.exported_symbols() and hasattr(lib, s) for s in NEW)
    hip, cpu = minitorch.TensorBackend(minitorch.HipKernelOps), minitorch.TensorBackend(NumpyOps)
    for attr in ("rmsnorm_fw", "rmsnorm_bw", "swiglu_fw", "swiglu_bw"):
        assert getattr(hip, attr) is not None and getattr(cpu, attr) is None
    lm = minitorch.DecoderLM(n_vocab=11, n_embd=8, n_head=2, n_positions=8, backend=cpu, n_layer=1, norm="rms", mlp="swiglu")
    assert isinstance(lm.ln, minitorch.FusedRMSNorm) and lm.t_layer_1.ff.linear_in.weights.value.shape == (8, 512)
    with pytest.raises(ValueError, match="norm must be"):
        minitorch.DecoderLM(n_vocab=11, n_embd=8, n_head=2, n_positions=8, backend=cpu, n_layer=1, norm="batch")
