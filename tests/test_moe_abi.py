"""The mixture-of-experts entry points: exported and bound, and their argument validation (CPU: every
refusal precedes the first device call, so dummy pointers are enough and nothing is launched), as
tests/test_llama_block_abi.py does for mt_linear_rows_ex."""
import ctypes

import pytest

P = 4096  # dummy "device" addresses, 16-byte aligned and far apart
NEW = ("mt_moe_rows_workspace_bytes", "mt_moe_route", "mt_moe_rows")


def _rows(lib, **kw):
    a = dict(x=P, M=8, K=256, norm=2, gamma=2 * P, beta=None, eps=1e-5, Wr=3 * P, E=8, k=2, W_in=16 * P, F=64,
             W_out=4096 * P, N=256, out=8192 * P, ws=9000 * P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.mt_moe_rows(a["x"], a["K"], a["M"], a["K"], a["norm"], a["gamma"], a["beta"], a["eps"], a["Wr"], a["E"],
                           a["k"], a["W_in"], None, a["F"], a["W_out"], None, a["N"], None, a["out"], None, None,
                           a["ws"], a["ws_bytes"], None)


def _route(lib, **kw):
    a = dict(x=P, K=256, norm=0, gamma=None, E=8, k=2, idx=5 * P)
    a.update(kw)
    return lib.mt_moe_route(a["x"], a["K"], 8, a["K"], a["norm"], a["gamma"], None, 1e-5, 3 * P, a["E"], a["k"], None,
                            a["idx"], None, None, None)


@pytest.mark.parametrize("call,name,msg", [
    (lambda L: _rows(L, x=None), b"mt_moe_rows", b"x is NULL"),
    (lambda L: _rows(L, x=P + 4), b"mt_moe_rows", b"misaligned"),
    (lambda L: _rows(L, W_in=None), b"mt_moe_rows", b"NULL"),
    (lambda L: _rows(L, out=None), b"mt_moe_rows", b"out is NULL"),
    (lambda L: _rows(L, ws=None), b"mt_moe_rows", b"workspace is NULL"),
    (lambda L: _rows(L, ws_bytes=1024), b"mt_moe_rows", b"workspace_bytes=1024"),
    (lambda L: _rows(L, M=65), b"mt_moe_rows", b"M=65"),
    (lambda L: _rows(L, K=1028), b"mt_moe_rows", b"K=1028"),
    (lambda L: _rows(L, F=0), b"mt_moe_rows", b"F=0"),
    (lambda L: _rows(L, E=1, k=1), b"mt_moe_rows", b"E=1"),
    (lambda L: _rows(L, k=0), b"mt_moe_rows", b"k=0"),
    (lambda L: _rows(L, E=16, k=9), b"mt_moe_rows", b"k=9"),
    (lambda L: _rows(L, E=4, k=5), b"mt_moe_rows", b"exceeds E=4"),
    (lambda L: _rows(L, norm=3), b"mt_moe_rows", b"norm=3"),
    (lambda L: _rows(L, norm=0), b"mt_moe_rows", b"norm=0 takes no gamma"),
    (lambda L: _rows(L, norm=1), b"mt_moe_rows", b"gamma and beta"),
    (lambda L: _rows(L, gamma=None), b"mt_moe_rows", b"needs gamma"),
    (lambda L: _rows(L, beta=5 * P), b"mt_moe_rows", b"no beta"),
    (lambda L: _rows(L, eps=-1.0), b"mt_moe_rows", b"eps"),
    (lambda L: _rows(L, out=P), b"mt_moe_rows", b"overlaps x"),
    (lambda L: _route(L, idx=None), b"mt_moe_route", b"every output is NULL"),
    (lambda L: _route(L, E=4, k=5), b"mt_moe_route", b"exceeds E=4"),
    (lambda L: _route(L, idx=5 * P + 1), b"mt_moe_route", b"misaligned"),
    (lambda L: L.mt_moe_rows_workspace_bytes(8, 256, 64, 256, 8, 2, None), b"mt_moe_rows_workspace_bytes", b"NULL"),
    (lambda L: L.mt_moe_rows_workspace_bytes(8, 256, 64, 256, 8, 9, ctypes.byref(ctypes.c_int64())),
     b"mt_moe_rows_workspace_bytes", b"k=9"),
])
def test_refusals(call, name, msg):
    from minitorch import _hip
    lib = _hip.lib()
    assert call(lib) != 0
    err = lib.mt_last_error()
    assert err.startswith(name + b":") and msg in err, err


def test_binding_and_model_arguments():
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    lib = _hip.lib()
    assert all(s in _hip.exported_symbols() and hasattr(lib, s) for s in NEW)
    # xh [8, 256] | idx [16] | gate [16] | h [16, 64] | y [16, 256] fp32
    assert _hip.moe_rows_workspace_bytes(8, 256, 64, 256, 8, 2) == 4 * (8 * 256 + 16 + 16 + 16 * 64 + 16 * 256)
    hip, cpu = minitorch.TensorBackend(minitorch.HipKernelOps), minitorch.TensorBackend(NumpyOps)
    assert hip.moe_mlp is not None and hip.moe_route is not None and cpu.moe_mlp is None
    kw = dict(n_vocab=11, n_embd=8, n_head=2, n_positions=8, backend=cpu, n_layer=1)
    lm = minitorch.DecoderLM(mlp="moe", n_experts=4, moe_top_k=2, use_fused_kernel=True, fused_step=True, **kw)
    ff = lm.t_layer_1.ff
    assert isinstance(ff, minitorch.MoEFeedForward)
    assert ff.router.value.shape == (8, 4) and ff.w_in.value.shape == (4, 8, 512) and ff.w_out.value.shape == (4, 256, 8)
    with pytest.raises(ValueError, match="mixture-of-experts"):
        lm.quantize_weights("bf16")
    with pytest.raises(ValueError, match="mlp must be"):
        minitorch.DecoderLM(mlp="experts", **kw)
    with pytest.raises(ValueError, match="top_k"):
        minitorch.DecoderLM(mlp="moe", n_experts=4, moe_top_k=5, **kw)
