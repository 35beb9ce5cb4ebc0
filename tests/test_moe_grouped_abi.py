"""The routed mixture-of-experts entry points (mt_moe_sort, mt_moe_grouped_gemm, mt_moe_combine,
mt_moe_gate_grad): exported and bound, their refusals (CPU: every refusal precedes the first device
call, so dummy pointers are enough and nothing is launched, as in tests/test_moe_abi.py), and a
backend without the kernels taking the dense path."""
import numpy as np
import pytest

P = 4096  # dummy "device" addresses, 16-byte aligned and far apart
NEW = ("mt_moe_sort_workspace_bytes", "mt_moe_sort", "mt_moe_grouped_gemm", "mt_moe_combine", "mt_moe_gate_grad")


def _gemm(lib, **kw):
    a = dict(form=0, A=P, src=None, B=2 * P, srcb=None, bias=None, offsets=3 * P, E=8, Kd=64, N=128, C=4 * P, db=None)
    a.update(kw)
    return lib.mt_moe_grouped_gemm(a["form"], a["A"], 512, a["src"], None, a["B"], 512, a["srcb"], a["bias"], a["offsets"],
                                   512, a["E"], a["Kd"], a["N"], a["C"], a["db"], None)


def _sort(lib, **kw):
    a = dict(idx=P, E=8, k=2, pos=4 * P, ws=5 * P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.mt_moe_sort(a["idx"], None, 256, a["E"], a["k"], 2 * P, 3 * P, a["pos"], None, None, a["ws"],
                           a["ws_bytes"], None)


@pytest.mark.parametrize("call,name,msg", [
    (lambda L: _gemm(L, form=3), b"mt_moe_grouped_gemm", b"form=3"),
    (lambda L: _gemm(L, A=None), b"mt_moe_grouped_gemm", b"NULL"),
    (lambda L: _gemm(L, offsets=None), b"mt_moe_grouped_gemm", b"offsets is NULL"),
    (lambda L: _gemm(L, B=2 * P + 4), b"mt_moe_grouped_gemm", b"misaligned"),
    (lambda L: _gemm(L, Kd=66), b"mt_moe_grouped_gemm", b"Kd=66"),
    (lambda L: _gemm(L, N=2), b"mt_moe_grouped_gemm", b"N=2"),
    (lambda L: _gemm(L, E=1), b"mt_moe_grouped_gemm", b"E=1"),
    (lambda L: _gemm(L, form=1, bias=5 * P), b"mt_moe_grouped_gemm", b"no bias"),
    (lambda L: _gemm(L, db=5 * P), b"mt_moe_grouped_gemm", b"TN form"),
    (lambda L: _sort(L, idx=None), b"mt_moe_sort", b"topk_idx is NULL"),
    (lambda L: _sort(L, E=1, k=1), b"mt_moe_sort", b"E=1"),
    (lambda L: _sort(L, E=4, k=5), b"mt_moe_sort", b"exceeds E=4"),
    (lambda L: _sort(L, pos=4 * P + 2), b"mt_moe_sort", b"misaligned"),
    (lambda L: _sort(L, ws_bytes=16), b"mt_moe_sort", b"workspace_bytes=16"),
    (lambda L: L.mt_moe_combine(P, 2 * P, None, None, None, 3 * P, 8, 30, 8, 2, None), b"mt_moe_combine", b"N=30"),
    (lambda L: L.mt_moe_combine(P, 2 * P, 4 * P, None, None, 3 * P, 8, 32, 8, 2, None), b"mt_moe_combine", b"go together"),
    (lambda L: L.mt_moe_gate_grad(P, 2 * P, 3 * P, 4 * P, None, 8, 32, 8, 2, None), b"mt_moe_gate_grad", b"NULL"),
    (lambda L: L.mt_moe_gate_grad(P + 4, 2 * P, 3 * P, 4 * P, 5 * P, 8, 32, 8, 2, None), b"mt_moe_gate_grad", b"misaligned"),
])
def test_refusals(call, name, msg):
    from minitorch import _hip
    lib = _hip.lib()
    assert call(lib) != 0
    err = lib.mt_last_error()
    assert err.startswith(name + b":") and msg in err, err


def test_binding_and_the_dense_fallback():
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    lib = _hip.lib()
    assert all(s in _hip.exported_symbols() and hasattr(lib, s) for s in NEW)
    calls = _hip.moe_grouped_calls
    hip, cpu = minitorch.TensorBackend(minitorch.HipKernelOps), minitorch.TensorBackend(NumpyOps)
    assert hip.moe_routed_fw is not None and hip.moe_routed_bw is not None
    assert cpu.moe_routed_fw is None and cpu.moe_routed_bw is None
    kw = dict(n_vocab=11, n_embd=8, n_head=2, n_positions=8, backend=cpu, n_layer=1, mlp="moe", n_experts=4, moe_top_k=2,
              p_dropout=0.0)
    np.random.seed(0)
    routed = minitorch.DecoderLM(moe_routed=True, **kw)
    np.random.seed(0)
    dense = minitorch.DecoderLM(**kw)
    assert routed.t_layer_1.ff.routed and not dense.t_layer_1.ff.routed
    x = minitorch.tensor_from_numpy(np.array([[1, 5, 2, 7]], np.float32), cpu)
    assert np.array_equal(routed(x).to_numpy(), dense(x).to_numpy()), "a CPU model runs the dense path"
    assert _hip.moe_grouped_calls == calls
