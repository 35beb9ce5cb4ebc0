"""mt_select_token's argument validation (CPU: every refusal precedes the first device call, so
NULL or dummy pointers are enough and nothing is launched)."""
import ctypes

import pytest

DUMMY = ctypes.c_void_p(256)


def _call(lib, **kw):
    a = dict(logits=DUMMY, B=2, V=8, row_stride=8, temperature=0.0, top_k=0, seed=0, seed_dev=None, eos_id=-1,
             next_f32=DUMMY, next_i32=DUMMY, done=None, history=None, history_stride=0, step_dev=None, stream=None)
    a.update(kw)
    return lib.mt_select_token(a["logits"], a["B"], a["V"], a["row_stride"], a["temperature"], a["top_k"],
                               a["seed"], a["seed_dev"], a["eos_id"], a["next_f32"], a["next_i32"], a["done"],
                               a["history"], a["history_stride"], a["step_dev"], a["stream"])


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), b"bad sizes"),
    (dict(B=-1), b"bad sizes"),
    (dict(V=0, row_stride=0), b"bad sizes"),
    (dict(V=-3), b"bad sizes"),
    (dict(row_stride=7), b"row_stride"),
    (dict(temperature=-0.5), b"temperature"),
    (dict(temperature=float("nan")), b"temperature"),
    (dict(logits=None), b"logits is NULL"),
    (dict(next_f32=None, next_i32=None), b"both outputs"),
    (dict(history=DUMMY, history_stride=4, step_dev=None), b"step_dev"),
    (dict(V=32769, row_stride=32769), b"limit"),
])
def test_refusals(kw, msg):
    from minitorch import _hip
    lib = _hip.lib()
    assert _call(lib, **kw) != 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


def test_abi_version_and_binding():
    from minitorch import _hip
    lib = _hip.lib()
    assert lib.mt_abi_version() == 3
    assert "mt_select_token" in _hip.exported_symbols()
    assert callable(_hip.select_token)


def test_backend_binds_select_token_optionally():
    import minitorch
    from cpu_backend import NumpyOps
    assert minitorch.TensorBackend(NumpyOps).select_token is None
    assert minitorch.TensorBackend(minitorch.HipKernelOps).select_token is not None


def test_graph_and_sampling_need_the_kernel():
    """generate(graph=True) without the cache, and sampling or graph on a backend without the
    select_token kernel, are refused by name (no GPU needed: refused before any device work)."""
    import numpy as np
    import minitorch
    from cpu_backend import NumpyOps
    cpu = minitorch.TensorBackend(NumpyOps)
    np.random.seed(0)
    lm = minitorch.DecoderLM(n_vocab=11, n_embd=8, n_head=2, n_positions=8, p_dropout=0.0, backend=cpu, n_layer=1)
    with pytest.raises(ValueError, match="use_cache"):
        lm.generate([[1, 2]], 2, use_cache=False, graph=True)
    with pytest.raises(ValueError, match="select_token"):
        lm.generate([[1, 2]], 2, graph=True)
    with pytest.raises(ValueError, match="select_token"):
        lm.generate([[1, 2]], 2, use_cache=False, temperature=0.7)
    # the defaults are today's greedy host loop
    assert len(lm.generate([[1, 2]], 2, use_cache=False)[0]) == 2
