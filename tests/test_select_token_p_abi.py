"""mt_select_token_p / mt_spec_accept_p on the CPU: the exports, the ABI version, every refusal
the two entries add (top_p, min_p) and those they inherit, by message (made before any device
call, so dummy pointers are enough and nothing is launched), and generate(top_p=, min_p=) on a
backend without the kernel."""
import ctypes

import pytest

P = ctypes.c_void_p(256)  # non-NULL, 4-B aligned, never dereferenced: every call below is refused first
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


def select_args(**over):
    a = dict(logits=P, B=2, V=8, row_stride=8, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=0, seed_dev=None,
             eos_id=-1, next_f32=P, next_i32=P, done=None, history=None, history_stride=0, step_dev=None, stream=None)
    a.update(over)
    return list(a.values())


def accept_args(**over):
    a = dict(logits=P, B=2, k=3, V=97, batch_stride=4 * 97, row_stride=97, feed_i32=P, n_draft=P, temperature=1.0,
             top_k=0, top_p=1.0, min_p=0.0, seed=0, seed_dev=None, eos_id=-1, limit=P, count=P, held=P, cache_len=P,
             done=P, drafted=P, accepted=P, steps=P, tokens=P, S=16, token_stride=16, history=P, history_stride=16,
             scratch=P, stream=None)
    a.update(over)
    return list(a.values())


NEW_REFUSALS = [
    (dict(top_p=0.0), b"top_p must be in (0, 1] (got 0)"),
    (dict(top_p=-0.25), b"top_p must be in (0, 1] (got -0.25)"),
    (dict(top_p=1.5), b"top_p must be in (0, 1] (got 1.5)"),
    (dict(top_p=NAN), b"top_p must be in (0, 1]"),
    (dict(min_p=-0.5), b"min_p must be in [0, 1] (got -0.5)"),
    (dict(min_p=1.25), b"min_p must be in [0, 1] (got 1.25)"),
    (dict(min_p=NAN), b"min_p must be in [0, 1]"),
    # greedy ignores the filters' values, not their ranges
    (dict(temperature=0.0, top_p=2.0), b"top_p must be in (0, 1] (got 2)"),
    (dict(temperature=0.0, min_p=-1.0), b"min_p must be in [0, 1] (got -1)"),
]


def test_exports_and_abi_version(lib):
    from minitorch import _hip
    assert {"mt_select_token_p", "mt_spec_accept_p"} <= set(_hip.exported_symbols())
    assert hasattr(lib, "mt_select_token_p") and hasattr(lib, "mt_spec_accept_p")
    assert hasattr(lib, "mt_select_token") and hasattr(lib, "mt_spec_accept"), "the old entries stay"
    assert lib.mt_abi_version() == 3


@pytest.mark.parametrize("over,msg", NEW_REFUSALS + [
    (dict(B=0), b"bad sizes"),
    (dict(V=0, row_stride=0), b"bad sizes"),
    (dict(V=32769, row_stride=32769), b"above the limit of 32768"),
    (dict(row_stride=7), b"row_stride 7 is below V=8"),
    (dict(temperature=-0.5), b"temperature must be >= 0"),
    (dict(temperature=NAN), b"temperature must be >= 0"),
    (dict(logits=None), b"logits is NULL"),
    (dict(logits=ctypes.c_void_p(258)), b"not 4-B aligned"),
    (dict(next_f32=None, next_i32=None), b"both outputs"),
    (dict(history=P, history_stride=4, step_dev=None), b"history needs step_dev"),
    (dict(history=P, history_stride=0, step_dev=P), b"history_stride 0 must be positive"),
])
def test_select_token_p_refusals(lib, over, msg):
    assert lib.mt_select_token_p(*select_args(**over)) != 0
    err = lib.mt_last_error()
    assert err.startswith(b"mt_select_token_p:") and msg in err, err


@pytest.mark.parametrize("over,msg", NEW_REFUSALS + [
    (dict(k=0), b"k=0 is outside 1..7"),
    (dict(k=8), b"k=8 is outside 1..7"),
    (dict(B=0), b"bad sizes"),
    (dict(V=32769, row_stride=32769, batch_stride=4 * 32769), b"above the limit of 32768"),
    (dict(S=4, token_stride=4), b"S=4 is below k + 2 = 5"),
    (dict(row_stride=96), b"row_stride 96 is below V=97"),
    (dict(batch_stride=4 * 97 - 1), b"batch_stride 387 is below"),
    (dict(token_stride=15), b"token_stride 15 is below S=16"),
    (dict(history_stride=0), b"history_stride 0 must be positive"),
    (dict(temperature=-1.0), b"temperature must be >= 0"),
    (dict(logits=None), b"logits is NULL"),
    (dict(scratch=None), b"scratch is NULL"),
    (dict(done=None), b"done is NULL"),
])
def test_spec_accept_p_refusals(lib, over, msg):
    assert lib.mt_spec_accept_p(*accept_args(**over)) != 0
    err = lib.mt_last_error()
    assert err.startswith(b"mt_spec_accept_p:") and msg in err, err


def test_python_bindings_take_the_keywords():
    import inspect
    import minitorch
    from minitorch import _hip
    for fn in (_hip.select_token, _hip.spec_accept):
        sig = inspect.signature(fn).parameters
        assert sig["top_p"].default == 1.0 and sig["min_p"].default == 0.0, fn.__name__
    gen = inspect.signature(minitorch.DecoderLM.generate).parameters
    assert gen["top_p"].default is None and gen["min_p"].default is None


def test_generate_refusals_and_greedy_on_the_numpy_backend():
    """Out-of-range values and sampling without the kernel are refused before any device work;
    greedy decoding ignores both filters and stays today's host loop."""
    import numpy as np
    import minitorch
    from cpu_backend import NumpyOps
    cpu = minitorch.TensorBackend(NumpyOps)
    np.random.seed(0)
    lm = minitorch.DecoderLM(n_vocab=11, n_embd=8, n_head=2, n_positions=8, p_dropout=0.0, backend=cpu, n_layer=1)
    prompts = [[1, 2]]
    for bad in (0.0, -0.1, 1.01, NAN):
        with pytest.raises(ValueError, match="top_p must be"):
            lm.generate(prompts, 2, use_cache=False, top_p=bad)
        with pytest.raises(ValueError, match="top_p must be"):
            lm.generate(prompts, 2, use_cache=False, temperature=0.7, top_p=bad)
    for bad in (-0.1, 1.01, NAN):
        with pytest.raises(ValueError, match="min_p must be"):
            lm.generate(prompts, 2, use_cache=False, min_p=bad)
    with pytest.raises(ValueError, match="select_token"):
        lm.generate(prompts, 2, use_cache=False, temperature=0.7, top_p=0.9)
    with pytest.raises(ValueError, match="select_token"):
        lm.generate(prompts, 2, use_cache=False, temperature=0.7, min_p=0.05)
    want = lm.generate(prompts, 4, use_cache=False)
    assert len(want[0]) == 4
    assert lm.generate(prompts, 4, use_cache=False, temperature=0, top_p=0.5) == want
    assert lm.generate(prompts, 4, use_cache=False, temperature=0, top_p=0.5, min_p=0.3) == want
    assert lm.generate(prompts, 4, use_cache=False, top_p=1.0, min_p=0.0) == want
