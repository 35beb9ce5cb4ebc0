"""mt_spec_draft / mt_spec_accept on the CPU: the exports, every refusal with its message (made
before any device call, so no GPU is needed), the ABI version, and generate(speculate=...) on a
backend without the kernels."""
import ctypes

import pytest

P = ctypes.c_void_p(16)  # a non-NULL pointer that is never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


def draft_args(**over):
    a = dict(tokens=P, B=2, S=16, token_stride=16, held=P, k=3, max_ngram=3, feed_f32=P, feed_i32=P, n_draft=P,
             stream=None)
    a.update(over)
    return list(a.values())


def accept_args(**over):
    a = dict(logits=P, B=2, k=3, V=97, batch_stride=4 * 97, row_stride=97, feed_i32=P, n_draft=P, temperature=0.0,
             top_k=0, seed=0, seed_dev=None, eos_id=-1, limit=P, count=P, held=P, cache_len=P, done=P, drafted=P,
             accepted=P, steps=P, tokens=P, S=16, token_stride=16, history=P, history_stride=16, scratch=P,
             stream=None)
    a.update(over)
    return list(a.values())


def test_exports_and_abi_version(lib):
    from minitorch import _hip
    assert {"mt_spec_draft", "mt_spec_accept"} <= set(_hip.exported_symbols())
    assert hasattr(lib, "mt_spec_draft") and hasattr(lib, "mt_spec_accept")
    assert lib.mt_abi_version() == 3


@pytest.mark.parametrize("over,msg", [
    (dict(k=0), b"k=0 is outside 1..7"),
    (dict(k=8), b"k=8 is outside 1..7"),
    (dict(max_ngram=0), b"max_ngram=0 is outside 1..8"),
    (dict(max_ngram=9), b"max_ngram=9 is outside 1..8"),
    (dict(B=0), b"bad sizes"),
    (dict(S=0), b"bad sizes"),
    (dict(S=4, token_stride=4), b"S=4 is below k + 2 = 5"),
    (dict(token_stride=15), b"token_stride 15 is below S=16"),
    (dict(tokens=None), b"tokens is NULL"),
    (dict(held=None), b"held is NULL"),
    (dict(n_draft=None), b"n_draft is NULL"),
    (dict(feed_f32=None, feed_i32=None), b"both outputs"),
])
def test_draft_refusals(lib, over, msg):
    assert lib.mt_spec_draft(*draft_args(**over)) != 0
    err = lib.mt_last_error()
    assert err.startswith(b"mt_spec_draft") and msg in err, err


@pytest.mark.parametrize("over,msg", [
    (dict(k=0), b"k=0 is outside 1..7"),
    (dict(k=8), b"k=8 is outside 1..7"),
    (dict(B=0), b"bad sizes"),
    (dict(V=0), b"bad sizes"),
    (dict(S=0), b"bad sizes"),
    (dict(V=32769, row_stride=32769, batch_stride=4 * 32769), b"above the limit of 32768"),
    (dict(S=4, token_stride=4), b"S=4 is below k + 2 = 5"),
    (dict(row_stride=96), b"row_stride 96 is below V=97"),
    (dict(batch_stride=4 * 97 - 1), b"batch_stride 387 is below"),
    (dict(token_stride=15), b"token_stride 15 is below S=16"),
    (dict(history_stride=0), b"history_stride 0 must be positive"),
    (dict(temperature=-1.0), b"temperature must be >= 0"),
    (dict(temperature=float("nan")), b"temperature must be >= 0"),
    (dict(logits=None), b"logits is NULL"),
    (dict(feed_i32=None), b"feed_i32 is NULL"),
    (dict(n_draft=None), b"n_draft is NULL"),
    (dict(limit=None), b"limit is NULL"),
    (dict(count=None), b"count is NULL"),
    (dict(held=None), b"held is NULL"),
    (dict(done=None), b"done is NULL"),
    (dict(tokens=None), b"tokens is NULL"),
    (dict(history=None), b"history is NULL"),
    (dict(scratch=None), b"scratch is NULL"),
])
def test_accept_refusals(lib, over, msg):
    assert lib.mt_spec_accept(*accept_args(**over)) != 0
    err = lib.mt_last_error()
    assert err.startswith(b"mt_spec_accept") and msg in err, err


def test_generate_speculate_needs_the_kernels_and_a_cache():
    import minitorch
    from cpu_backend import NumpyOps
    cpu = minitorch.TensorBackend(NumpyOps)
    lm = minitorch.DecoderLM(n_vocab=31, n_embd=16, n_head=2, n_positions=16, p_dropout=0.0, backend=cpu, n_layer=1)
    prompts = [[1, 2, 3]]
    with pytest.raises(ValueError, match="spec_draft / spec_accept"):
        lm.generate(prompts, 4, speculate=2)
    with pytest.raises(ValueError, match="use_cache"):
        lm.generate(prompts, 4, speculate=2, use_cache=False)
    for bad in (8, -1, 2.5):
        with pytest.raises(ValueError, match="speculate must be"):
            lm.generate(prompts, 4, speculate=bad)
    for bad in (0, 9, 1.5):
        with pytest.raises(ValueError, match="ngram must be"):
            lm.generate(prompts, 4, speculate=2, ngram=bad)
    assert lm.spec_stats is None, "a refused call ran nothing"
