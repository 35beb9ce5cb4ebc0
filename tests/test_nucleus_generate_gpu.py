"""DecoderLM.generate(top_p=, min_p=): every generation path chooses by the same kernel, so the
eager, graph-replayed and speculative ids of one call are equal, on every cache kind; the ids
are those of prefill plus one-token steps done by hand and lie inside the reference's kept set
(tests/nucleus_ref.py); top_p = 1e-6 and min_p = 1 are greedy; the captured graphs are keyed by
both values, and the off values are the call without them.

The model is test_generate_graph_gpu.py's (n_vocab 97, n_embd 64, 4 heads, 48 positions, no
dropout, prompts of 3 / 9 / 14 tokens, 16 new tokens)."""
import gc

import numpy as np
import pytest

import nucleus_ref as R
from spec_ref import simulate, totals

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16
S = dict(temperature=0.8, top_k=20, top_p=0.7, min_p=0.05, seed=1234)


def expect(ids, prompts, k, ngram=3, max_new=NEW):
    """spec_stats as simulate() has them for the plain ids of a call."""
    return totals([simulate(row, p, k, ngram, min(max_new, KW["n_positions"] - len(p) + 1), None)
                   for row, p in zip(ids, prompts)])


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from minitorch import _hip
    _hip.lib()
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    np.random.seed(0)
    lm = minitorch.DecoderLM(backend=hip, **KW)
    lm.eval()
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    # computed once, shared: the eager continuations
    w = dict(minitorch=minitorch, hip=hip, lm=lm, prompts=prompts, greedy=lm.generate(prompts, NEW),
             eager=lm.generate(prompts, NEW, **S))
    yield w
    # the model's graphs go here and now, not whenever the collector next runs
    w.clear()
    del lm
    gc.collect()


def test_paths_agree(world):
    lm, prompts, eager = world["lm"], world["prompts"], world["eager"]
    assert all(len(t) == NEW for t in eager)
    assert eager != world["greedy"], "the sampled tokens are the greedy ones: nothing was shown"
    unfiltered = lm.generate(prompts, NEW, **dict(S, top_p=None, min_p=None))
    assert eager != unfiltered, "the filters changed no id: nothing was shown"
    assert lm.generate(prompts, NEW, graph=True, **S) == eager
    assert lm.generate(prompts, NEW, **S) == eager
    for k in (4, 7):
        for graph in (False, True):
            assert lm.generate(prompts, NEW, speculate=k, graph=graph, **S) == eager, (k, graph)
            assert lm.spec_stats == expect(eager, prompts, k), (k, graph)


@pytest.mark.parametrize("mode", [dict(kv_dtype="fp8"), dict(page_size=16), dict(pos_encoding="rope"),
                                  dict(prefill_chunk=8)], ids=lambda m: "-".join(f"{a}={b}" for a, b in m.items()))
def test_paths_agree_on_every_cache_mode(world, mode):
    mt, hip, prompts = world["minitorch"], world["hip"], world["prompts"]
    lm, kw = world["lm"], mode
    if "pos_encoding" in mode:  # a model of its own, dropped with its graphs below
        np.random.seed(0)
        lm, kw = mt.DecoderLM(backend=hip, **KW, **mode), {}
        lm.eval()
    try:
        eager = lm.generate(prompts, NEW, **kw, **S)
        assert lm.generate(prompts, NEW, graph=True, **kw, **S) == eager
        for graph in (False, True):
            assert lm.generate(prompts, NEW, speculate=4, graph=graph, **kw, **S) == eager, graph
            assert lm.spec_stats == expect(eager, prompts, 4), graph
    finally:
        if lm is not world["lm"]:
            lm.drop_decode_graphs()


def test_by_hand(world):
    """Prefill plus one-token steps with backend.select_token(seed + t) are the eager ids, and
    every id lies in the widest prefix the reference allows for that step's logits."""
    mt, hip, lm, prompts, eager = world["minitorch"], world["hip"], world["lm"], world["prompts"], world["eager"]
    B = len(prompts)
    lens = np.array([len(p) for p in prompts], dtype=np.int64)
    idx = np.zeros((B, int(lens.max())), dtype=np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    cache = lm.new_cache(B)
    logits, rows = lm._prefill_logits(idx, lens, cache, None)
    ids, cut = [], 0
    for t in range(NEW):
        host = logits.to_numpy()
        host = host[np.arange(B), rows] if rows is not None else host[:, 0]
        nxt = hip.select_token(logits, S["temperature"], S["top_k"], S["seed"] + t, rows=rows, top_p=S["top_p"],
                               min_p=S["min_p"])[1].cpu().numpy()
        for b in range(B):
            row = R.Row(host[b], S["temperature"], S["top_k"])
            _, hi = row.bounds(S["top_p"], S["min_p"])
            assert int(nxt[b]) in row.prefix(hi).tolist(), (t, b, int(nxt[b]))
            cut += hi < S["top_k"]
        ids.append(nxt.copy())
        if t + 1 < NEW:
            logits, rows = lm.forward(mt.tensor_from_numpy(nxt.astype(np.float32).reshape(B, 1), backend=hip),
                                      cache=cache), None
    assert np.stack(ids, axis=1).tolist() == eager
    assert cut > 0, "the filters cut nothing below top_k at any step: nothing was shown"


def test_exact_settings_are_greedy(world):
    lm, prompts, greedy = world["lm"], world["prompts"], world["greedy"]
    for graph in (False, True):
        assert lm.generate(prompts, NEW, temperature=1.0, top_p=1e-6, seed=5, graph=graph) == greedy
        assert lm.generate(prompts, NEW, temperature=1.0, min_p=1.0, seed=5, graph=graph) == greedy
    assert lm.generate(prompts, NEW, temperature=1.0, top_p=1e-6, seed=5, speculate=4) == greedy
    # greedy decoding ignores both
    assert lm.generate(prompts, NEW, top_p=0.3, min_p=0.5) == greedy
    assert lm.generate(prompts, NEW, top_p=0.3, min_p=0.5, graph=True) == greedy


def test_graph_keys_hold_both_values(world):
    lm, prompts = world["lm"], world["prompts"]
    a = lm.generate(prompts, NEW, graph=True, **S)
    n = lm.graph_captures
    b = lm.generate(prompts, NEW, graph=True, **dict(S, top_p=0.3))
    assert lm.graph_captures == n + 1, "another top_p must capture its own graph"
    assert b == lm.generate(prompts, NEW, **dict(S, top_p=0.3)) and b != a
    c = lm.generate(prompts, NEW, graph=True, **dict(S, min_p=0.4))
    assert lm.graph_captures == n + 2, "another min_p must capture its own graph"
    assert c == lm.generate(prompts, NEW, **dict(S, min_p=0.4))
    # repeats replay what was captured
    assert lm.generate(prompts, NEW, graph=True, **S) == a
    assert lm.generate(prompts, NEW, graph=True, **dict(S, top_p=0.3)) == b
    assert lm.graph_captures == n + 2
    # the speculative graphs are keyed the same way
    assert lm.generate(prompts, NEW, speculate=4, graph=True, **S) == a
    m = lm.graph_captures
    assert lm.generate(prompts, NEW, speculate=4, graph=True, **dict(S, top_p=0.3)) == b
    assert lm.graph_captures == m + 1
    assert lm.generate(prompts, NEW, speculate=4, graph=True, **S) == a
    assert lm.graph_captures == m + 1


def test_off_values_are_the_call_without_them(world):
    lm, prompts = world["lm"], world["prompts"]
    plain = dict(temperature=0.8, top_k=20, seed=1234)
    want = lm.generate(prompts, NEW, graph=True, **plain)
    assert want == lm.generate(prompts, NEW, **plain)
    n = lm.graph_captures
    assert lm.generate(prompts, NEW, graph=True, top_p=1.0, min_p=0.0, **plain) == want
    assert lm.generate(prompts, NEW, graph=True, top_p=None, min_p=0.0, **plain) == want
    assert lm.graph_captures == n, "the off values must replay the graph of the call without them"
    assert lm.generate(prompts, NEW, top_p=1.0, min_p=0.0, **plain) == want
    assert lm.generate(prompts, NEW, speculate=4, top_p=1.0, **plain) == want


def test_misuse_raises_before_any_launch(world):
    lm, prompts = world["lm"], world["prompts"]
    n = lm.graph_captures
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(min_p=-0.1), dict(min_p=2.0)):
        with pytest.raises(ValueError, match="must be None or in"):
            lm.generate(prompts, 4, graph=True, temperature=0.8, **kw)
    assert lm.graph_captures == n
