"""DecoderLM.generate(speculate=k): the ids are those of the same call without speculation
(exact-match verification), greedy and sampled, eager and graph-replayed, in every mode generate
has; lm.spec_stats equals tests/spec_ref.py's simulate() run on the plain ids, exactly.

The model is test_generate_graph_gpu.py's (n_vocab 97, n_embd 64, 4 heads, 48 positions, prompts
of 3 / 9 / 14 tokens, 16 new tokens).

Acceptance: the greedy continuation of the 3-token prompt of that set runs into 82 82 82 82, which
prompt lookup drafts (found with the same weights on the CPU backend: 2 drafts accepted at k = 4
and 7, 1 at k = 1; at 34 new tokens all three rows accept). The tests assert accepted > 0 from
simulate() on the ids the GPU returned, so a set that stops accepting fails them."""
import gc

import numpy as np
import pytest

from spec_ref import simulate, totals

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16
LONG = 34
SAMPLE = dict(temperature=0.8, top_k=5, seed=1234)


def make_prompts(seed=0, sizes=(3, 9, 14)):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in sizes]


def expect(ids, prompts, k, ngram, max_new, eos=None):
    """spec_stats as simulate() has them for the plain ids of a call."""
    return totals([simulate(row, p, k, ngram, min(max_new, KW["n_positions"] - len(p) + 1), eos)
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
    prompts = make_prompts()
    # computed once, shared: the plain (non-speculative) continuations
    w = dict(minitorch=minitorch, hip=hip, lm=lm, prompts=prompts, torch=torch,
             greedy=lm.generate(prompts, NEW), sampled=lm.generate(prompts, NEW, **SAMPLE),
             long=lm.generate(prompts, LONG))
    yield w
    # the model's graphs go here and now, not whenever the collector next runs (which may be
    # inside another module's stream capture)
    w.clear()
    del lm
    gc.collect()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_ids_and_stats_equal_plain(world, k, graph):
    lm, prompts = world["lm"], world["prompts"]
    want = expect(world["greedy"], prompts, k, 3, NEW)
    assert want["accepted"] > 0, "no draft is ever accepted: choose other prompts"
    assert lm.generate(prompts, NEW, speculate=k, graph=graph) == world["greedy"]
    assert lm.spec_stats == want
    assert want["tokens"] == 3 * NEW
    assert lm.generate(prompts, NEW, speculate=k, graph=graph, **SAMPLE) == world["sampled"]
    assert lm.spec_stats == expect(world["sampled"], prompts, k, 3, NEW)
    # another n-gram length drafts otherwise and returns the same ids
    assert lm.generate(prompts, NEW, speculate=k, ngram=1, graph=graph, sync_every=1) == world["greedy"]
    assert lm.spec_stats == expect(world["greedy"], prompts, k, 1, NEW)


def test_long_run_accepts_in_every_row(world):
    lm, prompts, long = world["lm"], world["prompts"], world["long"]
    rows = [simulate(row, p, 4, 3, LONG) for row, p in zip(long, prompts)]
    assert sum(r["accepted"] > 0 for r in rows) >= 2
    assert lm.generate(prompts, LONG, speculate=4, graph=True) == long
    assert lm.spec_stats == totals(rows)
    assert lm.generate(prompts, LONG, speculate=4) == long
    assert lm.spec_stats == totals(rows)


def test_explicit_drafts_accept_exactly_j(world):
    """The true greedy continuation corrupted at draft j, fed through the model's cached path and
    spec_accept: j drafts are accepted, greedy's next j + 1 tokens emitted, the cache's device
    length is held - 1, and a plain one-token step from there yields greedy's next id."""
    mt, hip, lm, prompts, greedy, torch = (world[n] for n in ("minitorch", "hip", "lm", "prompts", "greedy", "torch"))
    B, k, m = len(prompts), 3, 4  # m tokens emitted so far
    n = k + 1
    lens = np.array([len(p) for p in prompts])
    rows = [p + g[:m] for p, g in zip(prompts, greedy)]  # what each row holds; the cache lacks the last
    T = int(lens.max()) + m - 1
    idx = np.zeros((B, T), dtype=np.float32)
    for b, r in enumerate(rows):
        idx[b, :len(r) - 1] = r[:-1]
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device="cuda")  # noqa: E731
    for j in range(n):
        cache = lm.new_cache(B)
        lm(mt.tensor_from_numpy(idx, backend=hip), kv_len=(lens + m - 1).astype(np.float32), cache=cache)
        feed = np.array([g[m - 1:m + k] for g in greedy])
        if j < k:
            feed[:, 1 + j] = (feed[:, 1 + j] + 1) % KW["n_vocab"]
        logits = lm(mt.tensor_from_numpy(feed.astype(np.float32), backend=hip), cache=cache)
        cache.set_length(lens + m - 1)  # the forward counted all k + 1 rows: spec_accept decides how many stay
        tokens = torch.zeros((B, KW["n_positions"] + 1), dtype=torch.int32, device="cuda")
        for b, r in enumerate(rows):
            tokens[b, :len(r)] = i32(r)
        history = torch.zeros((B, KW["n_positions"]), dtype=torch.int32, device="cuda")
        count, held, limit, done = i32([m] * B), i32(lens + m), i32([NEW] * B), i32([0] * B)
        drafted, accepted = i32([0] * B), i32([0] * B)
        hip.spec_accept(logits, i32(feed), i32([k] * B), limit, count, held, done, tokens, history,
                        cache_len=cache.length, drafted=drafted, accepted=accepted)
        assert accepted.cpu().tolist() == [j] * B and drafted.cpu().tolist() == [k] * B
        assert count.cpu().tolist() == [m + j + 1] * B and done.cpu().tolist() == [0] * B
        assert history[:, m:m + j + 2].cpu().tolist() == [g[m:m + j + 1] + [0] for g in greedy]
        for b, r in enumerate(rows):
            assert tokens[b, :len(r) + j + 2].cpu().tolist() == r + greedy[b][m:m + j + 1] + [0]
        assert cache.length.cpu().tolist() == (held.cpu() - 1).tolist() == (lens + m + j).tolist()
        # the rejected rows are simply overwritten: a plain step continues greedy
        cache.set_length(cache.length.cpu().numpy())
        last = np.array([[g[m + j]] for g in greedy], dtype=np.float32)
        nxt = lm(mt.tensor_from_numpy(last, backend=hip), cache=cache).to_numpy()[:, 0].argmax(-1)
        assert nxt.tolist() == [g[m + j + 1] for g in greedy], j


def _eos_of(rows):
    """A token that stops one row (not at its first step) and spares another, as
    test_generate_graph_gpu.py::test_greedy_eos_stops_one_row picks it."""
    for tok in sorted({t for row in rows for t in row[1:]}):
        cut = [row.index(tok) if tok in row else None for row in rows]
        if any(c is not None and c >= 1 for c in cut) and any(c is None for c in cut):
            return tok
    raise AssertionError("no token stops one row and spares another: choose other seeds")


def _eos_in_run(rows, prompts, k, max_new):
    """A token whose first occurrence in some row is chosen inside an accepted run: in the step
    that chooses it at least one draft before it was accepted."""
    for tok in sorted({t for row in rows for t in row[1:]}):
        for row, p in zip(rows, prompts):
            if tok in row and row.index(tok) >= 1:
                last = simulate(row[:row.index(tok)], p, k, 3, max_new, tok)["per_step"][-1]
                if last[2] >= 2:
                    return tok
    raise AssertionError("no eos falls inside an accepted run: choose other seeds")


def test_eos_stops_one_row(world):
    lm, prompts, greedy, long = world["lm"], world["prompts"], world["greedy"], world["long"]
    eos = _eos_of(greedy)
    want = [row[:row.index(eos)] if eos in row else row for row in greedy]
    assert any(len(w) < NEW for w in want) and any(len(w) == NEW for w in want)
    for graph, sync_every in ((False, 8), (True, 1), (True, 1000)):
        assert lm.generate(prompts, NEW, eos_id=eos, speculate=4, graph=graph, sync_every=sync_every) == want
        assert lm.spec_stats == expect(want, prompts, 4, 3, NEW, eos)
    # an eos chosen inside an accepted run
    eos = _eos_in_run(long, prompts, 4, LONG)
    want = [row[:row.index(eos)] if eos in row else row for row in long]
    for graph in (False, True):
        assert lm.generate(prompts, LONG, eos_id=eos, speculate=4, graph=graph) == want
        assert lm.spec_stats == expect(want, prompts, 4, 3, LONG, eos)
    # sampled, with an eos
    eos = _eos_of(world["sampled"])
    want = [row[:row.index(eos)] if eos in row else row for row in world["sampled"]]
    assert lm.generate(prompts, NEW, eos_id=eos, speculate=7, graph=True, **SAMPLE) == want
    assert lm.spec_stats == expect(want, prompts, 7, 3, NEW, eos)


def test_fills_n_positions(world):
    """A full row (44 + 5 tokens) beside a short one that runs on: no emitted token sits past the
    last position, the finished row's discarded slots fit the cache."""
    lm = world["lm"]
    prompts = make_prompts(1, (44, 5))
    plain = lm.generate(prompts, 12)
    assert [len(t) for t in plain] == [KW["n_positions"] + 1 - 44, 12]
    every = lm.generate(prompts, 100)  # more tokens than any row can hold
    assert [len(t) for t in every] == [5, 44]
    for k in (4, 7):
        for graph in (False, True):
            assert lm.generate(prompts, 12, speculate=k, graph=graph) == plain
            assert lm.spec_stats == expect(plain, prompts, k, 3, 12)
            assert lm.generate(prompts, 100, speculate=k, graph=graph) == every
            assert lm.spec_stats == expect(every, prompts, k, 3, 100)
    # a prompt that fills the model: one token, from the prefill
    full = make_prompts(2, (48, 6))
    assert lm.generate(full, 5, speculate=4, graph=True) == lm.generate(full, 5)


def test_few_new_tokens(world):
    lm, prompts, greedy = world["lm"], world["prompts"], world["greedy"]
    for graph in (False, True):
        assert lm.generate(prompts, 0, speculate=4, graph=graph) == [[], [], []]
        assert lm.spec_stats == dict(steps=0, tokens=0, drafted=0, accepted=0)
        for new in (1, 2):
            assert lm.generate(prompts, new, speculate=4, graph=graph) == [g[:new] for g in greedy]
            assert lm.spec_stats == expect([g[:new] for g in greedy], prompts, 4, 3, new)


@pytest.mark.parametrize("mode", [dict(kv_dtype="bf16"), dict(kv_dtype="fp8"), dict(page_size=16),
                                  dict(pos_encoding="rope"), dict(n_kv_head=2), dict(prefill_chunk=8)],
                         ids=lambda m: "-".join(f"{a}={b}" for a, b in m.items()))
def test_every_mode_against_its_own_plain_ids(world, mode):
    mt, hip, prompts = world["minitorch"], world["hip"], world["prompts"]
    lm, kw = world["lm"], mode
    if "pos_encoding" in mode or "n_kv_head" in mode:  # a model of its own, dropped with its graphs below
        np.random.seed(0)
        lm, kw = mt.DecoderLM(backend=hip, **KW, **mode), {}
        lm.eval()
    try:
        plain = lm.generate(prompts, LONG, **kw)
        want = expect(plain, prompts, 4, 3, LONG)
        assert want["accepted"] > 0
        for graph in (False, True):
            assert lm.generate(prompts, LONG, speculate=4, graph=graph, **kw) == plain, graph
            assert lm.spec_stats == want
        sampled = lm.generate(prompts, NEW, **kw, **SAMPLE)
        assert lm.generate(prompts, NEW, speculate=7, graph=True, **kw, **SAMPLE) == sampled
        assert lm.spec_stats == expect(sampled, prompts, 7, 3, NEW)
    finally:
        if lm is not world["lm"]:
            lm.drop_decode_graphs()


def test_graph_reuse(world):
    lm, prompts, greedy = world["lm"], world["prompts"], world["greedy"]
    assert lm.generate(prompts, NEW, graph=True) == greedy
    assert lm.generate(prompts, NEW, speculate=4, ngram=2, graph=True) == greedy
    n = lm.graph_captures
    assert lm.generate(prompts, NEW, speculate=4, ngram=2, graph=True) == greedy
    assert lm.generate(prompts, 9, speculate=4, ngram=2, graph=True) == [g[:9] for g in greedy]
    assert lm.graph_captures == n, "the same call must replay the kept graph"
    # speculate=None afterwards: the plain graph is still in its slot
    assert lm.generate(prompts, NEW, graph=True) == greedy
    assert lm.generate(prompts, NEW, speculate=0, graph=True) == greedy
    assert lm.graph_captures == n
    # k and ngram are part of the key
    assert lm.generate(prompts, NEW, speculate=4, ngram=1, graph=True) == greedy
    assert lm.graph_captures == n + 1
    assert lm.generate(prompts, NEW, speculate=2, ngram=2, graph=True) == greedy
    assert lm.graph_captures == n + 2
    # the eager speculative call keeps nothing on the model
    kept = len(lm._decode_graphs)
    assert lm.generate(prompts, NEW, speculate=5) == greedy
    assert len(lm._decode_graphs) == kept and lm.graph_captures == n + 2


def test_misuse_raises_before_any_launch(world):
    lm, prompts = world["lm"], world["prompts"]
    n = lm.graph_captures
    with pytest.raises(ValueError, match="use_cache"):
        lm.generate(prompts, 4, speculate=2, use_cache=False)
    for bad in (8, -1, 1.5):
        with pytest.raises(ValueError, match="speculate must be"):
            lm.generate(prompts, 4, speculate=bad)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="ngram must be"):
            lm.generate(prompts, 4, speculate=2, ngram=bad)
    with pytest.raises(ValueError, match="temperature"):
        lm.generate(prompts, 4, speculate=2, temperature=-1.0)
    assert lm.graph_captures == n
