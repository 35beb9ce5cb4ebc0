"""DecoderLM.generate with tokens chosen on the device: the graph-replayed decode step against
the cached-eager and uncached legs (greedy: id for id; sampling: graph == cached-eager bit for
bit, the same kernels in the same order), reproducibility from the seed, independence of
sync_every, and the reuse / re-capture of the graph kept on the model.

The model is test_generate_gpu.py's (n_vocab 97, n_embd 64, 4 heads, 48 positions, no dropout,
prompts of 3 / 9 / 14 tokens)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16
SAMPLE = dict(temperature=0.8, top_k=5, seed=1234)


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
    # computed once, shared: the greedy and the sampled continuation of the eager legs
    greedy = lm.generate(prompts, NEW, use_cache=False)
    sampled = lm.generate(prompts, NEW, **SAMPLE)
    w = dict(minitorch=minitorch, hip=hip, lm=lm, prompts=prompts, greedy=greedy, sampled=sampled)
    yield w
    # the model's graphs go here and now, not whenever the collector next runs (which may be
    # inside another module's stream capture)
    import gc
    w.clear()
    del lm
    gc.collect()


def test_greedy_three_legs_agree(world):
    lm, prompts, greedy = world["lm"], world["prompts"], world["greedy"]
    assert all(len(t) == NEW for t in greedy)
    assert lm.generate(prompts, NEW, use_cache=True) == greedy
    assert lm.generate(prompts, NEW, graph=True) == greedy
    assert lm.graph_captures >= 1
    assert not lm.training
    lm.train()
    assert lm.generate(prompts[:1], 2, graph=True) == [greedy[0][:2]] and lm.training, "generate restores train()"
    lm.eval()


def test_greedy_fills_n_positions(world):
    """A full row (44 + 5 tokens) beside a short one that runs on: the device clamp of the cache
    lengths does what the host loop does."""
    lm = world["lm"]
    rng = np.random.default_rng(1)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (44, 5)]
    plain = lm.generate(prompts, 12, use_cache=False)
    assert [len(t) for t in plain] == [KW["n_positions"] + 1 - 44, 12]
    assert lm.generate(prompts, 12, use_cache=True) == plain
    assert lm.generate(prompts, 12, graph=True) == plain
    assert lm.generate(prompts, 12, graph=True, sync_every=1) == plain
    # more tokens than any row can hold
    assert lm.generate(prompts, 100, graph=True) == lm.generate(prompts, 100, use_cache=True)


def _eos_of(rows):
    """A token that stops one row (not at its first step) and spares another, as
    test_generate_gpu.py::test_eos_stops_one_row picks it."""
    for tok in sorted({t for row in rows for t in row[1:]}):
        cut = [row.index(tok) if tok in row else None for row in rows]
        if any(c is not None and c >= 1 for c in cut) and any(c is None for c in cut):
            return tok
    raise AssertionError("no token stops one row and spares another: choose other seeds")


def test_greedy_eos_stops_one_row(world):
    lm, prompts, greedy = world["lm"], world["prompts"], world["greedy"]
    eos = _eos_of(greedy)
    want = [row[:row.index(eos)] if eos in row else row for row in greedy]
    assert any(len(w) < NEW for w in want) and any(len(w) == NEW for w in want)
    assert lm.generate(prompts, NEW, eos_id=eos, use_cache=False) == want
    assert lm.generate(prompts, NEW, eos_id=eos, use_cache=True) == want
    for sync_every in (1, 8, 1000):
        assert lm.generate(prompts, NEW, eos_id=eos, graph=True, sync_every=sync_every) == want, sync_every
    # an eos met at the third step of row 0 (and wherever else it falls)
    first = greedy[0][2]
    every = [row[:row.index(first)] if first in row else row for row in greedy]
    assert lm.generate(prompts, NEW, eos_id=first, graph=True, sync_every=1) == every
    assert lm.generate(prompts, NEW, eos_id=first, use_cache=True) == every


def test_sampling_graph_equals_cached_eager(world):
    lm, prompts, sampled = world["lm"], world["prompts"], world["sampled"]
    assert all(len(t) == NEW for t in sampled)
    assert all(0 <= t < KW["n_vocab"] for row in sampled for t in row)
    assert sampled != world["greedy"], "the sampled tokens are the greedy ones: nothing was shown"
    assert lm.generate(prompts, NEW, graph=True, **SAMPLE) == sampled
    # the same seed twice, and another seed
    assert lm.generate(prompts, NEW, **SAMPLE) == sampled
    assert lm.generate(prompts, NEW, graph=True, **SAMPLE) == sampled
    other = dict(SAMPLE, seed=4321)
    again = lm.generate(prompts, NEW, graph=True, **other)
    assert again != sampled
    assert lm.generate(prompts, NEW, **other) == again
    # seed=None draws from NumPy's global generator
    np.random.seed(7)
    a = lm.generate(prompts, NEW, temperature=0.8, top_k=5, graph=True)
    np.random.seed(7)
    assert lm.generate(prompts, NEW, temperature=0.8, top_k=5) == a
    # the uncached leg samples too (each prompt as row 0 of its own batch), reproducibly
    one = lm.generate(prompts[:1], NEW, use_cache=False, **SAMPLE)
    assert one == lm.generate(prompts[:1], NEW, use_cache=False, **SAMPLE)
    assert len(one[0]) == NEW


def test_sampling_with_eos_and_sync_every(world):
    lm, prompts, sampled = world["lm"], world["prompts"], world["sampled"]
    eos = _eos_of(sampled)
    want = [row[:row.index(eos)] if eos in row else row for row in sampled]
    assert lm.generate(prompts, NEW, eos_id=eos, **SAMPLE) == want
    assert lm.generate(prompts, NEW, eos_id=eos, graph=True, sync_every=1, **SAMPLE) == want
    assert lm.generate(prompts, NEW, eos_id=eos, graph=True, sync_every=1000, **SAMPLE) == want


def test_graph_reuse_and_recapture(world):
    mt, hip, lm, prompts = world["minitorch"], world["hip"], world["lm"], world["prompts"]
    want = lm.generate(prompts, NEW, graph=True, **SAMPLE)
    greedy = lm.generate(prompts, NEW, graph=True)
    n = lm.graph_captures
    # the sampled and the greedy graph of one batch size are kept side by side
    assert lm.generate(prompts, NEW, graph=True, **SAMPLE) == want
    assert lm.generate(prompts, NEW, graph=True) == greedy == world["greedy"]
    assert lm.generate(prompts, 5, graph=True, **dict(SAMPLE, seed=5)) == lm.generate(prompts, 5, **dict(SAMPLE, seed=5))
    assert lm.graph_captures == n, "the same batch size and arguments must replay the kept graph"
    # a different batch size gets its own graph, and the first one is kept
    two = lm.generate(prompts[:2], NEW, graph=True, **SAMPLE)
    assert lm.graph_captures == n + 1
    assert two == lm.generate(prompts[:2], NEW, **SAMPLE)
    assert lm.generate(prompts, NEW, graph=True, **SAMPLE) == want
    assert lm.graph_captures == n + 1
    # Parameter.update swaps a weight's storage: re-capture, and the new weights are used
    p = dict(lm.named_parameters())["lm_head.weights"]
    old = p.value.to_numpy().copy()
    rng = np.random.default_rng(3)
    try:
        p.update(mt.tensor_from_numpy((old + 0.5 * rng.standard_normal(old.shape)).astype(np.float32), hip))
        eager = lm.generate(prompts, NEW, **SAMPLE)
        assert eager != want, "the new weights changed nothing: nothing was shown"
        assert lm.generate(prompts, NEW, graph=True, **SAMPLE) == eager
        assert lm.graph_captures == n + 2
    finally:
        p.update(mt.tensor_from_numpy(old, hip))
    assert lm.generate(prompts, NEW, graph=True, **SAMPLE) == want


def test_greedy_graph_leaves_numpy_rng_alone(world):
    lm, prompts = world["lm"], world["prompts"]
    np.random.seed(11)
    before = np.random.get_state()[1].copy()
    assert lm.generate(prompts, 4, graph=True) == [g[:4] for g in world["greedy"]]
    assert (np.random.get_state()[1] == before).all(), "a greedy call drew from NumPy's generator"


def test_kept_batch_sizes_are_capped_and_droppable(world):
    mt, hip = world["minitorch"], world["hip"]
    np.random.seed(2)
    lm = mt.DecoderLM(backend=hip, **KW)
    cap = lm.MAX_DECODE_BATCH_SIZES
    for B in range(1, cap + 2):
        assert len(lm.generate([[1, 2, 3]] * B, 3, graph=True)) == B
    assert sorted(lm._decode_graphs) == list(range(2, cap + 2)), "the least recently used batch size goes"
    n = lm.graph_captures
    want = lm.generate([[1, 2, 3]] * 2, 3, graph=True)
    assert lm.graph_captures == n
    lm.drop_decode_graphs()
    assert not lm._decode_graphs
    assert lm.generate([[1, 2, 3]] * 2, 3, graph=True) == want
    assert lm.graph_captures == n + 1


def test_graphs_die_with_the_model(world):
    """The captured graphs are freed by reference count when the model goes: left to the cyclic
    collector they could be destroyed inside a later, unrelated stream capture."""
    import gc
    import weakref
    mt, hip, prompts = world["minitorch"], world["hip"], world["prompts"]
    np.random.seed(1)
    lm = mt.DecoderLM(backend=hip, **KW)
    assert len(lm.generate(prompts[:2], 4, graph=True)) == 2
    assert lm.graph_captures == 1
    step_graph = next(iter(lm._decode_graphs[2]["graphs"].values()))[0]
    dead = weakref.ref(step_graph)
    del step_graph
    was = gc.isenabled()
    gc.disable()
    try:
        del lm
        assert dead() is None, "the model and its graph are in a reference cycle"
    finally:
        if was:
            gc.enable()


def test_misuse_raises(world):
    mt, lm, prompts = world["minitorch"], world["lm"], world["prompts"]
    with pytest.raises(ValueError, match="use_cache"):
        lm.generate(prompts, 4, use_cache=False, graph=True)
    from cpu_backend import NumpyOps
    cpu = mt.TensorBackend(NumpyOps)
    lm_c = mt.DecoderLM(backend=cpu, **KW)
    with pytest.raises(ValueError, match="select_token"):
        lm_c.generate(prompts, 4, graph=True)
    with pytest.raises(ValueError, match="select_token"):
        lm_c.generate(prompts, 4, use_cache=False, temperature=0.5)
    with pytest.raises(ValueError, match="temperature"):
        lm.generate(prompts, 4, temperature=-1.0)
    assert lm.generate(prompts, 0, graph=True) == [[], [], []]
