"""Extend steps through KVCache, MultiHeadAttention and DecoderLM on the HIP backend (a filled
cache and kv_len: a right-padded batch of any number of new tokens per row), and
generate(prefill_chunk=...), against the same model on the CPU test backend.

The models and the tolerance rule are those of tests/test_generate_gpu.py: n_positions = 48, and
every real position's logits within the larger of 1e-5 max|logit| and twice the deviation the full
HIP forward (no cache) shows from the CPU model on the same sequences; the smallest top-2 gap of
the deciding logits is at least 10x that tolerance, so a flipped argmax is an error, not a tie.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16
FIRST = 5  # tokens of every row that go in as the prefill


def _world(n_kv_head):
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    _hip.lib()
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    cpu = minitorch.TensorBackend(NumpyOps)
    kw = dict(KW) if n_kv_head is None else dict(KW, n_kv_head=n_kv_head)
    np.random.seed(0)
    lm_h = minitorch.DecoderLM(backend=hip, **kw)
    lm_c = minitorch.DecoderLM(backend=cpu, **kw)
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    assert ph.keys() == pc.keys()
    for name, p in ph.items():
        pc[name].update(minitorch.tensor_from_numpy(p.value.to_numpy().copy(), cpu))
    lm_h.eval()
    lm_c.eval()
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    cpu_new = lm_c.generate(prompts, NEW, use_cache=False)
    assert all(len(t) == NEW for t in cpu_new)
    full = [p + t for p, t in zip(prompts, cpu_new)]

    def forward(lm, backend, seq):
        idx = minitorch.tensor_from_numpy(np.asarray([seq], dtype=np.float32), backend)
        return lm(idx).to_numpy()[0]
    cpu_logits = [forward(lm_c, cpu, s) for s in full]
    hip_logits = [forward(lm_h, hip, s) for s in full]
    scale = max(float(np.abs(x).max()) for x in cpu_logits)
    dev = max(float(np.abs(a - b).max()) for a, b in zip(hip_logits, cpu_logits))
    tol = max(1e-5 * scale, 2.0 * dev)
    gap = min(float(np.diff(np.sort(x[len(p) - 1:len(p) - 1 + NEW], axis=-1)[:, -2:], axis=-1).min())
              for x, p in zip(cpu_logits, prompts))
    print(f"n_kv_head {n_kv_head}: max|logit| {scale:.3f}; full HIP forward vs CPU {dev:.3e}; tolerance {tol:.3e}; "
          f"smallest top-2 gap {gap:.3e}")
    assert gap > 10 * tol, "the seeds give a near-tie: choose others"
    return dict(minitorch=minitorch, hip=hip, cpu=cpu, lm_h=lm_h, lm_c=lm_c, prompts=prompts, cpu_new=cpu_new,
                full=full, cpu_logits=cpu_logits, tol=tol)


@pytest.fixture(scope="module")
def world():
    return _world(None)


@pytest.fixture(scope="module")
def world_gqa():
    return _world(2)


def _teacher_forced(w, pattern, parity_record, case):
    """Prefill the first FIRST tokens of every row, then feed the rest of prompt + continuation in
    extend steps: row b of step k gets pattern[(b + k) % len(pattern)] tokens (fewer at its end)."""
    mt, hip, lm = w["minitorch"], w["hip"], w["lm_h"]
    full, ref, tol = w["full"], w["cpu_logits"], w["tol"]
    B = len(full)
    total = np.array([len(s) for s in full])
    cache = lm.new_cache(B)
    idx = np.array([s[:FIRST] for s in full], np.float32)
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=np.full(B, FIRST, np.float32), cache=cache).to_numpy()
    worst = max(float(np.abs(logits[b] - ref[b][:FIRST]).max()) for b in range(B))
    fed = np.full(B, FIRST)
    k = 0
    widest = 0
    while (fed < total).any():
        cnt = np.minimum(np.array([pattern[(b + k) % len(pattern)] for b in range(B)]), total - fed)
        k += 1
        T = max(int(cnt.max()), 1)
        widest = max(widest, T)
        step = np.zeros((B, T), np.float32)
        for b in range(B):
            step[b, :cnt[b]] = full[b][fed[b]:fed[b] + cnt[b]]
        logits = lm(mt.tensor_from_numpy(step, hip), kv_len=cnt.astype(np.float32), cache=cache).to_numpy()
        assert logits.shape == (B, T, KW["n_vocab"])
        assert np.isfinite(logits).all(), "logits at padding slots must be finite"
        for b in range(B):
            if cnt[b]:
                worst = max(worst, float(np.abs(logits[b, :cnt[b]] - ref[b][fed[b]:fed[b] + cnt[b]]).max()))
        fed = fed + cnt
        assert list(cache.length_host) == list(fed)
        assert list(cache.length.cpu().numpy()) == list(fed)
        assert k < 64
    assert widest > 8, "no step was wider than a decode step"
    assert list(fed) == list(total)
    print(f"{case}: worst |dlogit| {worst:.3e}, tolerance {tol:.3e}, {k} extend steps, widest {widest}")
    parity_record("test_extend_teacher_forced", case, max_abs=worst, bound=tol)
    assert worst <= tol


@pytest.mark.parametrize("pattern", [(9,), (16,), (9, 0, 13)], ids=["9", "16", "ragged-9-0-13"])
def test_teacher_forced_logits_through_extend_steps(world, pattern, parity_record):
    _teacher_forced(world, pattern, parity_record, f"steps of {pattern}")


def test_teacher_forced_logits_grouped_query(world_gqa, parity_record):
    assert world_gqa["lm_h"].n_kv_head == 2
    _teacher_forced(world_gqa, (9, 0, 13), parity_record, "n_kv_head=2, steps of (9, 0, 13)")


def test_generate_with_chunked_prefill(world):
    lm, prompts, cpu_new = world["lm_h"], world["prompts"], world["cpu_new"]
    assert lm.generate(prompts, NEW) == cpu_new
    assert lm.generate(prompts, NEW, use_cache=False) == cpu_new
    assert lm.generate(prompts, NEW, graph=True) == cpu_new
    captures = lm.graph_captures
    assert captures >= 1
    for chunk in (4, 9):
        assert lm.generate(prompts, NEW, prefill_chunk=chunk) == cpu_new, f"eager, prefill_chunk={chunk}"
        assert lm.generate(prompts, NEW, prefill_chunk=chunk, graph=True) == cpu_new, f"graph, prefill_chunk={chunk}"
    assert lm.graph_captures == captures, "chunking the prefill must not re-capture the decode step"
    # a sampled draw depends on (seed, b) alone: the chunked prefill draws what the one-shot prefill draws
    kw = dict(temperature=0.9, top_k=20, seed=77)
    want = lm.generate(prompts, NEW, **kw)
    assert lm.generate(prompts, NEW, prefill_chunk=4, **kw) == want
    assert lm.generate(prompts, NEW, prefill_chunk=9, graph=True, **kw) == want
    lm.drop_decode_graphs()


def test_misuse_raises(world):
    mt, hip, lm = world["minitorch"], world["hip"], world["lm_h"]
    prompts = world["prompts"]
    B = len(prompts)
    with pytest.raises(ValueError, match="use_cache"):
        lm.generate(prompts, 4, use_cache=False, prefill_chunk=4)
    with pytest.raises(ValueError, match="prefill_chunk"):
        lm.generate(prompts, 4, prefill_chunk=0)
    cache = lm.new_cache(B)
    held = np.array([40, 3, 3])
    idx = np.zeros((B, 40), np.float32)
    lm(mt.tensor_from_numpy(idx, hip), kv_len=held.astype(np.float32), cache=cache)
    assert list(cache.length_host) == list(held)
    step = mt.tensor_from_numpy(np.zeros((B, 9), np.float32), hip)
    # row 0 would hold 49 > n_positions = 48 tokens
    with pytest.raises(ValueError, match="n_positions"):
        lm(step, kv_len=np.array([9, 1, 1], np.float32), cache=cache)
    # a count above the step's width, a negative one, a fractional one
    for bad in ([1, 10, 1], [1, -1, 1], [1, 1.5, 1]):
        with pytest.raises(ValueError, match="kv_len"):
            lm(step, kv_len=np.array(bad, np.float32), cache=cache)
    assert list(cache.length_host) == list(held) and list(cache.length.cpu().numpy()) == list(held), \
        "a refused step must not advance the cache"
    # the same step within the limits goes through: row 0 fills its last 8 positions
    out = lm(step, kv_len=np.array([8, 9, 0], np.float32), cache=cache).to_numpy()
    assert np.isfinite(out).all()
    assert list(cache.length_host) == [48, 12, 3]
    # without kv_len a 9-token step on a filled cache is still refused
    with pytest.raises(ValueError, match="at most 8"):
        lm(step, cache=cache)
