"""DecoderLM generation through the KV cache on the HIP backend, against the same model on the
CPU test backend (tests/cpu_backend.py: NumPy ops, the CPU oracle for the attention).

* Teacher-forced logits: prefill the prompts, then feed the CPU model's own greedy tokens
  through the cache one at a time (and in chunks of 3); every step's logits are held to the CPU
  model's full-forward logits at that position, within the larger of 1e-5 max|logits| and twice
  the deviation the full HIP forward (no cache: the training path) shows from the CPU model on
  the same sequences -- the yardstick is that existing path, not the new code.
* Tokens: generate(use_cache=True) == generate(use_cache=False) == the CPU model's greedy tokens,
  id for id, every step.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    _hip.lib()
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    cpu = minitorch.TensorBackend(NumpyOps)
    np.random.seed(0)
    lm_h = minitorch.DecoderLM(backend=hip, **KW)
    lm_c = minitorch.DecoderLM(backend=cpu, **KW)
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    assert ph.keys() == pc.keys()
    for name, p in ph.items():
        pc[name].update(minitorch.tensor_from_numpy(p.value.to_numpy().copy(), cpu))
    lm_h.eval()
    lm_c.eval()
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    # the CPU model's greedy continuation and its full-forward logits over prompt + continuation
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
    # the smallest top-2 gap of the logits that decide a token: a flipped argmax is an error, not a tie
    gap = min(float(np.diff(np.sort(x[len(p) - 1:len(p) - 1 + NEW], axis=-1)[:, -2:], axis=-1).min())
              for x, p in zip(cpu_logits, prompts))
    print(f"max|logit| {scale:.3f}; full HIP forward vs CPU {dev:.3e}; tolerance {tol:.3e}; "
          f"smallest top-2 gap {gap:.3e} = {gap / scale:.2e} of max|logit|")
    assert gap > 10 * tol, "the seeds give a near-tie: choose others"
    return dict(minitorch=minitorch, hip=hip, cpu=cpu, lm_h=lm_h, lm_c=lm_c, prompts=prompts, cpu_new=cpu_new,
                cpu_logits=cpu_logits, tol=tol, scale=scale)


def _padded(prompts):
    lens = np.array([len(p) for p in prompts])
    idx = np.zeros((len(prompts), int(lens.max())), np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    return idx, lens


@pytest.mark.parametrize("chunk", [1, 3])
def test_teacher_forced_logits_through_the_cache(world, chunk, parity_record):
    mt, hip, lm = world["minitorch"], world["hip"], world["lm_h"]
    prompts, cpu_new, ref, tol = world["prompts"], world["cpu_new"], world["cpu_logits"], world["tol"]
    B = len(prompts)
    idx, lens = _padded(prompts)
    cache = lm.new_cache(B)
    assert cache.empty
    worst = 0.0
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache).to_numpy()
    assert list(cache.length_host) == list(lens)
    for b in range(B):  # every prompt position of every row, not only the last
        worst = max(worst, float(np.abs(logits[b, :lens[b]] - ref[b][:lens[b]]).max()))
    s = 0
    while s < NEW:
        T = min(chunk, NEW - s)
        step = np.array([t[s:s + T] for t in cpu_new], np.float32)
        logits = lm(mt.tensor_from_numpy(step, hip), cache=cache).to_numpy()
        assert logits.shape == (B, T, KW["n_vocab"])
        for b in range(B):
            worst = max(worst, float(np.abs(logits[b] - ref[b][lens[b] + s:lens[b] + s + T]).max()))
        s += T
    assert list(cache.length_host) == list(lens + NEW)
    assert list(cache.length.cpu().numpy()) == list(lens + NEW)
    print(f"chunk {chunk}: worst |dlogit| {worst:.3e}, tolerance {tol:.3e}")
    parity_record("test_teacher_forced_logits_through_the_cache", f"chunk={chunk}", max_abs=worst, bound=tol)
    assert worst <= tol
    cache.reset()
    assert cache.empty and not cache.length.any()


def test_generate_tokens_match(world):
    lm, prompts, cpu_new = world["lm_h"], world["prompts"], world["cpu_new"]
    plain = lm.generate(prompts, NEW, use_cache=False)
    cached = lm.generate(prompts, NEW, use_cache=True)
    assert plain == cpu_new
    assert cached == cpu_new
    assert not lm.training
    lm.train()
    assert lm.generate(prompts[:1], 2) == [cpu_new[0][:2]] and lm.training, "generate restores train()"
    lm.eval()


def test_generate_fills_n_positions(world):
    """A row stops once it holds more than n_positions tokens; both legs agree up to there, with
    a short row still running beside a full one."""
    lm = world["lm_h"]
    rng = np.random.default_rng(1)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (44, 5)]
    plain = lm.generate(prompts, 12, use_cache=False)
    cached = lm.generate(prompts, 12, use_cache=True)
    assert [len(t) for t in plain] == [KW["n_positions"] + 1 - 44, 12]
    assert cached == plain


def test_eos_stops_one_row(world):
    lm, prompts, cpu_new = world["lm_h"], world["prompts"], world["cpu_new"]
    eos = None
    for tok in sorted({t for row in cpu_new for t in row[1:]}):
        cut = [row.index(tok) if tok in row else None for row in cpu_new]
        if any(c is not None and c >= 1 for c in cut) and any(c is None for c in cut):
            eos = tok
            break
    assert eos is not None, "no token stops one row and spares another: choose other seeds"
    want = [row[:row.index(eos)] if eos in row else row for row in cpu_new]
    assert any(len(w) < NEW for w in want) and any(len(w) == NEW for w in want)
    assert lm.generate(prompts, NEW, eos_id=eos, use_cache=True) == want
    assert lm.generate(prompts, NEW, eos_id=eos, use_cache=False) == want


def test_misuse_raises(world):
    mt, hip, lm = world["minitorch"], world["hip"], world["lm_h"]
    prompts = world["prompts"]
    idx, lens = _padded(prompts)
    # a cache on a model without flash attention
    kw = dict(KW, use_flash_attention=False)
    plain = mt.DecoderLM(backend=hip, **kw)
    cache = mt.KVCache(4, len(prompts), KW["n_head"], KW["n_positions"], KW["n_embd"] // KW["n_head"], hip)
    with pytest.raises(ValueError, match="use_flash_attention"):
        plain(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache)
    # a decode step of 9 tokens
    lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache)
    with pytest.raises(ValueError, match="at most 8"):
        lm(mt.tensor_from_numpy(np.zeros((len(prompts), 9), np.float32), hip), cache=cache)
    assert list(cache.length_host) == list(lens), "a refused step must not advance the cache"
    # a prompt longer than n_positions
    with pytest.raises(ValueError, match="n_positions"):
        lm.generate([[1] * (KW["n_positions"] + 1)], 4)
    with pytest.raises(ValueError, match="n_positions"):
        lm.generate([[1] * (KW["n_positions"] + 1)], 4, use_cache=False)
    # a head dim the kernel declines, and a backend without the kernels
    with pytest.raises(ValueError, match="head_dim"):
        mt.KVCache(1, 1, 1, 8, 6, hip)
    with pytest.raises(ValueError, match="backend"):
        mt.KVCache(1, 1, 1, 8, 16, world["cpu"])
