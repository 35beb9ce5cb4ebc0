"""Grouped-query attention through the modules on the HIP backend: MultiHeadAttention /
TransformerLayer / DecoderLM with n_kv_head < n_head, the smaller KVCache and generation, against
the same model on the CPU test backend (tests/cpu_backend.py), as tests/test_generate_gpu.py does
for n_kv_head = n_head.

* Teacher-forced logits through the cache (chunks of 1 and 3) against the CPU model's full
  forward, within the larger of 1e-5 max|logit| and twice the deviation the full HIP forward (no
  cache: K / V repeated to n_head heads, the existing flash kernel) shows from the CPU model on
  the same sequences: the yardstick is that existing path, not the grouped decode kernel.
* Tokens: generate(use_cache=False) == generate(use_cache=True) == generate(graph=True) == the CPU
  model's greedy tokens, id for id; one sampled call, graph == cached eager.
* Training path: MultiHeadAttention(n_kv_head=2) forward + backward against the n_head = 4 module
  whose K / V weight columns are the grouped module's, repeated per group; both are held to a
  float64 NumPy restatement and the grouped module may deviate twice as far as the tied one.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_kv_head=2, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16
SAMPLE = dict(temperature=0.8, top_k=20, seed=1234)


def _build(n_kv_head, seed):
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    _hip.lib()
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    cpu = minitorch.TensorBackend(NumpyOps)
    kw = dict(KW, n_kv_head=n_kv_head)
    np.random.seed(seed)
    lm_h = minitorch.DecoderLM(backend=hip, **kw)
    lm_c = minitorch.DecoderLM(backend=cpu, **kw)
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    assert ph.keys() == pc.keys()
    for name, p in ph.items():
        pc[name].update(minitorch.tensor_from_numpy(p.value.to_numpy().copy(), cpu))
    lm_h.eval()
    lm_c.eval()
    rng = np.random.default_rng(seed)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    cpu_new = lm_c.generate(prompts, NEW, use_cache=False)
    assert all(len(t) == NEW for t in cpu_new)
    return minitorch, hip, cpu, lm_h, lm_c, prompts, cpu_new


@pytest.fixture(scope="module")
def world():
    minitorch, hip, cpu, lm_h, lm_c, prompts, cpu_new = _build(2, 0)
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


def test_parameter_shapes(world):
    mt, hip, lm = world["minitorch"], world["hip"], world["lm_h"]
    shapes = {n: tuple(p.value.shape) for n, p in lm.named_parameters()}
    for i in range(1, 5):
        for proj, cols in (("q_projection", 64), ("k_projection", 32), ("v_projection", 32), ("out_projection", 64)):
            assert shapes[f"t_layer_{i}.attention.{proj}.weights"] == (64, cols)
            assert shapes[f"t_layer_{i}.attention.{proj}.bias"] == (cols,)
    # n_kv_head unset: today's names and shapes, and no n_kv_head argument needed anywhere
    kw = {k: v for k, v in KW.items() if k != "n_kv_head"}
    unset = {n: tuple(p.value.shape) for n, p in mt.DecoderLM(backend=hip, **kw).named_parameters()}
    same = {n: tuple(p.value.shape) for n, p in mt.DecoderLM(backend=hip, **dict(kw, n_kv_head=4)).named_parameters()}
    assert unset == same and unset.keys() == shapes.keys()
    for n, s in unset.items():
        assert s == ((64, 64) if n.endswith(("k_projection.weights", "v_projection.weights")) else
                     (64,) if n.endswith(("k_projection.bias", "v_projection.bias")) else shapes[n]), n
    cache = lm.new_cache(3)
    assert (cache.n_head, cache.n_kv_head) == (4, 2)
    assert tuple(cache.layer(0).k.shape) == (3, 2, 48, 16) and tuple(cache.layer(3).v.shape) == (3, 2, 48, 16)
    assert mt.KVCache(1, 2, 4, 8, 16, hip).n_kv_head == 4


@pytest.mark.parametrize("chunk", [1, 3])
def test_teacher_forced_logits_through_the_gqa_cache(world, chunk, parity_record):
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
    parity_record("test_teacher_forced_logits_through_the_gqa_cache", f"chunk={chunk}", max_abs=worst, bound=tol)
    assert worst <= tol


def test_generated_tokens_match(world):
    lm, prompts, cpu_new = world["lm_h"], world["prompts"], world["cpu_new"]
    assert lm.generate(prompts, NEW, use_cache=False) == cpu_new
    assert lm.generate(prompts, NEW, use_cache=True) == cpu_new
    assert lm.generate(prompts, NEW, graph=True) == cpu_new
    sampled = lm.generate(prompts, NEW, **SAMPLE)
    assert lm.generate(prompts, NEW, graph=True, **SAMPLE) == sampled
    assert sampled != cpu_new, "the sampled call must not be the greedy one"
    lm.drop_decode_graphs()


def test_multi_query_tokens_match():
    """n_kv_head = 1: every query head reads the one kv head."""
    _mt, _hip, _cpu, lm, _lm_c, prompts, cpu_new = _build(1, 1)
    assert tuple(lm.t_layer_1.attention.k_projection.weights.value.shape) == (64, 16)
    assert lm.generate(prompts, NEW, use_cache=False) == cpu_new
    assert lm.generate(prompts, NEW, use_cache=True) == cpu_new
    assert lm.generate(prompts, NEW, graph=True) == cpu_new
    lm.drop_decode_graphs()


def _mha_f64(x, w, g, H, Hkv):
    """Float64 restatement of causal grouped-query MultiHeadAttention, forward and backward:
    w = (Wq, bq, Wk, bk, Wv, bv, Wo, bo) with Wk / Wv [E, Hkv d]; g = dL/dY. Returns Y and the
    gradients by name; 'k_rep' / 'v_rep' are the per-query-head [E, H d] / [H d] gradients of the
    repeated projections (what a module with n_head K / V heads and tied columns gets)."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    wq, bq, wk, bk, wv, bv, wo, bo = (np.asarray(a, np.float64) for a in w)
    B, T, E = x.shape
    d, G = E // H, H // Hkv
    X = x.reshape(B * T, E)

    def heads(a, n):
        return a.reshape(B, T, n, d).transpose(0, 2, 1, 3)

    def flat(a):
        return a.transpose(0, 2, 1, 3).reshape(B * T, -1)
    q = heads(X @ wq + bq, H)
    k = np.repeat(heads(X @ wk + bk, Hkv), G, axis=1)
    v = np.repeat(heads(X @ wv + bv, Hkv), G, axis=1)
    s = np.einsum("bhqd,bhkd->bhqk", q, k) / np.sqrt(d)
    s = np.where(np.triu(np.ones((T, T), bool), 1), -np.inf, s)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = flat(np.einsum("bhqk,bhkd->bhqd", p, v))
    y = (o @ wo + bo).reshape(B, T, E)
    dy = g.reshape(B * T, E)
    do = heads(dy @ wo.T, H)
    dv = np.einsum("bhqk,bhqd->bhkd", p, do)
    dp = np.einsum("bhqd,bhkd->bhqk", do, v)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True))
    dq = np.einsum("bhqk,bhkd->bhqd", ds, k) / np.sqrt(d)
    dk = np.einsum("bhqk,bhqd->bhkd", ds, q) / np.sqrt(d)
    dqf, dkf, dvf = flat(dq), flat(dk), flat(dv)

    def group_sum(a):  # [.., H d] -> [.., Hkv d]
        return a.reshape(*a.shape[:-1], Hkv, G, d).sum(-2).reshape(*a.shape[:-1], Hkv * d)
    dkg, dvg = group_sum(dkf), group_sum(dvf)
    grads = {"x": (dqf @ wq.T + dkg @ wk.T + dvg @ wv.T).reshape(B, T, E),
             "q_w": X.T @ dqf, "q_b": dqf.sum(0), "o_w": o.T @ dy, "o_b": dy.sum(0),
             "k_w": X.T @ dkg, "k_b": dkg.sum(0), "v_w": X.T @ dvg, "v_b": dvg.sum(0)}
    return y, grads, group_sum


def test_training_path_against_tied_heads(world, parity_record):
    mt, hip = world["minitorch"], world["hip"]
    E, H, Hkv, B, T = 64, 4, 2, 2, 16
    d, G = E // H, H // Hkv
    rng = np.random.default_rng(21)
    shapes = [(E, E), (E,), (E, Hkv * d), (Hkv * d,), (E, Hkv * d), (Hkv * d,), (E, E), (E,)]
    w = [(0.3 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    x_np = rng.standard_normal((B, T, E)).astype(np.float32)
    g_np = rng.standard_normal((B, T, E)).astype(np.float32)

    def repeat_cols(a):  # [.., Hkv d] -> [.., H d], block h = block h // G
        return np.repeat(a.reshape(*a.shape[:-1], Hkv, d), G, axis=-2).reshape(*a.shape[:-1], H * d)
    w_tied = [w[0], w[1], repeat_cols(w[2]), repeat_cols(w[3]), repeat_cols(w[4]), repeat_cols(w[5]), w[6], w[7]]

    def run(n_kv_head, weights):
        mha = mt.MultiHeadAttention(E, H, causal=True, p_dropout=0.0, backend=hip, use_flash_attention=True,
                                    n_kv_head=n_kv_head)
        lin = (mha.q_projection, mha.k_projection, mha.v_projection, mha.out_projection)
        for i, layer in enumerate(lin):
            assert tuple(layer.weights.value.shape) == weights[2 * i].shape
            layer.weights.update(mt.tensor_from_numpy(weights[2 * i].copy(), backend=hip, requires_grad=True))
            layer.bias.update(mt.tensor_from_numpy(weights[2 * i + 1].copy(), backend=hip, requires_grad=True))
        x = mt.tensor_from_numpy(x_np.copy(), backend=hip, requires_grad=True)
        y = mha(x)
        y.backward(mt.tensor_from_numpy(g_np.copy(), backend=hip))
        out = {"y": y.to_numpy(), "x": x.grad.to_numpy()}
        for nm, layer in zip("qkvo", lin):
            out[f"{nm}_w"] = layer.weights.value.grad.to_numpy()
            out[f"{nm}_b"] = layer.bias.value.grad.to_numpy()
        return out
    gqa, tied = run(Hkv, w), run(None, w_tied)
    y_ref, ref, group_sum = _mha_f64(x_np, w, g_np, H, Hkv)
    ref["y"] = y_ref
    assert gqa["k_w"].shape == (E, Hkv * d) and tied["k_w"].shape == (E, H * d)
    for nm in ("k_w", "k_b", "v_w", "v_b"):  # the tied module's column blocks, summed per group
        tied[nm] = group_sum(tied[nm].astype(np.float64))
    failed = []
    for nm in ("y", "x", "q_w", "q_b", "o_w", "o_b", "k_w", "k_b", "v_w", "v_b"):
        dev_gqa = float(np.abs(gqa[nm] - ref[nm]).max())
        dev_tied = float(np.abs(tied[nm] - ref[nm]).max())
        tol = max(2.0 * dev_tied, 1e-5 * float(np.abs(ref[nm]).max()))
        print(f"{nm}: max|ref| {float(np.abs(ref[nm]).max()):.3e}; grouped module vs float64 {dev_gqa:.3e}, "
              f"tied n_head module vs float64 {dev_tied:.3e}, tolerance {tol:.3e}")
        parity_record("test_training_path_against_tied_heads", nm, max_abs=dev_gqa, tied_max_abs=dev_tied, bound=tol)
        if not dev_gqa <= tol:
            failed.append(nm)
    assert not failed, failed


def test_misuse_raises(world):
    mt, hip, lm = world["minitorch"], world["hip"], world["lm_h"]
    with pytest.raises(ValueError, match="n_kv_head"):
        mt.MultiHeadAttention(64, 4, backend=hip, n_kv_head=3)
    with pytest.raises(ValueError, match="n_kv_head"):
        mt.DecoderLM(backend=hip, **dict(KW, n_kv_head=3))
    with pytest.raises(ValueError, match="n_kv_head"):
        mt.KVCache(1, 1, 4, 8, 16, hip, n_kv_head=3)
    # a cache of another n_kv_head than the model's: refused, and the cache does not advance
    idx, lens = _padded(world["prompts"])
    for other in (None, 1):
        cache = mt.KVCache(4, len(lens), KW["n_head"], KW["n_positions"], KW["n_embd"] // KW["n_head"], hip,
                           n_kv_head=other)
        with pytest.raises(ValueError, match="KV cache was built for"):
            lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache)
        assert cache.empty and not cache.length.any(), "a refused step must not advance the cache"
