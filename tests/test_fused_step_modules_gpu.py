"""DecoderLM(fused_step=True) on the HIP backend against the same model on the CPU test backend,
built as tests/test_generate_gpu.py builds its world, over {learned, rope} x {n_kv_head None, 2}.
The tolerance is that file's: max(1e-5 max|logit|, 2 dev), dev the deviation of the full HIP
forward (no cache: the unfused path) from the CPU model; ids are compared under its top-2 gap
condition. _hip.fused_linear_calls tells which path a step took: a fused step of this 4-layer
model is 4 launches per layer and one for ln + lm_head."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16
PER_STEP = 4 * 4 + 1
SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9, seed=11)


@pytest.fixture(scope="module", params=[(pe, kv) for pe in ("learned", "rope") for kv in (None, 2)],
                ids=lambda p: f"{p[0]}-kv{p[1]}")
def world(request):
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from cpu_backend import NumpyOps
    pos_encoding, n_kv_head = request.param
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    cpu = minitorch.TensorBackend(NumpyOps)
    kw = dict(KW, pos_encoding=pos_encoding, n_kv_head=n_kv_head)
    np.random.seed(2)
    lm_h = minitorch.DecoderLM(backend=hip, fused_step=True, **kw)
    lm_c = minitorch.DecoderLM(backend=cpu, **kw)
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    assert ph.keys() == pc.keys()
    rng = np.random.default_rng(2)
    for name, p in ph.items():
        if name.endswith(("ln_1.weights", "ln_2.weights", "ln.weights", "ln_1.bias", "ln_2.bias", "ln.bias")):
            # non-trivial gamma / beta (the constructor's are 1 and 0)
            p.update(minitorch.tensor_from_numpy(
                (p.value.to_numpy() + 0.2 * rng.standard_normal(p.value.shape)).astype(np.float32), hip))
        pc[name].update(minitorch.tensor_from_numpy(p.value.to_numpy().copy(), cpu))
    lm_h.eval()
    lm_c.eval()
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    cpu_new = lm_c.generate(prompts, NEW, use_cache=False)
    full = [p + t for p, t in zip(prompts, cpu_new)]

    def forward(lm, backend, seq):
        return lm(minitorch.tensor_from_numpy(np.asarray([seq], dtype=np.float32), backend)).to_numpy()[0]
    cpu_logits = [forward(lm_c, cpu, s) for s in full]
    hip_logits = [forward(lm_h, hip, s) for s in full]  # no cache: the unfused path, the yardstick
    scale = max(float(np.abs(x).max()) for x in cpu_logits)
    dev = max(float(np.abs(a - b).max()) for a, b in zip(hip_logits, cpu_logits))
    tol = max(1e-5 * scale, 2.0 * dev)
    gap = min(float(np.diff(np.sort(x[len(p) - 1:len(p) - 1 + NEW], axis=-1)[:, -2:], axis=-1).min())
              for x, p in zip(cpu_logits, prompts))
    print(f"max|logit| {scale:.3f}; unfused full HIP forward vs CPU {dev:.3e}; tolerance {tol:.3e}; "
          f"smallest top-2 gap {gap:.3e}")
    assert gap > 10 * tol, "the seeds give a near-tie: choose others"
    return dict(minitorch=minitorch, hip=hip, cpu=cpu, lm=lm_h, lm_c=lm_c, prompts=prompts, cpu_new=cpu_new, cpu_logits=cpu_logits,
                tol=tol)


def _padded(prompts):
    lens = np.array([len(p) for p in prompts])
    idx = np.zeros((len(prompts), int(lens.max())), np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    return idx, lens


@pytest.mark.parametrize("chunk", [1, 3])
def test_teacher_forced_logits_through_the_cache(world, chunk):
    from minitorch import _hip
    mt, hip, lm = world["minitorch"], world["hip"], world["lm"]
    prompts, cpu_new, ref, tol = world["prompts"], world["cpu_new"], world["cpu_logits"], world["tol"]
    B = len(prompts)
    idx, lens = _padded(prompts)
    cache = lm.new_cache(B)
    calls = _hip.fused_linear_calls
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache).to_numpy()
    assert _hip.fused_linear_calls == calls, "the prefill takes the unfused path"
    worst = max(float(np.abs(logits[b, :lens[b]] - ref[b][:lens[b]]).max()) for b in range(B))
    steps = 0
    for s in range(0, NEW, chunk):
        T = min(chunk, NEW - s)
        step = np.array([t[s:s + T] for t in cpu_new], np.float32)
        logits = lm(mt.tensor_from_numpy(step, hip), cache=cache).to_numpy()
        steps += 1
        for b in range(B):
            worst = max(worst, float(np.abs(logits[b] - ref[b][lens[b] + s:lens[b] + s + T]).max()))
    assert _hip.fused_linear_calls == calls + steps * PER_STEP, "every decode step ran fused"
    print(f"chunk {chunk}: worst |dlogit| {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol


def test_generate_ids_every_mode(world):
    from minitorch import _hip
    lm, prompts, cpu_new = world["lm"], world["prompts"], world["cpu_new"]
    calls = _hip.fused_linear_calls
    assert lm.generate(prompts, NEW) == cpu_new, "eager"
    assert _hip.fused_linear_calls == calls + (NEW - 1) * PER_STEP, "the eager decode steps ran fused"
    assert lm.generate(prompts, NEW, graph=True) == cpu_new, "graph"
    assert lm.generate(prompts, NEW, speculate=4, graph=True) == cpu_new, "speculate, graph"
    assert lm.generate(prompts, NEW, kv_dtype="bf16") == cpu_new, "bf16 cache"
    assert lm.generate(prompts, NEW, page_size=16) == cpu_new, "paged cache"
    # by determinism, not tolerance: a (k + 1)-token verify step and a one-token step give the same rows
    sampled = lm.generate(prompts, NEW, **SAMPLED)
    assert lm.generate(prompts, NEW, graph=True, **SAMPLED) == sampled, "sampled, graph"
    assert lm.generate(prompts, NEW, speculate=4, **SAMPLED) == sampled, "sampled, speculate"


def test_large_steps_fall_back_and_still_match(world):
    """An extend step of B T = 3 x 24 > 64 rows takes the unfused path; the same tokens fed in
    fused steps of 8 columns run fused; both match the CPU model's full forward."""
    from minitorch import _hip
    mt, hip, lm, tol = world["minitorch"], world["hip"], world["lm"], world["tol"]
    rng = np.random.default_rng(5)
    seq = rng.integers(0, KW["n_vocab"], (3, 32)).astype(np.float32)
    want = world["lm_c"](mt.tensor_from_numpy(seq, world["cpu"])).to_numpy()[:, 8:]
    eight = np.full(3, 8, np.float32)
    big, small = lm.new_cache(3), lm.new_cache(3)
    for cache in (big, small):
        lm(mt.tensor_from_numpy(np.ascontiguousarray(seq[:, :8]), hip), kv_len=eight, cache=cache)
    calls = _hip.fused_linear_calls
    one = lm(mt.tensor_from_numpy(np.ascontiguousarray(seq[:, 8:]), hip), kv_len=3 * eight, cache=big).to_numpy()
    assert _hip.fused_linear_calls == calls, "72 rows are past the fused kernel's 64"
    three = np.concatenate([lm(mt.tensor_from_numpy(np.ascontiguousarray(seq[:, s:s + 8]), hip), kv_len=eight,
                               cache=small).to_numpy() for s in (8, 16, 24)], axis=1)
    assert _hip.fused_linear_calls == calls + 3 * PER_STEP
    assert float(np.abs(one - want).max()) <= tol and float(np.abs(three - want).max()) <= tol
