"""A mixture-of-experts DecoderLM (mlp="moe", 4 experts, top 2; norm="rms", rope, n_kv_head=2,
fused_step=True) on the HIP backend against the same model on the CPU test backend, under
tests/test_llama_block_modules_gpu.py's rule: logits within max(1e-5 max|logit|, 2 dev), dev the
deviation of the full HIP forward (no cache: the tensor-op MoE) from the CPU model; ids compared
under its top-2 gap condition. The fixture also asserts, on the CPU twin, that at every layer and
position it visits the router's k-th and (k+1)-th logits are further apart than
2 (K + 8) 2^-24 max_e (|xh| @ |Wr|) (tests/test_moe_rows_gpu.py's selection condition), so both
models route alike. A fused step is 3 skinny-linear launches and one mt_moe_rows call per layer.
The training step's tolerance, atol = rtol = 1e-5, is that file's too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True, n_layer=2, norm="rms", mlp="moe", n_experts=4, moe_top_k=2, pos_encoding="rope",
          n_kv_head=2)
NEW = 16
SEED = 6


def _twins(fused_step=True, **over):
    """(minitorch, hip backend, cpu backend, HIP model, CPU model with the same parameters, gamma moved off 1)."""
    import minitorch
    from cpu_backend import NumpyOps
    hip, cpu = minitorch.TensorBackend(minitorch.HipKernelOps), minitorch.TensorBackend(NumpyOps)
    kw = dict(KW, **over)
    np.random.seed(SEED)
    lm_h, lm_c = minitorch.DecoderLM(backend=hip, fused_step=fused_step, **kw), minitorch.DecoderLM(backend=cpu, **kw)
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    assert ph.keys() == pc.keys()
    rng = np.random.default_rng(SEED)
    for name, p in ph.items():
        v = p.value.to_numpy()
        if name.endswith(("ln_1.weights", "ln_2.weights", "ln.weights")):
            v = (v + 0.2 * rng.standard_normal(v.shape)).astype(np.float32)
        p.update(minitorch.tensor_from_numpy(v.copy(), hip, requires_grad=True))
        pc[name].update(minitorch.tensor_from_numpy(v.copy(), cpu, requires_grad=True))
    return minitorch, hip, cpu, lm_h, lm_c


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    mt, hip, cpu, lm_h, lm_c = _twins()
    lm_h.eval()
    lm_c.eval()
    rng = np.random.default_rng(SEED)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    cpu_new = lm_c.generate(prompts, NEW, use_cache=False)
    full = [p + t for p, t in zip(prompts, cpu_new)]
    # the router's margin on the CPU twin, at every layer and position of the full sequences
    margins, K, k = [], KW["n_embd"], KW["moe_top_k"]
    for i in range(KW["n_layer"]):
        ff = getattr(lm_c, f"t_layer_{i + 1}").ff
        inner = ff._mask

        def spy(flat, logits, ff=ff, inner=inner):
            xh, wr = flat.to_numpy().astype(np.float64), ff.router.value.to_numpy().astype(np.float64)
            r = np.sort(xh @ wr, axis=1)[:, ::-1]
            margins.append(float(((r[:, k - 1] - r[:, k]) / (2 * (K + 8) * 2.0 ** -24 * (np.abs(xh) @ np.abs(wr)).max(1))).min()))
            return inner(flat, logits)
        ff._mask = spy
    forward = lambda lm, be, seq: lm(mt.tensor_from_numpy(np.asarray([seq], dtype=np.float32), be)).to_numpy()[0]  # noqa: E731
    cpu_logits = [forward(lm_c, cpu, s) for s in full]
    hip_logits = [forward(lm_h, hip, s) for s in full]  # no cache: the unfused path, the yardstick
    scale = max(float(np.abs(x).max()) for x in cpu_logits)
    dev = max(float(np.abs(a - b).max()) for a, b in zip(hip_logits, cpu_logits))
    tol = max(1e-5 * scale, 2.0 * dev)
    gap = min(float(np.diff(np.sort(x[len(p) - 1:len(p) - 1 + NEW], axis=-1)[:, -2:], axis=-1).min())
              for x, p in zip(cpu_logits, prompts))
    print(f"max|logit| {scale:.3f}; unfused full HIP forward vs CPU {dev:.3e}; tolerance {tol:.3e}; top-2 gap {gap:.3e}; "
          f"router gap / bound {min(margins):.1f}")
    assert gap > 10 * tol, "the seeds give a near-tie: choose others"
    assert len(margins) == KW["n_layer"] * len(full) and min(margins) > 1, "a router near-tie: choose another seed"
    return dict(mt=mt, hip=hip, lm=lm_h, prompts=prompts, cpu_new=cpu_new, cpu_logits=cpu_logits, tol=tol)


@pytest.mark.parametrize("chunk", [1, 3])
def test_teacher_forced_logits_through_the_cache(world, chunk):
    from minitorch import _hip
    mt, hip, lm = world["mt"], world["hip"], world["lm"]
    prompts, cpu_new, ref, tol = world["prompts"], world["cpu_new"], world["cpu_logits"], world["tol"]
    B, lens = len(prompts), np.array([len(p) for p in prompts])
    idx = np.zeros((B, int(lens.max())), np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    cache = lm.new_cache(B)
    calls = _hip.moe_rows_calls
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache).to_numpy()
    assert _hip.moe_rows_calls == calls, "the prefill takes the tensor-op path"
    worst = max(float(np.abs(logits[b, :lens[b]] - ref[b][:lens[b]]).max()) for b in range(B))
    steps = 0
    for s in range(0, NEW, chunk):
        T = min(chunk, NEW - s)
        logits = lm(mt.tensor_from_numpy(np.array([t[s:s + T] for t in cpu_new], np.float32), hip), cache=cache).to_numpy()
        steps += 1
        for b in range(B):
            worst = max(worst, float(np.abs(logits[b] - ref[b][lens[b] + s:lens[b] + s + T]).max()))
    assert _hip.moe_rows_calls == calls + steps * KW["n_layer"], "one mt_moe_rows call per layer and decode step"
    print(f"chunk {chunk}: worst |dlogit| {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol


def test_generate_ids_every_mode(world):
    from minitorch import _hip
    lm, prompts, cpu_new = world["lm"], world["prompts"], world["cpu_new"]
    calls = _hip.moe_rows_calls
    assert lm.generate(prompts, NEW) == cpu_new, "eager"
    assert _hip.moe_rows_calls == calls + (NEW - 1) * KW["n_layer"], "the eager decode steps ran the kernel"
    assert lm.generate(prompts, NEW, graph=True) == cpu_new, "graph"
    assert lm.generate(prompts, NEW, speculate=4) == cpu_new, "speculate"
    assert lm.generate(prompts, NEW, page_size=16) == cpu_new, "paged"
    fp8 = lm.generate(prompts, NEW, kv_dtype="fp8")
    assert lm.generate(prompts, NEW, kv_dtype="fp8", graph=True) == fp8, "fp8 cache: graph against its own eager ids"


def test_training_step_matches_the_cpu_twin():
    mt, hip, cpu, lm_h, lm_c = _twins(fused_step=False, n_vocab=50, n_embd=32, n_positions=12, n_layer=1)
    B, T, V = 4, 12, 50
    tok = np.random.default_rng(1).integers(0, V, size=(B, T + 1)).astype(np.float32)

    def loss(lm, be):
        logits = lm(mt.tensor_from_numpy(tok[:, :-1].copy(), be)).view(B * T, V)
        out = mt.softmax_loss(logits, mt.tensor_from_numpy(tok[:, 1:].reshape(-1).copy(), be)).sum() / (B * T)
        out.backward()
        return out.item()
    lh, lc = loss(lm_h, hip), loss(lm_c, cpu)
    assert abs(lh - lc) <= 1e-5 * abs(lc)
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    for name in ph:
        a, b = ph[name].value.grad.to_numpy(), pc[name].value.grad.to_numpy()
        print(f"{name}: max|dgrad| {float(np.abs(a - b).max()):.3e}")
        np.testing.assert_allclose(a, b, atol=1e-5, rtol=1e-5, err_msg=name)
