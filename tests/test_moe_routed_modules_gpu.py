"""DecoderLM(mlp="moe", moe_routed=True) on the HIP backend (the MoERouted Function: sort, grouped
GEMMs, combine) against tests/test_moe_modules_gpu.py's CPU twin, which falls back to the dense
path: that file's models, seeds, rules and router-margin condition. Logits within
max(1e-5 max|logit|, 2 dev), dev the deviation of the dense HIP forward (a moe_routed=False model
with the same parameters: the code this path replaces, never the code under test) from the CPU
twin; the training step at atol = rtol = 1e-5, bitwise repeatable and replayed by a StepGraph."""
import numpy as np
import pytest

from test_moe_modules_gpu import KW, NEW, SEED, _twins

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    mt, hip, cpu, lm_r, lm_c = _twins(moe_routed=True)
    lm_d = _twins()[3]  # the same parameters on the dense tensor-op path
    for lm in (lm_r, lm_c, lm_d):
        lm.eval()
    rng = np.random.default_rng(SEED)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    full = [p + t for p, t in zip(prompts, lm_c.generate(prompts, NEW, use_cache=False))]
    margins, K, k = [], KW["n_embd"], KW["moe_top_k"]
    for i in range(KW["n_layer"]):  # the router's margin on the CPU twin, as in that file
        ff = getattr(lm_c, f"t_layer_{i + 1}").ff
        assert ff.routed and not ff._takes_routed(mt.tensor_from_numpy(np.zeros((1, K), np.float32), cpu))

        def spy(flat, logits, ff=ff, inner=ff._mask):
            xh, wr = flat.to_numpy().astype(np.float64), ff.router.value.to_numpy().astype(np.float64)
            r = np.sort(xh @ wr, axis=1)[:, ::-1]
            margins.append(float(((r[:, k - 1] - r[:, k]) / (2 * (K + 8) * 2.0 ** -24 * (np.abs(xh) @ np.abs(wr)).max(1))).min()))
            return inner(flat, logits)
        ff._mask = spy
    forward = lambda lm, be, seq: lm(mt.tensor_from_numpy(np.asarray([seq], dtype=np.float32), be)).to_numpy()[0]  # noqa: E731
    cpu_logits = [forward(lm_c, cpu, s) for s in full]
    assert len(margins) == KW["n_layer"] * len(full) and min(margins) > 1, "a router near-tie: choose another seed"
    dev = max(float(np.abs(forward(lm_d, hip, s) - c).max()) for s, c in zip(full, cpu_logits))
    tol = max(1e-5 * max(float(np.abs(x).max()) for x in cpu_logits), 2.0 * dev)
    print(f"dense HIP forward vs CPU {dev:.3e}; tolerance {tol:.3e}; router gap / bound {min(margins):.1f}")
    return dict(mt=mt, hip=hip, lm=lm_r, prompts=prompts, full=full, cpu_logits=cpu_logits, tol=tol, forward=forward)


def test_full_forward_and_prefill_logits(world):
    from minitorch import _hip
    mt, hip, lm, prompts, ref, tol = (world[n] for n in ("mt", "hip", "lm", "prompts", "cpu_logits", "tol"))
    calls = _hip.moe_grouped_calls
    worst = max(float(np.abs(world["forward"](lm, hip, s) - c).max()) for s, c in zip(world["full"], ref))
    assert _hip.moe_grouped_calls == calls + KW["n_layer"] * len(ref), "one routed forward per layer"
    lens = np.array([len(p) for p in prompts])
    idx = np.zeros((len(prompts), int(lens.max())), np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    calls, rows = _hip.moe_grouped_calls, _hip.moe_rows_calls
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=lm.new_cache(len(prompts))).to_numpy()
    assert _hip.moe_grouped_calls == calls + KW["n_layer"] and _hip.moe_rows_calls == rows, "the prefill is routed"
    prefill = max(float(np.abs(logits[b, :lens[b]] - ref[b][:lens[b]]).max()) for b in range(len(prompts)))
    print(f"worst |dlogit|: full forward {worst:.3e}, prefill {prefill:.3e}; tolerance {tol:.3e}")
    assert max(worst, prefill) <= tol


def test_chunked_prefill_returns_the_same_ids(world):
    lm, prompts = world["lm"], world["prompts"]
    assert lm.generate(prompts, NEW, prefill_chunk=4) == lm.generate(prompts, NEW)


@pytest.mark.parametrize("B,T", [(4, 12), (8, 12)], ids=["48 rows", "96 rows"])
def test_training_step_matches_the_cpu_twin(B, T):
    import torch
    from minitorch import _hip
    from minitorch.graphs import StepGraph
    V = 50
    mt, hip, cpu, lm_h, lm_c = _twins(fused_step=False, n_vocab=V, n_embd=32, n_positions=T, n_layer=1, moe_routed=True)
    tok = np.random.default_rng(1).integers(0, V, size=(B, T + 1)).astype(np.float32)

    def step(lm, be):
        x, y = mt.tensor_from_numpy(tok[:, :-1].copy(), be), mt.tensor_from_numpy(tok[:, 1:].reshape(-1).copy(), be)

        def run():
            for p in lm.parameters():
                p.value.zero_grad_()
            out = mt.softmax_loss(lm(x).view(B * T, V), y).sum() / (B * T)
            out.backward()
            return out
        return run
    run_h, calls = step(lm_h, hip), _hip.moe_grouped_calls
    lh, lc = run_h().to_numpy(), step(lm_c, cpu)().to_numpy()
    assert _hip.moe_grouped_calls == calls + 1, "the training forward is routed"
    assert abs(lh[0] - lc[0]) <= 1e-5 * abs(lc[0])
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    grads = {name: p.value.grad.to_numpy().copy() for name, p in ph.items()}
    for name, a in grads.items():
        b = pc[name].value.grad.to_numpy()
        print(f"{name}: max|dgrad| {float(np.abs(a - b).max()):.3e}")
        np.testing.assert_allclose(a, b, atol=1e-5, rtol=1e-5, err_msg=name)
    again = run_h().to_numpy()  # a second eager step: the same bits (no atomics, fixed orders)
    assert again.tobytes() == lh.tobytes()
    for name, a in grads.items():
        assert np.array_equal(ph[name].value.grad.to_numpy().view(np.uint32), a.view(np.uint32)), name
    g = StepGraph(run_h, warmup=1)
    for _ in range(2):
        loss = g.replay()
        torch.cuda.synchronize()
        assert loss.to_numpy().tobytes() == lh.tobytes(), "a replay returns the eager loss bits"
