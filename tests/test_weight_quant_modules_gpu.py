"""DecoderLM.quantize_weights against its twin: the same fused_step model whose linears hold the
dequantised weights W' in fp32. The prefill (dequantise + matmul) and the decode step (the quantised
skinny linear) are the twin's bit for bit, so generate returns the twin's ids in every mode."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=128, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True, n_layer=2, fused_step=True)
ARCHS = {"gpt": {}, "llama": dict(norm="rms", mlp="swiglu", n_kv_head=2, pos_encoding="rope")}
NEW = 8
PER_STEP = 2 * 4 + 1  # fused launches of a step: four per layer and the head


def _model(arch, **over):
    import minitorch
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    np.random.seed(11)
    lm = minitorch.DecoderLM(backend=hip, **dict(KW, **ARCHS[arch], **over))
    lm.eval()
    return minitorch, hip, lm


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "int4"])
def test_quantised_model_is_its_twin(arch, fmt):
    from minitorch import _hip
    mt, hip, lm = _model(arch)
    twin = _model(arch)[2]
    shapes = [(lin.weights.value.shape, glu) for _, lin, glu in lm._linears()]
    before = lm.weight_nbytes
    assert before == sum(4 * k * n for (k, n), _ in shapes)
    lm.quantize_weights(fmt)
    want = sum(sum(_hip.weight_quant_bytes(_hip.WEIGHT_FORMATS[fmt], k, n // 2 if glu else n, glu)) for (k, n), glu in shapes)
    print(f"{arch} {fmt}: weight bytes {before} -> {lm.weight_nbytes} ({lm.weight_nbytes / before:.3f})")
    assert lm.weight_nbytes == want < before
    assert not {f"{name}.weights" for name, _, _ in lm._linears()} & dict(lm.named_parameters()).keys(), \
        "the fp32 weights are released"
    for (_, q, _), (_, t, _) in zip(lm._linears(), twin._linears()):
        t.weights.update(mt.tensor_from_numpy(q.qweight.dequantize().cpu().numpy(), hip, requires_grad=True))

    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    lens = np.array([len(p) for p in prompts])
    idx = np.zeros((3, 14), np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    step = rng.integers(0, KW["n_vocab"], (3, 1)).astype(np.float32)

    def logits(m):
        cache = m.new_cache(3)
        calls = _hip.fused_linear_calls
        pre = m(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache).to_numpy()
        assert _hip.fused_linear_calls == calls, "the prefill takes the unfused path"
        dec = m(mt.tensor_from_numpy(step, hip), cache=cache).to_numpy()
        assert _hip.fused_linear_calls == calls + PER_STEP, "the decode step ran fused"
        return pre, dec
    for name, a, b in zip(("prefill", "decode step"), logits(lm), logits(twin)):
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name

    for mode in (dict(), dict(graph=True), dict(speculate=2, kv_dtype="fp8")):
        assert lm.generate(prompts, NEW, **mode) == twin.generate(prompts, NEW, **mode), mode
    with pytest.raises(RuntimeError, match="cannot be trained"):
        lm.train()


def test_quantize_weights_refusals():
    lm = _model("gpt", n_embd=96)[2]
    with pytest.raises(ValueError, match=r"t_layer_1\.attention\.q_projection has an input width of 96"):
        lm.quantize_weights("int4")
    assert lm.quantized is None and lm.t_layer_1.attention.q_projection.qweight is None
    with pytest.raises(ValueError, match="fused_step=True"):
        _model("gpt", fused_step=False)[2].quantize_weights("fp8")
    with pytest.raises(ValueError, match="fmt must be"):
        _model("gpt")[2].quantize_weights("int8")
