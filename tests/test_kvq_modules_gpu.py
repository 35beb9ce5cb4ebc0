"""The quantised KV cache through KVCache, MultiHeadAttention and DecoderLM on the HIP backend.

Model: V = 97, E = 64, 4 heads (d = 16), 2 layers, n_positions = 48, also with n_kv_head = 2.

Equivalence: a step on a quantised cache against the same step on an fp32 cache that holds the
quantised cache's dequantised rows. The new tokens' own K / V rows are quantised in one cache
only, so the fp32 cache's append is replaced by a copy of the quantised cache's rows of that
layer, dequantised (its rounded values are written into the fp32 cache before the step). Both
steps then run fp32 kernels that each meet 1e-5 on identical K / V values, over two layers:
the logits agree to 1e-4 + 1e-4 |x|.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LAYER = 2
KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True, n_layer=N_LAYER)
NEW = 12
KV_DTYPES = ["bf16", "fp8"]


def _world(n_kv_head):
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from minitorch import _hip
    _hip.lib()
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    kw = dict(KW) if n_kv_head is None else dict(KW, n_kv_head=n_kv_head)
    np.random.seed(0)
    lm = minitorch.DecoderLM(backend=hip, **kw)
    lm.eval()
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    return dict(minitorch=minitorch, hip=hip, lm=lm, prompts=prompts, torch=torch, _hip=_hip)


@pytest.fixture(scope="module", params=[None, 2], ids=["mha", "gqa2"])
def world(request):
    w = _world(request.param)
    yield w
    w["lm"].drop_decode_graphs()


@pytest.mark.parametrize("kv_dtype", [None, "fp32"] + KV_DTYPES)
def test_nbytes(world, kv_dtype):
    lm = world["lm"]
    B, P, d, Hkv = 3, KW["n_positions"], KW["n_embd"] // KW["n_head"], lm.n_kv_head
    cache = lm.new_cache(B, kv_dtype)
    fp32 = N_LAYER * 2 * B * Hkv * P * d * 4
    if kv_dtype in (None, "fp32"):
        assert cache.nbytes == fp32 and not cache.quantised and cache.kv_dtype == "fp32"
    elif kv_dtype == "bf16":
        assert cache.nbytes * 2 == fp32
        assert all(l.k.dtype == world["torch"].bfloat16 and l.k_scale is None for l in cache.layers)
    else:
        assert cache.nbytes == N_LAYER * 2 * (B * Hkv * P * d + B * Hkv * P * 4)
        assert cache.nbytes * 4 * d == fp32 * (d + 4)
        assert all(l.k.dtype == world["torch"].uint8 and l.k_scale.shape == (B, Hkv, P) for l in cache.layers)
    held = sum(t.numel() * t.element_size() for l in cache.layers for t in (l.k, l.v, l.k_scale, l.v_scale)
               if t is not None and not isinstance(t, world["minitorch"].Tensor))
    if cache.quantised:
        assert held == cache.nbytes


def _prefill(w, kv_dtype):
    mt, hip, lm, prompts = w["minitorch"], w["hip"], w["lm"], w["prompts"]
    B = len(prompts)
    lens = np.array([len(p) for p in prompts])
    idx = np.zeros((B, int(lens.max())), np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    cache = lm.new_cache(B, kv_dtype)
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache).to_numpy()
    assert list(cache.length_host) == list(lens)
    return cache, logits, lens


def _mirror(w, cq):
    """An fp32 KVCache holding cq's dequantised rows and lengths."""
    from minitorch.hip_kernel_ops import _torch_view
    _hip, lm = w["_hip"], w["lm"]
    cf = lm.new_cache(cq.batch_size)
    for lq, lf in zip(cq.layers, cf.layers):
        for t in (lf.k, lf.v):
            _torch_view(t).fill_(float("nan"))  # rows past the lengths are never read
        _hip.kv_cache_dequant(lq.k, lq.v, lq.k_scale, lq.v_scale, kv_len=cq.length,
                              k_out=_torch_view(lf.k), v_out=_torch_view(lf.v))
    cf.set_length(cq.length_host)
    return cf


def _step_both(w, monkeypatch, cq, step, kv_len=None):
    """The step on the quantised cache, then on its fp32 mirror with the append replaced by a copy
    of the quantised cache's (already appended) rows of the same layer."""
    from minitorch.hip_kernel_ops import _torch_view
    mt, hip, lm, _hip = w["minitorch"], w["hip"], w["lm"], w["_hip"]
    cf = _mirror(w, cq)
    kw = {} if kv_len is None else dict(kv_len=np.asarray(kv_len, np.float32))
    got = lm(mt.tensor_from_numpy(step, hip), cache=cq, **kw).to_numpy()
    layer_of = {_torch_view(l.k).data_ptr(): i for i, l in enumerate(cf.layers)}
    calls = []

    def rounded_append(knew, vnew, kc, vc, pos):
        lq = cq.layers[layer_of[_torch_view(kc).data_ptr()]]
        calls.append(1)
        _hip.kv_cache_dequant(lq.k, lq.v, lq.k_scale, lq.v_scale, kv_len=cq.length,
                              k_out=_torch_view(kc), v_out=_torch_view(vc))
    monkeypatch.setattr(hip, "kv_cache_append", rounded_append)
    want = lm(mt.tensor_from_numpy(step, hip), cache=cf, **kw).to_numpy()
    monkeypatch.undo()
    assert len(calls) == N_LAYER
    assert list(cf.length_host) == list(cq.length_host)
    return got, want


def _close(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    tol = 1e-4 + 1e-4 * np.abs(want)
    print(f"{what}: worst |dlogit| / tolerance {float((err / tol).max()):.3f}, max |dlogit| {float(err.max()):.3e}")
    assert np.isfinite(got).all()
    assert (err <= tol).all(), f"{what}: {float((err / tol).max()):.2f}x the tolerance"


@pytest.mark.parametrize("kv_dtype", KV_DTYPES)
def test_decode_and_extend_steps_equal_the_fp32_cache_on_the_same_values(world, kv_dtype, monkeypatch):
    cq, logits, lens = _prefill(world, kv_dtype)
    # the prefill attends the fresh fp32 K / V: its logits are the fp32 cache's, bit for bit
    _, logits_f, _ = _prefill(world, None)
    assert np.array_equal(logits.view(np.uint32), logits_f.view(np.uint32))
    B = len(lens)
    nxt = np.array([[5.0], [11.0], [96.0]], np.float32)
    got, want = _step_both(world, monkeypatch, cq, nxt)
    assert got.shape == (B, 1, KW["n_vocab"]) and list(cq.length_host) == list(lens + 1)
    _close(got, want, f"{kv_dtype} decode step")
    # an extend step of ragged counts (5, 0, 2) through the dequant scratch
    cnt = np.array([5, 0, 2])
    step = np.zeros((B, 5), np.float32)
    step[0] = [7, 1, 33, 64, 2]
    step[2, :2] = [90, 17]
    got, want = _step_both(world, monkeypatch, cq, step, kv_len=cnt)
    assert list(cq.length_host) == list(lens + 1 + cnt)
    for b in range(B):
        if cnt[b]:
            _close(got[b, :cnt[b]], want[b, :cnt[b]], f"{kv_dtype} extend step, row {b}")
    # and a 3-token decode step (Nq = 3) after it
    got, want = _step_both(world, monkeypatch, cq, np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32))
    _close(got, want, f"{kv_dtype} 3-token decode step")


@pytest.mark.parametrize("kv_dtype", KV_DTYPES)
def test_generate_forms_agree(world, kv_dtype):
    """Eager and graph=True give the same ids, greedy and sampled. prefill_chunk=4 runs and
    returns ids of the right shape; they may differ from the one-shot prefill's, because the
    later chunks already see the quantised prefix."""
    lm, prompts = world["lm"], world["prompts"]
    greedy = lm.generate(prompts, NEW, kv_dtype=kv_dtype)
    assert [len(t) for t in greedy] == [NEW] * len(prompts)
    assert all(0 <= t < KW["n_vocab"] for row in greedy for t in row)
    captures = lm.graph_captures or 0
    assert lm.generate(prompts, NEW, kv_dtype=kv_dtype, graph=True) == greedy
    assert lm.graph_captures == captures + 1
    assert lm.generate(prompts, NEW, kv_dtype=kv_dtype, graph=True) == greedy
    assert lm.graph_captures == captures + 1, "a second call replays the held graph"
    kw = dict(temperature=0.8, top_k=5, seed=7)
    sampled = lm.generate(prompts, NEW, kv_dtype=kv_dtype, **kw)
    assert [len(t) for t in sampled] == [NEW] * len(prompts)
    assert lm.generate(prompts, NEW, kv_dtype=kv_dtype, graph=True, **kw) == sampled
    for graph in (False, True):
        chunked = lm.generate(prompts, NEW, kv_dtype=kv_dtype, prefill_chunk=4, graph=graph)
        assert [len(t) for t in chunked] == [NEW] * len(prompts)
        assert all(0 <= t < KW["n_vocab"] for row in chunked for t in row)
    lm.drop_decode_graphs()


def test_misuse_raises(world):
    lm, prompts = world["lm"], world["prompts"]
    with pytest.raises(ValueError, match="use_cache"):
        lm.generate(prompts, 4, kv_dtype="fp8", use_cache=False)
    with pytest.raises(ValueError, match="kv_dtype"):
        lm.generate(prompts, 4, kv_dtype="int4")
    with pytest.raises(ValueError, match="kv_dtype"):
        lm.new_cache(2, "fp16")


def test_unset_kv_dtype_is_the_fp32_path_bit_for_bit(world):
    """kv_dtype=None and "fp32" take today's code path: the same ids, and the same logits from a
    prefill and a decode step, bit for bit."""
    mt, hip, lm, prompts = world["minitorch"], world["hip"], world["lm"], world["prompts"]
    want = lm.generate(prompts, NEW)
    assert lm.generate(prompts, NEW, kv_dtype=None) == want
    assert lm.generate(prompts, NEW, kv_dtype="fp32") == want
    assert lm.generate(prompts, NEW, kv_dtype="fp32", graph=True) == want
    assert list(lm._decode_graphs) == [len(prompts)], "the fp32 cache keeps its graph slot"
    lm.drop_decode_graphs()
    outs = []
    for args in ((), (None,), ("fp32",)):
        B = len(prompts)
        lens = np.array([len(p) for p in prompts])
        idx = np.zeros((B, int(lens.max())), np.float32)
        for b, p in enumerate(prompts):
            idx[b, :len(p)] = p
        cache = lm.new_cache(B, *args)
        assert type(cache.layers[0].k) is mt.Tensor
        a = lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache).to_numpy()
        b_ = lm(mt.tensor_from_numpy(np.array([[5.0], [11.0], [96.0]], np.float32), hip), cache=cache).to_numpy()
        outs.append((a, b_))
    for a, b_ in outs[1:]:
        assert np.array_equal(a.view(np.uint32), outs[0][0].view(np.uint32))
        assert np.array_equal(b_.view(np.uint32), outs[0][1].view(np.uint32))
