"""Grouped-query attention for training and prefill (mt_flash_attn_fwd_gqa / _bwd_gqa, fa_gqa.hip)
on the GPU: K, V, dK, dV at Hkv heads, query head h on kv head h // G.

* The kernels against the CPU oracle on K / V repeated to H heads, its dK / dV summed over each
  group in float64. Bounds: O, dQ 1e-5 max-abs and l 1e-5 relative (the project's fp32 bound,
  tests/test_varlen_gpu.py); dK, dV G * 1e-5 (a sum of G terms each under that bound).
* The model's storage layout gives the dense call's bits; a second call gives the same bits.
* Hkv == H is flash_fwd / flash_bwd, bit for bit.
* MultiHeadAttention(fused_gqa=True) against the float64 restatement, allowed twice the
  deviation of the same module with fused_gqa=False; DecoderLM.generate returns the same ids.
"""
import numpy as np
import pytest

from oracle import attention as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _np(t):
    return t.cpu().numpy()


CASES = [  # (B, H, Hkv, N, d, kv_len)
    (3, 4, 2, 200, 32, (200, 77, 0)),   # G = 2; kv_len N, inside a tile, 0
    (3, 4, 1, 130, 64, (1, 130, 64)),   # G = 4 (multi-query); kv_len 1
    (2, 8, 1, 130, 32, None),           # G = 8: two slices of four heads
    (2, 6, 2, 200, 64, (200, 45)),      # G = 3: a group the wave packing does not divide
    (2, 4, 2, 130, 128, (130, 40)),     # d = 128
    (1, 4, 2, 20, 64, None),            # N below one tile
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,Hkv,N,d,kv", CASES)
def test_gqa_vs_oracle(torch, B, H, Hkv, N, d, kv, causal):
    from minitorch import _hip
    G = H // Hkv
    rng = np.random.default_rng(N + d + H)
    q, do = (rng.standard_normal((B, H, N, d)).astype(np.float32) for _ in range(2))
    k, v = (rng.standard_normal((B, Hkv, N, d)).astype(np.float32) for _ in range(2))
    tq, tk, tv, tdo = (_dev(torch, x) for x in (q, k, v, do))
    o, m, l = _hip.flash_fwd_gqa(tq, tk, tv, causal, kv_len=kv)
    dq, dk, dv = _hip.flash_bwd_gqa(tq, tk, tv, o, tdo, m, l, causal, kv_len=kv)
    torch.cuda.synchronize()
    assert dk.shape == tk.shape and dv.shape == tv.shape
    kr, vr = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
    o_ref, m_ref, l_ref = A.attention_fwd(q, kr, vr, causal, kv)
    dq_ref, dk_ref, dv_ref = A.attention_bwd(q, kr, vr, o_ref, do, m_ref, l_ref, causal, kv)
    dk_ref, dv_ref = (x.astype(np.float64).reshape(B, Hkv, G, N, d).sum(2) for x in (dk_ref, dv_ref))
    for name, got, ref in (("o", o, o_ref), ("dq", dq, dq_ref), ("dk", dk, dk_ref), ("dv", dv, dv_ref)):
        print(f"{name}: max|err| {float(np.abs(_np(got) - ref).max()):.3e}")
    np.testing.assert_allclose(_np(o), o_ref, atol=1e-5, rtol=0)
    np.testing.assert_allclose(_np(l), l_ref, rtol=1e-5, atol=0)
    np.testing.assert_allclose(_np(dq), dq_ref, atol=1e-5, rtol=0)
    np.testing.assert_allclose(_np(dk), dk_ref, atol=G * 1e-5, rtol=0)
    np.testing.assert_allclose(_np(dv), dv_ref, atol=G * 1e-5, rtol=0)
    for b, n in enumerate(kv or ()):  # padding keys: exactly zero dK / dV; an empty row: all zero
        assert not _np(dk[b, :, n:]).any() and not _np(dv[b, :, n:]).any()
        if n == 0:
            assert not _np(o[b]).any() and not _np(dq[b]).any() and not _np(l[b]).any()
            assert np.isneginf(_np(m[b])).all()


@pytest.mark.parametrize("causal", [False, True])
def test_model_layout_and_repeat_give_the_same_bits(torch, causal):
    """[B,N,H,d] storage seen as [B,H,N,d] (K / V [B,N,Hkv,d]), every output in that layout too."""
    from minitorch import _hip
    B, H, Hkv, N, d, kv = 2, 4, 2, 130, 64, (130, 50)
    g = torch.Generator(device="cpu").manual_seed(5)
    q, do = (torch.randn(B, N, H, d, generator=g).cuda().permute(0, 2, 1, 3) for _ in range(2))
    k, v = (torch.randn(B, N, Hkv, d, generator=g).cuda().permute(0, 2, 1, 3) for _ in range(2))

    def run(q, k, v, do, strided):
        like = (lambda t: torch.empty_like(t.permute(0, 2, 1, 3).contiguous()).permute(0, 2, 1, 3)) if strided else \
               (lambda t: torch.empty_like(t, memory_format=torch.contiguous_format))
        o, m, l = _hip.flash_fwd_gqa(q, k, v, causal, out=like(q), kv_len=kv)
        grads = _hip.flash_bwd_gqa(q, k, v, o, do, m, l, causal, dq=like(q), dk=like(k), dv=like(v), kv_len=kv)
        assert all(t.is_contiguous() != strided for t in (o, *grads))
        return (o, m, l, *grads)
    first = run(q, k, v, do, True)
    again = run(q, k, v, do, True)
    dense = run(*(t.contiguous() for t in (q, k, v, do)), False)
    for a, b, c in zip(first, again, dense):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("causal", [False, True])
def test_hkv_equal_h_is_the_plain_call(torch, causal):
    from minitorch import _hip
    B, H, N, d, kv = 2, 4, 130, 64, (130, 50)
    g = torch.Generator(device="cpu").manual_seed(6)
    q, k, v, do = (torch.randn(B, H, N, d, generator=g).cuda() for _ in range(4))
    o, m, l = _hip.flash_fwd(q, k, v, causal, kv_len=kv)
    want = (o, m, l, *_hip.flash_bwd(q, k, v, o, do, m, l, causal, kv_len=kv))
    o2, m2, l2 = _hip.flash_fwd_gqa(q, k, v, causal, kv_len=kv)
    got = (o2, m2, l2, *_hip.flash_bwd_gqa(q, k, v, o2, do, m2, l2, causal, kv_len=kv))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def _mha_f64(x, w, g, H, Hkv, kv):
    """Float64 causal grouped-query MultiHeadAttention with key padding, forward and backward:
    w = (Wq, bq, Wk, bk, Wv, bv, Wo, bo), g = dL/dY. Returns y and the gradients by name."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    wq, bq, wk, bk, wv, bv, wo, bo = (np.asarray(a, np.float64) for a in w)
    B, T, E = x.shape
    d, G = E // H, H // Hkv
    X = x.reshape(B * T, E)
    heads = lambda a, n: a.reshape(B, T, n, d).transpose(0, 2, 1, 3)  # noqa: E731
    flat = lambda a: a.transpose(0, 2, 1, 3).reshape(B * T, -1)       # noqa: E731
    q = heads(X @ wq + bq, H)
    k, v = (np.repeat(heads(X @ a + b, Hkv), G, axis=1) for a, b in ((wk, bk), (wv, bv)))
    s = np.einsum("bhqd,bhkd->bhqk", q, k) / np.sqrt(d)
    hidden = np.triu(np.ones((T, T), bool), 1)[None, None] | (np.arange(T)[None, None, None, :] >=
                                                              np.asarray(kv).reshape(B, 1, 1, 1))
    s = np.where(hidden, -np.inf, s)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = flat(np.einsum("bhqk,bhkd->bhqd", p, v))
    dy = g.reshape(B * T, E)
    do = heads(dy @ wo.T, H)
    dp = np.einsum("bhqd,bhkd->bhqk", do, v)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True))
    group_sum = lambda a: a.reshape(B * T, Hkv, G, d).sum(2).reshape(B * T, Hkv * d)  # noqa: E731
    dqf = flat(np.einsum("bhqk,bhkd->bhqd", ds, k)) / np.sqrt(d)
    dkg = group_sum(flat(np.einsum("bhqk,bhqd->bhkd", ds, q))) / np.sqrt(d)
    dvg = group_sum(flat(np.einsum("bhqk,bhqd->bhkd", p, do)))
    return {"y": (o @ wo + bo).reshape(B, T, E), "x": (dqf @ wq.T + dkg @ wk.T + dvg @ wv.T).reshape(B, T, E),
            "q_w": X.T @ dqf, "q_b": dqf.sum(0), "o_w": o.T @ dy, "o_b": dy.sum(0),
            "k_w": X.T @ dkg, "k_b": dkg.sum(0), "v_w": X.T @ dvg, "v_b": dvg.sum(0)}


@pytest.mark.parametrize("kv", [None, (16, 9)])
def test_module_fused_gqa(torch, kv, parity_record, monkeypatch):
    """The shapes and the rule of test_gqa_modules_gpu.py::test_training_path_against_tied_heads."""
    import minitorch as mt
    from minitorch import _hip
    calls = []
    for name in ("flash_fwd_gqa", "flash_bwd_gqa"):  # only the fused module may reach the kernels
        monkeypatch.setattr(_hip, name, lambda *a, _f=getattr(_hip, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    hip = mt.TensorBackend(mt.HipKernelOps)
    E, H, Hkv, B, T = 64, 4, 2, 2, 16
    d = E // H
    rng = np.random.default_rng(21)
    shapes = [(E, E), (E,), (E, Hkv * d), (Hkv * d,), (E, Hkv * d), (Hkv * d,), (E, E), (E,)]
    w = [(0.3 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    x_np, g_np = (rng.standard_normal((B, T, E)).astype(np.float32) for _ in range(2))
    with pytest.raises(ValueError, match="use_flash_attention"):
        mt.MultiHeadAttention(E, H, backend=hip, n_kv_head=Hkv, fused_gqa=True)

    def run(fused):
        mha = mt.MultiHeadAttention(E, H, causal=True, p_dropout=0.0, backend=hip, use_flash_attention=True,
                                    n_kv_head=Hkv, fused_gqa=fused)
        lin = (mha.q_projection, mha.k_projection, mha.v_projection, mha.out_projection)
        for i, layer in enumerate(lin):
            layer.weights.update(mt.tensor_from_numpy(w[2 * i].copy(), backend=hip, requires_grad=True))
            layer.bias.update(mt.tensor_from_numpy(w[2 * i + 1].copy(), backend=hip, requires_grad=True))
        x = mt.tensor_from_numpy(x_np.copy(), backend=hip, requires_grad=True)
        y = mha(x) if kv is None else mha(x, kv_len=list(kv))
        y.backward(mt.tensor_from_numpy(g_np.copy(), backend=hip))
        out = {"y": y.to_numpy(), "x": x.grad.to_numpy()}
        for nm, layer in zip("qkvo", lin):
            out[f"{nm}_w"] = layer.weights.value.grad.to_numpy()
            out[f"{nm}_b"] = layer.bias.value.grad.to_numpy()
        return out
    fused = run(True)
    assert calls == ["flash_fwd_gqa", "flash_bwd_gqa"]
    plain = run(False)
    assert len(calls) == 2, "fused_gqa unset must keep the repeat path"
    ref = _mha_f64(x_np, w, g_np, H, Hkv, (T,) * B if kv is None else kv)
    failed = []
    for nm, r in ref.items():
        dev_f, dev_p = (float(np.abs(a[nm] - r).max()) for a in (fused, plain))
        tol = max(2.0 * dev_p, 1e-5 * float(np.abs(r).max()))
        print(f"{nm}: max|ref| {float(np.abs(r).max()):.3e}; fused_gqa vs float64 {dev_f:.3e}, repeat path {dev_p:.3e}, "
              f"tolerance {tol:.3e}")
        parity_record("test_module_fused_gqa", f"kv={kv} {nm}", max_abs=dev_f, repeat_max_abs=dev_p, bound=tol)
        if not dev_f <= tol:
            failed.append(nm)
    assert not failed, failed


def test_generate_with_fused_gqa_returns_the_same_ids(torch):
    import minitorch as mt
    hip = mt.TensorBackend(mt.HipKernelOps)
    kw = dict(n_vocab=97, n_embd=64, n_head=4, n_kv_head=2, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
              use_flash_attention=True, backend=hip)
    np.random.seed(0)
    plain = mt.DecoderLM(**kw)
    fused = mt.DecoderLM(fused_gqa=True, **kw)
    for (n, p), (n2, p2) in zip(plain.named_parameters(), fused.named_parameters()):
        assert n == n2
        p2.update(mt.tensor_from_numpy(p.value.to_numpy().copy(), hip))
    plain.eval()
    fused.eval()
    prompts = [[int(t) for t in np.random.default_rng(0).integers(0, 97, n)] for n in (3, 9, 14)]
    want = plain.generate(prompts, 16)
    assert fused.generate(prompts, 16) == want
    assert fused.generate(prompts, 16, use_cache=False) == want
