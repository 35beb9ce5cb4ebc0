"""DecoderLM(pos_encoding="rope") on the HIP backend against the same model on the CPU test
backend (tests/cpu_backend.py), which runs the tensor-op form of the rotation: the reference.

Built like tests/test_generate_gpu.py's world, with its KW plus pos_encoding="rope", and its
tolerance rule: the larger of 1e-5 max|logit| and twice `dev`. `dev` is measured on the existing
path, not the new one: the full-forward deviation of the learned-position HIP model from its CPU
twin at the same KW, seeds and sequences. The rotation adds about 1e-7 relative error to Q and K,
far below the GEMM and attention deviation `dev` captures, so that file's margin of 2 carries over.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16


def _twins(minitorch, hip, cpu, seed=0, **kw):
    np.random.seed(seed)
    lm_h = minitorch.DecoderLM(backend=hip, **kw)
    lm_c = minitorch.DecoderLM(backend=cpu, **kw)
    _copy_params(minitorch, lm_h, lm_c, cpu)
    lm_h.eval()
    lm_c.eval()
    return lm_h, lm_c


def _copy_params(minitorch, src, dst, backend):
    ps, pd = dict(src.named_parameters()), dict(dst.named_parameters())
    assert ps.keys() == pd.keys()
    for name, p in ps.items():
        pd[name].update(minitorch.tensor_from_numpy(p.value.to_numpy().copy(), backend))


def _forward(minitorch, lm, backend, seq):
    idx = minitorch.tensor_from_numpy(np.asarray([seq], dtype=np.float32), backend)
    return lm(idx).to_numpy()[0]


@pytest.fixture(scope="module")
def world(parity_record):
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from cpu_backend import NumpyOps
    from minitorch import _hip
    _hip.lib()
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    cpu = minitorch.TensorBackend(NumpyOps)
    lm_h, lm_c = _twins(minitorch, hip, cpu, pos_encoding="rope", **KW)
    assert not any("position_embeddings" in n for n, _ in lm_h.named_parameters())
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (3, 9, 14)]
    cpu_new = lm_c.generate(prompts, NEW, use_cache=False)
    assert all(len(t) == NEW for t in cpu_new)
    full = [p + t for p, t in zip(prompts, cpu_new)]
    # teacher-forced rows that fill all n_positions (the extend steps, the position clamp)
    long = [[int(t) for t in rng.integers(0, KW["n_vocab"], KW["n_positions"])] for _ in range(3)]
    cpu_logits = [_forward(minitorch, lm_c, cpu, s) for s in full]
    hip_logits = [_forward(minitorch, lm_h, hip, s) for s in full]
    long_logits = [_forward(minitorch, lm_c, cpu, s) for s in long]
    scale = max(float(np.abs(x).max()) for x in cpu_logits + long_logits)
    # the yardstick: the learned-position model, HIP against CPU, on the same sequences
    ln_h, ln_c = _twins(minitorch, hip, cpu, **KW)
    dev = max(float(np.abs(_forward(minitorch, ln_h, hip, s) - _forward(minitorch, ln_c, cpu, s)).max())
              for s in full + long)
    tol = max(1e-5 * scale, 2.0 * dev)
    gap = min(float(np.diff(np.sort(x[len(p) - 1:len(p) - 1 + NEW], axis=-1)[:, -2:], axis=-1).min())
              for x, p in zip(cpu_logits, prompts))
    print(f"max|logit| {scale:.3f}; learned-position HIP forward vs CPU {dev:.3e}; tolerance {tol:.3e}; "
          f"smallest top-2 gap {gap:.3e}")
    parity_record("test_rope_modules_world", "yardstick", scale=scale, dev_learned=dev, bound=tol, top2_gap=gap)
    assert gap > 10 * tol, "the seeds give a near-tie: choose others"
    return dict(minitorch=minitorch, hip=hip, cpu=cpu, lm_h=lm_h, lm_c=lm_c, prompts=prompts, cpu_new=cpu_new,
                cpu_logits=cpu_logits, hip_logits=hip_logits, long=long, long_logits=long_logits, tol=tol,
                scale=scale)


def _padded(prompts):
    lens = np.array([len(p) for p in prompts])
    idx = np.zeros((len(prompts), int(lens.max())), np.float32)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = p
    return idx, lens


def test_full_forward(world, parity_record):
    worst = max(float(np.abs(a - b).max()) for a, b in zip(world["hip_logits"], world["cpu_logits"]))
    print(f"full forward: worst |dlogit| {worst:.3e}, tolerance {world['tol']:.3e}")
    parity_record("test_rope_full_forward", "fused kernel + flash", max_abs=worst, bound=world["tol"])
    assert worst <= world["tol"]
    # the positions matter: the same model without them would give other logits
    a = world["hip_logits"][0]
    assert np.abs(a[2] - _forward(world["minitorch"], world["lm_h"], world["hip"], world["prompts"][0][2:3])[0]).max() > 0


def test_tensor_op_form_on_hip(world, parity_record):
    """use_fused_kernel=False, use_flash_attention=False: the rotation is x*C + (x@P)*S on the
    HIP backend's generic kernels and the attention the plain composition."""
    mt, hip = world["minitorch"], world["hip"]
    np.random.seed(1)
    lm = mt.DecoderLM(backend=hip, pos_encoding="rope", **dict(KW, use_fused_kernel=False, use_flash_attention=False))
    _copy_params(mt, world["lm_h"], lm, hip)
    lm.eval()
    worst = 0.0
    for s, ref in zip(world["prompts"], world["cpu_logits"]):
        full = ref.shape[0]
        seq = s + world["cpu_new"][world["prompts"].index(s)]
        assert len(seq) == full
        worst = max(worst, float(np.abs(_forward(mt, lm, hip, seq) - ref).max()))
    print(f"tensor-op form on HIP: worst |dlogit| {worst:.3e}, tolerance {world['tol']:.3e}")
    parity_record("test_rope_full_forward", "tensor-op form + plain attention", max_abs=worst, bound=world["tol"])
    assert worst <= world["tol"]


@pytest.mark.parametrize("chunk", [1, 3])
def test_teacher_forced_logits_through_the_cache(world, chunk, parity_record):
    mt, hip, lm = world["minitorch"], world["hip"], world["lm_h"]
    prompts, cpu_new, ref, tol = world["prompts"], world["cpu_new"], world["cpu_logits"], world["tol"]
    B = len(prompts)
    idx, lens = _padded(prompts)
    cache = lm.new_cache(B)
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=lens.astype(np.float32), cache=cache).to_numpy()
    worst = max(float(np.abs(logits[b, :lens[b]] - ref[b][:lens[b]]).max()) for b in range(B))
    s = 0
    while s < NEW:
        T = min(chunk, NEW - s)
        step = np.array([t[s:s + T] for t in cpu_new], np.float32)
        logits = lm(mt.tensor_from_numpy(step, hip), cache=cache).to_numpy()
        assert logits.shape == (B, T, KW["n_vocab"])
        for b in range(B):
            worst = max(worst, float(np.abs(logits[b] - ref[b][lens[b] + s:lens[b] + s + T]).max()))
        s += T
    assert list(cache.length.cpu().numpy()) == list(lens + NEW)
    print(f"chunk {chunk}: worst |dlogit| {worst:.3e}, tolerance {tol:.3e}")
    parity_record("test_rope_teacher_forced_through_the_cache", f"chunk={chunk}", max_abs=worst, bound=tol)
    assert worst <= tol


def test_extend_steps_ragged_with_the_position_clamp(world, parity_record):
    """Extend steps with ragged kv_len on rows that fill all 48 positions. Row 0 is held at 44
    and gets 4 real tokens in a step of T = 8: its padding slots would sit at 48 .. 51 and take
    the last table row (the clamp); row 1 gets no token in that step (kv_len = 0)."""
    mt, hip, lm = world["minitorch"], world["hip"], world["lm_h"]
    seqs, ref, tol = world["long"], world["long_logits"], world["tol"]
    B, n_pos = len(seqs), KW["n_positions"]
    held = np.array([44, 10, 20])
    cache = lm.new_cache(B)
    idx = np.zeros((B, int(held.max())), np.float32)
    for b in range(B):
        idx[b, :held[b]] = seqs[b][:held[b]]
    logits = lm(mt.tensor_from_numpy(idx, hip), kv_len=held.astype(np.float32), cache=cache).to_numpy()
    worst = max(float(np.abs(logits[b, :held[b]] - ref[b][:held[b]]).max()) for b in range(B))
    for cnt, T in (([4, 0, 8], 8), ([0, 13, 5], 13), ([0, 9, 15], 15)):
        cnt = np.array(cnt)
        assert ((held + cnt) <= n_pos).all()
        step = np.zeros((B, T), np.float32)
        for b in range(B):
            step[b, :cnt[b]] = seqs[b][held[b]:held[b] + cnt[b]]
        logits = lm(mt.tensor_from_numpy(step, hip), kv_len=cnt.astype(np.float32), cache=cache).to_numpy()
        assert logits.shape == (B, T, KW["n_vocab"])
        assert np.isfinite(logits).all(), "logits at padding slots must be finite"
        for b in range(B):
            if cnt[b]:
                worst = max(worst, float(np.abs(logits[b, :cnt[b]] - ref[b][held[b]:held[b] + cnt[b]]).max()))
        held = held + cnt
        assert list(cache.length.cpu().numpy()) == list(held)
    assert list(held) == [48, 32, 48]
    print(f"extend steps: worst |dlogit| {worst:.3e}, tolerance {tol:.3e}")
    parity_record("test_rope_extend_steps", "ragged, kv_len=0 row, clamp at 44+8", max_abs=worst, bound=tol)
    assert worst <= tol


def test_generate_greedy_every_mode(world):
    lm, prompts, cpu_new = world["lm_h"], world["prompts"], world["cpu_new"]
    assert lm.generate(prompts, NEW, use_cache=False) == cpu_new, "uncached"
    assert lm.generate(prompts, NEW, use_cache=True) == cpu_new, "cached"
    assert lm.generate(prompts, NEW, graph=True) == cpu_new, "graph"
    assert lm.graph_captures >= 1
    assert lm.generate(prompts, NEW, prefill_chunk=4) == cpu_new, "prefill_chunk=4"
    assert lm.generate(prompts, NEW, page_size=16) == cpu_new, "page_size=16"
    assert lm.generate(prompts, NEW, page_size=16, graph=True) == cpu_new, "page_size=16, graph"
    kw = dict(temperature=0.9, top_k=20, seed=77)
    want = lm.generate(prompts, NEW, **kw)
    assert all(len(t) == NEW for t in want)
    assert lm.generate(prompts, NEW, graph=True, **kw) == want, "sampled, graph"
    lm.drop_decode_graphs()


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_generate_quantised_caches_run(world, kv_dtype):
    lm, prompts = world["lm_h"], world["prompts"]
    out = lm.generate(prompts, NEW, kv_dtype=kv_dtype)
    assert [len(t) for t in out] == [NEW] * len(prompts)
    assert all(0 <= t < KW["n_vocab"] for row in out for t in row)


def test_generate_grouped_query(world):
    mt, hip = world["minitorch"], world["hip"]
    np.random.seed(2)
    lm = mt.DecoderLM(backend=hip, pos_encoding="rope", n_kv_head=2, **KW)
    lm.eval()
    assert lm.n_kv_head == 2 and lm.n_head == 4
    prompts = world["prompts"]
    plain = lm.generate(prompts, NEW, use_cache=False)
    assert all(len(t) == NEW for t in plain)
    assert lm.generate(prompts, NEW, use_cache=True) == plain


def _training_setup(minitorch, backend, seed=0):
    np.random.seed(seed)
    B, T, V = 4, 12, 50
    lm = minitorch.DecoderLM(n_vocab=V, n_embd=32, n_head=4, n_positions=T, p_dropout=0.0, backend=backend,
                             use_fused_kernel=True, use_flash_attention=True, n_layer=1, pos_encoding="rope")
    rng = np.random.default_rng(1)
    tok = rng.integers(0, V, size=(B, T + 1)).astype(np.float32)
    kv = np.array([12, 7, 9, 1], dtype=np.int64)
    w = (np.arange(T)[None, :] < kv[:, None]).astype(np.float32)
    x = minitorch.tensor_from_numpy(tok[:, :-1].copy(), backend)
    y = minitorch.tensor_from_numpy(tok[:, 1:].reshape(-1).copy(), backend)
    wt = minitorch.tensor_from_numpy(w.reshape(-1).copy(), backend)

    def loss_fn():
        logits = lm(x, kv_len=kv).view(B * T, V)
        return (minitorch.softmax_loss(logits, y) * wt).sum() / wt.sum()
    return lm, loss_fn


def test_training_step_gradients_match_the_cpu_twin(world, parity_record):
    """One forward and backward of a one-layer rotary DecoderLM (n_embd 32, 4 heads, T = 12,
    ragged kv_len): every parameter gradient within atol = rtol = 1e-5 of the CPU twin's, whose
    rotation is differentiated by autodiff through the tensor-op form."""
    mt, hip, cpu = world["minitorch"], world["hip"], world["cpu"]
    lm_h, loss_h = _training_setup(mt, hip)
    lm_c, loss_c = _training_setup(mt, cpu)
    _copy_params(mt, lm_h, lm_c, cpu)
    lh, lc = loss_h(), loss_c()
    lh.backward()
    lc.backward()
    assert abs(lh.item() - lc.item()) <= 1e-5 * abs(lc.item())
    ph, pc = dict(lm_h.named_parameters()), dict(lm_c.named_parameters())
    worst = 0.0
    for name in ph:
        a, b = ph[name].value.grad, pc[name].value.grad
        assert a is not None and b is not None, name
        a, b = a.to_numpy(), b.to_numpy()
        ratio = float((np.abs(a - b) / (1e-5 + 1e-5 * np.abs(b))).max())
        worst = max(worst, ratio)
        print(f"{name}: max|dgrad| {float(np.abs(a - b).max()):.3e}, error / (atol + rtol |ref|) {ratio:.3f}")
    parity_record("test_rope_training_step", "n_embd=32 H=4 T=12 ragged", max_ratio=worst, bound=1.0)
    for name in ph:
        np.testing.assert_allclose(ph[name].value.grad.to_numpy(), pc[name].value.grad.to_numpy(),
                                   atol=1e-5, rtol=1e-5, err_msg=name)


def test_training_step_graph_matches_eager_bitwise(world):
    import torch
    mt, hip = world["minitorch"], world["hip"]
    from minitorch.graphs import StepGraph
    warmup, replays = 2, 3

    def run(graph):
        lm, loss_fn = _training_setup(mt, hip)
        opt = mt.Adam(lm.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            loss = loss_fn()
            loss.backward()
            opt.step()
            return loss
        np.random.seed(123)
        losses = []
        if graph:
            g = StepGraph(step, warmup=warmup)
            for _ in range(replays):
                loss = g.replay()
                torch.cuda.synchronize()
                losses.append(float(loss.to_numpy()[0]))
        else:
            for _ in range(warmup + replays):
                losses.append(float(step().to_numpy()[0]))
            losses = losses[warmup:]
        torch.cuda.synchronize()
        return losses, [p.value.to_numpy().copy() for p in lm.parameters()]
    eager_losses, eager_params = run(False)
    graph_losses, graph_params = run(True)
    assert graph_losses == eager_losses, (graph_losses, eager_losses)
    for a, b in zip(eager_params, graph_params):
        np.testing.assert_array_equal(a, b)
