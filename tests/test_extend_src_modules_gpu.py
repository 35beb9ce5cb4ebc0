"""Extend steps on a paged and on a quantised KV cache through KVCache / PagedKVCache,
MultiHeadAttention and DecoderLM on the HIP backend: the extend kernel reads the cache in place
(mt_flash_attn_extend_paged / mt_flash_attn_extend_kvq), so no step calls the gather or the
dequantising copy and no cache holds a scratch.

Model: V = 97, E = 64, 4 heads (d = 16), 2 layers, n_positions = 48, also with n_kv_head = 2.

Every comparison is between two runs of the same step shapes on the same weights, so the GEMMs
around the attention see the same operands; the direct kernels return the bits of the plain fp32
kernel on the same rows, and so the logits are compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LAYER = 2
KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True, n_layer=N_LAYER)
NEW = 12
P = 16
KV_DTYPES = ["bf16", "fp8"]
SHARED = 32


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
    toks = lambda n: [int(t) for t in rng.integers(0, KW["n_vocab"], n)]  # noqa: E731
    return dict(minitorch=minitorch, hip=hip, lm=lm, prompts=[toks(n) for n in (3, 9, 14)], torch=torch, _hip=_hip,
                full=[toks(n) for n in (40, 33, 47)], recycle=dict(a=toks(17), b=toks(8), c=toks(11)),
                shared=[toks(SHARED)] * 3, tails=[toks(9), toks(9), toks(9)])


@pytest.fixture(scope="module", params=[None, 2], ids=["mha", "gqa2"])
def world(request):
    w = _world(request.param)
    yield w
    w["lm"].drop_decode_graphs()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _feed(w, cache, step, kv_len=None):
    mt, hip, lm = w["minitorch"], w["hip"], w["lm"]
    kw = {} if kv_len is None else dict(kv_len=np.asarray(kv_len, np.float32))
    return lm(mt.tensor_from_numpy(np.asarray(step, np.float32), hip), cache=cache, **kw).to_numpy()


def _prefill(w, cache, seqs, lens=None):
    lens = np.array([len(s) for s in seqs]) if lens is None else np.asarray(lens)
    idx = np.zeros((len(seqs), int(lens.max())), np.float32)
    for b, s in enumerate(seqs):
        idx[b, :lens[b]] = s[:lens[b]]
    out = _feed(w, cache, idx, kv_len=lens)
    assert list(cache.length_host) == list(lens)
    return out


def _ragged_steps(w, caches, check):
    """Teacher-forced extend steps of ragged counts (9, 0, 13) rotating over the rows, after a 5-token
    prefill, on every cache of `caches` in turn; check(step index, counts, logits per cache)."""
    full = w["full"]
    B = len(full)
    total = np.array([len(s) for s in full])
    first = np.full(B, 5)
    check(-1, first, [_prefill(w, c, full, first) for c in caches])
    fed, k, pattern = first.copy(), 0, (9, 0, 13)
    while (fed < total).any():
        cnt = np.minimum(np.array([pattern[(b + k) % 3] for b in range(B)]), total - fed)
        T = max(int(cnt.max()), 1)
        step = np.zeros((B, T), np.float32)
        for b in range(B):
            step[b, :cnt[b]] = full[b][fed[b]:fed[b] + cnt[b]]
        check(k, cnt, [_feed(w, c, step, kv_len=cnt) for c in caches])
        fed = fed + cnt
        k += 1
        for c in caches:
            assert list(c.length_host) == list(fed) and list(c.length.cpu().numpy()) == list(fed)
        assert k < 64
    assert k >= 4
    return k


def _no_scratch(w, cache):
    """The cache holds nothing but what nbytes counts."""
    torch, mt = w["torch"], w["minitorch"]
    assert not hasattr(cache, "scratch") and not hasattr(cache, "_scratch")
    from minitorch.hip_kernel_ops import _torch_view
    held = 0
    for name, val in vars(cache).items():
        if name in ("length", "layers", "_workspaces", "_visible"):
            continue
        assert not isinstance(val, (torch.Tensor, mt.Tensor)) or name == "block_table", f"{name} holds device memory"
    for lkv in cache.layers:
        assert set(vars(lkv)) == {"cache", "k", "v", "k_scale", "v_scale"}
        for t in (lkv.k, lkv.v, lkv.k_scale, lkv.v_scale):
            if t is not None:
                t = _torch_view(t) if isinstance(t, mt.Tensor) else t
                held += t.numel() * t.element_size()
    if cache.paged:
        held += cache.block_table.numel() * 4
    assert held == cache.nbytes


def _raise(name):
    def fn(*a, **k):
        raise AssertionError(f"{name} was called: the extend step must read the cache in place")
    return fn


def _two_launch_kvq(w):
    """flash_attention_extend_kvq as the two launches it replaces: the dequantising copy into an fp32
    pair, then the plain fp32 extend kernel (the library calls, not the backend's patched attributes)."""
    torch, _hip, hip = w["torch"], w["_hip"], w["hip"]
    from minitorch.hip_kernel_ops import HipKernelOps, _torch_view

    def fn(q, kc, vc, k_scale, v_scale, kv_len, q_len, causal=True):
        kv = HipKernelOps._i32(kv_len)
        kf, vf = (torch.full(tuple(kc.shape), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
        _hip.kv_cache_dequant(kc, vc, k_scale, v_scale, kv_len=kv, k_out=kf, v_out=vf)
        o, _, _ = _hip.flash_extend(_torch_view(q).contiguous(), kf, vf, kv_len=kv, q_len=HipKernelOps._i32(q_len),
                                    causal=causal)
        return w["minitorch"].tensor_from_numpy(o.cpu().numpy(), hip)
    return fn


def test_gather_and_dequant_are_not_called(world, monkeypatch):
    """With kv_cache_gather_paged and kv_cache_dequant patched to raise, ragged extend steps and
    chunked-prefill generation still run on a paged and on a quantised cache and return the ids of
    the unpatched contiguous fp32 model (with this model's weights the quantisation moves no argmax).
    Paged: the logits are the contiguous cache's too. Quantised: the ids are also those of the same
    generation with the extend step done as dequant + plain extend, which is exact."""
    w = world
    lm, hip, prompts = w["lm"], w["hip"], w["prompts"]
    want = lm.generate(prompts, NEW)
    want_chunked = {c: lm.generate(prompts, NEW, prefill_chunk=c) for c in (4, 9)}
    assert all(v == want for v in want_chunked.values())
    # the quantised ids with the extend step as the two launches it replaces, before anything is patched to raise
    two = {}
    monkeypatch.setattr(hip, "flash_attention_extend_kvq", _two_launch_kvq(w))
    for kv_dtype in KV_DTYPES:
        for c in (4, 9):
            two[kv_dtype, c] = lm.generate(prompts, NEW, prefill_chunk=c, kv_dtype=kv_dtype)
    monkeypatch.undo()

    monkeypatch.setattr(hip, "kv_cache_gather_paged", _raise("kv_cache_gather_paged"))
    monkeypatch.setattr(hip, "kv_cache_dequant", _raise("kv_cache_dequant"))
    B = len(w["full"])
    caches = [lm.new_cache(B, page_size=P), lm.new_cache(B)] + [lm.new_cache(B, kv) for kv in KV_DTYPES]

    def check(k, cnt, logits):
        assert all(np.isfinite(x).all() for x in logits)
        ids = [x.argmax(-1) for x in logits]
        for b in range(B):
            assert np.array_equal(_bits(logits[0][b, :cnt[b]]), _bits(logits[1][b, :cnt[b]])), f"paged, step {k}, row {b}"
            assert np.array_equal(ids[0][b, :cnt[b]], ids[1][b, :cnt[b]])
            for kv, x in zip(KV_DTYPES, ids[2:]):
                moved[kv] += int((x[b, :cnt[b]] != ids[1][b, :cnt[b]]).sum())
    moved = dict.fromkeys(KV_DTYPES, 0)
    _ragged_steps(w, caches, check)
    print(f"ragged extend steps: ids that differ from the fp32 cache's {moved}")
    assert not any(moved.values()), "the ids of the contiguous fp32 model"
    for chunk in (4, 9):
        assert lm.generate(prompts, NEW, prefill_chunk=chunk, page_size=P) == want, f"eager, chunk {chunk}"
        assert lm.generate(prompts, NEW, prefill_chunk=chunk, page_size=P, graph=True) == want, f"graph, chunk {chunk}"
        for kv_dtype in KV_DTYPES:
            got = lm.generate(prompts, NEW, prefill_chunk=chunk, kv_dtype=kv_dtype)
            assert got == two[kv_dtype, chunk], f"{kv_dtype}, chunk {chunk}: differs from dequant + extend"
            assert lm.generate(prompts, NEW, prefill_chunk=chunk, kv_dtype=kv_dtype, graph=True) == got
            same = sum(a == b for x, y in zip(got, want) for a, b in zip(x, y))
            print(f"{kv_dtype}, chunk {chunk}: {same} of {NEW * len(prompts)} ids are the fp32 cache's")
            assert got == want, f"{kv_dtype}, chunk {chunk}: the ids of the contiguous fp32 model"
    lm.drop_decode_graphs()
    for c in caches:
        _no_scratch(w, c)


def test_paged_extend_steps_are_bit_equal_to_the_contiguous_cache(world):
    w = world
    lm = w["lm"]
    B = len(w["full"])
    paged, plain = lm.new_cache(B, page_size=P), lm.new_cache(B)

    def check(k, cnt, logits):
        a, b = logits
        for r in range(B):
            assert np.array_equal(_bits(a[r, :cnt[r]]), _bits(b[r, :cnt[r]])), f"step {k}, row {r}, counts {cnt}"
        # the pages follow the tokens: the padding columns took none
    steps = _ragged_steps(w, [paged, plain], check)
    assert steps >= 4
    assert [(row >= 0).sum() for row in paged.table_host] == [-(-int(n) // P) for n in paged.length_host]
    _no_scratch(w, paged)


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


def _step_both(w, monkeypatch, cq, step, kv_len):
    """The step on the quantised cache, then on its fp32 mirror with the append replaced by a copy
    of the quantised cache's (already appended) rows of the same layer."""
    from minitorch.hip_kernel_ops import _torch_view
    hip, _hip = w["hip"], w["_hip"]
    cf = _mirror(w, cq)
    got = _feed(w, cq, step, kv_len)
    layer_of = {_torch_view(l.k).data_ptr(): i for i, l in enumerate(cf.layers)}
    calls = []

    def rounded_append(knew, vnew, kc, vc, pos):
        lq = cq.layers[layer_of[_torch_view(kc).data_ptr()]]
        calls.append(1)
        _hip.kv_cache_dequant(lq.k, lq.v, lq.k_scale, lq.v_scale, kv_len=cq.length,
                              k_out=_torch_view(kc), v_out=_torch_view(vc))
    monkeypatch.setattr(hip, "kv_cache_append", rounded_append)
    want = _feed(w, cf, step, kv_len)
    monkeypatch.undo()
    assert len(calls) == N_LAYER
    assert list(cf.length_host) == list(cq.length_host)
    return got, want


@pytest.mark.parametrize("kv_dtype", KV_DTYPES)
def test_quantised_extend_steps_are_bit_equal_to_the_fp32_mirror(world, kv_dtype, monkeypatch):
    """An extend step on a quantised cache against the same step on an fp32 cache holding the
    dequantised rows (the new tokens' rows included): the kernel stages the same fp32 values, so the
    logits of the real tokens are equal bit for bit."""
    w = world
    lm, full = w["lm"], w["full"]
    B = len(full)
    cq = lm.new_cache(B, kv_dtype)
    _prefill(w, cq, full, np.full(B, 5))
    fed = np.full(B, 5)
    for k, cnt in enumerate(([9, 0, 13], [13, 9, 0], [0, 13, 9], [9, 6, 13])):
        cnt = np.array(cnt)
        step = np.zeros((B, int(cnt.max())), np.float32)
        for b in range(B):
            step[b, :cnt[b]] = full[b][fed[b]:fed[b] + cnt[b]]
        got, want = _step_both(w, monkeypatch, cq, step, cnt)
        assert np.isfinite(got).all()
        for b in range(B):
            assert np.array_equal(_bits(got[b, :cnt[b]]), _bits(want[b, :cnt[b]])), f"{kv_dtype} step {k}, row {b}"
        fed = fed + cnt
        assert list(cq.length_host) == list(fed)
    _no_scratch(w, cq)


def test_row_recycling_through_an_extend_step(world):
    """free_row(1), then a new prompt enters row 1 through an extend step with counts [0, 7] while row
    0 goes on: the logits are those of a contiguous cache whose row 1 was set back to length 0."""
    w = world
    lm = w["lm"]
    a, b, c = (w["recycle"][k] for k in "abc")

    def run(cache):
        _prefill(w, cache, [a[:9], b[:5]])
        for i in range(3):
            _feed(w, cache, [[a[9 + i]], [b[5 + i]]])
        assert list(cache.length_host) == [12, 8]
        if cache.paged:
            free = cache.pages_free
            cache.free_row(1)
            assert cache.pages_free == free + 1 and (cache.block_table.cpu().numpy()[1] == -1).all()
        else:
            cache.set_length([12, 0])
        assert list(cache.length_host) == [12, 0]
        step = np.zeros((2, 9), np.float32)
        step[0, :2] = a[12:14]
        step[1] = c[:9]
        outs = [_feed(w, cache, step, kv_len=[2, 9])]
        assert list(cache.length_host) == [14, 9]
        for i in range(2):
            outs.append(_feed(w, cache, [[a[14 + i]], [c[9 + i]]]))
        return outs
    got, want = run(lm.new_cache(2, page_size=P)), run(lm.new_cache(2))
    assert np.array_equal(_bits(got[0][0, :2]), _bits(want[0][0, :2])), "row 0 in the recycling step"
    assert np.array_equal(_bits(got[0][1]), _bits(want[0][1])), "the new prompt in row 1"
    for x, y in zip(got[1:], want[1:]):
        assert np.array_equal(_bits(x), _bits(y)), "the decode steps after it"


def test_prefix_sharing_extend_steps_leave_the_shared_pages(world):
    """After share_prefix the rows take different 9-token continuations in one extend step: the shared
    pages' bytes are unchanged, and the logits are those of a contiguous cache fed the same tokens."""
    w = world
    lm, seqs, tails = w["lm"], w["shared"], w["tails"]
    cache, plain = lm.new_cache(3, page_size=P), lm.new_cache(3)
    a, b = _prefill(w, cache, seqs), _prefill(w, plain, seqs)
    assert np.array_equal(_bits(a), _bits(b))
    cache.share_prefix(0, [1, 2], SHARED)
    t = cache.table_host.copy()
    assert (t[1, :2] == t[0, :2]).all() and (t[2, :2] == t[0, :2]).all()
    shared_pages = [int(p) for p in t[0, :2]]
    assert all(cache.refcount(p) == 3 for p in shared_pages)

    def pages():
        return [x[p].cpu().numpy().copy() for lkv in cache.layers for x in (lkv.k, lkv.v) for p in shared_pages]
    before = pages()
    cnt = [9, 4, 7]
    step = np.zeros((3, 9), np.float32)
    for r in range(3):
        step[r, :cnt[r]] = tails[r][:cnt[r]]
    got, want = _feed(w, cache, step, kv_len=cnt), _feed(w, plain, step, kv_len=cnt)
    for r in range(3):
        assert np.array_equal(_bits(got[r, :cnt[r]]), _bits(want[r, :cnt[r]])), f"row {r}"
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, pages())), \
        "a page with more than one reference was written"
    assert (cache.table_host[:, :2] == t[:, :2]).all() and (cache.table_host[:, 2] >= 0).all()
    assert len(set(cache.table_host[:, 2].tolist())) == 3
    _no_scratch(w, cache)
