"""The paged KV cache through PagedKVCache, MultiHeadAttention and DecoderLM on the HIP backend.

Model: V = 97, E = 64, 4 heads (d = 16), n_positions = 48 = 3 pages of 16, also with n_kv_head = 2;
ragged batches. A decode step through pages is the contiguous cache's, bit for bit (the same plan,
the same arithmetic). Extend steps go through the gather and a contiguous scratch; their logits
are held to the rule of tests/test_extend_modules_gpu.py: within the larger of 1e-5 max|logit| and
twice the deviation the full HIP forward (no cache) shows from the CPU model on the same sequences.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_vocab=97, n_embd=64, n_head=4, n_positions=48, p_dropout=0.0, use_fused_kernel=True,
          use_flash_attention=True)
NEW = 16
P = 16
SHARED = 40  # the prompt the three rows of the prefix-sharing tests have in common


def _world(n_kv_head, with_cpu):
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
    prompts = [toks(n) for n in (3, 9, 14)]
    w = dict(minitorch=minitorch, hip=hip, lm=lm, prompts=prompts, torch=torch, _hip=_hip)
    base = toks(SHARED)
    w["shared"] = [base + toks(4) for _ in range(3)]
    w["recycle"] = dict(a=toks(17), b=toks(8), c=toks(11))
    if not with_cpu:
        return w
    from cpu_backend import NumpyOps
    cpu = minitorch.TensorBackend(NumpyOps)
    lm_c = minitorch.DecoderLM(backend=cpu, **kw)
    ph, pc = dict(lm.named_parameters()), dict(lm_c.named_parameters())
    assert ph.keys() == pc.keys()
    for name, p in ph.items():
        pc[name].update(minitorch.tensor_from_numpy(p.value.to_numpy().copy(), cpu))
    lm_c.eval()
    cpu_new = lm_c.generate(prompts, NEW, use_cache=False)
    full = [p + t for p, t in zip(prompts, cpu_new)]
    seqs = full + w["shared"] + list(w["recycle"].values())

    def forward(m, backend, seq):
        return m(minitorch.tensor_from_numpy(np.asarray([seq], dtype=np.float32), backend)).to_numpy()[0]
    cpu_logits = [forward(lm_c, cpu, s) for s in seqs]
    hip_logits = [forward(lm, hip, s) for s in seqs]
    scale = max(float(np.abs(x).max()) for x in cpu_logits)
    dev = max(float(np.abs(a - b).max()) for a, b in zip(hip_logits, cpu_logits))
    tol = max(1e-5 * scale, 2.0 * dev)
    gap = min(float(np.diff(np.sort(x[len(p) - 1:len(p) - 1 + NEW], axis=-1)[:, -2:], axis=-1).min())
              for x, p in zip(cpu_logits, prompts))
    print(f"max|logit| {scale:.3f}; full HIP forward vs CPU {dev:.3e}; tolerance {tol:.3e}; top-2 gap {gap:.3e}")
    assert gap > 10 * tol, "the seeds give a near-tie: choose others"
    w.update(cpu_new=cpu_new, full=full, cpu_logits=cpu_logits[:len(full)], tol=tol)
    return w


@pytest.fixture(scope="module")
def world():
    w = _world(None, True)
    yield w
    w["lm"].drop_decode_graphs()


@pytest.fixture(scope="module")
def world_gqa():
    w = _world(2, False)
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
    assert list(cache.length_host) == list(lens) and list(cache.length.cpu().numpy()) == list(lens)
    return out


def _pages(cache, pages):
    """The bytes of the given pages in every layer's K and V pool."""
    return [t[int(p)].cpu().numpy().copy() for lkv in cache.layers for t in (lkv.k, lkv.v) for p in pages]


@pytest.mark.parametrize("which", ["mha", "gqa2"])
def test_teacher_forced_decode_equals_the_contiguous_cache_bit_for_bit(world, world_gqa, which):
    w = world if which == "mha" else world_gqa
    lm, prompts = w["lm"], w["prompts"]
    assert lm.n_kv_head == (4 if which == "mha" else 2)
    B = len(prompts)
    paged, plain = lm.new_cache(B, page_size=P), lm.new_cache(B)
    assert paged.paged and not plain.paged and paged.width * P == plain.n_positions
    assert paged.pages_free == B * 3 and (paged.block_table.cpu().numpy() == -1).all()
    a, b = _prefill(w, paged, prompts), _prefill(w, plain, prompts)
    assert np.array_equal(_bits(a), _bits(b)), "prefill"
    # the pages follow the tokens held: ceil(len / 16) per row
    assert paged.pages_free == B * 3 - 3
    rng = np.random.default_rng(1)
    for width in (1, 1, 4, 1, 4, 4, 1, 1, 1):  # 18 tokens: row 2 passes both page edges (14 -> 32)
        step = rng.integers(0, KW["n_vocab"], (B, width)).astype(np.float32)
        a, b = _feed(w, paged, step), _feed(w, plain, step)
        assert a.shape == (B, width, KW["n_vocab"])
        assert np.array_equal(_bits(a), _bits(b)), f"a step of {width} at lengths {plain.length_host - width}"
        assert list(paged.length_host) == list(plain.length_host)
        assert list(paged.length.cpu().numpy()) == list(plain.length_host)
    assert list(paged.length_host) == [21, 27, 32]
    table = paged.block_table.cpu().numpy()
    assert np.array_equal(table, paged.table_host)
    assert [(row >= 0).sum() for row in table] == [2, 2, 2] and paged.pages_free == 3
    used = table[table >= 0]
    assert len(set(used.tolist())) == len(used) and all(paged.refcount(p) == 1 for p in used)


@pytest.mark.parametrize("which", ["mha", "gqa2"])
def test_generate_forms_agree(world, world_gqa, which):
    w = world if which == "mha" else world_gqa
    lm, prompts = w["lm"], w["prompts"]
    greedy = lm.generate(prompts, NEW)
    if "cpu_new" in w:
        assert greedy == w["cpu_new"]
    assert lm.generate(prompts, NEW, page_size=P) == greedy
    captures = lm.graph_captures or 0
    assert lm.generate(prompts, NEW, page_size=P, graph=True) == greedy
    assert lm.graph_captures == captures + 1
    assert lm.generate(prompts, NEW, page_size=P, graph=True) == greedy
    assert lm.graph_captures == captures + 1, "a second call replays the held graph"
    kw = dict(temperature=0.8, top_k=5, seed=7)
    sampled = lm.generate(prompts, NEW, **kw)
    assert lm.generate(prompts, NEW, page_size=P, **kw) == sampled
    assert lm.generate(prompts, NEW, page_size=P, graph=True, **kw) == sampled
    # a row that fills the cache: the budget stops at n_positions, the last slot is re-written
    long = [prompts[2] + prompts[1] + prompts[2], prompts[0]]
    assert len(long[0]) == 37
    want = lm.generate(long, NEW)
    assert [len(t) for t in want] == [12, 16]
    assert lm.generate(long, NEW, page_size=P) == want
    assert lm.generate(long, NEW, page_size=P, graph=True) == want
    lm.drop_decode_graphs()


@pytest.mark.parametrize("new", [1, 2, 3])
def test_graph_capture_with_few_new_tokens(world, new):
    """Capturing the step runs two warm-up steps and the captured one whatever max_new_tokens: with
    prompts of 14 and 30 tokens and P = 16, len + 2 ends a page exactly, so a pool sized to
    len + max_new_tokens alone would lack the page of the third step. The graph path budgets it."""
    lm = world["lm"]
    rng = np.random.default_rng(9)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (14, 30)]
    want = lm.generate(prompts, new)
    assert [len(t) for t in want] == [new, new]
    lm.drop_decode_graphs()
    captures = lm.graph_captures or 0
    assert lm.generate(prompts, new, page_size=P, graph=True) == want
    assert lm.graph_captures == captures + (1 if new > 1 else 0)
    assert lm.generate(prompts, new, page_size=P) == want
    if new > 1:
        (entry,) = lm._decode_graphs.values()
        cache = entry["state"].cache
        # the table was final before the capture: every page of the budget reserved, none taken later
        assert cache.n_pages == sum(-(-(n + 3) // P) for n in (14, 30)) == 5 and cache.pages_free == 0
    lm.drop_decode_graphs()


def test_prefill_chunk_and_extend_steps_through_the_gather(world):
    """Multi-turn extend steps (ragged counts, a row with none) on a paged cache against the CPU
    model's logits, and generate(prefill_chunk=...) with pages, eager and graph."""
    w = world
    lm, full, ref, tol = w["lm"], w["full"], w["cpu_logits"], w["tol"]
    B = len(full)
    total = np.array([len(s) for s in full])
    cache = lm.new_cache(B, page_size=P)
    first = 5
    logits = _prefill(w, cache, full, np.full(B, first))
    worst = max(float(np.abs(logits[b] - ref[b][:first]).max()) for b in range(B))
    fed = np.full(B, first)
    pattern, k = (9, 0, 13), 0
    while (fed < total).any():
        cnt = np.minimum(np.array([pattern[(b + k) % 3] for b in range(B)]), total - fed)
        k += 1
        T = max(int(cnt.max()), 1)
        step = np.zeros((B, T), np.float32)
        for b in range(B):
            step[b, :cnt[b]] = full[b][fed[b]:fed[b] + cnt[b]]
        logits = _feed(w, cache, step, kv_len=cnt)
        assert np.isfinite(logits).all(), "logits at padding slots must be finite"
        for b in range(B):
            if cnt[b]:
                worst = max(worst, float(np.abs(logits[b, :cnt[b]] - ref[b][fed[b]:fed[b] + cnt[b]]).max()))
        fed = fed + cnt
        assert list(cache.length_host) == list(fed) and list(cache.length.cpu().numpy()) == list(fed)
        # the pages follow the tokens: the padding columns took none
        assert [(row >= 0).sum() for row in cache.table_host] == [-(-int(n) // P) for n in fed]
        assert k < 64
    print(f"extend steps through the gather: worst |dlogit| {worst:.3e}, tolerance {tol:.3e}, {k} steps")
    assert worst <= tol
    prompts, cpu_new = w["prompts"], w["cpu_new"]
    for chunk in (4, 9):
        assert lm.generate(prompts, NEW, prefill_chunk=chunk, page_size=P) == cpu_new, f"eager, chunk {chunk}"
        assert lm.generate(prompts, NEW, prefill_chunk=chunk, page_size=P, graph=True) == cpu_new, f"graph, chunk {chunk}"
    lm.drop_decode_graphs()


def test_memory_follows_the_tokens(monkeypatch):
    """Prompts of (200, 8, 8, 8) tokens, 8 new tokens, P = 16: the pool holds sum ceil((len + 8) / 16)
    = 13 + 1 + 1 + 1 pages, all of them reserved, against 4 x 256 rows of a contiguous cache."""
    import minitorch
    from minitorch import _hip
    _hip.lib()
    hip = minitorch.TensorBackend(minitorch.HipKernelOps)
    np.random.seed(1)
    lm = minitorch.DecoderLM(backend=hip, **dict(KW, n_positions=256, n_layer=2))
    lm.eval()
    rng = np.random.default_rng(2)
    prompts = [[int(t) for t in rng.integers(0, KW["n_vocab"], n)] for n in (200, 8, 8, 8)]
    made = []
    new_cache = lm.new_cache

    def recording(*a, **k):
        made.append(new_cache(*a, **k))
        return made[-1]
    monkeypatch.setattr(lm, "new_cache", recording)
    want = lm.generate(prompts, 8)
    got = lm.generate(prompts, 8, page_size=P)
    assert got == want and [len(t) for t in got] == [8] * 4
    plain, paged = made
    assert paged.paged and not plain.paged
    pages = sum(-(-(len(p) + 8) // P) for p in prompts)
    assert pages == 16 and paged.n_pages == pages
    assert paged.pages_free == 0, "every row was reserved to its final length"
    assert [(row >= 0).sum() for row in paged.table_host] == [13, 1, 1, 1]
    d, Hkv = KW["n_embd"] // KW["n_head"], lm.n_kv_head
    assert paged.nbytes == 2 * 2 * pages * P * Hkv * d * 4 + 4 * 16 * 4
    assert plain.nbytes == 2 * 2 * 4 * 256 * Hkv * d * 4
    assert paged.nbytes < plain.nbytes
    held = sum(t.numel() * t.element_size() for lkv in paged.layers for t in (lkv.k, lkv.v))
    assert held + paged.block_table.numel() * 4 == paged.nbytes


def test_row_recycling(world):
    """Row 1 finishes, free_row(1) gives its pages back, and a new prompt enters row 1 through an
    extend step with kv_len = [0, t], while row 0 goes on undisturbed."""
    w = world
    lm, tol = w["lm"], w["tol"]
    a, b, c = (w["recycle"][k] for k in "abc")

    def run(replace):
        cache = lm.new_cache(2, page_size=P)
        _prefill(w, cache, [a[:9], b[:5]])
        for i in range(3):
            _feed(w, cache, [[a[9 + i]], [b[5 + i]]])
        assert list(cache.length_host) == [12, 8]
        row1 = []
        if replace:
            free, held = cache.pages_free, int((cache.table_host[1] >= 0).sum())
            assert held == 1
            cache.free_row(1)
            assert cache.pages_free == free + held
            assert list(cache.length_host) == [12, 0] and list(cache.length.cpu().numpy()) == [12, 0]
            assert (cache.block_table.cpu().numpy()[1] == -1).all()
            step = np.zeros((2, 7), np.float32)
            step[1] = c[:7]
            row1.append(_feed(w, cache, step, kv_len=[0, 7])[1])
            assert list(cache.length_host) == [12, 7]
        row0 = []
        for i in range(4):
            out = _feed(w, cache, [[a[12 + i]], [c[7 + i] if replace else b[i]]])
            row0.append(out[0])
            row1.append(out[1])
        return np.concatenate(row0), np.concatenate(row1)
    kept0, _ = run(False)
    got0, got1 = run(True)
    assert np.array_equal(_bits(got0), _bits(kept0)), "row 0 must not notice that row 1 was replaced"
    # a fresh one-row run of the new prompt on a contiguous cache
    fresh = lm.new_cache(1)
    want = [_prefill(w, fresh, [c[:7]])[0]]
    for i in range(4):
        want.append(_feed(w, fresh, [[c[7 + i]]])[0])
    want = np.concatenate(want)
    assert got1.shape == want.shape == (11, KW["n_vocab"])
    err = float(np.abs(got1 - want).max())
    print(f"recycled row against a fresh run: max |dlogit| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


def _shared_scenario(w, shorten):
    """Three rows prefilled with the same 40-token prompt, rows 1 and 2 then sharing row 0's pages;
    one 4-token step of different continuations; with `shorten`, row 1 is then cut back to 20 tokens
    (inside the shared second page) and every row takes one more token. Returns what was seen."""
    lm, seqs = w["lm"], w["shared"]
    cache = lm.new_cache(3, page_size=P)
    _prefill(w, cache, [s[:SHARED] for s in seqs])
    assert cache.pages_free == 0
    cache.share_prefix(0, [1, 2], SHARED)
    t = cache.table_host.copy()
    assert np.array_equal(cache.block_table.cpu().numpy(), t)
    assert list(cache.length_host) == [SHARED] * 3 and list(cache.length.cpu().numpy()) == [SHARED] * 3
    seen = dict(table=t, refs=[[cache.refcount(p) for p in row] for row in t], free=cache.pages_free)
    shared_pages = [t[0, 0], t[0, 1]]
    before = _pages(cache, shared_pages)
    seen["step"] = _feed(w, cache, [s[SHARED:] for s in seqs])
    after = _pages(cache, shared_pages)
    seen["shared_untouched"] = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, after))
    assert np.array_equal(cache.table_host, t), "appending into private pages takes none"
    if shorten:
        cache.set_length([44, 20, 44])
        seen["table2"] = cache.table_host.copy()
        seen["refs2"] = (cache.refcount(t[0, 1]), cache.refcount(cache.table_host[1, 1]))
        assert np.array_equal(cache.block_table.cpu().numpy(), cache.table_host)
    calls, make_room = [], cache._make_room
    cache._make_room = lambda *a: (calls.append(1), make_room(*a))[1]
    seen["last"] = _feed(w, cache, [[11.0], [22.0], [33.0]])
    del cache._make_room
    seen["make_room_calls"] = len(calls)
    seen["shared_untouched2"] = all(np.array_equal(x.view(np.uint32), y.view(np.uint32))
                                    for x, y in zip(before, _pages(cache, shared_pages)))
    return seen


def test_prefix_sharing(world):
    w = world
    lm, seqs, tol = w["lm"], w["shared"], w["tol"]
    s = _shared_scenario(w, shorten=True)
    t = s["table"]
    assert (t[1, :2] == t[0, :2]).all() and (t[2, :2] == t[0, :2]).all(), "the two full pages are shared"
    assert len({int(t[0, 2]), int(t[1, 2]), int(t[2, 2])}) == 3 and (t[:, 2] >= 0).all(), "the third is private"
    assert s["refs"] == [[3, 3, 1]] * 3
    assert s["free"] == 9 - 5
    assert s["shared_untouched"] and s["shared_untouched2"], "a page with more than one reference was written"
    assert s["make_room_calls"] == 1, "with shared pages only a step's first layer walks the table"
    # against an unshared contiguous cache fed the whole sequences
    plain = lm.new_cache(3)
    _prefill(w, plain, [q[:SHARED] for q in seqs])
    want = _feed(w, plain, [q[SHARED:] for q in seqs])
    err = float(np.abs(s["step"] - want).max())
    print(f"shared prefix against an unshared cache: max |dlogit| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    # set_length into the shared second page: row 1 got a private copy of it, the others kept theirs
    t2 = s["table2"]
    assert t2[1, 1] != t[0, 1] and t2[1, 0] == t[0, 0] and (t2[[0, 2]] == t[[0, 2]]).all()
    assert s["refs2"] == (2, 1)
    plain.set_length([44, 20, 44])
    want = _feed(w, plain, [[11.0], [22.0], [33.0]])
    err = float(np.abs(s["last"] - want).max())
    print(f"after set_length into a shared page: max |dlogit| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    # rows 0 and 2 are those of a run in which row 1 was never cut back
    kept = _shared_scenario(w, shorten=False)
    assert np.array_equal(_bits(s["step"]), _bits(kept["step"]))
    assert np.array_equal(_bits(s["last"][[0, 2]]), _bits(kept["last"][[0, 2]]))


def test_misuse_raises_before_any_launch(world):
    mt, lm, prompts, torch = world["minitorch"], world["lm"], world["prompts"], world["torch"]
    cache = lm.new_cache(2, page_size=P, n_pages=3)
    cache.reserve([16, 17])
    assert cache.pages_free == 0
    table, dev_table = cache.table_host.copy(), cache.block_table.clone()
    with pytest.raises(mt.PoolExhausted, match="exhausted"):
        cache.reserve([17, 17])
    assert np.array_equal(cache.table_host, table) and torch.equal(cache.block_table, dev_table)
    assert list(cache.length_host) == [0, 0] and list(cache.length.cpu().numpy()) == [0, 0]
    assert cache.pages_free == 0 and [cache.refcount(p) for p in range(3)] == [1, 1, 1]
    # through the model: the prefill of 20 + 20 tokens needs 4 pages, the pool has 3
    with pytest.raises(mt.PoolExhausted):
        _prefill(world, cache, [list(range(20)), list(range(20))])
    assert np.array_equal(cache.table_host, table) and list(cache.length_host) == [0, 0]
    with pytest.raises(ValueError, match="kv_dtype"):
        lm.generate(prompts, 4, page_size=P, kv_dtype="bf16")
    with pytest.raises(ValueError, match="kv_dtype"):
        lm.new_cache(2, "fp8", page_size=P)
    with pytest.raises(ValueError, match="power of two"):
        lm.generate(prompts, 4, page_size=24)
    with pytest.raises(ValueError, match="power of two"):
        lm.new_cache(2, page_size=8)
    with pytest.raises(ValueError, match="use_cache"):
        lm.generate(prompts, 4, page_size=P, use_cache=False)
