"""The paged KV-cache kernels on the GPU: mt_flash_attn_decode_paged, mt_kv_cache_append_paged and
mt_kv_cache_gather_paged (include/minitorch_hip.h).

Shapes: B = 2, H = 4 with Hkv in {4, 1}, logical capacity W * P = 512 keys, so the plan has several
splits. The pools are [n_pages, P, Hkv, d] storage seen as [n_pages, Hkv, P, d] (the model's
layout); pages are handed to the two rows in a shuffled order, interleaved; every table entry past
a row's last visible page names a poison page inside the pool that holds NaN, so a wrong read shows
as a NaN, never as a fault.

Decode is checked three ways: bit for bit against mt_flash_attn_decode_gqa on the contiguous
cache that holds the same rows (built on the host from the pool, and through
mt_kv_cache_gather_paged), against the float64 reference within decode_cases.bound, and for
independence of everything it must not read (NaN against zeros there)."""
import functools

import numpy as np
import pytest

import decode_cases as DC

pytestmark = pytest.mark.gpu

B, H, NK = 2, 4, 512
CODES = {"f32": 0, "bf16": 1, "bf16_f32out": 2}
SENT_BITS = 0x7FC12345  # a NaN with a payload: a footprint sentinel no kernel produces


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def _tin(torch, name):
    return torch.float32 if name == "f32" else torch.bfloat16


def _tout(torch, name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _bits(t):
    """A device tensor's bytes as a numpy integer array."""
    import torch
    it = {4: torch.int32, 2: torch.int16}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy()


def _plan(_hip, name, Hkv, nq, P, d):
    return _hip.decode_paged_splits(CODES[name], B, H, nq, NK // P, P, d, Hkv)


def _table(P, nvis, seed, shared=False):
    """(table [B, W] int32, n_pages, poison): shuffled pages, interleaved between the rows; entries
    past ceil(n / P) name the poison page. shared: row 1's first page is row 0's."""
    W = NK // P
    n_pages = B * W + 5  # the rows' pages, the poison page and four nobody references
    rng = np.random.default_rng([seed, P])
    perm = rng.permutation(n_pages)
    poison = int(perm[-1])
    table = np.empty((B, W), np.int32)
    for b in range(B):
        table[b] = perm[b:B * W:B]
    if shared:
        table[1, 0] = table[0, 0]
    for b in range(B):
        table[b, -(-int(nvis[b]) // P):] = poison
    return table, n_pages, poison


@functools.lru_cache(maxsize=None)
def _inputs(bf16, d, Hkv, nq, lengths):
    """q [B,H,nq,d], k / v [B,Hkv,NK,d] (decode_cases' boundary-sensitive values; the query heads of
    a group differ by a quarter-size noise), read-only."""
    q0, k, v = DC.make_inputs(d, nq, bf16, lengths, nmax=NK, heads=Hkv)
    G = H // Hkv
    q = np.repeat(q0, G, axis=1)
    if G > 1:
        from oracle import attention as A
        q = q + 0.25 * np.random.default_rng([5, d, nq]).standard_normal(q.shape).astype(np.float32)
        q = A.bf16_round(q) if bf16 else q.astype(np.float32)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def _build(hip, name, d, Hkv, P, nq, lengths, shared=False, stale=None):
    """The pools filled through the table from decode_cases' logical K / V, and the contiguous
    cache holding the same rows. stale: a value written beforehand to everything a decode must not
    read (the rows >= n of the last visible page, the poison page, the unreferenced pages).
    Returns a dict of device tensors and host arrays."""
    torch, _hip = hip
    bf16 = name != "f32"
    tin = _tin(torch, name)
    q, k, v = _inputs(bf16, d, Hkv, nq, tuple(lengths))
    nvis = np.array([DC.visible(L, NK) for L in lengths], np.int32)
    table, n_pages, poison = _table(P, nvis, seed=d + nq, shared=shared)
    fill = np.nan if stale is None else stale
    pools = [np.full((n_pages, P, Hkv, d), fill, np.float32) for _ in range(2)]
    for b in range(B):
        n = int(nvis[b])
        for idx in range(-(-n // P)):
            rows = min(P, n - idx * P) if stale is not None else P
            for pool, src in zip(pools, (k, v)):
                pool[table[b, idx], :rows] = src[b, :, idx * P:idx * P + rows].transpose(1, 0, 2)
    pools[0][poison] = fill
    pools[1][poison] = fill
    # the contiguous cache holding the same rows: read back through the table (a shared page gives
    # both rows the same keys); rows >= n keep decode_cases' finite stale values
    kc, vc = k.copy(), v.copy()
    for b in range(B):
        for j in range(int(nvis[b])):
            kc[b, :, j] = pools[0][table[b, j // P], j % P]
            vc[b, :, j] = pools[1][table[b, j // P], j % P]
    dev = lambda a, t=tin: torch.from_numpy(np.array(a)).cuda().to(t)  # noqa: E731 (a copy: the inputs are read-only)
    kp, vp = (dev(p).permute(0, 2, 1, 3) for p in pools)  # [n_pages, Hkv, P, d] views
    return dict(q=dev(q), kp=kp, vp=vp, table=torch.from_numpy(table).cuda(), kv_len=torch.from_numpy(nvis).cuda(),
                kc=dev(kc), vc=dev(vc), qh=q, kh=kc, vh=vc, nvis=nvis, poison=poison, n_pages=n_pages)


def _paged(hip, name, c, causal, ws_fill=None, Hkv=None, nq=None, P=None, d=None):
    torch, _hip = hip
    ws = None
    if ws_fill is not None:
        need = _hip.decode_paged_workspace_bytes(CODES[name], B, H, nq, NK // P, P, d, Hkv)
        ws = torch.full((max(need, 4) // 4,), ws_fill, dtype=torch.float32, device="cuda")
    o, m, l = _hip.flash_decode_paged(c["q"], c["kp"], c["vp"], c["table"], kv_len=c["kv_len"], causal=causal,
                                      out_dtype=_tout(torch, name), workspace=ws)
    torch.cuda.synchronize()
    return o, m, l


def _same_bits(a, b, what):
    for x, y, nm in zip(a, b, "Oml"):
        assert np.array_equal(_bits(x), _bits(y)), f"{what}: {nm} differs"


def _lengths(span, P):
    vals = [1, P - 1, P, P + 1, span - 1, span, span + 1, NK]
    return [(vals[i], vals[7 - i]) for i in range(4)]


# fp32 d = 128 is there for LPK = 32, which no other configuration reaches
CONFIGS = [("f32", d) for d in (20, 32, 64, 128, 256)] + [("bf16", 32), ("bf16", 128), ("bf16_f32out", 32)]
CASES = [(n, d, Hkv, P) for n, d in CONFIGS for Hkv in (4, 1) for P in (16, 64)]
IDS = [f"{n}-d{d}-Hkv{k}-P{P}" for n, d, k, P in CASES]


@pytest.mark.parametrize("name,d,Hkv,P", CASES, ids=IDS)
def test_decode_equals_the_plain_kernel_and_meets_the_bound(hip, name, d, Hkv, P):
    torch, _hip = hip
    bf16 = name != "f32"
    for nq in (1, 3, 8):
        nsplit, span, _ = _plan(_hip, name, Hkv, nq, P, d)
        assert nsplit >= 2 and (nsplit, span) == _hip.decode_splits(CODES[name], B, H, nq, NK, d, Hkv)[:2]
        for li, lengths in enumerate(_lengths(span, P)):
            c = _build(hip, name, d, Hkv, P, nq, lengths, shared=(li == 1))
            # the contiguous cache once more, through the gather kernel (rows >= n stay NaN: never read)
            kg = torch.full((B, Hkv, NK, d), float("nan"), dtype=c["kp"].dtype, device="cuda")
            vg = torch.full_like(kg, float("nan"))
            _hip.kv_cache_gather_paged(c["kp"], c["vp"], c["table"], kv_len=c["kv_len"], k_out=kg, v_out=vg)
            G = H // Hkv
            kr, vr = np.repeat(c["kh"], G, axis=1), np.repeat(c["vh"], G, axis=1)
            for causal in (True, False):
                what = f"nq={nq} lengths={lengths} causal={causal}"
                got = _paged(hip, name, c, causal)
                for kc, vc, how in ((c["kc"], c["vc"], "host-built"), (kg, vg, "gathered")):
                    want = _hip.flash_decode(c["q"], kc, vc, kv_len=c["kv_len"], causal=causal,
                                             out_dtype=_tout(torch, name))
                    _same_bits(got, want, f"{what}, {how} contiguous cache")
                lim = DC.limits(lengths, nq, causal, nmax=NK)
                o_ref, _, pv = DC.ref64(c["qh"], kr, vr, lim)
                o = got[0].float().cpu().numpy().astype(np.float64)
                m, l = got[1].cpu().numpy(), got[2].cpu().numpy()
                err, tol = np.abs(o - o_ref), DC.bound(bf16, o_ref, pv)
                print(f"{what}: worst |dO| / bound {float((err / tol).max()):.3f}")
                assert np.isfinite(o).all(), what
                assert (err <= tol).all(), f"{what}: {float((err / tol).max()):.2f}x the bound"
                none = np.broadcast_to((lim == 0)[:, None, :], m.shape)
                assert (o[none] == 0).all() and np.isneginf(m[none]).all() and (l[none] == 0).all(), what


@pytest.mark.parametrize("name,d,Hkv,P", CASES, ids=IDS)
def test_stale_content_does_not_matter(hip, name, d, Hkv, P):
    """NaN against zeros in the rows >= n of the last visible page, the poison page, every
    unreferenced page and the workspace: O, m and l keep their bits."""
    torch, _hip = hip
    for nq in (1, 3, 8):
        _, span, _ = _plan(_hip, name, Hkv, nq, P, d)
        for lengths in _lengths(span, P):
            for causal in (True, False):
                runs = []
                for fill in (float("nan"), 0.0):
                    c = _build(hip, name, d, Hkv, P, nq, lengths, stale=fill)
                    runs.append(_paged(hip, name, c, causal, ws_fill=fill, Hkv=Hkv, nq=nq, P=P, d=d))
                _same_bits(runs[0], runs[1], f"nq={nq} lengths={lengths} causal={causal}")
                assert torch.isfinite(runs[0][0].float()).all()


def _sentinel(torch, shape, dtype):
    n = int(np.prod(shape))
    if dtype == torch.float32:
        return torch.full((n,), SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32).reshape(shape)
    return torch.full((n,), 0x7FC5, dtype=torch.int16, device="cuda").view(torch.bfloat16).reshape(shape)


@pytest.mark.parametrize("with_count", [True, False], ids=["count", "nocount"])
@pytest.mark.parametrize("layout", ["dense", "bnhd"])
@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_append_footprint(hip, name, layout, with_count):
    """From pools filled with a sentinel bit pattern: after the append the pools equal, byte for
    byte, the sentinel pools with exactly the addressed rows replaced by the source rows.
    Positions at page edges, counts of 0, partial and full (and a negative one, taken as 0), rows past
    W * P and before row 0 (a negative pos), a -1 table entry."""
    torch, _hip = hip
    tin = _tin(torch, name)
    Bq, Hkv, nq, d, P, W = 7, 2, 5, 32, 16, 4
    n_pages = Bq * W + 2
    rng = np.random.default_rng(3)
    table = rng.permutation(n_pages)[:Bq * W].reshape(W, Bq).T.astype(np.int32).copy()  # interleaved
    table[3, 2] = -1    # row 3's third page is unallocated
    table[4, 1] = table[0, 3]  # a page named by two rows (row 4 does not write there)
    # crosses a page edge; starts a page; runs past W * P; runs into the -1 entry; a partial count at
    # row 0; starts 2 rows before row 0 (logical rows -2, -1 are dropped, 0..2 land); a negative count
    pos = np.array([14, 16, 62, 30, 0, -2, 20], np.int32)
    count = np.array([5, 0, 5, 3, 2, 5, -3], np.int32)
    new = [rng.standard_normal((Bq, Hkv, nq, d)).astype(np.float32) for _ in range(2)]
    if layout == "dense":
        kn, vn = (torch.from_numpy(a).cuda().to(tin) for a in new)
    else:  # the model's projection layout: [B, Nq, Hkv, d] storage
        kn, vn = (torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1, 3))).cuda().to(tin).permute(0, 2, 1, 3)
                  for a in new)
    pools = [_sentinel(torch, (n_pages, P, Hkv, d), tin).permute(0, 2, 1, 3) for _ in range(2)]
    want = [p.clone() for p in pools]
    cnt = count if with_count else np.full(Bq, nq, np.int32)
    landed = 0
    for b in range(Bq):
        for i in range(int(cnt[b])):
            row = int(pos[b]) + i
            if row < 0 or row >= W * P or table[b, row // P] < 0:
                continue
            landed += 1
            for w, src in zip(want, (kn, vn)):
                w[int(table[b, row // P]), :, row % P] = src[b, :, i]
    assert landed == (5 + 0 + 2 + 2 + 2 + 3 + 0 if with_count else 5 + 5 + 2 + 2 + 5 + 3 + 5)
    _hip.kv_cache_append_paged(kn, vn, pools[0], pools[1], torch.from_numpy(table).cuda(), torch.from_numpy(pos).cuda(),
                               torch.from_numpy(count).cuda() if with_count else None)
    torch.cuda.synchronize()
    for got, w, nm in zip(pools, want, "KV"):
        assert np.array_equal(_bits(got), _bits(w)), f"{nm} pool: the append's footprint or values are wrong"


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_gather_footprint(hip, name):
    """Rows < n of the sentinel-filled output equal the pool's through the table, rows >= n keep
    the sentinel; table entries at or past ceil(n / P) name a NaN page and are never followed."""
    torch, _hip = hip
    tin = _tin(torch, name)
    Bq, Hkv, d, P, W = 4, 2, 32, 16, 4
    n_pages = Bq * W + 1
    rng = np.random.default_rng(4)
    perm = rng.permutation(n_pages)
    table = perm[:Bq * W].reshape(W, Bq).T.astype(np.int32).copy()
    n = np.array([0, 17, 64, 31], np.int32)
    kv_len = n + np.array([-3, 0, 9, 0], np.int32)  # clamped to [0, W * P]
    for b in range(Bq):
        table[b, -(-int(n[b]) // P):] = perm[-1]
    host = [rng.standard_normal((n_pages, P, Hkv, d)).astype(np.float32) for _ in range(2)]
    for a in host:
        a[perm[-1]] = np.nan
    pools = [torch.from_numpy(a).cuda().to(tin).permute(0, 2, 1, 3) for a in host]
    outs = [_sentinel(torch, (Bq, W * P, Hkv, d), tin).permute(0, 2, 1, 3) for _ in range(2)]
    want = [o.clone() for o in outs]
    for b in range(Bq):
        for j in range(int(n[b])):
            for w, p in zip(want, pools):
                w[b, :, j] = p[int(table[b, j // P]), :, j % P]
    _hip.kv_cache_gather_paged(pools[0], pools[1], torch.from_numpy(table).cuda(), kv_len=torch.from_numpy(kv_len).cuda(),
                               k_out=outs[0], v_out=outs[1])
    torch.cuda.synchronize()
    for got, w, nm in zip(outs, want, "KV"):
        assert np.array_equal(_bits(got), _bits(w)), f"{nm}: the gather's footprint or values are wrong"


@pytest.mark.parametrize("name,P", [("f32", 16), ("bf16", 64)])
def test_graph_replay_as_the_cache_fills(hip, name, P):
    """One captured decode launch, the table filled ahead, replayed at the lengths 1, P, P + 1 and
    2 span + 1 (row 1 runs through them backwards): each replay equals the eager call, bit for bit."""
    torch, _hip = hip
    Hkv, nq, d = 1, 1, 64
    nsplit, span, _ = _plan(_hip, name, Hkv, nq, P, d)
    assert nsplit >= 3
    lens = (1, P, P + 1, 2 * span + 1)
    c = _build(hip, name, d, Hkv, P, nq, (NK, NK))  # every page allocated and filled: the table is final
    tout = _tout(torch, name)
    o = torch.empty((B, H, nq, d), dtype=tout, device="cuda")
    m, l = (torch.empty((B, H, nq), dtype=torch.float32, device="cuda") for _ in range(2))
    kvl = torch.zeros(B, dtype=torch.int32, device="cuda")
    ws = torch.empty(_hip.decode_paged_workspace_bytes(CODES[name], B, H, nq, NK // P, P, d, Hkv) // 4,
                     dtype=torch.float32, device="cuda")

    def step():
        _hip.flash_decode_paged(c["q"], c["kp"], c["vp"], c["table"], kv_len=kvl, causal=True, out=o, m=m, l=l,
                                workspace=ws)
    side = torch.cuda.Stream()
    kvl.fill_(1)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in range(len(lens)):
        L = np.array([lens[i], lens[len(lens) - 1 - i]], np.int32)
        kvl.copy_(torch.from_numpy(L).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = (o.clone(), m.clone(), l.clone())
        want = _hip.flash_decode_paged(c["q"], c["kp"], c["vp"], c["table"], kv_len=kvl, causal=True, out_dtype=tout)
        torch.cuda.synchronize()
        _same_bits(got, want, f"replay at lengths {L.tolist()}")
        assert torch.isfinite(got[0].float()).all()
