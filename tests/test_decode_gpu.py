"""KV-cache decode attention (csrc/fa_decode.hip through mt_flash_attn_decode) and the cache
append (mt_kv_cache_append) on the GPU.

Inputs: tests/decode_cases.py (tests/test_decode_edges.py shows on the CPU that they tell a
visible-key count from that count +- 1 by >= 16x the bounds used here). One batch row per cache
length; the lengths come from the library's own split answer (span S, wave tile t): every edge
of a tile, a span and two spans, the ends of the cache and one length above its capacity.

Reference: oracle.cref.attn_fwd on the full [B, 2, 1104, d] problem with kv_len = L and the Nq
queries placed at their positions (causal), or kv_len alone (non-causal).
Bounds: fp32 |dO| <= 1e-5 + 1e-5 |O| and |d(m + log l)| <= 1e-5 + 1e-5 |lse|; bf16
|dO| <= 1e-3 + 2^-7 (P|V|) (tests/bounds.py, P|V| in fp64 from the bf16-rounded inputs) and the
log-sum-exp within 2e-3 (test_flash_gpu._check_ml's figure).
"""
import functools

import numpy as np
import pytest

import decode_cases as DC

pytestmark = pytest.mark.gpu

CODES = {"f32": 0, "bf16": 1, "bf16_f32o": 2}
DTYPE_D = [("f32", 16), ("f32", 32), ("f32", 64), ("f32", 128), ("bf16", 64), ("bf16", 128), ("bf16_f32o", 64)]
CASES = [(n, d, nq, True) for n, d in DTYPE_D for nq in (1, 5, 8)] + \
        [("f32", 64, 5, False), ("bf16", 128, 5, False), ("bf16_f32o", 64, 5, False)]
IDS = [f"{n}-d{d}-nq{nq}-{'causal' if c else 'full'}" for n, d, nq, c in CASES]
B_ROWS = 18
SENT = 768.0  # exact in bf16


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def _lengths(_hip, name, d, nq):
    n, S, t = _hip.decode_splits(CODES[name], B_ROWS, DC.H, nq, DC.NMAX, d)
    L = [0, 1, nq - 1, nq, nq + 1, t - 1, t, t + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1,
         1099, 1100, DC.NMAX, DC.NMAX + 7]
    assert len(L) == B_ROWS and 2 * S + 1 <= DC.NMAX
    return n, L


@functools.lru_cache(maxsize=None)
def _reference(bf16, d, nq, causal, lengths):
    """Inputs and the oracle's (O, m, l) [B,H,nq,...] for one case, computed once."""
    from oracle import cref
    q, k, v = DC.make_inputs(d, nq, bf16, lengths)
    nvis = np.array([DC.visible(L) for L in lengths], np.int32)
    B = len(lengths)
    if causal:
        qf, pos = DC.place_queries(q, lengths)
    else:  # kv_len alone masks: the rows the queries sit in do not matter
        qf = np.zeros((B, DC.H, DC.NMAX, d), np.float32)
        qf[:, :, :nq] = q
        pos = np.broadcast_to(np.arange(nq), (B, nq)).copy()
    of, mf, lf = cref.attn_fwd(qf, k, v, causal=causal, kv_len=nvis)
    o = np.zeros((B, DC.H, nq, d), np.float32)
    m = np.full((B, DC.H, nq), -np.inf, np.float32)
    l = np.zeros((B, DC.H, nq), np.float32)
    for b in range(B):
        for i in range(nq):
            if pos[b, i] >= 0:
                o[b, :, i], m[b, :, i], l[b, :, i] = of[b, :, pos[b, i]], mf[b, :, pos[b, i]], lf[b, :, pos[b, i]]
    _, _, pv = DC.ref64(q, k, v, DC.limits(lengths, nq, causal))
    for a in (q, k, v, o, m, l, pv):
        a.setflags(write=False)
    return q, k, v, o, m, l, pv


def _run(hip, name, q, k, v, lengths, causal, layout="dense", stale=None, footprint=False):
    """One decode call; returns (O, m, l) as numpy (O as float32). layout 'bnhd': the caches as
    [B,Nmax,H,d] storage, Q and O as [B,Nq,H,d] storage. stale: a value written to every cache
    row >= the row's visible length and to the whole workspace beforehand."""
    torch, _hip = hip
    code = CODES[name]
    tin = torch.float32 if name == "f32" else torch.bfloat16
    tout = torch.bfloat16 if name == "bf16" else torch.float32
    B, H, nq, d = q.shape
    k, v = k.copy(), v.copy()
    if stale is not None:
        for b, L in enumerate(lengths):
            k[b, :, DC.visible(L):] = stale
            v[b, :, DC.visible(L):] = stale

    def put(a):
        t = torch.from_numpy(np.array(a)).to("cuda").to(tin)
        if layout == "bnhd":
            t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
            assert t.shape[2] == 1 or not t.is_contiguous()
        return t
    tq, tk, tv = put(q), put(k), put(v)
    kv = torch.tensor(list(lengths), dtype=torch.int32, device="cuda")
    pad = 64
    oshape = (B, nq, H, d) if layout == "bnhd" else (B, H, nq, d)
    obuf = torch.full((B * H * nq * d + 2 * pad,), SENT, dtype=tout, device="cuda")
    o = obuf[pad:pad + B * H * nq * d].view(oshape)
    if layout == "bnhd":
        o = o.permute(0, 2, 1, 3)
    mbuf = torch.full((B * H * nq + 2 * pad,), SENT, dtype=torch.float32, device="cuda")
    lbuf = torch.full((B * H * nq + 2 * pad,), SENT, dtype=torch.float32, device="cuda")
    m = mbuf[pad:pad + B * H * nq].view(B, H, nq)
    l = lbuf[pad:pad + B * H * nq].view(B, H, nq)
    need = _hip.decode_workspace_bytes(code, B, H, nq, k.shape[2], d)
    assert need % 4 == 0
    wbuf = torch.full((need // 4 + pad,), SENT if stale is None else float(stale), dtype=torch.float32, device="cuda")
    if stale is not None:
        wbuf[need // 4:] = SENT
    ws = wbuf[:need // 4] if need else None
    before = [t.clone() for t in (tq, tk, tv)]
    _hip.flash_decode(tq, tk, tv, kv_len=kv, causal=causal, out=o, m=m, l=l, workspace=ws)
    torch.cuda.synchronize()
    if footprint:
        for buf, n in ((obuf, B * H * nq * d), (mbuf, B * H * nq), (lbuf, B * H * nq)):
            assert bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all()), "wrote outside O / m / l"
        assert bool((wbuf[need // 4:] == SENT).all()), "wrote past the advertised workspace"
        for t, t0 in zip((tq, tk, tv), before):
            assert torch.equal(t.view(torch.int16 if tin == torch.bfloat16 else torch.int32),
                               t0.view(torch.int16 if tin == torch.bfloat16 else torch.int32)), "inputs changed"
    return o.float().cpu().numpy(), m.cpu().numpy(), l.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(hip, name, d, nq, causal):
    n, lengths = _lengths(hip[1], name, d, nq)
    assert n >= 3, f"{n} splits: the case does not exercise the split-KV path"
    return tuple(lengths), _reference(name != "f32", d, nq, causal, tuple(lengths))


@pytest.mark.parametrize("name,d,nq,causal", CASES, ids=IDS)
def test_decode_matches_oracle(hip, name, d, nq, causal, parity_record):
    lengths, (q, k, v, o_ref, m_ref, l_ref, pv) = _case(hip, name, d, nq, causal)
    o, m, l = _run(hip, name, q, k, v, lengths, causal, footprint=True)
    assert np.isfinite(o).all()
    bf16 = name != "f32"
    bnd = DC.bound(bf16, o_ref, pv)
    err = np.abs(o.astype(np.float64) - o_ref)
    worst = float((err / bnd).max())
    none = l_ref == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        lse, lse_ref = m + np.log(l), m_ref + np.log(l_ref)
    lse_tol = (2e-3 if bf16 else 1e-5) + 1e-5 * np.abs(lse_ref[~none])
    lse_err = np.abs(lse[~none].astype(np.float64) - lse_ref[~none])
    worst_lse = float((lse_err / lse_tol).max())
    print(f"{name} d={d} nq={nq} causal={causal}: worst |dO| / bound {worst:.3f}, worst |dlse| / bound {worst_lse:.3f}, "
          f"max |dO| {float(err.max()):.3e}")
    parity_record("test_decode_matches_oracle", f"{name} d={d} nq={nq} causal={causal}",
                  max_abs=float(err.max()), worst_over_bound=worst, lse_over_bound=worst_lse, bound=1.0)
    assert worst <= 1.0
    assert worst_lse <= 1.0
    # a query with no visible key: O = 0, m = -inf, l = 0 exactly
    assert none.any()
    assert np.isneginf(m[none]).all() and not l[none].any() and not o[none].any()
    assert np.isfinite(m[~none]).all() and (l[~none] > 0).all()


@pytest.mark.parametrize("name,d,nq,causal", CASES, ids=IDS)
def test_layouts_stale_rows_and_repeat_are_bit_equal(hip, name, d, nq, causal):
    lengths, (q, k, v, *_r) = _case(hip, name, d, nq, causal)
    base = _run(hip, name, q, k, v, lengths, causal)
    again = _run(hip, name, q, k, v, lengths, causal)
    strided = _run(hip, name, q, k, v, lengths, causal, layout="bnhd", footprint=True)
    nan = _run(hip, name, q, k, v, lengths, causal, stale=np.nan, footprint=True)
    nan_strided = _run(hip, name, q, k, v, lengths, causal, layout="bnhd", stale=np.nan)
    for a in nan:
        assert not np.isnan(a).any(), "a stale cache row or the workspace's old content reached the output"
    assert np.isfinite(nan[0]).all()
    for what, other in (("repeat", again), ("[B,N,H,d] storage", strided), ("NaN stale rows", nan),
                        ("NaN stale rows, strided", nan_strided)):
        for x, y, nm in zip(base, other, "Oml"):
            assert np.array_equal(_bits(x), _bits(y)), f"{nm} differs: {what}"


def test_many_heads_single_split(hip, parity_record):
    """(64,8,Nq=1,Nk=40,d=32) fp32, config 5's generation shape: one split, pass 1 writes O directly."""
    from oracle import cref
    torch, _hip = hip
    B, H, Nk, d = 64, 8, 40, 32
    assert _hip.decode_splits(0, B, H, 1, Nk, d)[0] == 1
    assert _hip.decode_workspace_bytes(0, B, H, 1, Nk, d) == 0
    rng = np.random.default_rng(5)
    k, v = (rng.standard_normal((B, H, Nk, d)).astype(np.float32) for _ in range(2))
    q = rng.standard_normal((B, H, 1, d)).astype(np.float32)
    lengths = np.array([(7 * b) % Nk + 1 for b in range(B)], np.int32)
    qf = np.zeros((B, H, Nk, d), np.float32)
    for b, L in enumerate(lengths):
        qf[b, :, L - 1] = q[b, :, 0]
        k[b, :, L:] = np.nan
        v[b, :, L:] = np.nan
    of, mf, lf = cref.attn_fwd(qf, np.nan_to_num(k), np.nan_to_num(v), causal=True, kv_len=lengths)
    idx = np.arange(B)
    o_ref, m_ref, l_ref = of[idx, :, lengths - 1], mf[idx, :, lengths - 1], lf[idx, :, lengths - 1]
    o, m, l = _hip.flash_decode(*(torch.from_numpy(a).cuda() for a in (q, k, v)),
                                kv_len=torch.from_numpy(lengths).cuda(), causal=True)
    torch.cuda.synchronize()
    o, m, l = o.cpu().numpy()[:, :, 0], m.cpu().numpy()[:, :, 0], l.cpu().numpy()[:, :, 0]
    err = np.abs(o.astype(np.float64) - o_ref)
    worst = float((err / (1e-5 + 1e-5 * np.abs(o_ref))).max())
    lse, lse_ref = m + np.log(l), m_ref + np.log(l_ref)
    worst_lse = float((np.abs(lse - lse_ref) / (1e-5 + 1e-5 * np.abs(lse_ref))).max())
    print(f"single split: worst |dO| / bound {worst:.3f}, lse {worst_lse:.3f}")
    parity_record("test_many_heads_single_split", "f32 (64,8,1,40,32)", max_abs=float(err.max()),
                  worst_over_bound=worst, lse_over_bound=worst_lse, bound=1.0)
    assert worst <= 1.0 and worst_lse <= 1.0


@pytest.mark.parametrize("layout", ["dense", "bnhd"])
@pytest.mark.parametrize("name,d", [("f32", 16), ("f32", 68), ("bf16", 64)])
def test_kv_cache_append(hip, name, d, layout):
    torch, _hip = hip
    tin = torch.float32 if name == "f32" else torch.bfloat16
    ity = torch.int32 if name == "f32" else torch.int16
    B, H, nq, nmax = 5, 2, 3, 16
    pos = [0, 5, 14, 16, 13]  # 14: rows 14, 15 land and 16 is dropped; 16: nothing lands
    g = torch.Generator(device="cpu").manual_seed(3)
    kn, vn = (torch.randn((B, H, nq, d), generator=g).to(tin).cuda() for _ in range(2))

    def cache():
        c = torch.full((B, H, nmax, d), float("nan"), dtype=tin, device="cuda")
        if layout == "bnhd":
            c = c.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        return c
    kc, vc = cache(), cache()
    if layout == "bnhd":
        kn, vn = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (kn, vn))
    _hip.kv_cache_append(kn, vn, kc, vc, torch.tensor(pos, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for new, c in ((kn, kc), (vn, vc)):
        want = torch.full((B, H, nmax, d), float("nan"), dtype=tin, device="cuda")
        for b, p in enumerate(pos):
            for i in range(nq):
                if p + i < nmax:
                    want[b, :, p + i] = new[b, :, i]
        assert torch.equal(c.contiguous().view(ity), want.view(ity)), "the cache differs from source rows + NaN elsewhere"


def test_graph_replay_as_the_cache_fills(hip):
    """append + decode captured once (one stream, no parallel branches), replayed for three
    successive lengths by updating pos / kv_len / the new rows on the device: each replay is
    bit-equal to the eager call at that length."""
    torch, _hip = hip
    B, H, nq, d, nmax = 3, 2, 1, 64, DC.NMAX
    n, S, t = _hip.decode_splits(0, B, H, nq, nmax, d)
    assert n >= 3
    rng = np.random.default_rng(11)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    kc, vc = (dev(rng.standard_normal((B, nmax, H, d)).astype(np.float32)).permute(0, 2, 1, 3) for _ in range(2))
    L0 = np.array([S - 1, 2 * S - 2, 5], np.int32)  # the first two rows cross a span edge while replaying
    steps = [[dev(rng.standard_normal((B, H, nq, d)).astype(np.float32)) for _ in range(3)] for _ in range(3)]
    q, kn, vn = (torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda") for _ in range(3))
    pos = torch.zeros(B, dtype=torch.int32, device="cuda")
    kvl = torch.zeros(B, dtype=torch.int32, device="cuda")
    o = torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda")
    m, l = (torch.empty((B, H, nq), dtype=torch.float32, device="cuda") for _ in range(2))
    ws = torch.empty(_hip.decode_workspace_bytes(0, B, H, nq, nmax, d) // 4, dtype=torch.float32, device="cuda")
    kc_e, vc_e = kc.clone(), vc.clone()  # the eager leg's caches (clone keeps the strides)

    def step():
        _hip.kv_cache_append(kn, vn, kc, vc, pos)
        _hip.flash_decode(q, kc, vc, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)

    def load(i):
        for dst, src in zip((q, kn, vn), steps[i]):
            dst.copy_(src)
        pos.copy_(dev(L0 + i))
        kvl.copy_(dev(L0 + i + 1))
    side = torch.cuda.Stream()
    load(0)
    kc0, vc0 = kc.clone(), vc.clone()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kc.copy_(kc0)
    vc.copy_(vc0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in range(3):
        load(i)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in (o, m, l)]
        _hip.kv_cache_append(steps[i][1], steps[i][2], kc_e, vc_e, dev(L0 + i))
        ref = _hip.flash_decode(steps[i][0], kc_e, vc_e, kv_len=dev(L0 + i + 1), causal=True)
        torch.cuda.synchronize()
        for x, y, nm in zip(got, ref, "Oml"):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"replay {i}: {nm} differs from the eager call"
        assert torch.equal(kc.contiguous().view(torch.int32), kc_e.contiguous().view(torch.int32))
        assert torch.equal(vc.contiguous().view(torch.int32), vc_e.contiguous().view(torch.int32))
