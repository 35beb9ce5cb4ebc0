"""Extend attention (csrc/fa_extend.hip through mt_flash_attn_extend) on the GPU: Nq new queries per
row, t of them real, at the end of n cached keys, n and t per batch row on the device.

Inputs: tests/extend_cases.py (tests/test_extend_edges.py shows on the CPU that they tell a
visible-key count from that count +- 1 by >= 16x the bounds used here, per head and per query).
One batch row per (cache length, real queries) pair; the pairs come from the library's own plan
answer (BQ query rows per workgroup, BK keys per tile): t in {1, BQ - 1, BQ, BQ + 1, Nq} against
a prefix n - t in {0, 1, BK - 1, BK, BK + 1}, a full cache, a length above the capacity, t = 0 and
rows with fewer keys than new tokens. Nq = 168 (a second, ragged query block), Nk = 448.

Reference: decode_cases.ref64 (float64) with the contract's limits.
Bounds (decode's): fp32 |dO| <= 1e-5 + 1e-5 |O| and |d(m + log l)| <= 1e-5 + 1e-5 |lse|; bf16
|dO| <= 1e-3 + 2^-7 (P|V|) and the log-sum-exp within 2e-3 + 1e-5 |lse|.
Yardstick (fp32): mt_flash_attn_fwd_varlen on the same problem with the queries placed at their
positions in a full-length Q; should that kernel itself exceed its bound on these inputs, the new
kernel is held to 1.5x its worst ratio instead (a different tile order moves individual
roundings, not their size).
"""
import functools

import numpy as np
import pytest

import decode_cases as DC
import extend_cases as EC

pytestmark = pytest.mark.gpu

CODES = {"f32": 0, "bf16": 1, "bf16_f32o": 2}
CASES = [("f32", 16, True), ("f32", 64, True), ("f32", 68, True), ("f32", 128, True), ("f32", 256, True),
         ("bf16", 64, True), ("bf16", 128, True), ("bf16", 256, True), ("bf16_f32o", 64, True),
         ("f32", 64, False), ("bf16", 128, False), ("bf16_f32o", 64, False)]
IDS = [f"{n}-d{d}-{'causal' if c else 'full'}" for n, d, c in CASES]
SENT = 768.0  # exact in bf16


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def _rows(_hip, name, d, heads=EC.H, kv_heads=None):
    kid, bq, bk = _hip.extend_plan(CODES[name], 27, heads, EC.NQ, EC.NMAX, d, Hkv=kv_heads)
    # the rows tests/test_extend_edges.py checked on the CPU: BQ = 128, BK = 32 (fp32) / 64 (bf16)
    if d <= 128:
        assert (bq, bk) == (128, 32 if name == "f32" else 64), (bq, bk)
    rows = EC.gpu_rows(bq, bk)
    assert EC.NQ >= bq + 33 and EC.NMAX >= 3 * bq + 64 and EC.NMAX >= 3 * bk
    return rows


@functools.lru_cache(maxsize=None)
def _reference(bf16, d, causal, rows, heads=EC.H, kv_heads=None):
    """Inputs and the float64 (O, lse, P|V|) [B,H,Nq,...] of one case, computed once, read-only."""
    q, k, v = EC.make_inputs(d, EC.NQ, bf16, rows, heads=heads, kv_heads=kv_heads)
    lim = EC.limits(rows, EC.NQ, causal)
    o, lse, pv = EC.ref64(q, EC.repeat_kv(k, heads), EC.repeat_kv(v, heads), lim)
    none = np.broadcast_to((lim == 0)[:, None, :], lse.shape).copy()
    for a in (q, k, v, o, lse, pv, none):
        a.setflags(write=False)
    return q, k, v, o, lse, pv, none


def _run(hip, name, q, k, v, rows, causal, layout="dense", nan=False, footprint=False, q_len=True):
    """One extend call; returns (O, m, l) as numpy (O as float32). layout 'bnhd': the caches as
    [B,Nmax,Hkv,d] storage, Q and O as [B,Nq,H,d] storage. nan: NaN in every cache row >= the
    row's n and every Q row >= its t. kv_len / q_len go in as given (unclamped)."""
    torch, _hip = hip
    tin = torch.float32 if name == "f32" else torch.bfloat16
    tout = torch.bfloat16 if name == "bf16" else torch.float32
    ity = torch.int16 if tin == torch.bfloat16 else torch.int32
    B, H, nq, d = q.shape
    nmax = k.shape[2]
    q, k, v = q.copy(), k.copy(), v.copy()
    if nan:
        for b, (L, t) in enumerate(rows):
            k[b, :, EC.visible(L, nmax):] = np.nan
            v[b, :, EC.visible(L, nmax):] = np.nan
            if q_len:
                q[b, :, EC.real(t, nq):] = np.nan

    def put(a):
        t = torch.from_numpy(np.array(a)).to("cuda").to(tin)
        if layout == "bnhd":
            t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
            assert t.shape[1] == 1 or t.shape[2] == 1 or not t.is_contiguous()
        return t
    tq, tk, tv = put(q), put(k), put(v)
    kv = torch.tensor([L for L, _ in rows], dtype=torch.int32, device="cuda")
    ql = torch.tensor([t for _, t in rows], dtype=torch.int32, device="cuda") if q_len else None
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
    before = [t.clone() for t in (tq, tk, tv)]
    _hip.flash_extend(tq, tk, tv, kv_len=kv, q_len=ql, causal=causal, out=o, m=m, l=l)
    torch.cuda.synchronize()
    if footprint:
        for buf, n in ((obuf, B * H * nq * d), (mbuf, B * H * nq), (lbuf, B * H * nq)):
            assert bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all()), "wrote outside O / m / l"
        for t, t0 in zip((tq, tk, tv), before):
            assert torch.equal(t.view(ity), t0.view(ity)), "inputs changed"
    return o.float().cpu().numpy(), m.cpu().numpy(), l.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ratios(bf16, o, m, l, o_ref, lse_ref, pv, none):
    """(worst |dO| / bound, worst |dlse| / bound, max |dO|) over the queries that see a key."""
    bnd = EC.bound(bf16, o_ref, pv)
    err = np.abs(o.astype(np.float64) - o_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = m.astype(np.float64) + np.log(l.astype(np.float64))
    lse_tol = (2e-3 if bf16 else 1e-5) + 1e-5 * np.abs(lse_ref[~none])
    lse_err = np.abs(lse[~none] - lse_ref[~none])
    return float((err / bnd).max()), float((lse_err / lse_tol).max()), float(err.max())


def _check_none(o, m, l, none):
    """A query >= t, or one with no visible key: O = 0, m = -inf, l = 0 exactly."""
    assert none.any() and not none.all()
    assert np.isneginf(m[none]).all() and not l[none].any() and not o[none].any()
    assert np.isfinite(m[~none]).all() and (l[~none] > 0).all()


def _yardstick(hip, q, k, v, rows, causal, o_ref, lse_ref, pv, none):
    """The worst ratios of mt_flash_attn_fwd_varlen (fp32) on the same problem: the queries at their
    positions in a full-length Q (causal), or in the first rows (non-causal: kv_len alone masks)."""
    torch, _hip = hip
    B, H, nq, d = q.shape
    nvis = np.array([EC.visible(L) for L, _ in rows], np.int32)
    if causal:
        qf, pos = EC.place_queries(q, rows)
    else:
        qf = np.zeros((B, H, EC.NMAX, d), np.float32)
        qf[:, :, :nq] = q
        pos = np.where(np.arange(nq)[None, :] < np.array([EC.real(t, nq) for _, t in rows])[:, None],
                       np.arange(nq)[None, :], -1)
    of, mf, lf = (x.cpu().numpy() for x in _hip.flash_fwd(*(torch.from_numpy(np.array(a)).cuda() for a in (qf, k, v)),
                                                          causal=causal, kv_len=torch.from_numpy(nvis).cuda()))
    o = np.zeros((B, H, nq, d), np.float32)
    m = np.full((B, H, nq), -np.inf, np.float32)
    l = np.zeros((B, H, nq), np.float32)
    for b in range(B):
        for i in range(nq):
            if pos[b, i] >= 0 and not none[b, 0, i]:
                o[b, :, i], m[b, :, i], l[b, :, i] = of[b, :, pos[b, i]], mf[b, :, pos[b, i]], lf[b, :, pos[b, i]]
    return _ratios(False, o, m, l, o_ref, lse_ref, pv, none)


@pytest.mark.parametrize("name,d,causal", CASES, ids=IDS)
def test_extend_matches_reference(hip, name, d, causal, parity_record):
    rows = _rows(hip[1], name, d)
    bf16 = name != "f32"
    q, k, v, o_ref, lse_ref, pv, none = _reference(bf16, d, causal, rows)
    o, m, l = _run(hip, name, q, k, v, rows, causal, footprint=True)
    assert np.isfinite(o).all()
    worst, worst_lse, max_abs = _ratios(bf16, o, m, l, o_ref, lse_ref, pv, none)
    limit = limit_lse = 1.0
    extra = {}
    if not bf16:
        y, y_lse, _ = _yardstick(hip, q, k, v, rows, causal, o_ref, lse_ref, pv, none)
        extra = dict(fwd_varlen_over_bound=y, fwd_varlen_lse_over_bound=y_lse)
        print(f"{name} d={d} causal={causal}: mt_flash_attn_fwd_varlen worst |dO| / bound {y:.3f}, lse {y_lse:.3f}")
        # the inputs, not the new kernel, are at fault where the existing kernel exceeds its bound
        limit, limit_lse = max(1.0, 1.5 * y), max(1.0, 1.5 * y_lse)
    print(f"{name} d={d} causal={causal}: worst |dO| / bound {worst:.3f}, worst |dlse| / bound {worst_lse:.3f}, "
          f"max |dO| {max_abs:.3e}")
    parity_record("test_extend_matches_reference", f"{name} d={d} causal={causal}", max_abs=max_abs,
                  worst_over_bound=worst, lse_over_bound=worst_lse, bound=limit, **extra)
    assert worst <= limit
    assert worst_lse <= limit_lse
    _check_none(o, m, l, none)


@pytest.mark.parametrize("name,d,causal", CASES, ids=IDS)
def test_layouts_stale_rows_and_repeat_are_bit_equal(hip, name, d, causal):
    rows = _rows(hip[1], name, d)
    q, k, v, *_r = _reference(name != "f32", d, causal, rows)
    base = _run(hip, name, q, k, v, rows, causal)
    again = _run(hip, name, q, k, v, rows, causal)
    strided = _run(hip, name, q, k, v, rows, causal, layout="bnhd", footprint=True)
    nan = _run(hip, name, q, k, v, rows, causal, nan=True, footprint=True)
    nan_strided = _run(hip, name, q, k, v, rows, causal, layout="bnhd", nan=True)
    for a in nan:
        assert not np.isnan(a).any(), "a stale cache row or a padding query reached the output"
    assert np.isfinite(nan[0]).all()
    for what, other in (("repeat", again), ("[B,N,H,d] storage", strided), ("NaN stale rows", nan),
                        ("NaN stale rows, strided", nan_strided)):
        for x, y, nm in zip(base, other, "Oml"):
            assert np.array_equal(_bits(x), _bits(y)), f"{nm} differs: {what}"


@pytest.mark.parametrize("nq", [1, 8])
@pytest.mark.parametrize("name,d", [("f32", 16), ("f32", 64), ("f32", 128), ("bf16", 64), ("bf16", 128)])
def test_decode_contract_subset(hip, name, d, nq, parity_record):
    """q_len = NULL and Nq <= 8: mt_flash_attn_decode's contract, on its test inputs and lengths
    (below Nq, around the tile edges, the ends of the cache, above its capacity)."""
    _, bq, bk = hip[1].extend_plan(CODES[name], 18, DC.H, nq, DC.NMAX, d)
    lengths = (0, 1, nq - 1, nq, nq + 1, 3, bk - 1, bk, bk + 1, 2 * bk - 1, 2 * bk, 2 * bk + 1, 511, 513,
               1099, 1100, DC.NMAX, DC.NMAX + 7)
    bf16 = name != "f32"
    q, k, v = DC.make_inputs(d, nq, bf16, lengths)
    lim = DC.limits(lengths, nq, True)
    o_ref, lse_ref, pv = DC.ref64(q, k, v, lim)
    none = np.broadcast_to((lim == 0)[:, None, :], lse_ref.shape)
    rows = tuple((L, nq) for L in lengths)
    o, m, l = _run(hip, name, q, k, v, rows, True, footprint=True, q_len=False)
    nan = _run(hip, name, q, k, v, rows, True, nan=True, q_len=False)
    worst, worst_lse, max_abs = _ratios(bf16, o, m, l, o_ref, lse_ref, pv, none)
    print(f"{name} d={d} nq={nq}: worst |dO| / bound {worst:.3f}, worst |dlse| / bound {worst_lse:.3f}")
    parity_record("test_decode_contract_subset", f"{name} d={d} nq={nq}", max_abs=max_abs, worst_over_bound=worst,
                  lse_over_bound=worst_lse, bound=1.0)
    assert worst <= 1.0 and worst_lse <= 1.0
    _check_none(o, m, l, none)
    for x, y in zip((o, m, l), nan):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("name", ["f32", "bf16"])
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (3, 1)])
def test_gqa(hip, name, heads, kv_heads, parity_record):
    d, bf16 = 64, name != "f32"
    rows = _rows(hip[1], name, d, heads, kv_heads)
    q, k, v, o_ref, lse_ref, pv, none = _reference(bf16, d, True, rows, heads, kv_heads)
    assert k.shape[1] == kv_heads and q.shape[1] == heads
    o, m, l = _run(hip, name, q, k, v, rows, True, footprint=True)
    strided = _run(hip, name, q, k, v, rows, True, layout="bnhd", nan=True, footprint=True)
    worst, worst_lse, max_abs = _ratios(bf16, o, m, l, o_ref, lse_ref, pv, none)
    print(f"{name} H={heads} Hkv={kv_heads}: worst |dO| / bound {worst:.3f}, worst |dlse| / bound {worst_lse:.3f}")
    parity_record("test_extend_gqa", f"{name} H={heads} Hkv={kv_heads} d={d}", max_abs=max_abs,
                  worst_over_bound=worst, lse_over_bound=worst_lse, bound=1.0)
    assert worst <= 1.0 and worst_lse <= 1.0
    _check_none(o, m, l, none)
    for x, y, nm in zip((o, m, l), strided, "Oml"):
        assert np.array_equal(_bits(x), _bits(y)), f"{nm} differs: [B,N,Hkv,d] storage with NaN stale rows"


def test_graph_replay_with_changing_lengths(hip):
    """append + extend captured once (one stream, no parallel branches), replayed for three
    (kv_len, q_len) settings written on the device: row 0 crosses a query-block edge, row 1 a
    key-tile edge, row 2 goes from no new token to a full step. Each replay is bit-equal to the
    eager call."""
    torch, _hip = hip
    B, H, nq, d, nmax = 3, 2, EC.NQ, 64, EC.NMAX
    _, bq, bk = _hip.extend_plan(0, B, H, nq, nmax, d)
    assert nq > bq + 1
    rng = np.random.default_rng(11)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    kc, vc = (dev(rng.standard_normal((B, nmax, H, d)).astype(np.float32)).permute(0, 2, 1, 3) for _ in range(2))
    T = np.array([[bq - 1, 5, 0], [bq, 5, nq], [bq + 1, 5, 1]], np.int32)             # real new tokens
    N = np.array([[bq + 9, bk - 1, 50], [bq + 10, bk, 300], [bq + 11, bk + 1, 1]], np.int32)  # keys held after
    steps = [[dev(rng.standard_normal((B, H, nq, d)).astype(np.float32)) for _ in range(3)] for _ in range(3)]
    q, kn, vn = (torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda") for _ in range(3))
    pos, kvl, qln = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    o = torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda")
    m, l = (torch.empty((B, H, nq), dtype=torch.float32, device="cuda") for _ in range(2))
    kc_e, vc_e = kc.clone(), vc.clone()  # the eager leg's caches (clone keeps the strides)

    def step():
        _hip.kv_cache_append(kn, vn, kc, vc, pos)
        _hip.flash_extend(q, kc, vc, kv_len=kvl, q_len=qln, causal=True, out=o, m=m, l=l)

    def load(i):
        for dst, src in zip((q, kn, vn), steps[i]):
            dst.copy_(src)
        pos.copy_(dev(N[i] - T[i]))
        kvl.copy_(dev(N[i]))
        qln.copy_(dev(T[i]))
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
        _hip.kv_cache_append(steps[i][1], steps[i][2], kc_e, vc_e, dev(N[i] - T[i]))
        ref = _hip.flash_extend(steps[i][0], kc_e, vc_e, kv_len=dev(N[i]), q_len=dev(T[i]), causal=True)
        torch.cuda.synchronize()
        for x, y, nm in zip(got, ref, "Oml"):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"replay {i}: {nm} differs from the eager call"
        assert bool((got[2][0, :, :int(T[i][0])] > 0).all()) and not bool(got[2][0, :, int(T[i][0]):].any())
        assert torch.equal(kc.contiguous().view(torch.int32), kc_e.contiguous().view(torch.int32))
        assert torch.equal(vc.contiguous().view(torch.int32), vc_e.contiguous().view(torch.int32))
