"""The quantised KV cache kernels on the GPU (csrc/fa_kvq.hip): mt_kv_cache_append_quant,
mt_flash_attn_decode_kvq and mt_kv_cache_dequant for bf16 and fp8 (e4m3) caches.

Inputs: tests/decode_cases.py through tests/kvq_cases.py, one batch row per cache length
(EDGE_LENGTHS, 0 and NMAX + 5). The caches are quantised by the append kernel itself, which is
held to the format's definition on its own (all codes, append round trip). The decode oracle is
decode_cases.ref64 on the DEQUANTISED cache read back from the device, so quantisation error is
not in the comparison: the bound is the project's fp32 criterion |dO| <= 1e-5 + 1e-5 |O|,
which the fp32 decode kernel meets with the same arithmetic, and the log-sum-exp bound is
test_decode_gpu.py's, 1e-5 + 1e-5 |lse|.
"""
import functools

import numpy as np
import pytest

import kvq_cases as KC

pytestmark = pytest.mark.gpu

KVS = {"bf16": KC.KV_BF16, "fp8": KC.KV_FP8}
LENGTHS = tuple(KC.EDGE_LENGTHS) + (0, KC.NMAX + 5)
SENT = 768.0


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _new_cache(torch, kv, shape, fill=None, layout="bnhd"):
    """An empty cache pair as [B,Hkv,N,d] views ([B,N,Hkv,d] storage for 'bnhd') with scales."""
    B, Hkv, N, d = shape
    dt = torch.bfloat16 if kv == KC.KV_BF16 else torch.uint8

    def one():
        st = (B, N, Hkv, d) if layout == "bnhd" else shape
        t = torch.zeros(st, dtype=dt, device="cuda")
        if fill is not None:
            t.view(torch.uint8).fill_(fill)
        return t.permute(0, 2, 1, 3) if layout == "bnhd" else t
    ks = vs = None
    if kv == KC.KV_FP8:
        ks, vs = (torch.full((B, Hkv, N), SENT, dtype=torch.float32, device="cuda") for _ in range(2))
    return one(), one(), ks, vs


def _read(torch, kv, c):
    """The cache's bit patterns as numpy [B,Hkv,N,d] (uint16 for bf16, uint8 for fp8)."""
    c = c.contiguous()
    if kv == KC.KV_BF16:
        return c.view(torch.int16).cpu().numpy().view(np.uint16)
    return c.cpu().numpy()


def _host_dequant(torch, kv, c, s):
    return KC.dequant(kv, _read(torch, kv, c), None if s is None else s.cpu().numpy())


def _quantise(hip, kv, k, v):
    """Device caches holding the quantised k / v [B,Hkv,N,d] (one append of all N rows at row 0)."""
    torch, _hip = hip
    B = k.shape[0]
    kc, vc, ks, vs = _new_cache(torch, kv, k.shape)
    kn, vn = (torch.from_numpy(np.array(a, np.float32)).cuda() for a in (k, v))
    _hip.kv_cache_append_quant(kn, vn, kc, vc, torch.zeros(B, dtype=torch.int32, device="cuda"), ks, vs)
    torch.cuda.synchronize()
    return kc, vc, ks, vs


@functools.lru_cache(maxsize=4)
def _inputs(d, nq, heads=KC.H):
    out = KC.make_inputs(d, nq, False, LENGTHS, heads=heads)
    for a in out:
        a.setflags(write=False)
    return out


_CACHES = {}


def _case(hip, name, d, nq, heads=KC.H):
    """(q, device caches, their dequantised values read back through mt_kv_cache_dequant)."""
    torch, _hip = hip
    key = (name, d, nq, heads)
    if key not in _CACHES:
        _CACHES.clear()  # one case's device caches at a time
        q, k, v = _inputs(d, nq, heads)
        kc, vc, ks, vs = _quantise(hip, KVS[name], k, v)
        kd, vd = _hip.kv_cache_dequant(kc, vc, ks, vs)
        torch.cuda.synchronize()
        _CACHES[key] = (q, (kc, vc, ks, vs), kd.cpu().numpy(), vd.cpu().numpy())
    return _CACHES[key]


def _decode(hip, q, caches, lengths, causal, stale=None, footprint=False, workspace=None):
    """One decode call; (O, m, l) as numpy. stale: 'nan' or 'zero' fills every cache row >= the
    row's visible length, its scales and the whole workspace first (on copies)."""
    torch, _hip = hip
    kc, vc, ks, vs = caches
    B, H, nq, d = q.shape
    Hkv, N = kc.shape[1], kc.shape[2]
    code = _hip.kv_code(kc)
    need = _hip.decode_kvq_workspace_bytes(code, B, H, nq, N, d, Hkv)
    pad = 64
    wbuf = torch.full((need // 4 + pad,), SENT, dtype=torch.float32, device="cuda")
    if stale is not None:
        kc, vc = kc.clone(), vc.clone()  # clone keeps the strides
        ks, vs = (None if s is None else s.clone() for s in (ks, vs))
        for b, L in enumerate(lengths):
            n = KC.visible(L, N)
            for c in (kc, vc):
                if stale == "zero":
                    c[b, :, n:] = 0
                elif c.dtype == torch.uint8:
                    c[b, :, n:] = 0x7F                 # e4m3 NaN
                else:
                    c[b, :, n:] = float("nan")         # bf16 NaN
            for s in (ks, vs):
                if s is not None:
                    s[b, :, n:] = 0.0 if stale == "zero" else float("nan")
        wbuf[:need // 4] = 0.0 if stale == "zero" else float("nan")
    ws = wbuf[:need // 4] if need else None
    if workspace is not None:
        ws = workspace
    tq = torch.from_numpy(np.array(q, np.float32)).cuda()
    obuf = torch.full((B * H * nq * d + 2 * pad,), SENT, dtype=torch.float32, device="cuda")
    o = obuf[pad:pad + B * H * nq * d].view(B, nq, H, d).permute(0, 2, 1, 3)  # [B,Nq,H,d] storage
    mbuf, lbuf = (torch.full((B * H * nq + 2 * pad,), SENT, dtype=torch.float32, device="cuda") for _ in range(2))
    m, l = (t[pad:pad + B * H * nq].view(B, H, nq) for t in (mbuf, lbuf))
    kv = torch.tensor([int(x) for x in lengths], dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (kc, vc)]
    _hip.flash_decode_kvq(tq, kc, vc, ks, vs, kv_len=kv, causal=causal, out=o, m=m, l=l, workspace=ws)
    torch.cuda.synchronize()
    if footprint:
        for buf, n in ((obuf, B * H * nq * d), (mbuf, B * H * nq), (lbuf, B * H * nq)):
            assert bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all()), "wrote outside O / m / l"
        assert bool((wbuf[need // 4:] == SENT).all()), "wrote past the advertised workspace"
        for t, t0 in zip((kc, vc), before):
            assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8)), "the caches changed"
    return o.contiguous().cpu().numpy(), m.cpu().numpy(), l.cpu().numpy()


def _compare(o, m, l, q, kd, vd, lim):
    """(worst |dO| / bound, worst |dlse| / bound, rows without a visible key) against ref64."""
    o_ref, lse_ref, pv = KC.ref64(q, kd, vd, lim)
    bnd = KC.bound(False, o_ref, pv)
    ratio = np.abs(o.astype(np.float64) - o_ref) / bnd
    none = np.isneginf(lse_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = m.astype(np.float64) + np.log(l.astype(np.float64))
    tol = 1e-5 + 1e-5 * np.abs(lse_ref[~none])
    with np.errstate(invalid="ignore"):
        lse_ratio = np.abs(lse[~none] - lse_ref[~none]) / tol
    lse_ratio = np.where(np.isnan(lse_ratio), np.inf, lse_ratio)
    return ratio, (float(lse_ratio.max()) if lse_ratio.size else 0.0), none


# ---- the format ------------------------------------------------------------------------------
def test_all_e4m3_codes_dequantise_to_the_table(hip):
    """Bytes 0..255 with scale 1 through mt_kv_cache_dequant: the 254 values bit for bit, NaN for
    0x7F / 0xFF. This pins what the hardware conversion reads as OCP e4m3fn."""
    torch, _hip = hip
    codes = torch.arange(256, dtype=torch.uint8, device="cuda").view(1, 1, 32, 8)
    ones = torch.ones((1, 1, 32), dtype=torch.float32, device="cuda")
    kd, vd = _hip.kv_cache_dequant(codes, codes.clone(), ones, ones)
    torch.cuda.synchronize()
    nan = np.isnan(KC.E4M3_F32)
    for got in (kd.cpu().numpy().reshape(256), vd.cpu().numpy().reshape(256)):
        assert np.isnan(got[nan]).all()
        bad = np.flatnonzero(_bits(got)[~nan] != _bits(KC.E4M3_F32)[~nan])
        assert bad.size == 0, f"codes read differently: {[(int(c), float(got[~nan][c])) for c in bad[:8]]}"


@pytest.mark.parametrize("layout", ["dense", "bnhd"])
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("d", [8, 40, 64, 256])
@pytest.mark.parametrize("name", ["bf16", "fp8"])
def test_append_round_trip_and_footprint(hip, name, d, nq, layout):
    from oracle import attention as A
    torch, _hip = hip
    kv = KVS[name]
    B, Hkv, nmax = 4, 2, 16
    pos = [0, 5, nmax - 1, nmax]  # nmax - 1: one row lands, the rest is dropped; nmax: nothing lands
    rng = np.random.default_rng([3, d, nq])
    new = [(rng.standard_normal((B, Hkv, nq, d)) * np.exp(rng.uniform(-6, 6, (B, Hkv, nq, 1)))).astype(np.float32)
           for _ in range(2)]
    new[0][1, 0, 0] = 0.0  # an all-zero row
    kc, vc, ks, vs = _new_cache(torch, kv, (B, Hkv, nmax, d), fill=0x55, layout=layout)

    def put(a):
        t = torch.from_numpy(a).cuda()
        if layout == "bnhd":
            return t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        if nq == 3:  # rows that start 4 bytes off a 16-B boundary: the element-load path of the new rows
            buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
            buf[1:].copy_(t.reshape(-1))
            t = buf[1:].view(t.shape)
            assert t.data_ptr() % 16 == 4
        return t
    _hip.kv_cache_append_quant(put(new[0]), put(new[1]), kc, vc, torch.tensor(pos, dtype=torch.int32, device="cuda"),
                               ks, vs)
    torch.cuda.synchronize()
    landed = np.zeros((B, nmax), bool)
    src = np.zeros((B, nmax), np.int64)
    for b, p in enumerate(pos):
        for i in range(nq):
            if p + i < nmax:
                landed[b, p + i], src[b, p + i] = True, i
    assert landed.sum() == 2 * nq + 1
    for x, c, s in ((new[0], kc, ks), (new[1], vc, vs)):
        raw = _read(torch, kv, c)  # [B,Hkv,nmax,d]
        sent = np.uint16(0x5555) if kv == KC.KV_BF16 else np.uint8(0x55)
        assert (raw[~landed.repeat(Hkv).reshape(B, nmax, Hkv).transpose(0, 2, 1)] == sent).all(), \
            "a cache byte outside the written rows changed"
        rows_x = np.stack([x[b, :, src[b, j]] for b in range(B) for j in range(nmax) if landed[b, j]])
        rows_c = np.stack([raw[b, :, j] for b in range(B) for j in range(nmax) if landed[b, j]])
        if kv == KC.KV_BF16:
            assert np.array_equal(_bits(KC.bf16_decode(rows_c)), _bits(A.bf16_round(rows_x))), "not bf16 round-to-nearest-even"
            continue
        sc = s.cpu().numpy()
        assert (sc[~landed[:, None, :].repeat(Hkv, 1)] == SENT).all(), "a scale outside the written rows changed"
        rows_s = np.stack([sc[b, :, j] for b in range(B) for j in range(nmax) if landed[b, j]])
        worst = KC.check_fp8_rows(rows_x, rows_c, rows_s)
        print(f"{name} d={d} nq={nq} {layout}: worst |value - x/s| / half spacing {worst:.6f}")


@pytest.mark.parametrize("name", ["bf16", "fp8"])
def test_dequant_footprint_and_values(hip, name):
    torch, _hip = hip
    d, nq = 40, 1
    q, (kc, vc, ks, vs), kd, vd = _case(hip, name, d, nq)
    B, Hkv, N, _ = kc.shape
    want = [_host_dequant(torch, KVS[name], c, s) for c, s in ((kc, ks), (vc, vs))]
    for full, w in zip((kd, vd), want):  # kv_len = None: every row
        assert np.array_equal(_bits(full), _bits(w))
    outs = [torch.full((B, N, Hkv, d), SENT, dtype=torch.float32, device="cuda").permute(0, 2, 1, 3) for _ in range(2)]
    kv = torch.tensor([int(x) for x in LENGTHS], dtype=torch.int32, device="cuda")
    _hip.kv_cache_dequant(kc, vc, ks, vs, kv_len=kv, k_out=outs[0], v_out=outs[1])
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        o = o.contiguous().cpu().numpy()
        for b, L in enumerate(LENGTHS):
            n = KC.visible(L)
            assert np.array_equal(_bits(o[b, :, :n]), _bits(w[b, :, :n])), f"row {b}: values"
            assert (o[b, :, n:] == SENT).all(), f"row {b}: wrote at or past kv_len"


# ---- decode ----------------------------------------------------------------------------------
PARITY = [(n, d, nq, c) for n in KVS for d in (8, 40, 64, 128, 256) for nq in (1, 3, 8) for c in (True, False)]


@pytest.mark.parametrize("name,d,nq,causal", PARITY,
                         ids=[f"{n}-d{d}-nq{nq}-{'causal' if c else 'full'}" for n, d, nq, c in PARITY])
def test_decode_matches_float64_on_the_dequantised_cache(hip, name, d, nq, causal):
    torch, _hip = hip
    q, caches, kd, vd = _case(hip, name, d, nq)
    n, S, t = _hip.decode_kvq_splits(KVS[name], len(LENGTHS), KC.H, nq, KC.NMAX, d)
    assert n >= 3, "the case must take the split-KV path"
    o, m, l = _decode(hip, q, caches, LENGTHS, causal, footprint=True)
    ratio, worst_lse, none = _compare(o, m, l, q, kd, vd, KC.limits(LENGTHS, nq, causal))
    print(f"{name} d={d} nq={nq} causal={causal}: {n} splits, worst |dO| / bound {float(ratio.max()):.3f}, "
          f"worst |dlse| / bound {worst_lse:.3f}")
    assert np.isfinite(o).all()
    assert float(ratio.max()) <= 1.0
    assert worst_lse <= 1.0
    # a query with no visible key: O = 0, m = -inf, l = 0 exactly
    assert none.any()
    assert np.isneginf(m[none]).all() and not l[none].any() and not o[none].any()
    assert np.isfinite(m[~none]).all() and (l[~none] > 0).all()


GQA = [(n, H, Hkv, nq) for n in KVS for H, Hkv in ((8, 2), (6, 2), (8, 1)) for nq in (1, 3, 5)]


@pytest.mark.parametrize("name,H,Hkv,nq", GQA, ids=[f"{n}-H{H}-Hkv{k}-nq{nq}" for n, H, k, nq in GQA])
def test_grouped_queries(hip, name, H, Hkv, nq):
    """Row packing: G = 4 packs (Nq = 1), G = 3 is ragged at Nq = 3, Nq = 5 leaves one head per
    workgroup. Query head h is kv head h // G's decode_cases query, scaled per group member."""
    torch, _hip = hip
    d, G = 64, H // Hkv
    qkv, caches, kd, vd = _case(hip, name, d, nq, heads=Hkv)
    q = np.repeat(qkv, G, axis=1) * (1.0 + 0.125 * (np.arange(H) % G))[None, :, None, None].astype(np.float32)
    o, m, l = _decode(hip, q, caches, LENGTHS, True, footprint=True)
    ratio, worst_lse, none = _compare(o, m, l, q, np.repeat(kd, G, axis=1), np.repeat(vd, G, axis=1),
                                      KC.limits(LENGTHS, nq, True))
    print(f"{name} H={H} Hkv={Hkv} nq={nq}: worst |dO| / bound {float(ratio.max()):.3f}, lse {worst_lse:.3f}")
    assert float(ratio.max()) <= 1.0 and worst_lse <= 1.0
    assert np.isneginf(m[none]).all() and not l[none].any() and not o[none].any()


@pytest.mark.parametrize("name,d,nq,causal", [(n, d, nq, c) for n in KVS for d, nq, c in
                                              ((64, 3, True), (40, 1, True), (128, 8, False))])
def test_stale_tail_and_workspace_content_do_not_matter(hip, name, d, nq, causal):
    q, caches, *_ = _case(hip, name, d, nq)
    nan = _decode(hip, q, caches, LENGTHS, causal, stale="nan", footprint=True)
    zero = _decode(hip, q, caches, LENGTHS, causal, stale="zero")
    base = _decode(hip, q, caches, LENGTHS, causal)
    for a in nan:
        assert not np.isnan(a).any(), "a stale row, its scale or the workspace's old content reached the output"
    for x, y, z, nm in zip(nan, zero, base, "Oml"):
        assert np.array_equal(_bits(x), _bits(y)), f"{nm}: NaN tail != zero tail"
        assert np.array_equal(_bits(x), _bits(z)), f"{nm}: NaN tail != the cache as appended"


@pytest.mark.parametrize("name", ["bf16", "fp8"])
def test_repeat_is_bit_equal_and_one_split_leaves_the_workspace(hip, name):
    torch, _hip = hip
    q, caches, *_ = _case(hip, name, 64, 3)
    a = _decode(hip, q, caches, LENGTHS, True)
    b = _decode(hip, q, caches, LENGTHS, True)
    for x, y, nm in zip(a, b, "Oml"):
        assert np.array_equal(_bits(x), _bits(y)), f"{nm} differs between two calls"
    # (64,8,1,40,32): one split, pass 1 writes O directly
    B, H, Nk, d = 64, 8, 40, 32
    assert _hip.decode_kvq_splits(KVS[name], B, H, 1, Nk, d)[0] == 1
    assert _hip.decode_kvq_workspace_bytes(KVS[name], B, H, 1, Nk, d) == 0
    rng = np.random.default_rng(5)
    k, v = (rng.standard_normal((B, H, Nk, d)).astype(np.float32) for _ in range(2))
    q1 = rng.standard_normal((B, H, 1, d)).astype(np.float32)
    lengths = [(7 * i) % Nk + 1 for i in range(B)]
    c1 = _quantise(hip, KVS[name], k, v)
    kd, vd = (t.cpu().numpy() for t in _hip.kv_cache_dequant(*c1))
    ws = torch.full((4096,), SENT, dtype=torch.float32, device="cuda")
    o, m, l = _decode(hip, q1, c1, lengths, True, footprint=True, workspace=ws)
    assert bool((ws == SENT).all()), "one split must not touch the workspace"
    ratio, worst_lse, _ = _compare(o, m, l, q1, kd, vd, KC.limits(lengths, 1, True, nmax=Nk))
    assert float(ratio.max()) <= 1.0 and worst_lse <= 1.0


@pytest.mark.parametrize("name,causal", [(n, c) for n in KVS for c in (True, False)])
def test_shifted_limits_fail(hip, name, causal):
    """The comparison sees an off-by-one: with every visible-key count moved by one key the
    oracle leaves the bound in every batch row that has a key to lose or to gain."""
    d, nq = 64, 3
    q, caches, kd, vd = _case(hip, name, d, nq)
    o, m, l = _decode(hip, q, caches, LENGTHS, causal)
    ratio, _, _ = _compare(o, m, l, q, kd, vd, KC.limits(LENGTHS, nq, causal))
    assert float(ratio.max()) <= 1.0
    for shift in (-1, 1):
        moved, _, _ = _compare(o, m, l, q, kd, vd, KC.limits(LENGTHS, nq, causal, shift))
        per_row = moved.max(axis=(1, 2, 3))
        for b, L in enumerate(LENGTHS):
            if nq < KC.visible(L) < KC.NMAX:
                assert per_row[b] > 1.0, f"L={L} shift {shift:+d}: the comparison still passes ({per_row[b]:.3g})"


@pytest.mark.parametrize("name", ["bf16", "fp8"])
def test_graph_replay_as_the_cache_fills(hip, name):
    """Append and decode captured once at (B, H, Nk, d) = (2, 2, 1104, 64), replayed at the lengths
    1, 256, 257, 1100 (row 1 runs through them backwards): each replay equals the eager call."""
    torch, _hip = hip
    kv = KVS[name]
    B, H, nq, d, nmax = 2, 2, 1, 64, KC.NMAX
    assert _hip.decode_kvq_splits(kv, B, H, nq, nmax, d)[0] >= 3
    rng = np.random.default_rng(11)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    base = [rng.standard_normal((B, H, nmax, d)).astype(np.float32) for _ in range(2)]
    kc, vc, ks, vs = _quantise(hip, kv, *base)
    eager = [None if t is None else t.clone() for t in (kc, vc, ks, vs)]
    lens = (1, 256, 257, 1100)
    steps = [[dev(rng.standard_normal((B, H, nq, d)).astype(np.float32)) for _ in range(3)] for _ in lens]
    q, kn, vn = (torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda") for _ in range(3))
    pos, kvl = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    o = torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda")
    m, l = (torch.empty((B, H, nq), dtype=torch.float32, device="cuda") for _ in range(2))
    ws = torch.empty(_hip.decode_kvq_workspace_bytes(kv, B, H, nq, nmax, d) // 4, dtype=torch.float32, device="cuda")

    def step():
        _hip.kv_cache_append_quant(kn, vn, kc, vc, pos, ks, vs)
        _hip.flash_decode_kvq(q, kc, vc, ks, vs, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)

    def load(i):
        L = np.array([lens[i], lens[len(lens) - 1 - i]], np.int32)
        for dst, src in zip((q, kn, vn), steps[i]):
            dst.copy_(src)
        pos.copy_(dev(L - 1))
        kvl.copy_(dev(L))
        return L
    side = torch.cuda.Stream()
    load(0)
    saved = [None if t is None else t.clone() for t in (kc, vc, ks, vs)]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, t0 in zip((kc, vc, ks, vs), saved):
        if t is not None:
            t.copy_(t0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in range(len(lens)):
        L = load(i)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in (o, m, l)]
        _hip.kv_cache_append_quant(steps[i][1], steps[i][2], eager[0], eager[1], dev(L - 1), eager[2], eager[3])
        ref = _hip.flash_decode_kvq(steps[i][0], *eager, kv_len=dev(L), causal=True)
        torch.cuda.synchronize()
        for x, y, nm in zip(got, ref, "Oml"):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"replay {i}: {nm} differs from the eager call"
        for t, t0 in zip((kc, vc, ks, vs), eager):
            if t is not None:
                assert torch.equal(t.contiguous().view(torch.uint8), t0.contiguous().view(torch.uint8))
