"""Grouped-query decode attention (csrc/fa_decode.hip through mt_flash_attn_decode_gqa) on the GPU:
H query heads against caches of Hkv < H heads, query head h reading kv head h // (H // Hkv).

Inputs: K / V of Hkv heads from tests/decode_cases.py, repeated to H heads (np.repeat, axis 1)
for the reference. The queries follow decode_cases's rule on the repeated K (a logit of about 8 on
the last visible key and on the first key a query must not see), plus, per query head, an N(0,1)
vector made orthogonal to those two keys: the heads of a group then differ (a kernel that mixed
them up inside a group would be seen) while the two boundary logits stay what the rule gives.
One batch row per cache length; the lengths come from the library's split answer for the GQA
sizes (span S, wave tile t): the edges of a tile, a span and two spans, 0, 1, Nq +- 1, the ends of
the cache and one length above its capacity.

Reference: oracle.cref.attn_fwd on the full [B, H, 1104, d] problem with the repeated K / V, as
tests/test_decode_gpu.py does. Bounds (decode_cases.bound): fp32 |dO| <= 1e-5 + 1e-5 |O| and the
log-sum-exp within 1e-5 + 1e-5 |lse|; bf16 |dO| <= 1e-3 + 2^-7 (P|V|) and the lse within 2e-3.
"""
import functools

import numpy as np
import pytest

import decode_cases as DC
from oracle import attention as A

pytestmark = pytest.mark.gpu

CODES = {"f32": 0, "bf16": 1, "bf16_f32o": 2}
# (dtype, d, H, Hkv, Nq, causal)
CASES = [
    ("f32", 64, 4, 1, 1, True),        # MQA, 4 rows packed (NQ = 4)
    ("f32", 64, 4, 2, 4, True),        # 2 heads x 4 queries = 8 rows (NQ = 8)
    ("f32", 16, 8, 1, 1, True),        # a full group of 8 in one workgroup, LPK = 4
    ("f32", 128, 6, 2, 3, True),       # G = 3, gs = 2: ragged last slice
    ("bf16", 64, 16, 1, 1, True),      # G = 16 > 8: two slices
    ("bf16", 128, 4, 2, 2, True),      # LPK = 16, 4 rows
    ("bf16_f32o", 64, 4, 1, 2, True),  # fp32 O, 8 rows
    ("f32", 64, 4, 2, 5, True),        # gs = 1: one head per workgroup
    ("bf16", 64, 4, 2, 3, False),
]
IDS = [f"{n}-d{d}-h{H}kv{Hkv}-nq{nq}-{'causal' if c else 'full'}" for n, d, H, Hkv, nq, c in CASES]
GS1 = ("f32", 64, 4, 2, 5, True)
B_ROWS = 18
SENT = 768.0  # exact in bf16


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def _lengths(_hip, name, d, H, Hkv, nq):
    n, S, t = _hip.decode_splits(CODES[name], B_ROWS, H, nq, DC.NMAX, d, Hkv=Hkv)
    L = [0, 1, nq - 1, nq, nq + 1, t - 1, t, t + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1,
         1099, 1100, DC.NMAX, DC.NMAX + 7]
    assert len(L) == B_ROWS and 2 * S + 1 <= DC.NMAX
    return n, L


def _queries(kr, nq, bf16, lengths, seed):
    """Q [B,H,nq,d] for the repeated keys kr [B,H,NMAX,d]: decode_cases's query
    8 sqrt(d) (K[p] / |K[p]|^2 + K[p+1] / |K[p+1]|^2) per head, plus an N(0,1) vector per query
    head with its components along K[p] and K[p+1] removed (float64 Gram-Schmidt)."""
    B, H, nmax, d = kr.shape
    rng = np.random.default_rng([seed, d, nq, H])
    q = rng.standard_normal((B, H, nq, d)).astype(np.float32)
    for b, L in enumerate(lengths):
        n = DC.visible(L)
        for i in range(nq):
            p = n - nq + i
            basis = []
            acc = np.zeros((H, d), np.float64)
            for j in (p, p + 1):
                if 0 <= j < nmax:
                    kj = kr[b, :, j].astype(np.float64)
                    acc += kj / (kj * kj).sum(-1, keepdims=True)
                    for e in basis:
                        kj = kj - (kj * e).sum(-1, keepdims=True) * e
                    basis.append(kj / np.sqrt((kj * kj).sum(-1, keepdims=True)))
            if basis:
                noise = q[b, :, i].astype(np.float64)
                for e in basis:
                    noise = noise - (noise * e).sum(-1, keepdims=True) * e
                q[b, :, i] = (8.0 * np.sqrt(d) * acc + noise).astype(np.float32)
    return A.bf16_round(q) if bf16 else q


@functools.lru_cache(maxsize=None)
def _reference(bf16, d, H, Hkv, nq, causal, lengths):
    """Inputs (q [B,H,..], k / v [B,Hkv,..]) and the oracle's (O, m, l) [B,H,nq,...] on the repeated
    K / V for one case, computed once."""
    from oracle import cref
    G = H // Hkv
    _, k, v = DC.make_inputs(d, nq, bf16, lengths, heads=Hkv)
    kr, vr = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
    q = _queries(kr, nq, bf16, lengths, seed=7)
    # the heads of a group must differ, or a mix-up inside a group would go unseen
    assert all(not np.array_equal(q[:, g * G], q[:, g * G + 1]) for g in range(Hkv))
    nvis = np.array([DC.visible(L) for L in lengths], np.int32)
    B = len(lengths)
    if causal:
        qf, pos = DC.place_queries(q, lengths)
    else:  # kv_len alone masks: the rows the queries sit in do not matter
        qf = np.zeros((B, H, DC.NMAX, d), np.float32)
        qf[:, :, :nq] = q
        pos = np.broadcast_to(np.arange(nq), (B, nq)).copy()
    of, mf, lf = cref.attn_fwd(qf, kr, vr, causal=causal, kv_len=nvis)
    o = np.zeros((B, H, nq, d), np.float32)
    m = np.full((B, H, nq), -np.inf, np.float32)
    l = np.zeros((B, H, nq), np.float32)
    for b in range(B):
        for i in range(nq):
            if pos[b, i] >= 0:
                o[b, :, i], m[b, :, i], l[b, :, i] = of[b, :, pos[b, i]], mf[b, :, pos[b, i]], lf[b, :, pos[b, i]]
    _, _, pv = DC.ref64(q, kr, vr, DC.limits(lengths, nq, causal))
    for a in (q, k, v, o, m, l, pv):
        a.setflags(write=False)
    return q, k, v, o, m, l, pv


def _run(hip, name, q, k, v, lengths, causal, layout="dense", stale=None, footprint=False, plain=False):
    """One decode call; returns (O, m, l) as numpy (O as float32). q [B,H,nq,d], k / v
    [B,Hkv,Nmax,d]. layout 'bnhd': the caches as [B,Nmax,Hkv,d] storage, Q and O as [B,Nq,H,d]
    storage. stale: a value written to every cache row >= the row's visible length and to the
    whole workspace beforehand. plain: through mt_flash_attn_decode (needs Hkv == H) instead of
    the binding's mt_flash_attn_decode_gqa."""
    torch, _hip = hip
    code = CODES[name]
    tin = torch.float32 if name == "f32" else torch.bfloat16
    tout = torch.bfloat16 if name == "bf16" else torch.float32
    B, H, nq, d = q.shape
    Hkv, nk = k.shape[1], k.shape[2]
    k, v = k.copy(), v.copy()
    if stale is not None:
        for b, L in enumerate(lengths):
            k[b, :, DC.visible(L):] = stale
            v[b, :, DC.visible(L):] = stale

    def put(a):
        t = torch.from_numpy(np.array(a)).to("cuda").to(tin)
        if layout == "bnhd":
            t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
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
    need = _hip.decode_workspace_bytes(code, B, H, nq, nk, d, Hkv=Hkv)
    assert need % 4 == 0
    wbuf = torch.full((need // 4 + pad,), SENT if stale is None else float(stale), dtype=torch.float32, device="cuda")
    if stale is not None:
        wbuf[need // 4:] = SENT
    ws = wbuf[:need // 4] if need else None
    before = [t.clone() for t in (tq, tk, tv)]
    if plain:
        assert Hkv == H and need == _hip.decode_workspace_bytes(code, B, H, nq, nk, d)
        _hip.check(_hip.lib().mt_flash_attn_decode(
            code, int(causal), tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), o.data_ptr(), m.data_ptr(), l.data_ptr(),
            B, H, nq, nk, d, _hip.strides3(tq), _hip.strides3(tk), _hip.strides3(tv), _hip.strides3(o),
            kv.data_ptr(), None if ws is None else ws.data_ptr(), need, _hip.stream_ptr(tq.device)),
            "mt_flash_attn_decode")
    else:
        _hip.flash_decode(tq, tk, tv, kv_len=kv, causal=causal, out=o, m=m, l=l, workspace=ws)
    torch.cuda.synchronize()
    if footprint:
        for buf, n in ((obuf, B * H * nq * d), (mbuf, B * H * nq), (lbuf, B * H * nq)):
            assert bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all()), "wrote outside O / m / l"
        assert bool((wbuf[need // 4:] == SENT).all()), "wrote past the advertised workspace"
        ity = torch.int16 if tin == torch.bfloat16 else torch.int32
        for t, t0 in zip((tq, tk, tv), before):
            assert torch.equal(t.view(ity), t0.view(ity)), "inputs changed"
    return o.float().cpu().numpy(), m.cpu().numpy(), l.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(hip, name, d, H, Hkv, nq, causal):
    n, lengths = _lengths(hip[1], name, d, H, Hkv, nq)
    assert n >= 3, f"{n} splits: the case does not exercise the split-KV path"
    return tuple(lengths), _reference(name != "f32", d, H, Hkv, nq, causal, tuple(lengths))


@pytest.mark.parametrize("name,d,H,Hkv,nq,causal", CASES, ids=IDS)
def test_gqa_decode_matches_oracle(hip, name, d, H, Hkv, nq, causal, parity_record):
    lengths, (q, k, v, o_ref, m_ref, l_ref, pv) = _case(hip, name, d, H, Hkv, nq, causal)
    o, m, l = _run(hip, name, q, k, v, lengths, causal, footprint=True)
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
    case = f"{name} d={d} H={H} Hkv={Hkv} nq={nq} causal={causal}"
    print(f"{case}: worst |dO| / bound {worst:.3f}, worst |dlse| / bound {worst_lse:.3f}, max |dO| {float(err.max()):.3e}")
    parity_record("test_gqa_decode_matches_oracle", case, max_abs=float(err.max()), worst_over_bound=worst,
                  lse_over_bound=worst_lse, bound=1.0)
    assert np.isfinite(o).all()
    assert worst <= 1.0
    assert worst_lse <= 1.0
    # a query with no visible key: O = 0, m = -inf, l = 0 exactly
    assert none.any()
    assert np.isneginf(m[none]).all() and not l[none].any() and not o[none].any()
    assert np.isfinite(m[~none]).all() and (l[~none] > 0).all()


@pytest.mark.parametrize("name,d,H,Hkv,nq,causal", CASES, ids=IDS)
def test_gqa_nan_tail_strided_and_repeat_are_bit_equal(hip, name, d, H, Hkv, nq, causal):
    lengths, (q, k, v, *_r) = _case(hip, name, d, H, Hkv, nq, causal)
    base = _run(hip, name, q, k, v, lengths, causal)
    nan_strided = _run(hip, name, q, k, v, lengths, causal, layout="bnhd", stale=np.nan, footprint=True)
    again = _run(hip, name, q, k, v, lengths, causal, layout="bnhd", stale=np.nan)
    for a in nan_strided:
        assert not np.isnan(a).any(), "a stale cache row or the workspace's old content reached the output"
    assert np.isfinite(nan_strided[0]).all()
    for what, other in (("NaN stale rows, [B,N,Hkv,d] storage", nan_strided), ("its repeat", again)):
        for x, y, nm in zip(base, other, "Oml"):
            assert np.array_equal(_bits(x), _bits(y)), f"{nm} differs: {what}"


@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=[IDS[1], IDS[5]])
def test_hkv_equal_h_is_mt_flash_attn_decode(hip, case):
    """Hkv = H through the new entry point against the plain one, same inputs (the case's K / V
    repeated to H heads): bit-equal O, m, l."""
    name, d, H, Hkv, nq, causal = case
    lengths, (q, k, v, *_r) = _case(hip, name, d, H, Hkv, nq, causal)
    kr, vr = np.repeat(k, H // Hkv, axis=1), np.repeat(v, H // Hkv, axis=1)
    gqa = _run(hip, name, q, kr, vr, lengths, causal, footprint=True)
    plain = _run(hip, name, q, kr, vr, lengths, causal, plain=True, footprint=True)
    for x, y, nm in zip(gqa, plain, "Oml"):
        assert np.array_equal(_bits(x), _bits(y)), f"{nm} differs"


def test_one_head_per_workgroup_equals_repeated_kv(hip):
    """gs = 1 (Nq = 5: one head's 5 queries fill a workgroup's rows): the plan is that of H plain
    heads and every workgroup does the plain kernel's work for one head, so the output is
    bit-equal to mt_flash_attn_decode on the repeated K / V."""
    name, d, H, Hkv, nq, causal = GS1
    _hip = hip[1]
    assert _hip.decode_splits(CODES[name], B_ROWS, H, nq, DC.NMAX, d, Hkv=Hkv) == \
        _hip.decode_splits(CODES[name], B_ROWS, H, nq, DC.NMAX, d)
    lengths, (q, k, v, *_r) = _case(hip, name, d, H, Hkv, nq, causal)
    kr, vr = np.repeat(k, H // Hkv, axis=1), np.repeat(v, H // Hkv, axis=1)
    gqa = _run(hip, name, q, k, v, lengths, causal)
    plain = _run(hip, name, q, kr, vr, lengths, causal, plain=True)
    for x, y, nm in zip(gqa, plain, "Oml"):
        assert np.array_equal(_bits(x), _bits(y)), f"{nm} differs"


def test_flash_decode_refuses_mismatched_heads(hip):
    torch, _hip = hip
    q = torch.zeros((1, 6, 1, 64), device="cuda")
    kc = torch.zeros((1, 4, 32, 64), device="cuda")
    with pytest.raises(ValueError, match="do not divide"):
        _hip.flash_decode(q, kc, kc)
    with pytest.raises(ValueError, match="do not match"):
        _hip.flash_decode(q, kc[:, :3], kc[:, :2])


@pytest.mark.parametrize("name,d", [("f32", 16), ("bf16", 64)])
def test_kv_cache_append_kv_heads(hip, name, d):
    """Hkv-head new rows ([B,Nq,Hkv,d] storage) into an Hkv-head cache ([B,Nmax,Hkv,d] storage)
    at per-row positions: rows outside the new ones keep their bits, a row past the capacity is
    dropped."""
    torch, _hip = hip
    tin = torch.float32 if name == "f32" else torch.bfloat16
    ity = torch.int32 if name == "f32" else torch.int16
    B, Hkv, nq, nmax = 4, 2, 3, 16
    pos = [0, 5, 14, 16]  # 14: rows 14, 15 land and 16 is dropped; 16: nothing lands
    g = torch.Generator(device="cpu").manual_seed(3)
    kn, vn = (torch.randn((B, nq, Hkv, d), generator=g).to(tin).cuda().permute(0, 2, 1, 3) for _ in range(2))
    kc, vc = (torch.full((B, nmax, Hkv, d), float("nan"), dtype=tin, device="cuda").permute(0, 2, 1, 3)
              for _ in range(2))
    _hip.kv_cache_append(kn, vn, kc, vc, torch.tensor(pos, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for new, c in ((kn, kc), (vn, vc)):
        want = torch.full((B, Hkv, nmax, d), float("nan"), dtype=tin, device="cuda")
        for b, p in enumerate(pos):
            for i in range(nq):
                if p + i < nmax:
                    want[b, :, p + i] = new[b, :, i]
        assert torch.equal(c.contiguous().view(ity), want.view(ity)), "the cache differs from source rows + NaN elsewhere"
