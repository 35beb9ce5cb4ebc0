"""Boundary-sensitive inputs for the KV-cache decode attention (test infrastructure;
tests/test_decode_edges.py runs the float64 side on the CPU, tests/test_decode_gpu.py the
kernels). Modelled on tests/varlen_cases.py.

One case is (dtype, d, Nq) with H = 2 heads and a cache of NMAX = 1104 rows; one batch row per
cache length L. With n = clamp(L, 0, NMAX) visible keys the Nq queries of a row sit at the
positions p_i = n - Nq + i, and query i sees the keys j < p_i + 1 (causal, aligned bottom-right)
or j < n (non-causal).

Values: N(0,1), rounded to bf16 for the bf16 cases. Per row the keys at the query positions and
every stale row >= n are x4 and the stale V rows are 64: all finite and bf16-exact (the GPU test
then overwrites the stale rows with NaN as well). Query i is

    8 sqrt(d) (K[p_i] / |K[p_i]|^2 + K[p_i + 1] / |K[p_i + 1]|^2)

which puts a logit of about 8 on its last visible key and on the first key it must not see,
whatever their norms. (The plain (K[p] + K[p + 1]) / sqrt(d) query of varlen_cases.py puts
|K|^2 / sqrt(d) on each, which at Nq = 1 differ by up to +-8 between the two keys, and some
heads then move by under 3x their bound.) A term whose key is outside [0, NMAX) is left out; a
query with neither key (p_i < -1) is N(0,1).
"""
import numpy as np

from oracle import attention as A

H = 2
NMAX = 1104
SPIKE = 4.0
STALE_V = 64.0
# the lengths tests/test_decode_edges.py checks on the CPU
EDGE_LENGTHS = (1, 2, 5, 6, 255, 256, 257, 511, 512, 513, 1099, 1100)


def visible(L, nmax=NMAX):
    return int(min(max(int(L), 0), nmax))


def make_inputs(d, nq, bf16, lengths, seed=0, nmax=NMAX, heads=H):
    """(q [B,H,nq,d], k [B,H,nmax,d], v [B,H,nmax,d]) fp32 arrays (bf16-exact when bf16), one
    batch row per entry of `lengths`."""
    rng = np.random.default_rng([seed, d, nq, int(bf16)])
    B = len(lengths)
    k = rng.standard_normal((B, heads, nmax, d)).astype(np.float32)
    v = rng.standard_normal((B, heads, nmax, d)).astype(np.float32)
    q = rng.standard_normal((B, heads, nq, d)).astype(np.float32)
    if bf16:
        q, k, v = (A.bf16_round(x) for x in (q, k, v))
    for b, L in enumerate(lengths):
        n = visible(L, nmax)
        for i in range(nq):
            p = n - nq + i
            if 0 <= p < n:
                k[b, :, p] *= np.float32(SPIKE)
        k[b, :, n:] *= np.float32(SPIKE)
        v[b, :, n:] = np.float32(STALE_V)
        for i in range(nq):
            p = n - nq + i
            acc = np.zeros((heads, d), np.float64)
            used = False
            for j in (p, p + 1):
                if 0 <= j < nmax:
                    kj = k[b, :, j].astype(np.float64)
                    acc += kj / (kj * kj).sum(-1, keepdims=True)
                    used = True
            if used:
                qi = (8.0 * np.sqrt(d) * acc).astype(np.float32)
                q[b, :, i] = A.bf16_round(qi) if bf16 else qi
    return q, k, v


def limits(lengths, nq, causal, shift=0, nmax=NMAX):
    """[B, nq] visible-key count per query; `shift` moves every count by that many keys (the
    off-by-one a kernel could make), clipped to [0, nmax]."""
    n = np.array([visible(L, nmax) for L in lengths])[:, None]
    lim = n - nq + 1 + np.arange(nq)[None, :] if causal else np.broadcast_to(n, (len(lengths), nq)).copy()
    return np.clip(np.clip(lim, 0, nmax) + shift, 0, nmax)


def ref64(q, k, v, lim):
    """Float64 decode attention with the visible-key counts lim [B, nq]: (O, lse, P|V|), a query
    with no visible key giving O = 0, lse = -inf."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    B, heads, nq, d = q.shape
    nmax = k.shape[2]
    s = np.einsum("bhqd,bhkd->bhqk", q, k) / np.sqrt(d)
    mask = np.arange(nmax)[None, None, None, :] >= np.asarray(lim)[:, None, :, None]
    s = np.where(mask, -np.inf, s)
    mx = s.max(-1, keepdims=True)
    ms = np.where(np.isneginf(mx), 0.0, mx)
    p = np.exp(s - ms)
    tot = p.sum(-1, keepdims=True)
    pn = np.where(tot > 0, p / np.where(tot > 0, tot, 1.0), 0.0)
    # the stale rows are masked by selection, never multiplied: zero them so that a non-finite
    # stale value cannot reach the products
    live = ~mask.all(axis=2, keepdims=True)              # [B,1,1,nmax]: some query sees the key
    vz = np.where(np.swapaxes(live, 2, 3), v, 0.0)
    o = np.einsum("bhqk,bhkd->bhqd", pn, vz)
    pv = np.einsum("bhqk,bhkd->bhqd", pn, np.abs(vz))
    with np.errstate(divide="ignore"):
        lse = (mx + np.log(tot))[..., 0]
    return o, lse, pv


def bound(dtype_bf16, o_ref, pv):
    """The elementwise O bound: fp32 1e-5 + 1e-5 |O| (the project's fp32 criterion), bf16
    1e-3 + 2^-7 P|V| (the forward line of tests/bounds.py)."""
    if dtype_bf16:
        from bounds import R_BF16
        return 1e-3 + R_BF16 * np.asarray(pv, np.float64)
    return 1e-5 + 1e-5 * np.abs(np.asarray(o_ref, np.float64))


def place_queries(q, lengths, nmax=NMAX):
    """The full-length problem of the oracle: Q [B,H,nmax,d] zero except the decode queries at
    their positions; returns (Qfull, pos [B, nq]) with pos < 0 for a query before the row's start."""
    B, heads, nq, d = q.shape
    qf = np.zeros((B, heads, nmax, d), np.float32)
    pos = np.empty((B, nq), np.int64)
    for b, L in enumerate(lengths):
        n = visible(L, nmax)
        for i in range(nq):
            p = n - nq + i
            pos[b, i] = p
            if p >= 0:
                qf[b, :, p] = q[b, :, i]
    return qf, pos
