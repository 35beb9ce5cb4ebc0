"""Boundary-sensitive inputs for the extend attention (test infrastructure; tests/test_extend_edges.py
runs the float64 side on the CPU, tests/test_extend_gpu.py the kernel). Modelled on
tests/decode_cases.py, whose float64 reference and bounds it reuses.

One case is (dtype, d, Nq, rows): H query heads, a cache of NMAX rows, and one batch row per
entry (L, t) of `rows`. With n = clamp(L, 0, NMAX) keys held and t = clamp(t, 0, Nq) real
queries, query i < t sits at position p_i = n - t + i and sees the keys j < clamp(p_i + 1, 0, n)
(causal, aligned bottom-right) or j < n (non-causal); a query i >= t sees none.

Values: N(0,1), rounded to bf16 for the bf16 cases. The key at every real query's position is
rescaled to the norm 4 sqrt(d), direction kept (re-rounded to bf16 for the bf16 cases). decode_cases
multiplies those keys by 4 instead; with up to 168 such keys per row a key that came out short then
yields a huge query, whose own key loses all its weight to that query's logits on the other
spiked keys (fp32 d = 16 fell below the 16x condition of test_extend_edges.py that way). Every
stale row >= n is x4 and the stale V rows are 64: finite and bf16-exact (the GPU test also runs
with NaN there). Query i is

    8 sqrt(d) (K[p_i] / |K[p_i]|^2 + K[p_i + 1] / |K[p_i + 1]|^2)

with K the query head's kv head: a logit of about 8 on its last visible key and on the first key
it must not see. A term whose key is outside [0, NMAX) is left out; a query with neither key, and
every query i >= t, is N(0,1).
"""
import numpy as np

import decode_cases as DC
from oracle import attention as A

H = 2
NMAX = 448
NQ = 168
STALE_K = 4.0
STALE_V = 64.0
ref64 = DC.ref64
bound = DC.bound
# the rows tests/test_extend_edges.py checks on the CPU, (cache length, real queries)
EDGE_ROWS = ((1, 1), (9, 9), (40, 9), (128, 128), (129, 128), (160, 33), (200, 168), (255, 127), (256, 129),
             (257, 64), (300, 1), (333, 168), (400, 160), (447, 130), (447, 2))


def visible(L, nmax=NMAX):
    return int(min(max(int(L), 0), nmax))


def real(t, nq):
    return int(min(max(int(t), 0), nq))


def gpu_rows(bq, bk, nq=NQ, nmax=NMAX):
    """The rows of tests/test_extend_gpu.py for a kernel that owns bq queries per workgroup and
    streams bk keys per tile: EDGE_ROWS with their edges replaced by t in {1, bq - 1, bq, bq + 1,
    nq} against a prefix n - t in {0, 1, bk - 1, bk, bk + 1} (every t with the prefixes of the same
    parity in that list, 13 pairs), then a full cache, a length past the capacity, a row with no
    new token and a row with more new tokens than keys."""
    ts = (1, bq - 1, bq, bq + 1, nq)
    pre = (0, 1, bk - 1, bk, bk + 1)
    rows = [(t + p, t) for a, t in enumerate(ts) for c, p in enumerate(pre) if (a + c) % 2 == 0]
    rows += [(40, 9), (160, 33), (257, 64), (300, 1), (400, 160), (447, 130), (447, 2)]
    rows += [(nmax, bq + 1), (nmax + 7, nq), (nmax, 1), (200, 0), (0, 0), (5, 9), (bq - 3, bq + 2)]
    assert all(L <= nmax + 7 for L, _ in rows) and nq >= bq + 33 and nmax >= 3 * bq + 64
    return tuple(rows)


def has_edge(row, nq=NQ, nmax=NMAX):
    """A row with a key to drop and a key to admit: some real query, and not a full cache."""
    return real(row[1], nq) > 0 and 0 < visible(row[0], nmax) < nmax


def make_inputs(d, nq, bf16, rows, seed=0, nmax=NMAX, heads=H, kv_heads=None):
    """(q [B,heads,nq,d], k [B,kv_heads,nmax,d], v likewise) fp32 arrays (bf16-exact when bf16), one
    batch row per entry (L, t) of `rows`. kv_heads (None: heads) must divide heads."""
    kv_heads = heads if kv_heads is None else kv_heads
    assert heads % kv_heads == 0
    group = heads // kv_heads
    rng = np.random.default_rng([seed, d, nq, int(bf16), heads, kv_heads])
    B = len(rows)
    k = rng.standard_normal((B, kv_heads, nmax, d)).astype(np.float32)
    v = rng.standard_normal((B, kv_heads, nmax, d)).astype(np.float32)
    q = rng.standard_normal((B, heads, nq, d)).astype(np.float32)
    rnd = A.bf16_round if bf16 else (lambda x: x)
    q, k, v = rnd(q), rnd(k), rnd(v)
    for b, (L, t) in enumerate(rows):
        n, t = visible(L, nmax), real(t, nq)
        lo = max(n - t, 0)
        if n > lo:  # the keys at the real queries' positions: norm 4 sqrt(d)
            kk = k[b, :, lo:n].astype(np.float64)
            kk *= 4.0 * np.sqrt(d) / np.sqrt((kk * kk).sum(-1, keepdims=True))
            k[b, :, lo:n] = rnd(kk.astype(np.float32))
        k[b, :, n:] *= np.float32(STALE_K)
        v[b, :, n:] = np.float32(STALE_V)
        for i in range(t):
            p = n - t + i
            acc = np.zeros((kv_heads, d), np.float64)
            used = False
            for j in (p, p + 1):
                if 0 <= j < nmax:
                    kj = k[b, :, j].astype(np.float64)
                    acc += kj / (kj * kj).sum(-1, keepdims=True)
                    used = True
            if used:
                qi = np.repeat((8.0 * np.sqrt(d) * acc).astype(np.float32), group, axis=0)
                q[b, :, i] = rnd(qi)
    return q, k, v


def raw_limits(rows, nq, nmax=NMAX):
    """[B, nq] the causal count n - t + 1 + i before it is clipped to [0, n] (real queries only;
    the others hold 0) and the [B, nq] mask of the real queries."""
    n = np.array([visible(L, nmax) for L, _ in rows])[:, None]
    t = np.array([real(t, nq) for _, t in rows])[:, None]
    i = np.arange(nq)[None, :]
    isreal = i < t
    return np.where(isreal, n - t + 1 + i, 0), isreal


def limits(rows, nq, causal, shift=0, nmax=NMAX):
    """[B, nq] visible-key count per query: clamp(n - t + 1 + i, 0, n) (causal) or n for a real
    query i < t, 0 for the others. `shift` moves every real query's count by that many keys (the
    off-by-one a kernel could make), clipped to [0, nmax]."""
    n = np.array([visible(L, nmax) for L, _ in rows])[:, None]
    raw, isreal = raw_limits(rows, nq, nmax)
    lim = np.clip(raw, 0, n) if causal else np.broadcast_to(n, raw.shape)
    return np.where(isreal, np.clip(lim + shift, 0, nmax), 0)


def repeat_kv(x, heads):
    """[B, kv_heads, ...] -> [B, heads, ...]: query head h reads kv head h // (heads // kv_heads)."""
    return np.repeat(x, heads // x.shape[1], axis=1)


def place_queries(q, rows, nmax=NMAX):
    """The full-length problem of a causal forward: Q [B,H,nmax,d], zero except the real queries at
    their positions; returns (Qfull, pos [B, nq]) with pos < 0 for a query that is not real or sits
    before the row's start."""
    B, heads, nq, d = q.shape
    qf = np.zeros((B, heads, nmax, d), np.float32)
    pos = np.full((B, nq), -1, np.int64)
    for b, (L, t) in enumerate(rows):
        n, t = visible(L, nmax), real(t, nq)
        for i in range(t):
            p = n - t + i
            if p >= 0:
                pos[b, i] = p
                qf[b, :, p] = q[b, :, i]
    return qf, pos
