"""The extend test inputs of tests/extend_cases.py can tell a visible-key count from that
count +- 1.

Float64 on the CPU only (no GPU): for every case, every row of EDGE_ROWS and of the rows
tests/test_extend_gpu.py runs (those with a key to drop and a key to admit), every head and both
directions, evaluating the attention with one key fewer or one key more visible per real query
moves some output of that (row, head) by at least 16x the bound the GPU test holds the kernel
to; in the causal cases the same holds for every single real query whose count is not clipped.
So a kernel that admits the first stale row of the cache, drops a query's newest key, or places
one query of a block a key off cannot pass there. The 16x is a condition on the inputs, not a
tolerance. bf16 d = 32 reaches only 14x per query and is not a case.
"""
import numpy as np
import pytest

import extend_cases as EC

# (bf16, d, keys per tile of the kernel that case runs on: the GPU test checks it against the plan)
CASES = [(True, 64, 64), (True, 128, 64), (False, 16, 32), (False, 32, 32), (False, 64, 32), (False, 68, 32),
         (False, 128, 32), (True, 256, 32), (False, 256, 32)]
BQ = 128


def _rows(bk):
    return EC.EDGE_ROWS + tuple(r for r in EC.gpu_rows(BQ, bk) if EC.has_edge(r))


# d = 256 runs causal only on the GPU
@pytest.mark.parametrize("bf16,d,bk,causal", [c + (causal,) for causal in (True, False) for c in CASES
                                              if causal or c[1] <= 128])
def test_visible_count_off_by_one_moves_every_head_and_query(bf16, d, bk, causal):
    rows = _rows(bk)
    assert all(EC.has_edge(r) for r in rows)
    q, k, v = EC.make_inputs(d, EC.NQ, bf16, rows)
    for x in (q, k, v):
        assert np.isfinite(x).all()
        if bf16:
            assert np.array_equal(EC.A.bf16_round(x), x)
    o, _, pv = EC.ref64(q, k, v, EC.limits(rows, EC.NQ, causal))
    bnd = EC.bound(bf16, o, pv)
    raw, isreal = EC.raw_limits(rows, EC.NQ)
    n = np.array([EC.visible(L) for L, _ in rows])[:, None]
    least_head = least_query = np.inf
    for shift in (-1, 1):
        o2, _, _ = EC.ref64(q, k, v, EC.limits(rows, EC.NQ, causal, shift))
        per_query = (np.abs(o2 - o) / bnd).max(axis=3)  # [B, H, Nq]
        per_head = per_query.max(axis=2)
        for b, row in enumerate(rows):
            for h in range(EC.H):
                assert per_head[b, h] >= 16.0, (f"row {row} head {h} shift {shift:+d}: moves no output by 16x "
                                                f"its bound ({per_head[b, h]:.2f})")
        least_head = min(least_head, float(per_head.min()))
        if causal:
            # a count the clamp to [0, n] leaves alone, and that the shift can move
            free = isreal & (raw >= 1) & (raw <= n)
            assert free.any(axis=1).all()
            moved = np.where(free[:, None, :], per_query, np.inf)
            b, h, i = np.unravel_index(np.argmin(moved), moved.shape)
            assert moved[b, h, i] >= 16.0, (f"row {rows[b]} head {h} query {i} shift {shift:+d}: moves by "
                                           f"{moved[b, h, i]:.2f}x its bound only")
            least_query = min(least_query, float(moved.min()))
    print(f"bf16={bf16} d={d} causal={causal}: smallest move / bound per head {least_head:.1f}, "
          f"per query {least_query:.1f}")


def test_stale_rows_and_padding_queries_do_not_reach_the_reference():
    """The float64 reference with NaN in the stale cache rows and in the Q rows >= t equals the
    finite one to the bit."""
    rows = _rows(32)
    q, k, v = EC.make_inputs(32, EC.NQ, False, rows)
    lim = EC.limits(rows, EC.NQ, True)
    a = EC.ref64(q, k, v, lim)
    qn, kn, vn = q.copy(), k.copy(), v.copy()
    for b, (L, t) in enumerate(rows):
        kn[b, :, EC.visible(L):] = np.nan
        vn[b, :, EC.visible(L):] = np.nan
        qn[b, :, EC.real(t, EC.NQ):] = np.nan
    assert np.isnan(qn).any() and np.isnan(kn).any()
    with np.errstate(invalid="ignore"):
        z = EC.ref64(qn, kn, vn, lim)
    for x, y in zip(a, z):
        np.testing.assert_array_equal(x, y)
