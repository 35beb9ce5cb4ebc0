"""The decode test inputs of tests/decode_cases.py can tell a visible-key count from that
count +- 1.

Float64 on the CPU only (no GPU): for every case, every cache length of EDGE_LENGTHS, every
head and both directions, evaluating the attention with one key fewer or one key more visible
per query moves some output of that head by at least 16x the bound tests/test_decode_gpu.py
holds the kernels to. So a kernel that admits the first stale row of the cache, or drops a
query's newest key, cannot pass there. The 16x is a condition on the inputs, not a tolerance.
No head is excluded: EDGE_LENGTHS has no full-cache row (the only row with no key to admit).
"""
import numpy as np
import pytest

import decode_cases as DC

CASES = [(True, 64), (True, 128), (False, 64), (False, 32), (False, 16)]


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("nq", [1, 5, 8])
@pytest.mark.parametrize("bf16,d", CASES)
def test_visible_count_off_by_one_moves_every_head(bf16, d, nq, causal):
    lengths = DC.EDGE_LENGTHS
    assert max(lengths) < DC.NMAX
    q, k, v = DC.make_inputs(d, nq, bf16, lengths)
    for x in (q, k, v):
        assert np.isfinite(x).all()
        if bf16:
            assert np.array_equal(DC.A.bf16_round(x), x)
    o, _, pv = DC.ref64(q, k, v, DC.limits(lengths, nq, causal))
    bnd = DC.bound(bf16, o, pv)
    least = np.inf
    for shift in (-1, 1):
        o2, _, _ = DC.ref64(q, k, v, DC.limits(lengths, nq, causal, shift))
        ratio = (np.abs(o2 - o) / bnd).max(axis=(2, 3))  # [B, H]
        for b, L in enumerate(lengths):
            for h in range(DC.H):
                assert ratio[b, h] >= 16.0, (f"L={L} head {h} shift {shift:+d}: moves no output by 16x its "
                                             f"bound ({ratio[b, h]:.2f})")
        least = min(least, float(ratio.min()))
    print(f"bf16={bf16} d={d} nq={nq} causal={causal}: smallest move / bound {least:.1f}")


def test_stale_rows_do_not_reach_the_reference():
    """The float64 reference with the stale cache rows set to NaN equals the finite one to the bit."""
    lengths = DC.EDGE_LENGTHS
    q, k, v = DC.make_inputs(32, 5, False, lengths)
    a = DC.ref64(q, k, v, DC.limits(lengths, 5, True))
    kn, vn = k.copy(), v.copy()
    for b, L in enumerate(lengths):
        kn[b, :, L:] = np.nan
        vn[b, :, L:] = np.nan
    with np.errstate(invalid="ignore"):
        z = DC.ref64(q, kn, vn, DC.limits(lengths, 5, True))
    for x, y in zip(a, z):
        np.testing.assert_array_equal(x, y)
