"""The key-padding test inputs of tests/varlen_cases.py can tell kv_len from kv_len +- 1.

Oracle only (no GPU): for every batch row of a case and both directions, moving that row's
kv_len by one key moves at least one of O, dQ, dK, dV by 3x its own error bound or more, so a
kernel that masks `j > kv_len`, or `j >= kv_len - 1`, cannot pass the GPU tests
(tests/test_varlen_matrix_gpu.py). The 3x is a condition on the inputs: a shape that cannot meet it
needs other inputs, not another factor. And the padding rows of K / V cannot reach the valid
region: zeroing them changes nothing there.
"""
import numpy as np
import pytest

import varlen_cases as VC


def _moved(base, other, bounds):
    """max over elements of |other - base| / bound per output (O, dQ, dK, dV), per (b, h)."""
    o, _, _, dq, dk, dv = base
    o2, _, _, dq2, dk2, dv2 = other
    return np.stack([(np.abs(np.asarray(y, np.float64) - x) / bd).max(axis=(2, 3))
                     for x, y, bd in zip((o, dq, dk, dv), (o2, dq2, dk2, dv2), bounds)])


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [20, 32, 48, 64, 96, 128])
def test_kv_len_off_by_one_moves_outputs_bf16(d, causal):
    """bf16 cases under the elementwise bounds of tests/bounds.py (the widest bounds the GPU
    tests use; the fp32 cases' flat bounds are 100x tighter), every head of every row."""
    H = 2
    kv = np.array(VC.KV_LEN)
    q, k, v, do = VC.make_inputs(d, H, bf16=True)
    for x in (q, k, v, do):
        assert np.isfinite(x).all() and np.array_equal(VC.A.bf16_round(x), x)
    base = VC.oracle_numpy(q, k, v, do, causal, kv)
    p_abs = VC.A.attention_fwd(q, k, np.abs(v), causal, kv)[0]
    bounds = VC.bf16_bounds(q, k, v, do, causal, kv, p_abs)
    least = np.inf
    for step in (-1, 1):
        kv2 = np.clip(kv + step, 0, VC.N)
        rows = np.nonzero(kv2 != kv)[0]  # kv_len = 0 has no key to drop, 300 none to admit
        assert len(rows) == len(kv) - 1
        ratio = _moved(base, VC.oracle_numpy(q, k, v, do, causal, kv2), bounds).max(axis=0)
        for b in rows:
            for h in range(H):
                assert ratio[b, h] >= 3.0, (f"kv_len {kv[b]} -> {kv2[b]} (head {h}) moves no output by 3x its "
                                            f"bound: {ratio[b, h]:.2f}")
        least = min(least, float(ratio[rows].min()))
    print(f"d={d} causal={causal}: smallest move / bound {least:.1f}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [18, 20, 64, 128, 200])
def test_kv_len_off_by_one_moves_outputs_fp32(d, causal):
    """fp32 cases under the project's fp32 bounds (1e-5 on O, 2e-5 x max|ref| on gradients)."""
    kv = np.array(VC.KV_LEN)
    q, k, v, do = VC.make_inputs(d, 1, bf16=False)
    base = VC.oracle_numpy(q, k, v, do, causal, kv)
    scale = max(1.0, *(float(np.abs(g).max()) for g in base[3:]))
    bounds = (1e-5, 2e-5 * scale, 2e-5 * scale, 2e-5 * scale)
    for step in (-1, 1):
        kv2 = np.clip(kv + step, 0, VC.N)
        rows = np.nonzero(kv2 != kv)[0]
        ratio = _moved(base, VC.oracle_numpy(q, k, v, do, causal, kv2), bounds).max(axis=0)
        assert (ratio[rows] >= 3.0).all(), (kv[rows], ratio[rows, 0])


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d,bf16", [(64, True), (128, True), (64, False)])
def test_padding_rows_do_not_reach_valid_region(d, bf16, causal):
    """The oracle with the padding rows of K / V zeroed: O, dQ, (m, l) and the valid rows of
    dK / dV are unchanged to the bit (a masked key has P = 0 exactly), and dK = dV = 0 past
    kv_len either way."""
    kv = VC.KV_LEN
    q, k, v, do = VC.make_inputs(d, 2, bf16)
    kz, vz = VC.zero_padding(k, v, kv)
    a = VC.oracle_numpy(q, k, v, do, causal, kv)
    z = VC.oracle_numpy(q, kz, vz, do, causal, kv)
    for x, y in zip(a[:4], z[:4]):  # o, m, l, dq
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a[4:], z[4:]):  # dk, dv
        for b, n in enumerate(kv):
            np.testing.assert_array_equal(x[b, :, :n], y[b, :, :n])
            assert not x[b, :, n:].any() and not y[b, :, n:].any()
    b0 = kv.index(0)
    assert not a[0][b0].any() and not a[3][b0].any()
    assert np.isneginf(a[1][b0]).all() and not a[2][b0].any()


@pytest.mark.parametrize("causal", [False, True])
def test_bounds_torch_form_matches_numpy_with_kv(causal):
    """bounds.grad_bounds_torch with kv (the GPU tests' form, all heads at once) gives the
    bounds of bounds.grad_bounds, the empty row included."""
    kv = VC.KV_LEN
    q, k, v, do = VC.make_inputs(32, 1, bf16=True)
    p_abs = VC.A.attention_fwd(q, k, np.abs(v), causal, kv)[0]
    for x, y in zip(VC.bf16_bounds(q, k, v, do, causal, kv, p_abs),
                    VC.bf16_bounds_torch(q, k, v, do, causal, kv, p_abs, "cpu")):
        np.testing.assert_allclose(y, x, rtol=1e-12, atol=0)
