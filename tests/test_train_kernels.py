"""The references, case tables and guard-band helpers of tests/train_kernels_ref.py, on the CPU:

    splitmix64_ref / uniform24_ref   the published splitmix64 vectors and a big-int restatement
    bias_gelu_ref / _bw_ref          torch's tanh GELU in float64 and its autograd
    xent_ref                         torch's cross_entropy in float64, -inf entries included
    embed_*_ref, the case tables     what the tables promise
    place_flat / footprint           a NumPy stand-in of every kernel passes; one that writes an
                                     element past its output, skips the last element or modifies
                                     an input is reported (as tests/test_flash_layouts.py does for
                                     the attention entry points)
"""
import numpy as np
import pytest
import torch

import train_kernels_ref as R

M64 = (1 << 64) - 1


def _mix_py(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _hash_py(seed, i):
    """csrc/rng.h in Python's unbounded integers, reduced mod 2^64 where uint64_t wraps."""
    return _mix_py((seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64)


def test_published_splitmix64_vectors():
    assert [int(h) for h in R.splitmix64_ref(0, [0, 1, 2])] == [
        0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert int(R.splitmix64_ref(1234567, 0)[0]) == 6457827717110365317
    assert _hash_py(0, 0) == 0xE220A8397B1DCDAF and _hash_py(1234567, 0) == 6457827717110365317


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63, 2 ** 64 - 1])
def test_uniform24_ref_vs_bigint(seed):
    idx = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5]
    got = R.uniform24_ref(seed, np.array(idx, dtype=np.int64))
    assert got.dtype == np.float32
    for i, u in zip(idx, got):
        h = _hash_py(seed, i)
        assert int(R.splitmix64_ref(seed, i)[0]) == h
        assert float(u) == (h >> 40) / 2.0 ** 24 and 0.0 <= u < 1.0
    # an index truncated to 32 bits would give index 5's draw at 2^32 + 5
    assert _hash_py(seed, 2 ** 32 + 5) != _hash_py(seed, 5)


def test_dropout_ref_and_zero_draw_seeds():
    x = np.arange(1, 1024, dtype=np.float32)
    for n, (seed, where) in R.DROPOUT_ZERO.items():
        u = R.uniform24_ref(seed, np.arange(n))
        assert u[where] == 0.0 and where < n
    seed, where = R.DROPOUT_ZERO[1023]
    u = R.uniform24_ref(seed, np.arange(1023))
    y = R.dropout_ref(x, 0.0, 1.0, seed)
    assert np.array_equal(np.flatnonzero(y == 0), np.flatnonzero(u == 0)) and y[where] == 0
    assert not R.dropout_ref(x, 1.0 - 2.0 ** -24, 2.0 ** 24, seed).any()  # the largest draw is 1 - 2^-24
    y = R.dropout_ref(x, 0.5, 2.0, seed)
    assert y.dtype == np.float32 and np.array_equal(y, np.where(u > 0.5, x * 2, 0))
    assert 0.4 < (y != 0).mean() < 0.6


@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 8), (33, 7), (64, 256)])
def test_gelu_refs_vs_torch(rows, cols):
    x, b, dy = R.gelu_inputs(rows, cols, np.random.default_rng(rows * 1000 + cols))
    u = (x.astype(np.float64) + b)
    if rows * ((cols + 2) // 3) >= len(R.GELU_PLANTED):
        for p in R.GELU_PLANTED:  # the planted values are the pre-activation itself
            assert (u == np.float64(np.float32(p))).any(), p
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.gelu(tx + torch.tensor(b, dtype=torch.float64), approximate="tanh")
    (y * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    # two float64 evaluations of the same formula: they differ by the roundings of 1 + t and
    # 1 - t^2 (2^-53 each) times their factors, at most 0.5 |u| = 15 forward and 0.5 |u| dt ~ 1500
    # backward at the largest planted u that does not saturate tanh to exactly +-1 (30), times |dy| < 5
    np.testing.assert_allclose(R.bias_gelu_ref(x, b), y.detach().numpy(), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(R.bias_gelu_bw_ref(dy, x, b), tx.grad.numpy(), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("C", [1, 3, 4, 1023])
def test_xent_ref_vs_torch(C):
    rng = np.random.default_rng(C)
    rows = 6
    x = (rng.standard_normal((rows, C)) * 3).astype(np.float32)
    t = rng.integers(0, C, rows)
    if C >= 4:  # rows with -inf entries, never on the target
        for r in (1, 4):
            cols = np.setdiff1d(rng.choice(C, C // 3, replace=False), [t[r]])
            x[r, cols] = -np.inf
    g = rng.standard_normal(rows)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    loss = torch.nn.functional.cross_entropy(tx, torch.tensor(t), reduction="none")
    (loss * torch.tensor(g)).sum().backward()
    lse, got, dx = R.xent_ref(x, t.astype(np.float32), g)
    np.testing.assert_allclose(got, loss.detach().numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dx, tx.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(lse, torch.logsumexp(tx, 1).detach().numpy(), rtol=1e-14)
    assert np.isfinite(lse).all() and (dx[~np.isfinite(x)] == 0).all()
    # a target outside [0, C) picks nothing
    lse2, loss2, dx2 = R.xent_ref(x, np.array([-1, C, -1, C, -1, C], dtype=np.float32), g)
    sm = torch.softmax(tx, 1).detach().numpy()
    np.testing.assert_array_equal(loss2, lse2)
    np.testing.assert_allclose(dx2, sm * g[:, None], rtol=1e-12, atol=1e-15)


def test_xent_case_helpers():
    for rows, C in R.XENT_SHAPES + (R.XENT_MISALIGNED,):
        ts = R.xent_targets(rows, C, np.random.default_rng(0))
        allt = np.concatenate(ts)
        assert all(len(t) == rows and t.dtype == np.float32 for t in ts)
        for want in (0, C - 1, -1, C, max(C - 2, 0)):
            assert (allt == want).any()
        assert allt.min() >= -1 and allt.max() <= C
    for C, _ in R.XENT_NEGINF:
        x, t = R.xent_neginf_rows(C, np.random.default_rng(C))
        assert np.isneginf(x[0, 0]) and np.isneginf(x[0]).sum() == 1
        assert np.isneginf(x[1, :256]).all() and np.isneginf(x[1, 0:1024:4]).all()
        assert 0.25 < np.isneginf(x[2]).mean() < 0.42 and np.isfinite(x[3]).all()
        assert np.isfinite(x[np.arange(4), t.astype(int)]).all()
        lse, loss, dx = R.xent_ref(x, t, np.ones(4))
        assert np.isfinite(lse).all() and np.isfinite(loss).all() and (dx[np.isneginf(x)] == 0).all()


def test_embed_refs_and_tables():
    W = np.arange(1, 9 * 3 + 1, dtype=np.float32).reshape(9, 3)
    ids = np.array([0, 8, 9, 12, -1, -0.0, 2.7, 4294967298.0, 1e30, np.inf, -np.inf, np.nan, 8.999], dtype=np.float32)
    want = [0, 8, None, None, None, 0, 2, None, None, None, None, None, 8]
    out = R.embed_fw_ref(ids, W)
    for o, w in zip(out, want):
        np.testing.assert_array_equal(o, W[w] if w is not None else np.zeros(3, np.float32))
    assert not np.signbit(out).any()
    dy = np.random.default_rng(0).standard_normal((len(ids), 3)).astype(np.float32)
    dW, cnt, sabs = R.embed_bw_ref(dy, ids, 9)
    assert cnt.tolist() == [2, 0, 1, 0, 0, 0, 0, 0, 2] and cnt.sum() == sum(w is not None for w in want)
    np.testing.assert_array_equal(dW[2], dy[6].astype(np.float64))
    np.testing.assert_allclose(dW[8], dy[1].astype(np.float64) + dy[12], rtol=1e-15)
    np.testing.assert_allclose(sabs[0], np.abs(dy[0]).astype(np.float64) + np.abs(dy[5]), rtol=1e-15)
    assert not dW[1].any()
    # the table: every value of every axis, every (V, E) pair, the two named cases, at most 30
    assert len(R.EMBED_CASES) <= 30 and len(set(R.EMBED_CASES)) == len(R.EMBED_CASES)
    assert {(V, E) for V, E, _ in R.EMBED_CASES} == {(V, E) for V in R.EMBED_V for E in R.EMBED_E}
    for n in R.EMBED_NTOK:
        assert sum(c[2] == n for c in R.EMBED_CASES) >= 2, n
    assert (9, 257, 2049) in R.EMBED_CASES and (17, 513, 4097) in R.EMBED_CASES
    for V, _, ntok in R.EMBED_CASES:
        ids, planted = R.embed_ids(V, ntok, np.random.default_rng(V * ntok))
        valid, row = R.embed_rows(ids, V)
        assert len(ids) == ntok and (ntok < 12 or len(planted) == len(R.embed_special_ids(V)))
        for pos, r in planted.items():
            assert (valid[pos], row[pos]) == ((True, r) if r is not None else (False, 0)), (V, ids[pos])


def test_adam_tables():
    for count in R.ADAM_COUNTS:
        s = R.adam_sizes(count, 12 if count == 25 else None)
        assert len(s) == count and set(s) - {0} == set(R.ADAM_SIZES)
        assert (s[12] == 0) == (count == 25)
    p, m, v = R.adam_ref(np.float32([1.0]), np.float32([0.5]), np.float32([0.0]), np.float32([0.0]), 1, 0.1, 0.9, 0.999, 1e-8)
    assert m.dtype == v.dtype == np.float32 and abs(float(p[0]) - 0.9) < 1e-6  # the first step moves by lr


# ---- the guard-band machinery on stand-in kernels ----------------------------------------------
def _standin_case(kernel, rng):
    """(inputs, outputs) of a NumPy stand-in of `kernel`: lists of flat float32 arrays; `inplace`
    outputs start from their own values."""
    f = np.float32
    if kernel == "rand_uniform":
        return [], [R.uniform24_ref(7, np.arange(257))]
    if kernel == "dropout":
        x = rng.standard_normal(1023).astype(f)
        return [x], [R.dropout_ref(x, 0.1, 1 / 0.9, 5)]
    if kernel in ("bias_gelu_fw", "bias_gelu_bw"):
        x, b, dy = R.gelu_inputs(33, 7, rng)
        if kernel == "bias_gelu_fw":
            return [x, b], [R.bias_gelu_ref(x, b).astype(f)]
        return [dy, x, b], [R.bias_gelu_bw_ref(dy, x, b).astype(f)]
    if kernel in ("embedding_fw", "embedding_bw"):
        ids, _ = R.embed_ids(9, 129, rng)
        W = rng.standard_normal((9, 5)).astype(f)
        dy = rng.standard_normal((129, 5)).astype(f)
        if kernel == "embedding_fw":
            return [ids, W], [R.embed_fw_ref(ids, W)]
        return [dy, ids], [R.embed_bw_ref(dy, ids, 9)[0].astype(f)]
    if kernel == "adam":
        sizes = (5, 1025, 3)
        p, g = ([rng.standard_normal(n).astype(f) for n in sizes] for _ in range(2))
        z = [np.zeros(n, f) for n in sizes]
        res = [R.adam_ref(a, b, c, d, 1, 1e-3, 0.9, 0.999, 1e-8) for a, b, c, d in zip(p, g, z, z)]
        return g, [r[k] for k in range(3) for r in res]
    x = (rng.standard_normal((5, 7)) * 3).astype(f)
    t = rng.integers(0, 7, 5).astype(f)
    g = rng.standard_normal(5).astype(f)
    lse, loss, dx = R.xent_ref(x, t, g)
    if kernel == "xent_fw":
        return [x, t], [loss.astype(f), lse.astype(f)]
    assert kernel == "xent_bw"
    return [g, x, t, lse.astype(f)], [dx.astype(f)]


KERNELS = ("rand_uniform", "dropout", "bias_gelu_fw", "bias_gelu_bw", "embedding_fw", "embedding_bw", "adam",
           "xent_fw", "xent_bw")


def _run_standin(kernel, mis, mut=None):
    """Place the tensors of `kernel`, let the stand-in write its outputs through the views with
    the mistake `mut`, and return footprint()'s failures."""
    ins, outs = _standin_case(kernel, np.random.default_rng(len(kernel)))
    pin, vin = R.place_flat([x.size for x in ins], "cpu", False, ins, mis)
    before = pin.bits()
    pout, vout = R.place_flat([y.size for y in outs], "cpu", True, None, mis)
    for v, x in zip(vin, ins):  # the views hand back what was placed
        np.testing.assert_array_equal(v.numpy().view(np.uint32), x.reshape(-1).view(np.uint32))
    for k, (v, y) in enumerate(zip(vout, outs)):
        y = torch.from_numpy(np.ascontiguousarray(y).reshape(-1))
        last = k == len(outs) - 1
        n = y.numel() - 1 if (mut == "skip_last" and last) else y.numel()
        v[:n].copy_(y[:n])
        if mut == "one_past" and last:
            pout.flat[v.storage_offset() + y.numel()] = 0.0
        if mut == "one_before" and k == 0:
            pout.flat[v.storage_offset() - 1] = 0.0
    if mut == "touch_input" and ins:
        vin[-1][-1] += 1.0
    return R.footprint([("out", pout, vout)], [("in", pin, before)])


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_standin_passes(kernel, mis):
    assert _run_standin(kernel, mis) == []


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_standin_faults_are_reported(kernel, mis):
    for mut, word in (("one_past", "outside the view were written"), ("one_before", "outside the view were written"),
                      ("skip_last", "are NaN"), ("touch_input", "elements changed")):
        if mut == "touch_input" and kernel == "rand_uniform":
            continue  # no input
        fails = _run_standin(kernel, mis, mut)
        assert len(fails) == 1 and word in fails[0], (mut, fails)


def test_place_flat_layout():
    """Bands of at least GUARD floats around every view, 16-byte starts (or one float past), and a
    zero-length view in the middle takes no element."""
    for mis in (False, True):
        p, views = R.place_flat([5, 0, 1024, 3], "cpu", True, None, mis)
        offs = [v.storage_offset() for v in views]
        assert all(o % 4 == int(mis) for o in offs) and offs[0] >= R.GUARD
        ends = [o + v.numel() for o, v in zip(offs, views)]
        assert all(b - a >= R.GUARD for a, b in zip(ends, offs[1:])) and p.flat.numel() - ends[-1] >= R.GUARD
        assert int(p.mask.sum()) == 5 + 1024 + 3 and views[1].numel() == 0
        assert R.footprint([("out", p, views)]) != []  # NaN inside: nothing written yet
        for v in views:
            v.fill_(1.0)
        assert R.footprint([("out", p, views)]) == []
