"""mt_select_token on the device against NumPy: greedy == np.argmax (ties, -inf, NaN), sampling
against a float64 CDF over the reference kept set with the uniform draw mt_rand_uniform gives,
the sampled distribution, and the device-resident seed / step / done / history plumbing,
eager and replayed from a captured graph.

Logits are rows of a larger NaN-filled buffer (row_stride = V + 5 > V, so the rows start at
every 16-byte phase): what lies between the rows must not matter.

The sampling bound: the returned id i must satisfy cdf[i-1] - eps <= u < cdf[i] + eps over the
kept set, eps = 1e-5 + V * 2^-24: 16 * 2^-23 * 2 for the rounded exponent argument (|logit / T|
<= 16) plus the worst case of an fp32 sum of V terms that total 1, with margin. Within eps of a
boundary either neighbour is accepted. The continuous sampling rows are 6 * N(0, 1) clipped to
+-16 (times T): peaked, so that the reference alone puts few draws inside an eps band (measured
on the CPU with the same generator and the same hash: 16 of the 2646 continuous row cases,
0.60 %, all of them full-vocabulary draws at V = 1025 and 4099; asserted < 1 %). The quantised
rows (8 levels) tie everywhere: they exercise the index-order rule of the kept set, are held to
the same bound, and are left out of that share: their equal neighbours put more draws in a band
(67 of 2646, 2.5 %; 66 of the 378 whole-vocabulary draws at V = 1025 and 4099), where the CDF
bound accepts either neighbour and only the kept-set check bites. That share is printed too.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VS = (1, 63, 64, 65, 97, 1025, 4099)
BS = (1, 3, 17)
GAP = 5
TEMPS = (0.5, 1.0, 2.0)


def top_ks(V):
    return (1, 2, 5, V - 1, V, V + 3)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def in_buffer(torch, rows):
    """rows [B, V] as a view of a NaN-filled [B, V + GAP] device buffer."""
    B, V = rows.shape
    buf = np.full((B, V + GAP), np.nan, np.float32)
    buf[:, :V] = rows
    t = torch.from_numpy(buf).cuda()
    return t[:, :V]


def ids_of(torch, _hip, rows, **kw):
    out, out_i = _hip.select_token(in_buffer(torch, rows), **kw)
    a, b = out.cpu().numpy(), out_i.cpu().numpy()
    assert a.dtype == np.float32 and b.dtype == np.int32
    assert (a == b).all(), "the fp32 and int32 outputs differ"
    return b


# ---- rows ------------------------------------------------------------------------------
def rows_normal(rng, B, V):
    return rng.standard_normal((B, V)).astype(np.float32)


def rows_quantised(rng, B, V):
    return (rng.integers(0, 8, (B, V)) * 0.5 - 1.75).astype(np.float32)


def rows_neg_inf(rng, B, V):
    x = rows_normal(rng, B, V)
    x[rng.random((B, V)) < 0.4] = -np.inf
    return x


def rows_two_nans(rng, B, V):
    x = rows_normal(rng, B, V)
    for b in range(B):
        for i in rng.choice(V, size=min(2, V), replace=False):
            x[b, i] = np.nan
    return x


def sampling_rows(rng, B, V, T, quantised):
    """|logit / T| <= 16: y in [-16, 16] times the fp32 T."""
    if quantised:
        y = rng.integers(0, 8, (B, V)) * 4.0 - 14.0
    else:
        y = np.clip(6.0 * rng.standard_normal((B, V)), -16.0, 16.0)
    return (y.astype(np.float32) * np.float32(T)).astype(np.float32)


def sampling_cases():
    """(V, B, T, top_k, quantised, seed, rows) of the sampling sweep, from one generator."""
    rng = np.random.default_rng(2024)
    n = 0
    for V in VS:
        for B in BS:
            for T in TEMPS:
                for k in top_ks(V):
                    for quantised in (False, True):
                        n += 1
                        yield V, B, T, k, quantised, 1000003 * n + 17, sampling_rows(rng, B, V, T, quantised)


def reference(x, T, top_k):
    """(kept indices ascending, float64 CDF over them) of one fp32 row."""
    V = x.size
    k = V if (top_k <= 0 or top_k >= V) else top_k
    order = np.lexsort((np.arange(V), -x.astype(np.float64)))  # value descending, index ascending
    kept = np.sort(order[:k])
    z = (x[kept].astype(np.float64) - float(x[kept].max())) / float(np.float32(T))
    p = np.exp(z)
    return kept, np.cumsum(p / p.sum())


def judge(i, kept, cdf, u, eps):
    """(in the kept set, inside the bound, u within eps of an inner boundary)."""
    j = int(np.searchsorted(kept, i))
    if j >= kept.size or kept[j] != i:
        return False, False, False
    lo = cdf[j - 1] if j else 0.0
    ok = lo - eps <= u < cdf[j] + eps
    band = bool(cdf.size > 1 and np.abs(cdf[:-1] - u).min() < eps)
    return True, bool(ok), band


# ---- greedy ----------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_greedy_is_np_argmax(hip, V, B):
    torch, _hip = hip
    rng = np.random.default_rng(100 * V + B)
    for make in (rows_normal, rows_quantised, rows_neg_inf, rows_two_nans):
        x = make(rng, B, V)
        got = ids_of(torch, _hip, x)
        assert got.tolist() == np.argmax(x, axis=-1).tolist(), make.__name__
    x = np.full((B, V), -np.inf, np.float32)  # nothing finite: index 0
    assert ids_of(torch, _hip, x).tolist() == [0] * B
    x = rows_normal(rng, B, V)
    x[:, V // 2] = np.inf
    assert ids_of(torch, _hip, x).tolist() == [V // 2] * B


def test_greedy_largest_rows(hip):
    """The two larger LDS variants of the kernel (V <= 16384, V <= 32768) and the size limit."""
    torch, _hip = hip
    rng = np.random.default_rng(5)
    for V in (4097, 16384, 16385, 32768):
        x = rows_quantised(rng, 2, V)
        assert ids_of(torch, _hip, x).tolist() == np.argmax(x, axis=-1).tolist(), V
    with pytest.raises(RuntimeError, match="limit"):
        _hip.select_token(torch.zeros((1, 32769), device="cuda"))


# ---- sampling --------------------------------------------------------------------------
def test_sampling_follows_the_reference_cdf(hip):
    torch, _hip = hip
    cases = bad = band_n = cont_n = qband_n = quant_n = qband_full = quant_full = 0
    worst = []
    for V, B, T, k, quantised, seed, x in sampling_cases():
        eps = 1e-5 + V * 2.0 ** -24
        u = _hip.rand_uniform(B, seed).cpu().numpy()
        got = ids_of(torch, _hip, x, temperature=T, top_k=k, seed=seed)
        if k == 1:
            assert got.tolist() == np.argmax(x, axis=-1).tolist(), "top_k = 1 is greedy"
        for b in range(B):
            kept, cdf = reference(x[b], T, k)
            kept_ok, ok, band = judge(int(got[b]), kept, cdf, float(u[b]), eps)
            cases += 1
            if not quantised:
                cont_n += 1
                band_n += band
            else:
                quant_n += 1
                qband_n += band
                if k >= V - 1 and V >= 1025:
                    quant_full += 1
                    qband_full += band
            if not (kept_ok and ok):
                bad += 1
                worst.append((V, B, T, k, quantised, b, int(got[b]), kept_ok))
    share = band_n / cont_n
    print(f"{cases} row cases, {bad} outside the bound; {band_n} of the {cont_n} continuous ones "
          f"({100 * share:.2f} %) had u within eps of a boundary")
    # what the CDF bound can still tell on the quantised rows (the kept-set check is unaffected)
    print(f"quantised rows: {qband_n} of {quant_n} ({100 * qband_n / quant_n:.1f} %) inside a band; at "
          f"V >= 1025 with the whole vocabulary kept {qband_full} of {quant_full}")
    assert bad == 0, worst[:10]
    assert share < 0.01


def test_sampling_larger_rows_and_every_kernel_variant(hip):
    """V = 10000 (the config-5 vocabulary, the 64 KiB variant) and 20000 (the 128 KiB one),
    top_k 50 and all, against the same bound."""
    torch, _hip = hip
    rng = np.random.default_rng(77)
    for V in (10000, 20000):
        eps = 1e-5 + V * 2.0 ** -24
        for k in (50, 0):
            for quantised in (False, True):
                x = sampling_rows(rng, 3, V, 1.0, quantised)
                u = _hip.rand_uniform(3, 99 + k).cpu().numpy()
                got = ids_of(torch, _hip, x, temperature=1.0, top_k=k, seed=99 + k)
                for b in range(3):
                    kept, cdf = reference(x[b], 1.0, k)
                    kept_ok, ok, _ = judge(int(got[b]), kept, cdf, float(u[b]), eps)
                    assert kept_ok and ok, (V, k, quantised, b, int(got[b]))


def test_sampling_negative_and_zero_maxima(hip):
    """The kernel rebuilds the row maximum from its order key: all-negative rows, and rows whose
    maximum is +0 or -0, against the same bound (whole vocabulary and top_k 5)."""
    torch, _hip = hip
    rng = np.random.default_rng(21)
    V, B = 1025, 6
    eps = 1e-5 + V * 2.0 ** -24
    x = sampling_rows(rng, B, V, 1.0, False)
    x -= x.max(axis=-1, keepdims=True)          # maximum 0
    x[1] -= 3.25                                # all negative
    x[2] -= 1e-3
    x[3, int(np.argmax(x[3]))] = -0.0           # the maximum is -0
    x[4] *= 0.25
    x[5] = np.minimum(x[5] - 20.0, -24.5)       # far below zero, many ties at the top
    for k in (0, 5):
        u = _hip.rand_uniform(B, 314 + k).cpu().numpy()
        got = ids_of(torch, _hip, x, temperature=1.0, top_k=k, seed=314 + k)
        for b in range(B):
            kept, cdf = reference(x[b], 1.0, k)
            kept_ok, ok, _ = judge(int(got[b]), kept, cdf, float(u[b]), eps)
            assert kept_ok and ok, (k, b, int(got[b]))


def test_sampling_special_rows(hip):
    """-inf entries have p = 0 and are never drawn; a row with a NaN, an infinite maximum or
    nothing finite takes the greedy id."""
    torch, _hip = hip
    rng = np.random.default_rng(9)
    V = 97
    x = rows_neg_inf(rng, 17, V)
    x[:, 3] = 0.0  # something finite in every row
    for seed in range(5):
        got = ids_of(torch, _hip, x, temperature=1.0, top_k=0, seed=seed)
        assert np.isfinite(x[np.arange(17), got]).all()
    y = rows_normal(rng, 4, V)
    y[0, 40] = np.nan
    y[0, 70] = np.nan
    y[1, 11] = np.inf
    y[2, :] = -np.inf
    got = ids_of(torch, _hip, y, temperature=0.7, top_k=5, seed=3)
    assert got[:3].tolist() == [40, 11, 0]
    assert 0 <= got[3] < V
    # everything but one entry underflows or is -inf: whatever u, the one entry of p > 0
    z = np.full((17, V), -np.inf, np.float32)
    z[:, ::2] = -200.0
    z[:, 31] = 0.0
    for seed in range(3):
        assert ids_of(torch, _hip, z, temperature=1.0, top_k=0, seed=seed).tolist() == [31] * 17


def test_distribution(hip):
    torch, _hip = hip
    p = np.array([0.30, 0.20, 0.15, 0.12, 0.10, 0.07, 0.04, 0.02])
    B = 4096
    x = np.tile(np.log(p).astype(np.float32), (B, 1))
    got = ids_of(torch, _hip, x, temperature=1.0, seed=20240607)
    freq = np.bincount(got, minlength=8) / B
    bound = 5 * np.sqrt(p * (1 - p) / B)
    print("frequencies", freq, "bounds", bound)
    assert (np.abs(freq - p) <= bound).all()


# ---- device-resident seed, step, done, history --------------------------------------------
def test_seed_dev_done_history_and_repeat(hip):
    torch, _hip = hip
    rng = np.random.default_rng(3)
    B, V, S = 17, 97, 6
    x = sampling_rows(rng, B, V, 1.0, False) / 4  # flat enough that the ids vary
    view = in_buffer(torch, x)
    seed = 2 ** 63 + 12345  # the high bit too
    want = ids_of(torch, _hip, x, temperature=1.0, top_k=7, seed=seed)
    assert len(set(want.tolist())) > 1
    seed_dev = torch.tensor([seed - 2 ** 64], dtype=torch.int64, device="cuda")
    eos = int(want[0])
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    done[1] = 1  # never cleared
    hist = torch.full((B, S), -7, dtype=torch.int32, device="cuda")
    step = torch.tensor([2], dtype=torch.int32, device="cuda")
    out, out_i = _hip.select_token(view, temperature=1.0, top_k=7, seed_dev=seed_dev, eos_id=eos, done=done,
                                   history=hist, step_dev=step)
    assert out_i.cpu().numpy().tolist() == want.tolist()
    d = (want == eos)
    d[1] = True
    assert done.cpu().numpy().astype(bool).tolist() == d.tolist()
    h = hist.cpu().numpy()
    assert h[:, 2].tolist() == want.tolist()
    assert (np.delete(h, 2, axis=1) == -7).all(), "history neighbours were written"
    # a repeated call is bit-equal; a step past the row writes nothing
    again, _ = _hip.select_token(view, temperature=1.0, top_k=7, seed_dev=seed_dev)
    assert torch.equal(again, out)
    step.fill_(S)
    _hip.select_token(view, temperature=1.0, top_k=7, seed_dev=seed_dev, history=hist, step_dev=step)
    step.fill_(-1)
    _hip.select_token(view, temperature=1.0, top_k=7, seed_dev=seed_dev, history=hist, step_dev=step)
    assert (hist.cpu().numpy() == h).all()
    # the id does not depend on what else is in the batch
    solo = ids_of(torch, _hip, x[:1], temperature=1.0, top_k=7, seed=seed)
    assert solo[0] == want[0]
    with pytest.raises(ValueError, match="step_dev"):
        _hip.select_token(view, history=hist)


def test_captured_launch_replays_with_device_seed_and_step(hip):
    """One launch captured on one stream; replayed after seed_dev and step_dev change on the
    device, it equals the eager call with those values."""
    torch, _hip = hip
    rng = np.random.default_rng(4)
    B, V, S = 5, 1025, 4
    x = sampling_rows(rng, B, V, 1.0, False) / 4
    view = in_buffer(torch, x)
    seed_dev = torch.tensor([11], dtype=torch.int64, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    hist = torch.full((B, S), -1, dtype=torch.int32, device="cuda")
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    out_i = torch.empty(B, dtype=torch.int32, device="cuda")

    def launch():
        _hip.select_token(view, temperature=0.9, top_k=40, seed_dev=seed_dev, out=out, out_i32=out_i,
                          history=hist, step_dev=step)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    hist.fill_(-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    want = []
    for s in range(S):
        seed_dev.fill_(500 + s)
        step.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        eager = ids_of(torch, _hip, x, temperature=0.9, top_k=40, seed=500 + s)
        assert out_i.cpu().numpy().tolist() == eager.tolist(), s
        want.append(eager)
    assert (hist.cpu().numpy() == np.stack(want, axis=1)).all()
    assert len({tuple(w.tolist()) for w in want}) > 1, "the seeds gave the same ids: nothing was shown"
