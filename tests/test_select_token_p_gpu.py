"""mt_select_token_p on the device against tests/nucleus_ref.py, the float64 restatement of its
contract: the sweep (every id inside the allowed prefix and the CDF bound), identity with
mt_select_token at the off values, the cases that hold exactly, the kept set of a hand-made row
by exhaustion over 4096 draws, the two larger LDS variants, and a captured launch.

Logits are rows of a larger NaN-filled buffer (row_stride = V + 5 > V, so the rows start at every
16-byte phase), as in test_select_token_gpu.py. The bounds are nucleus_ref's: eps = 1e-5 +
V 2^-24 on a cumulative probability and 1e-5 relative on an e_i against min_p; nothing here
widens them.
"""
import numpy as np
import pytest

import nucleus_ref as R

pytestmark = pytest.mark.gpu

GAP = 5


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
    return torch.from_numpy(buf).cuda()[:, :V]


def ids_of(torch, _hip, rows, **kw):
    view = rows if isinstance(rows, torch.Tensor) else in_buffer(torch, rows)
    out, out_i = _hip.select_token(view, **kw)
    a, b = out.cpu().numpy(), out_i.cpu().numpy()
    assert (a == b).all(), "the fp32 and int32 outputs differ"
    return b


def judge_rows(x, got, T, k, top_p, min_p, seed):
    """Failure tuples of one call's ids."""
    u = R.uniform24_ref(seed, np.arange(x.shape[0]))
    bad = []
    for b in range(x.shape[0]):
        j = R.Row(x[b], T, k).judge(int(got[b]), float(u[b]), top_p, min_p)
        if not (j["inside"] and j["ok"]):
            bad.append((b, int(got[b]), j))
    return bad


# ---- 1: the sweep ------------------------------------------------------------------------
def test_the_sweep_against_the_reference(hip):
    torch, _hip = hip
    n = amb = 0
    bad = []
    for V, B, T, k, quantised, rows, settings in R.sweep_cases():
        view = in_buffer(torch, rows)
        refs = [R.Row(rows[b], T, k) for b in range(B)]
        for top_p, min_p, seed in settings:
            got = ids_of(torch, _hip, view, temperature=T, top_k=k, top_p=top_p, min_p=min_p, seed=seed)
            u = R.uniform24_ref(seed, np.arange(B))
            for b in range(B):
                j = refs[b].judge(int(got[b]), float(u[b]), top_p, min_p)
                n += 1
                amb += j["ambiguous"]
                if not (j["inside"] and j["ok"]):
                    bad.append((V, B, T, k, quantised, top_p, min_p, b, int(got[b]), j))
    print(f"{n} row cases, {len(bad)} outside the bound, {amb} ambiguous")
    assert n == 2 * 13608
    assert not bad, bad[:10]


def test_the_uniform_is_rand_uniform(hip):
    """The host restatement of the uniform the sweep judges with is the device's."""
    torch, _hip = hip
    for seed in (0, 17, 2 ** 63 + 5):
        assert (_hip.rand_uniform(33, seed).cpu().numpy() == R.uniform24_ref(seed, np.arange(33))).all()


# ---- 2: identity at the off values ---------------------------------------------------------
def test_off_values_are_mt_select_token(hip):
    """mt_select_token_p(top_p = 1, min_p = 0) against mt_select_token itself (called through
    ctypes: the Python binding goes through the new entry), greedy and sampled."""
    torch, _hip = hip
    lib = _hip.lib()
    st = _hip.stream_ptr()
    n = 0
    for V, B, T, k, quantised, rows, settings in R.sweep_cases():
        if B == 1 and V not in (1, 4099):
            continue
        view = in_buffer(torch, rows)
        seed = settings[0][2]
        for temp in (0.0, T):
            old_f = torch.empty(B, dtype=torch.float32, device="cuda")
            old_i = torch.empty(B, dtype=torch.int32, device="cuda")
            _hip.check(lib.mt_select_token(view.data_ptr(), B, V, V + GAP, temp, k, seed, None, -1, old_f.data_ptr(),
                                           old_i.data_ptr(), None, None, 0, None, st), "mt_select_token")
            new_f, new_i = _hip.select_token(view, temperature=temp, top_k=k, seed=seed, top_p=1.0, min_p=0.0)
            dflt_f, dflt_i = _hip.select_token(view, temperature=temp, top_k=k, seed=seed)
            assert torch.equal(old_i, new_i) and torch.equal(old_f, new_f), (V, B, temp, k, quantised)
            assert torch.equal(old_i, dflt_i) and torch.equal(old_f, dflt_f), (V, B, temp, k, quantised)
            n += 1
    assert n > 100


# ---- 3: exact cases ------------------------------------------------------------------------
@pytest.mark.parametrize("V", R.VS + (10000,))
def test_tiny_top_p_and_full_min_p_are_argmax(hip, V):
    torch, _hip = hip
    rng = np.random.default_rng(300 + V)
    B = 17
    x = R.sampling_rows(rng, B, V, 1.0, False)
    q = R.sampling_rows(rng, B, V, 1.0, True)
    for seed in (1, 2):
        for k in (0, 5):
            # top_p = 1e-6 is below 1 / V: N is the first entry of K, ties by index: np.argmax
            for rows in (x, q):
                got = ids_of(torch, _hip, rows, temperature=1.0, top_k=k, top_p=1e-6, seed=seed)
                assert got.tolist() == np.argmax(rows, axis=-1).tolist(), (k, seed)
            # min_p = 1 keeps what equals the maximum: one entry on the continuous rows
            assert ((x == x.max(axis=-1, keepdims=True)).sum(axis=-1) == 1).all(), "a maximum is not unique"
            got = ids_of(torch, _hip, x, temperature=1.0, top_k=k, min_p=1.0, seed=seed)
            assert got.tolist() == np.argmax(x, axis=-1).tolist(), (k, seed)
            got = ids_of(torch, _hip, q, temperature=1.0, top_k=k, min_p=1.0, seed=seed)
            assert (q[np.arange(B), got] == q.max(axis=-1)).all(), (k, seed)
    if V >= 63:  # the ties at the maximum are drawn from, not only the first
        got = np.concatenate([ids_of(torch, _hip, q, temperature=1.0, min_p=1.0, seed=s) for s in range(8)])
        assert (got != np.tile(np.argmax(q, axis=-1), 8)).any()


def test_special_rows_behave_as_without_the_filters(hip):
    """-inf entries are never drawn; a row with a NaN, an infinite maximum or nothing finite
    takes the greedy id."""
    torch, _hip = hip
    rng = np.random.default_rng(9)
    V = 97
    x = rng.standard_normal((17, V)).astype(np.float32)
    x[rng.random((17, V)) < 0.4] = -np.inf
    x[:, 3] = 0.0  # something finite in every row
    for seed in range(5):
        got = ids_of(torch, _hip, x, temperature=1.0, top_p=0.9, min_p=0.01, seed=seed)
        assert np.isfinite(x[np.arange(17), got]).all()
        assert not judge_rows(x, got, 1.0, 0, 0.9, 0.01, seed)
    y = rng.standard_normal((4, V)).astype(np.float32)
    y[0, 40] = np.nan
    y[0, 70] = np.nan
    y[1, 11] = np.inf
    y[2, :] = -np.inf
    for kw in (dict(top_p=0.5), dict(min_p=0.2), dict(top_p=0.5, min_p=0.2, top_k=5)):
        got = ids_of(torch, _hip, y, temperature=0.7, seed=3, **kw)
        assert got[:3].tolist() == [40, 11, 0], kw
        assert 0 <= got[3] < V
    # everything but one entry underflows or is -inf: whatever u, the one entry of p > 0
    z = np.full((17, V), -np.inf, np.float32)
    z[:, ::2] = -200.0
    z[:, 31] = 0.0
    for kw in (dict(top_p=0.999), dict(min_p=1e-30), dict(top_p=0.5, min_p=0.5)):
        assert ids_of(torch, _hip, z, temperature=1.0, seed=1, **kw).tolist() == [31] * 17, kw
    # greedy ignores both filters
    g = rng.standard_normal((5, V)).astype(np.float32)
    assert ids_of(torch, _hip, g, top_p=0.3, min_p=0.9).tolist() == np.argmax(g, axis=-1).tolist()


# ---- 4: the kept set by exhaustion -----------------------------------------------------------
TOP = [5, 20, 41, 63]
TIES = [1, 7, 8, 15, 22, 30, 33, 40, 47, 52, 58, 61]


@pytest.mark.parametrize("top_k,n_ties", [(0, 7), (13, 2)])
def test_kept_set_by_exhaustion(hip, top_k, n_ties):
    """One row at V = 64, T = 1: 4 entries at 0, 12 at -1 on scattered indices, the rest at -3;
    top_p = 0.6. Over 4096 draws the ids returned are exactly the 4 maxima and the first n_ties
    ties by index, each within 5 sigma of its renormalised probability. top_k = 13 cuts inside
    the tie class first (K: the maxima and 9 ties). The boundary's float64 margins on both sides
    are asserted to exceed 100 eps, so no rounding of the kernel's can move it."""
    torch, _hip = hip
    V, B, top_p = 64, 4096, 0.6
    x = np.full(V, -3.0, np.float32)
    x[TOP] = 0.0
    x[TIES] = -1.0
    row = R.Row(x, 1.0, top_k)
    n = row.kept(top_p, 0.0)
    assert n == 4 + n_ties
    share = row.mass / row.mass[-1]
    margins = (share[n - 1] - top_p, top_p - share[n - 2])
    print("margins of the boundary", margins, "eps", row.eps)
    assert min(margins) > 100 * row.eps
    want = sorted(TOP + TIES[:n_ties])
    assert sorted(row.prefix(n).tolist()) == want
    got = ids_of(torch, _hip, np.tile(x, (B, 1)), temperature=1.0, top_k=top_k, top_p=top_p, seed=20250607)
    assert sorted(set(got.tolist())) == want
    p = np.where(np.isin(np.arange(V), TOP), 1.0, np.exp(-1.0))[want]
    p = p / p.sum()
    freq = np.bincount(got, minlength=V)[want] / B
    bound = 5 * np.sqrt(p * (1 - p) / B)
    print("frequencies", freq, "probabilities", p, "bounds", bound)
    assert (np.abs(freq - p) <= bound).all()


# ---- 5: the larger LDS variants --------------------------------------------------------------
@pytest.mark.parametrize("V", [10000, 20000])
def test_larger_variants(hip, V):
    torch, _hip = hip
    rng = np.random.default_rng(77 + V)
    for quantised in (False, True):
        x = R.sampling_rows(rng, 3, V, 1.0, quantised)
        for kw in (dict(top_k=0, top_p=0.5, min_p=0.0), dict(top_k=50, top_p=0.5, min_p=0.02)):
            got = ids_of(torch, _hip, x, temperature=1.0, seed=99, **kw)
            bad = judge_rows(x, got, 1.0, kw["top_k"], kw["top_p"], kw["min_p"], 99)
            assert not bad, (V, quantised, kw, bad)


# ---- 6: capture ------------------------------------------------------------------------------
def test_captured_launch_replays_with_device_seed_and_step(hip):
    torch, _hip = hip
    rng = np.random.default_rng(4)
    B, V, S = 5, 1025, 4
    x = R.sampling_rows(rng, B, V, 1.0, False) / 4
    view = in_buffer(torch, x)
    seed_dev = torch.tensor([11], dtype=torch.int64, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    hist = torch.full((B, S), -1, dtype=torch.int32, device="cuda")
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    out_i = torch.empty(B, dtype=torch.int32, device="cuda")
    kw = dict(temperature=0.9, top_k=40, top_p=0.8, min_p=0.05)

    def launch():
        _hip.select_token(view, seed_dev=seed_dev, out=out, out_i32=out_i, history=hist, step_dev=step, **kw)
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
        eager = ids_of(torch, _hip, view, seed=500 + s, **kw)
        assert out_i.cpu().numpy().tolist() == eager.tolist(), s
        assert not judge_rows(x, eager, 0.9, 40, 0.8, 0.05, 500 + s)
        want.append(eager)
    assert (hist.cpu().numpy() == np.stack(want, axis=1)).all()
    assert len({tuple(w.tolist()) for w in want}) > 1, "the seeds gave the same ids: nothing was shown"
