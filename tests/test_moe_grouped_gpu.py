"""The routed mixture-of-experts kernels (mt_moe_sort, mt_moe_grouped_gemm through _hip) against
float64 NumPy on handcrafted topk_idx: the sort exactly (a stable argsort), the three GEMM forms
under the project's dot-product rule of tests/test_moe_rows_gpu.py,
  |err| <= (L + 8 + scaled) 2^-24 |s| (|A| @ |B| + |bias|),
L the reduction length (the segment's row count for TN), one more rounding where a row scale is
applied; an empty expert's TN output exactly 0; an NN row bit for bit what the call on that entry
alone gives; and inf weights of an expert nobody chose changing no bit.
Shapes (Kd, N): a whole tile, ragged in both dimensions, a reduction that is no whole number of
16-wide chunks, and an output of at least 128 columns (the kernel's two-block column tile)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TM = 64  # _hip.MOE_GROUPED_TM, asserted below
U = 2.0 ** -24
SHAPES = ((64, 64), (36, 72), (260, 40), (40, 136))


def _routing(name):
    """(topk_idx [M, k] int32, E)."""
    rng = np.random.default_rng(5)
    if name == "edges":  # segment lengths 0, 1, TM, TM + 1, 2 TM + 2
        rows = [(1, 4)] + [(2, 4)] * TM + [(3, 4)] * (TM + 1)
        idx = np.array(rows)[rng.permutation(len(rows))]
        flip = rng.random(len(rows)) < 0.5
        idx[flip] = idx[flip][:, ::-1]
        assert np.bincount(idx.ravel(), minlength=5).tolist() == [0, 1, TM, TM + 1, 2 * TM + 2]
        return idx.astype(np.int32), 5
    if name == "one":  # every row on expert 1
        return np.ones((TM + 6, 1), np.int32), 2
    M = 200 if name == "random" else 50
    idx = np.argsort(rng.random((M, 8)), axis=1)[:, :2].astype(np.int32)
    if name == "dropped":
        idx[[3, 17]] = -1
    return idx, 8


def _sorted_ref(idx, E):
    flat = idx.ravel()
    valid = np.flatnonzero(flat >= 0)
    perm = valid[np.argsort(flat[valid], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat[valid], minlength=E))])
    pos = np.full(flat.size, -1)
    pos[perm] = np.arange(perm.size)
    return offsets, perm, pos.reshape(idx.shape)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sort(idx, E):
    from minitorch import _hip
    assert _hip.MOE_GROUPED_TM == TM
    return _hip.moe_sort(_dev(idx), E)


@pytest.mark.parametrize("name", ["edges", "one", "random", "dropped"])
def test_sort_is_a_stable_argsort(name):
    idx, E = _routing(name)
    offsets, perm, pos = _sorted_ref(idx, E)
    got = {n: t.cpu().numpy() for n, t in _sort(idx, E).items()}
    assert np.array_equal(got["offsets"], offsets) and np.array_equal(got["pos"], pos)
    assert np.array_equal(got["perm"][:perm.size], perm) and (got["perm"][perm.size:] == -1).all()
    assert np.array_equal(got["row"][:perm.size], perm // idx.shape[1])


def _operands(form, idx, E, Kd, N, full, seed):
    """NumPy operands of one call: A, B (stacked weights, or the TN form's rows), bias, src, srcb, s."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    (M, k), P = idx.shape, idx.size
    perm = _sorted_ref(idx, E)[1]
    row = np.zeros(P, np.int32)
    row[:perm.size] = perm // k
    d = dict(A=f(M if full else P, Kd), src=row if full else None, s=f(P) if full else None, bias=None, srcb=None)
    if form == "tn":
        d.update(B=f(M if full else P, N), srcb=row if full else None)
    else:
        d.update(B=f(E, Kd, N) if form == "nn" else f(E, N, Kd), bias=f(E, N) if full and form == "nn" else None)
    return d


def _call(form, d, offsets, want_db=False):
    from minitorch import _hip
    out = _hip.moe_grouped_gemm(form, _dev(d["A"]), _dev(d["B"]), offsets, src=_dev(d["src"]), s=_dev(d["s"]),
                                bias=_dev(d["bias"]), srcb=_dev(d["srcb"]), want_db=want_db)
    return tuple(t.cpu().numpy() for t in out) if form == "tn" else out.cpu().numpy()


def _check(name, got, want, mag, L, scaled):
    err, bound = np.abs(got - want), (L + 8 + scaled) * U * mag
    print(f"{name}: worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), name


@pytest.mark.parametrize("full", [False, True], ids=["plain", "src-s-bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", ["edges", "one", "random", "dropped"])
@pytest.mark.parametrize("form", ["nn", "nt", "tn"])
def test_parity(form, name, shape, full):
    idx, E = _routing(name)
    (Kd, N), P = shape, idx.size
    offsets = _sorted_ref(idx, E)[0]
    d = _operands(form, idx, E, Kd, N, full, seed=Kd + N)
    got = _call(form, d, _sort(idx, E)["offsets"], want_db=form == "tn")
    A, B = d["A"].astype(np.float64), d["B"].astype(np.float64)
    src = np.arange(P) if d["src"] is None else d["src"]
    s = np.ones(P) if d["s"] is None else d["s"].astype(np.float64)
    for e in range(E):
        seg = np.arange(offsets[e], offsets[e + 1])
        a = A[src[seg]]
        if form == "tn":
            b = s[seg, None] * B[seg if d["srcb"] is None else d["srcb"][seg]]
            if seg.size == 0:
                assert not got[0][e].any() and not got[1][e].any(), "an empty expert gets exact zeros"
                continue
            _check(f"dW[{e}]", got[0][e], a.T @ b, np.abs(a).T @ np.abs(b), seg.size, full)
            _check(f"db[{e}]", got[1][e], b.sum(0), np.abs(b).sum(0), seg.size, full)
        elif seg.size:
            w = B[e] if form == "nn" else B[e].T
            bias = np.zeros(N) if d["bias"] is None else d["bias"][e].astype(np.float64)
            _check(f"C[{e}]", got[seg], s[seg, None] * (a @ w + bias),
                   np.abs(s[seg, None]) * (np.abs(a) @ np.abs(w) + np.abs(bias)), Kd, full)


def test_row_independent_bitwise():
    idx, E = _routing("random")
    Kd, N = SHAPES[2]
    d = _operands("nn", idx, E, Kd, N, True, seed=3)
    full = _call("nn", d, _sort(idx, E)["offsets"])
    perm = _sorted_ref(idx, E)[1]
    for p in (0, 63, 64, 399):  # the entry at sorted position p alone: M = k = 1, its row of A, scale and expert
        entry = perm[p]
        one_idx = idx.ravel()[entry].reshape(1, 1)
        one = dict(d, A=d["A"][entry // 2][None], src=None, s=d["s"][p:p + 1])
        alone = _call("nn", one, _sort(one_idx, E)["offsets"])
        assert np.array_equal(alone[0].view(np.uint32), full[p].view(np.uint32)), f"position {p} depends on its neighbours"


@pytest.mark.parametrize("form", ["nn", "nt"])
def test_inf_weights_of_an_unchosen_expert_change_nothing(form):
    idx, E = _routing("edges")  # nobody chose expert 0
    d = _operands(form, idx, E, *SHAPES[1], True, seed=4)
    offsets = _sort(idx, E)["offsets"]
    d["B"][0] = 0.0
    zeroed = _call(form, d, offsets)
    d["B"][0] = np.inf
    got = _call(form, d, offsets)
    assert np.isfinite(got).all() and np.array_equal(got.view(np.uint32), zeroed.view(np.uint32))
