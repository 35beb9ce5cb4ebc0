"""mt_moe_rows (through _hip.moe_rows): the routed mixture-of-experts MLP against a float64 NumPy
restatement of its definition, the exact selection, and row independence bit for bit.

Selection: every case first asserts, on the reference alone, that each row's gap between its k-th
and (k+1)-th float64 logit exceeds 2 c_K max_e (|xh| @ |Wr|), c_K = (K + 8) 2^-24 (the project's
dot-product rule, twice: both logits may move); then topk_idx must equal the reference's.

Values: with delta(v) = c_K (|xh| @ |W_v| + |b_v|) for a pre-activation, h = silu(a) b carries
dh = 1.1 delta(a) |b| + |silu(a)| delta(b) (|silu'| <= 1.1), an expert's output
dy = dh @ |W_out| + c_F (|h| @ |W_out| + |b_out|), a gate (a ratio of exponentials of logits that
are each off by at most dr = c_K max_e |xh| @ |Wr|) a relative error of 2 dr + 8 2^-24 per
exponential, so 2 (2 dr + 8 2^-24) in all, and the sum
  bound = sum_j g_j dy_j + (4 dr + (k + 18) 2^-24) sum_j g_j |y_j| + c_K |residual|.
ATOL is 4 x the largest deviation from the same reference that the tensor-op path
(Tensor.rmsnorm / layernorm -> MoEFeedForward.forward on the HIP backend -> + residual) shows on
these same cases, measured once on an MI355X; the factor 4 is tests/test_fused_linear_gpu.py's.
topk_gate is held to the gate's share of that bound, g (4 dr + 16 2^-24); mt_moe_route must return
mt_moe_rows' idx and gate bits, the matching mask, and xh near the float64 normalised row: the fp32 sums
of a row round at most 14 times each (4 in the lane, 6 in the tree, the products, the division), so rstd
is off by at most 10 2^-24 relative for RMSNorm and 16 2^-24 |xh| covers it with the two products; for
LayerNorm the mean's error, 14 2^-24 mean|x|, enters x - mean absolutely and the variance's is amplified
by E[x^2] / var: 16 2^-24 (|gamma| rstd (|x| + mean|x| + |x - mean| E[x^2] / var) + |beta|)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 1e-5
SHAPES = ((64, 32, 64), (128, 40, 72), (260, 96, 130))  # a ragged gated tile, a ragged out tile, K % 16 != 0 (one wave)
# (M, (K, F, N), (E, k), norm, biases, residual); the last: F % 4 != 0, the element-wise loads of W_in and stores of h
CASES = [(1, SHAPES[0], (8, 2), 0, True, True), (3, SHAPES[1], (2, 1), 2, True, True),
         (17, SHAPES[2], (5, 5), 1, True, True), (64, SHAPES[0], (5, 5), 2, False, True),
         (64, SHAPES[1], (8, 2), 0, True, False), (64, SHAPES[2], (8, 2), 2, True, True),
         (17, SHAPES[1], (8, 2), 1, False, False), (3, SHAPES[2], (2, 1), 0, True, True),
         (1, SHAPES[2], (8, 2), 2, True, True), (17, SHAPES[0], (2, 1), 0, True, True),
         (1, SHAPES[1], (5, 5), 1, True, True), (3, SHAPES[0], (8, 2), 2, True, True),
         (17, (64, 30, 50), (8, 2), 2, True, True)]
# measured on an MI355X over CASES (worst: M = 64, (128, 40, 72), (8, 2), no norm, biases, no residual); the kernel's
# own worst error there was 2.988e-07 (M = 3, (260, 96, 130), (2, 1)) and every case also passed with ATOL = 0
UNFUSED_DEV = 3.396e-07
ATOL = 4 * UNFUSED_DEV


def _inputs(M, K, F, N, E, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    u = lambda n, *s: f(rng.uniform(-n ** -0.5, n ** -0.5, s))  # noqa: E731
    return dict(x=f(rng.normal(0.5, 1.0, (M, K))), gamma=f(1 + 0.3 * rng.standard_normal(K)),
                beta=f(0.2 * rng.standard_normal(K)), Wr=u(K, K, E), W_in=u(K, E, K, 2 * F), b_in=u(K, E, 2 * F),
                W_out=u(F, E, F, N), b_out=u(F, E, N), res=f(rng.standard_normal((M, N))))


def ref64(d, k, norm, bias=True, residual=True):
    """(out, bound without ATOL, idx, whether every row's selection gap is wide enough, gates, their bound, xh,
    its bound), float64."""
    g64 = lambda name: d[name].astype(np.float64)  # noqa: E731
    x, Wr, W_in, W_out = g64("x"), g64("Wr"), g64("W_in"), g64("W_out")
    (M, K), E, F = x.shape, Wr.shape[1], W_out.shape[1]
    b_in, b_out = (g64("b_in"), g64("b_out")) if bias else (np.zeros((E, 2 * F)), np.zeros((E, W_out.shape[2])))
    cK, cF, u = (K + 8) * 2.0 ** -24, (F + 8) * 2.0 ** -24, 2.0 ** -24
    dxh = np.zeros_like(x)  # no norm: xh is x
    if norm == 1:
        mean, var, ex2 = x.mean(1, keepdims=True), x.var(1, keepdims=True) + EPS, (x * x).mean(1, keepdims=True)
        amp = np.abs(x) + np.abs(x).mean(1, keepdims=True) + np.abs(x - mean) * ex2 / var
        dxh = 16 * u * (np.abs(g64("gamma")) * amp / np.sqrt(var) + np.abs(g64("beta")))
        x = g64("gamma") * (x - mean) / np.sqrt(var) + g64("beta")
    elif norm == 2:
        x = g64("gamma") * x / np.sqrt((x * x).mean(1, keepdims=True) + EPS)
        dxh = 16 * u * np.abs(x)
    r = np.stack([x @ Wr[:, e] for e in range(E)], 1)  # column by column: equal columns give equal logits
    dr = cK * (np.abs(x) @ np.abs(Wr)).max(1)
    order = np.argsort(-r, axis=1, kind="stable")  # descending logit, then index
    idx = order[:, :k]
    srt = np.take_along_axis(r, order, 1)
    wide = k == E or bool((srt[:, k - 1] - srt[:, k] > 2 * dr).all())
    out, bound = np.zeros((M, W_out.shape[2])), np.zeros((M, W_out.shape[2]))
    gates = np.exp(srt[:, :k] - srt[:, :1])
    gates /= gates.sum(1, keepdims=True)
    for m in range(M):
        for e, g in zip(idx[m], gates[m]):
            pre, dpre = x[m] @ W_in[e] + b_in[e], cK * (np.abs(x[m]) @ np.abs(W_in[e]) + np.abs(b_in[e]))
            a, b, silu = pre[:F], pre[F:], pre[:F] / (1 + np.exp(-pre[:F]))
            h, dh = silu * b, 1.1 * dpre[:F] * np.abs(b) + np.abs(silu) * dpre[F:]
            y = h @ W_out[e] + b_out[e]
            dy = dh @ np.abs(W_out[e]) + cF * (np.abs(h) @ np.abs(W_out[e]) + np.abs(b_out[e]))
            out[m] += g * y
            bound[m] += g * dy + (4 * dr[m] + (k + 18) * u) * g * np.abs(y)
    if residual:
        out, bound = out + d["res"], bound + cK * np.abs(d["res"])
    return out, bound, idx, wide, gates, gates * (4 * dr[:, None] + 16 * u), x, dxh


def _run(d, k, norm, bias=True, residual=True, rows=slice(None)):
    """(out, topk_idx, topk_gate, mt_moe_route's outputs on the same arguments) on the rows `rows` of the inputs."""
    import torch
    from minitorch import _hip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    M = d["x"][rows].shape[0]
    idx, gate = torch.empty((M, k), dtype=torch.int32, device="cuda"), torch.empty((M, k), device="cuda")
    nkw = dict(gamma=dev(d["gamma"]) if norm else None, beta=dev(d["beta"]) if norm == 1 else None,
               norm=(None, "layer", "rms")[norm], eps=EPS)
    out = _hip.moe_rows(dev(d["x"][rows]), dev(d["Wr"]), dev(d["W_in"]), dev(d["W_out"]),
                        dev(d["b_in"]) if bias else None, dev(d["b_out"]) if bias else None, k,
                        dev(d["res"][rows]) if residual else None, topk_idx=idx, topk_gate=gate, **nkw)
    route = _hip.moe_route(dev(d["x"][rows]), dev(d["Wr"]), k, want=("xh", "idx", "gate", "mask"), **nkw)
    return out.cpu().numpy(), idx.cpu().numpy(), gate.cpu().numpy(), {n: t.cpu().numpy() for n, t in route.items()}


def _seed(M, shape, ek):
    return M * 4099 + sum(shape) + 64 * ek[0] + ek[1]


@pytest.mark.parametrize("M,shape,ek,norm,bias,residual", CASES)
def test_parity(M, shape, ek, norm, bias, residual):
    d = _inputs(M, *shape, ek[0], seed=_seed(M, shape, ek))
    want, bound, idx, wide, gates, dgates, xh, dxh = ref64(d, ek[1], norm, bias, residual)
    assert wide, "a row's k-th and (k+1)-th logits are a near-tie: choose another seed"
    got, got_idx, got_gate, route = _run(d, ek[1], norm, bias, residual)
    assert np.array_equal(got_idx, idx) and (np.abs(got_gate - gates) <= dgates).all()
    assert np.array_equal(route["idx"], idx) and np.array_equal(route["gate"].view(np.uint32), got_gate.view(np.uint32))
    assert np.array_equal(np.argwhere(route["mask"] == 1)[:, 1].reshape(M, -1), np.sort(idx, 1)) and route["mask"].sum() == idx.size
    assert (np.abs(route["xh"] - xh) <= dxh).all()
    err = np.abs(got - want)
    print(f"max err {err.max():.3e}, worst err / bound {float((err / (bound + ATOL)).max()):.3f}, "
          f"passes with ATOL = 0: {bool((err <= bound).all())}")
    assert got.shape == want.shape and (err <= bound + ATOL).all()


def test_one_expert_takes_all_64_rows():
    d = _inputs(64, *SHAPES[0], 8, seed=11)
    d["Wr"][:, 3] += 1.0  # x has mean 0.5: logit 3 leads by about K / 2
    want, bound, idx, wide = ref64(d, 1, 0)[:4]
    assert wide and (idx == 3).all()
    got, got_idx = _run(d, 1, 0)[:2]
    assert np.array_equal(got_idx, idx) and (np.abs(got - want) <= bound + ATOL).all()


@pytest.mark.parametrize("k", [1, 2])
def test_exact_tie_goes_to_the_lower_index(k):
    d = _inputs(17, *SHAPES[1], 8, seed=12)
    d["Wr"][:, 2] += 1.0
    d["Wr"][:, 5] = d["Wr"][:, 2]  # equal columns: equal logits in the kernel and in the reference
    want, bound, idx = ref64(d, k, 2)[:3]
    assert (idx == [2, 5][:k]).all()
    got, got_idx = _run(d, k, 2)[:2]
    assert np.array_equal(got_idx, idx) and (np.abs(got - want) <= bound + ATOL).all()


def test_an_expert_nobody_chose_is_never_read():
    bits = lambda a: a.view(np.uint32)  # noqa: E731
    d = _inputs(64, *SHAPES[2], 8, seed=13)
    d["Wr"][:, 6] -= 1.0  # logit 6 trails by about K / 2
    assert not (ref64(d, 2, 0)[2] == 6).any()
    d["W_in"][6], d["W_out"][6] = 0.0, 0.0
    zeroed = _run(d, 2, 0)[0]
    d["W_in"][6], d["W_out"][6] = np.inf, np.inf
    got = _run(d, 2, 0)[0]
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(zeroed))
    d["x"][5, 7] = np.inf  # a non-finite logit: that row is NaN, the others are what they were
    bad = _run(d, 2, 0)[0]
    assert np.isnan(bad[5]).all() and np.array_equal(bits(np.delete(bad, 5, 0)), bits(np.delete(got, 5, 0)))


def test_row_independent_bitwise():
    d = _inputs(64, *SHAPES[2], 8, seed=14)  # 128 choices over 8 experts: every expert is shared
    full = _run(d, 2, 2)[0]
    for r in (0, 17, 63):  # a row of the 64-row call == the one-row call on that row
        one = _run(d, 2, 2, rows=slice(r, r + 1))[0]
        assert np.array_equal(one[0].view(np.uint32), full[r].view(np.uint32)), f"row {r} depends on the rows beside it"
