"""mt_linear_rows_ex (through _hip.fused_linear): the RMSNorm prologue and the gated epilogue against
a float64 NumPy restatement, and their row / group independence bit for bit.

Bound: delta(v) = (K + 8) 2^-24 (|xh| @ |W_v| + |b_v|) for a pre-activation v, the rule of
tests/test_fused_linear_gpu.py. Ungated: delta + (K + 8) 2^-24 |residual| + ATOL. Gated, with a the
gate and b the up pre-activation: 1.1 delta(a) |b| + |silu(a)| delta(b) + (K + 8) 2^-24 |residual|
+ ATOL, since |silu'| <= 1.1. ATOL is 4 x the largest deviation from the same reference that the
unfused path (Tensor.rmsnorm -> @ -> + bias -> Tensor.swiglu, + residual) shows on these same
inputs, measured once on an MI355X; the factor 4 as in that file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS = (1, 17, 64)
KNS = ((4, 1), (64, 63), (256, 256), (260, 130), (1024, 200))
FUSIONS = ("rms", "rms+bias+glu", "glu+residual", "rms+glu")
EPS = 1e-5
UNFUSED_DEV = 1.666e-06  # measured on an MI355X over CASES (worst: M = 64, (1024, 200), glu+residual)
ATOL = 4 * UNFUSED_DEV
# every (M, (K, N)) pair with two of the four fusions, so that each fusion meets each M and each (K, N)
CASES = [(m, kn, FUSIONS[(i + j + o) % 4]) for i, m in enumerate(MS) for j, kn in enumerate(KNS) for o in (0, 2)]


def _inputs(M, K, Ns, seed):
    """x with a non-zero mean, gamma around 1; per group a gated weight [K, 2 n] (an ungated launch uses its first n columns)."""
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(x=f(rng.normal(0.5, 1.0, (M, K))), gamma=f(1 + 0.3 * rng.standard_normal(K)),
                beta=f(0.2 * rng.standard_normal(K)),
                W=[f(rng.uniform(-K ** -0.5, K ** -0.5, (K, 2 * n))) for n in Ns],
                bias=[f(rng.uniform(-K ** -0.5, K ** -0.5, 2 * n)) for n in Ns], res=[f(rng.standard_normal((M, n))) for n in Ns])


def ref64(d, g, fusion):
    """(y, bound without ATOL) of group g in float64."""
    x, W, bias = d["x"].astype(np.float64), d["W"][g].astype(np.float64), d["bias"][g].astype(np.float64)
    K, n = x.shape[1], W.shape[1] // 2
    c = (K + 8) * 2.0 ** -24
    if "rms" in fusion:
        x = d["gamma"].astype(np.float64) * x / np.sqrt((x * x).mean(1, keepdims=True) + EPS)
    if "bias" not in fusion:
        bias = np.zeros_like(bias)
    pre = lambda w, b: (x @ w + b, c * (np.abs(x) @ np.abs(w) + np.abs(b)))  # noqa: E731
    a, da = pre(W[:, :n], bias[:n])
    if "glu" in fusion:
        b, db = pre(W[:, n:], bias[n:])
        silu = a / (1 + np.exp(-a))
        y, bound = silu * b, 1.1 * da * np.abs(b) + np.abs(silu) * db
    else:
        y, bound = a, da
    if "residual" in fusion:
        y, bound = y + d["res"][g], bound + c * np.abs(d["res"][g])
    return y, bound


def _run(d, fusion, groups=(0,), rows=slice(None), glu=None):
    import torch
    from minitorch import _hip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    glu = ["glu" in fusion] * len(groups) if glu is None else glu
    half = lambda a, g, on: a[g] if on else a[g][..., :a[g].shape[-1] // 2]  # noqa: E731
    outs = _hip.fused_linear(dev(d["x"][rows]), [dev(half(d["W"], g, on)) for g, on in zip(groups, glu)],
                             [dev(half(d["bias"], g, on)) for g, on in zip(groups, glu)] if "bias" in fusion else None,
                             [dev(d["res"][g][rows]) for g in groups] if "residual" in fusion else None,
                             gamma=dev(d["gamma"]) if "rms" in fusion else None, norm="rms" if "rms" in fusion else None,
                             eps=EPS, glu=glu)
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("M,kn,fusion", CASES)
def test_parity(M, kn, fusion):
    d = _inputs(M, kn[0], [kn[1]], seed=M * 4099 + kn[0] + kn[1])
    got = _run(d, fusion)[0]
    want, bound = ref64(d, 0, fusion)
    err = np.abs(got - want)
    print(f"{fusion}: max err {err.max():.3e}, worst err / bound {float((err / (bound + ATOL)).max()):.3f}")
    assert got.shape == want.shape and (err <= bound + ATOL).all()


@pytest.mark.parametrize("K,N", [(256, 256), (260, 130)])
def test_row_and_group_independent_bitwise(K, N):
    fusion = "rms+bias+glu"
    bits = lambda a: a.view(np.uint32)  # noqa: E731
    d = _inputs(64, K, [N, 64, 16], seed=K + N)
    full = _run(d, fusion)[0]
    for r in (0, 17, 63):  # a row of the 64-row call == the one-row call on that row
        one = _run(d, fusion, rows=slice(r, r + 1))[0]
        assert np.array_equal(bits(one[0]), bits(full[r])), f"row {r} depends on the rows beside it"
    # the gated group between two ungated ones == the gated group alone
    grouped = _run(d, fusion, groups=(1, 0, 2), glu=[False, True, False])
    assert np.array_equal(bits(grouped[1]), bits(full)), "the gated group depends on the groups beside it"
    for i, g in ((0, 1), (2, 2)):
        alone = _run(d, fusion, groups=(g,), glu=[False])[0]
        assert np.array_equal(bits(grouped[i]), bits(alone)), f"ungated group {g} depends on the gated one beside it"


@pytest.mark.parametrize("M,K,N", [(5, 256, 256), (64, 260, 130)])
def test_ex_returns_mt_linear_rows_bits(M, K, N):
    """norm = 1, eps = 1e-8, glu_mask = 0 through the new entry == the old entry, ln + bias + gelu."""
    import torch
    from minitorch import _hip
    d = _inputs(M, K, [N], seed=3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    args = (dev(d["x"]), [dev(d["W"][0][:, :N])], [dev(d["bias"][0][:N])])
    kw = dict(gamma=dev(d["gamma"]), beta=dev(d["beta"]), gelu=True)
    old = _hip.fused_linear(*args, **kw)[0].cpu().numpy()
    new = _hip.fused_linear(*args, norm="layer", eps=1e-8, **kw)[0].cpu().numpy()  # an eps given: mt_linear_rows_ex
    assert np.array_equal(old.view(np.uint32), new.view(np.uint32))
