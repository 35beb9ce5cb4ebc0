"""The fused skinny linear (mt_linear_rows through _hip.fused_linear) against a float64 NumPy
restatement of its contract, and its determinism / row independence bit for bit.

Bound per element: (K + 8) 2^-24 (|xh| @ |W| + |bias| + |residual|), an fp32 dot product in any
order plus the adds; with LayerNorm or GELU on, ATOL on top for the intrinsic error of the
statistics and of tanh. ATOL is 4 x the largest deviation from the same float64 reference that the
unfused path (Tensor.layernorm -> @ -> BiasGelu) shows on these same inputs, measured once on an
MI355X; the factor 4 rather than 2 allows for a different, equally valid summation order in both
the statistics and the product."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS = (1, 5, 16, 17, 64)  # below, at and past one row block, and the maximum
# smallest K; ragged N tiles; the model's shape; K % 16 != 0 (one wave owns K) with a partial last
# chunk; eight chunks per wave
KNS = ((4, 1), (64, 63), (256, 256), (260, 130), (1024, 200))
FUSIONS = ("plain", "bias", "ln+bias", "ln+bias+gelu", "bias+residual")
UNFUSED_DEV = 1.587e-06  # measured on an MI355X over CASES (worst: M = 64, (260, 130), ln+bias)
ATOL = 4 * UNFUSED_DEV
# every (M, (K, N)) pair with two of the five fusions, so that each fusion meets each M and each (K, N)
CASES = [(m, kn, FUSIONS[(i + j + o) % 5]) for i, m in enumerate(MS) for j, kn in enumerate(KNS) for o in (0, 2)]


def _inputs(M, K, Ns, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(x=f(rng.normal(0.5, 1.0, (M, K))), gamma=f(1 + 0.3 * rng.standard_normal(K)),
                beta=f(0.2 * rng.standard_normal(K)), W=[f(rng.uniform(-K ** -0.5, K ** -0.5, (K, n))) for n in Ns],
                bias=[f(rng.uniform(-K ** -0.5, K ** -0.5, n)) for n in Ns], res=[f(rng.standard_normal((M, n))) for n in Ns])


def ref64(x, W, bias=None, res=None, ln=None, gelu=False):
    """The contract in float64: (y, magnitude) with magnitude = |xh| @ |W| + |bias| + |residual|."""
    x, W = x.astype(np.float64), W.astype(np.float64)
    if ln is not None:
        mu = x.mean(1, keepdims=True)
        var = (x * x).mean(1, keepdims=True) - mu * mu + 1e-8
        x = ln[0].astype(np.float64) * (x - mu) / np.sqrt(var) + ln[1].astype(np.float64)
    y, mag = x @ W, np.abs(x) @ np.abs(W)
    if bias is not None:
        y, mag = y + bias, mag + np.abs(bias)
    if gelu:
        y = 0.5 * y * (1 + np.tanh(0.7978845608028654 * (y + 0.044715 * y ** 3)))
    if res is not None:
        y, mag = y + res, mag + np.abs(res)
    return y, mag


def _run(d, fusion, groups=None, rows=slice(None)):
    """One launch over the groups (default: all of d's) with the stages `fusion` names."""
    import torch
    from minitorch import _hip
    groups = range(len(d["W"])) if groups is None else groups
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ln = "ln" in fusion
    outs = _hip.fused_linear(dev(d["x"][rows]), [dev(d["W"][g]) for g in groups],
                             [dev(d["bias"][g]) for g in groups] if "bias" in fusion else None,
                             [dev(d["res"][g][rows]) for g in groups] if "residual" in fusion else None,
                             gamma=dev(d["gamma"]) if ln else None, beta=dev(d["beta"]) if ln else None,
                             gelu="gelu" in fusion)
    return [o.cpu().numpy() for o in outs]


def _check(d, fusion, got, g):
    K = d["x"].shape[1]
    want, mag = ref64(d["x"], d["W"][g], d["bias"][g] if "bias" in fusion else None,
                      d["res"][g] if "residual" in fusion else None,
                      (d["gamma"], d["beta"]) if "ln" in fusion else None, "gelu" in fusion)
    bound = (K + 8) * 2.0 ** -24 * mag + (ATOL if ("ln" in fusion or "gelu" in fusion) else 0.0)
    err = np.abs(got - want)
    print(f"{fusion} group {g}: max err {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert got.shape == want.shape and (err <= bound).all()


@pytest.mark.parametrize("M,kn,fusion", CASES)
def test_parity(M, kn, fusion):
    d = _inputs(M, kn[0], [kn[1]], seed=M * 4099 + kn[0] + kn[1])
    _check(d, fusion, _run(d, fusion)[0], 0)


def test_parity_grouped_gqa_projection():
    """G = 3 with N_g = (64, 16, 16): the Q / K / V launch of a width-64 model with 4 query heads and 1 kv head."""
    d = _inputs(5, 64, [64, 16, 16], seed=7)
    for g, got in enumerate(_run(d, "ln+bias")):
        _check(d, "ln+bias", got, g)


@pytest.mark.parametrize("K,N", [(256, 256), (1024, 200)])
def test_deterministic_and_row_independent_bitwise(K, N):
    fusion = "ln+bias+gelu+residual"
    bits = lambda a: a.view(np.uint32)  # noqa: E731
    d = _inputs(64, K, [N, 64, 16], seed=K + N)
    full = _run(d, fusion, groups=[0])[0]
    assert np.array_equal(bits(full), bits(_run(d, fusion, groups=[0])[0])), "two identical calls differ"
    for r in (0, 17, 63):  # a row of the 64-row call == the one-row call on that row
        one = _run(d, fusion, groups=[0], rows=slice(r, r + 1))[0]
        assert np.array_equal(bits(one[0]), bits(full[r])), f"row {r} depends on the rows beside it"
    # row 3 of the three-group call == each group's weights run alone
    grouped = _run(d, fusion, rows=slice(0, 5))
    for g in range(3):
        alone = _run(d, fusion, groups=[g], rows=slice(0, 5))[0]
        assert np.array_equal(bits(grouped[g][3]), bits(alone[3])), f"group {g} depends on the group count"
