"""mt_rmsnorm_fw / bw and mt_swiglu_fw / bw (through the HIP backend's ops) against float64 NumPy.

Shapes: the issue's four, plus hidden = 1028 (a wave holds at most 1024 columns in one register
pass: the scalar kernels), rows = 2053 (the register-resident backward has at most 512 first-stage
workgroups of 4 rows at a time: they loop) and (261, 6) (the scalar gamma_grad reduction's
first-stage block is 256 rows).

Bounds, per element, from the arithmetic done (u = 2^-24):
  rmsnorm y   8 u |y|              the mean of squares, sqrt, divide and two products
  rmsnorm dx  8 u (|rstd g| + |x| rstd^3 (|g|.|x|) / H) + (H + 8) u |x| rstd^3 (|g|.|x|) / H
              (the two terms' own roundings, and the H-term dot product in any order)
  gamma_grad  (rows + 8) u sum_r |dy x rstd|
  swiglu      8 u |out| for the forward, 8 u (|da| terms) for the backward (exp, divide, products)
each plus ATOL = 4 x the largest deviation from the same reference that the tensor-op fallback
(Tensor.rmsnorm / Tensor.swiglu with the kernels hidden from the backend, running on the HIP
backend's generic ops) shows on these same inputs, measured once on an MI355X, taken apart for
the elementwise outputs and for gamma_grad, whose sums over rows deviate more (the factor 4 as in
tests/test_fused_linear_gpu.py: an equally valid order of the sums on either side)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (3, 63), (5, 256), (33, 260), (2, 1028), (2053, 8), (261, 6))
EPS = 1e-5
U = 2.0 ** -24
# measured on an MI355X over SHAPES: the elementwise outputs (worst: rmsnorm at (5, 256)) and gamma_grad
# (worst: (2053, 8), where the fallback adds 2053 terms per column)
FALLBACK_DEV, FALLBACK_DEV_DGAMMA = 1.035e-06, 1.017e-05
ATOL, ATOL_DGAMMA = 4 * FALLBACK_DEV, 4 * FALLBACK_DEV_DGAMMA


def _inputs(rows, n):
    rng = np.random.default_rng(rows * 4099 + n)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(x=f(rng.normal(0.5, 1.0, (rows, n))), gamma=f(1 + 0.3 * rng.standard_normal(n)),
                dy=f(rng.standard_normal((rows, n))), gu=f(rng.normal(0.5, 1.0, (rows, 2 * n))))


def rms64(x, gamma, dy):
    """(y, dx, dgamma) and their bounds' magnitudes in float64."""
    x, gamma, dy = (a.astype(np.float64) for a in (x, gamma, dy))
    H = x.shape[1]
    rstd = 1 / np.sqrt((x * x).mean(1, keepdims=True) + EPS)
    g = gamma * dy
    dot, adot = (g * x).sum(1, keepdims=True) / H, (np.abs(g) * np.abs(x)).sum(1, keepdims=True) / H
    y, dx, dgamma = gamma * x * rstd, rstd * g - x * rstd ** 3 * dot, (dy * x * rstd).sum(0)
    bounds = (8 * U * np.abs(y), 8 * U * (np.abs(rstd * g) + np.abs(x) * rstd ** 3 * adot) + (H + 8) * U * np.abs(x) * rstd ** 3 * adot,
              (x.shape[0] + 8) * U * np.abs(dy * x * rstd).sum(0))
    return (y, dx, dgamma), bounds


def swiglu64(gu, dy):
    gu, dy = gu.astype(np.float64), dy.astype(np.float64)
    F = gu.shape[1] // 2
    a, b = gu[:, :F], gu[:, F:]
    s = 1 / (1 + np.exp(-a))
    out, da, db = a * s * b, dy * b * s * (1 + a * (1 - s)), dy * a * s
    mag = np.abs(dy * b * s) * (1 + np.abs(a * (1 - s)))
    return (out, np.concatenate([da, db], 1)), (8 * U * np.abs(out), 8 * U * np.concatenate([mag, np.abs(db)], 1))


def _close(name, got, want, bound):
    bound = bound + (ATOL_DGAMMA if name == "dgamma" else ATOL)
    err = np.abs(got.astype(np.float64).reshape(want.shape) - want)
    print(f"{name}: max err {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), name


@pytest.fixture(scope="module")
def hip():
    import minitorch
    return minitorch, minitorch.TensorBackend(minitorch.HipKernelOps)


@pytest.mark.parametrize("rows,n", SHAPES)
def test_rmsnorm_and_swiglu(hip, rows, n):
    mt, be = hip
    d = _inputs(rows, n)
    x, gamma, dy = (mt.tensor_from_numpy(d[k], be) for k in ("x", "gamma", "dy"))
    y, rstd = be.rmsnorm_fw(x, gamma, EPS)
    dx, dgamma = be.rmsnorm_bw(dy, x, gamma, rstd)
    want, bounds = rms64(d["x"], d["gamma"], d["dy"])
    for name, got, w, b in zip(("y", "dx", "dgamma"), (y, dx, dgamma), want, bounds):
        _close(name, got.to_numpy(), w, b)
    again = be.rmsnorm_bw(dy, x, gamma, rstd)[1].to_numpy()
    assert np.array_equal(again.view(np.uint32), dgamma.to_numpy().view(np.uint32)), "gamma_grad is not deterministic"
    gu = mt.tensor_from_numpy(d["gu"], be)
    want, bounds = swiglu64(d["gu"], d["dy"])
    _close("out", be.swiglu_fw(gu).to_numpy(), want[0], bounds[0])
    _close("dgu", be.swiglu_bw(dy, gu).to_numpy(), want[1], bounds[1])


def test_autodiff_is_wired(hip):
    """Tensor.rmsnorm(...).swiglu() and backward() run the four kernels on the saved values: the
    same bits as the ops called by hand (whose values the tests above check)."""
    mt, be = hip
    d = _inputs(33, 260)
    x, gamma = (mt.tensor_from_numpy(d[k], be, requires_grad=True) for k in ("x", "gamma"))
    dy = mt.tensor_from_numpy(d["dy"][:, :130].copy(), be)
    out = x.rmsnorm(gamma, EPS).swiglu()
    out.backward(dy)
    y, rstd = be.rmsnorm_fw(x.detach(), gamma.detach(), EPS)
    dx, dgamma = be.rmsnorm_bw(be.swiglu_bw(dy, y), x.detach(), gamma.detach(), rstd)
    for name, got, want in (("out", out, be.swiglu_fw(y)), ("dx", x.grad, dx), ("dgamma", gamma.grad, dgamma)):
        assert np.array_equal(got.to_numpy().ravel().view(np.uint32), want.to_numpy().ravel().view(np.uint32)), name
