"""mt_matmul_f32 on every kernel variant, layout and edge of tests/gemm_cases.py, on an MI355X.

Exact input kinds (ints, wide_a, wide_b: every partial sum an integer below 2^24) must give the
float64 product bit for bit on every backend, so an indexing, tail, slice or bf16-plane mistake
is a wrong integer and no tolerance hides it. Every case first asserts that the library's plan
for its real pointers and strides is the one the table states, then checks the write footprint
(sentinels around and between C's rows untouched, operands unchanged, no NaN padding in a
product) and that a second call is bitwise equal. The gauss kind holds each backend to the
project's accuracy figures and to bitwise invariance under power-of-two row / column scaling.
The last tests run `Tensor @ Tensor` through each branch of HipKernelOps.matrix_multiply.

Zeros are compared by value (a sum of products that are all -0 is -0 in float64 and +0 in a
kernel that starts its accumulator at +0); every other element by bit pattern.
"""
import ctypes

import numpy as np
import pytest

import gemm_cases as G

pytestmark = pytest.mark.gpu

BACKENDS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    return torch, _hip, _hip.lib()


@pytest.fixture
def backend(request, dev):
    _, _, lib = dev
    lib.mt_set_gemm_backend(request.param)
    try:
        yield request.param
    finally:
        lib.mt_set_gemm_backend(0)


def _s3(v):
    return (ctypes.c_int64 * 3)(*[int(x) for x in v])


def _bits(x):
    """fp32 bit patterns with -0 folded onto +0."""
    x = np.ascontiguousarray(x, np.float32)
    return np.where(x == 0, np.float32(0), x).view(np.uint32)


def run_case(dev, case, backend, a_vals, b_vals):
    """Place the operands, assert the plan, run mt_matmul_f32 twice into sentinel-filled C
    buffers, check footprint and repeatability; returns (C [batch, M, N], plan)."""
    torch, _hip, lib = dev
    g = G.geometry(case)
    shape_c = (case.batch, case.M, case.N)
    abuf = G.place(a_vals, g["a_off"], g["sa"], g["a_size"], np.nan)
    bbuf = G.place(b_vals, g["b_off"], g["sb"], g["b_size"], np.nan)
    cbuf = G.place(None, g["c_off"], g["sc"], g["c_size"], G.SENTINEL)
    ta, tb = torch.from_numpy(abuf).cuda(), torch.from_numpy(bbuf).cuda()
    tc = [torch.from_numpy(cbuf).cuda(), torch.from_numpy(cbuf).cuda()]
    assert all(t.data_ptr() % 16 == 0 for t in (ta, tb, *tc))
    pa, pb = ta.data_ptr() + 4 * g["a_off"], tb.data_ptr() + 4 * g["b_off"]
    want = G.expected(case)[backend]
    outs = []
    for t in tc:
        pc = t.data_ptr() + 4 * g["c_off"]
        plan = _hip.matmul_plan(backend, case.batch, case.M, case.N, case.K, g["sa"], g["sb"], g["sc"], pa, pb, pc)
        assert plan == want, f"{case.name} backend {backend}: plan {plan}, the table states {want}"
        _hip.check(lib.mt_matmul_f32(pc, pa, pb, case.batch, case.M, case.N, case.K, _s3(g["sa"]), _s3(g["sb"]),
                                     _s3(g["sc"]), _hip.stream_ptr()), "mt_matmul_f32")
        torch.cuda.synchronize()
        outs.append(t.cpu().numpy())
    # footprint: nothing but C's elements written, the operands untouched
    outside = G.outside_mask(g["c_size"], g["c_off"], g["sc"], shape_c)
    hit = np.flatnonzero(outs[0].view(np.uint32)[outside] != G.SENTINEL)
    assert hit.size == 0, (f"{case.name} backend {backend}: {hit.size} floats outside C written, first at "
                           f"buffer offset {np.flatnonzero(outside)[hit[0]]} (C starts at {g['c_off']}, strides {g['sc']})")
    assert np.array_equal(ta.cpu().numpy().view(np.uint32), abuf.view(np.uint32)), "A was modified"
    assert np.array_equal(tb.cpu().numpy().view(np.uint32), bbuf.view(np.uint32)), "B was modified"
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "a second call differs"
    c = G.view(outs[0], g["c_off"], g["sc"], shape_c).copy()
    unwritten = c.view(np.uint32) == G.SENTINEL
    assert not unwritten.any(), f"{case.name} backend {backend}: C{tuple(np.argwhere(unwritten)[0])} never written"
    assert not np.isnan(c).any(), f"{case.name} backend {backend}: NaN padding reached C{tuple(np.argwhere(np.isnan(c))[0])}"
    return c, want


def assert_bitwise(case, backend, plan, got, want32, what):
    bad = np.argwhere(_bits(got) != _bits(want32))
    if bad.size:
        b, m, n = (int(v) for v in bad[0])
        raise AssertionError(
            f"{case.name} backend {backend} {what}: {len(bad)} of {got.size} wrong, first C[{b}, {m}, {n}] = "
            f"{got[b, m, n]!r}, want {want32[b, m, n]!r} (difference {float(got[b, m, n]) - float(want32[b, m, n])!r}); "
            f"plan {plan}; {G.locate(case, plan, b, m, n)}")


@pytest.mark.parametrize("kind", ["ints", "wide_a", "wide_b"])
@pytest.mark.parametrize("backend", BACKENDS, indirect=True)
@pytest.mark.parametrize("case", G.TABLE, ids=lambda c: c.name)
def test_exact(dev, case, backend, kind):
    a, b = G.inputs(case, kind)
    got, plan = run_case(dev, case, backend, a, b)
    assert_bitwise(case, backend, plan, got, G.ref64(case, kind).astype(np.float32), kind)


@pytest.mark.parametrize("backend", BACKENDS, indirect=True)
@pytest.mark.parametrize("case", G.TABLE, ids=lambda c: c.name)
def test_gauss(dev, case, backend, parity_record):
    """The project's accuracy figures (test_matmul's elementwise bound on every backend,
    test_matmul_x3_128_tiles' 1e-6 of max|C| on backends 2 and 3), then the scaled twin."""
    a, b = G.inputs(case, "gauss")
    got, plan = run_case(dev, case, backend, a, b)
    ref = G.ref64(case, "gauss")
    err = np.abs(got.astype(np.float64) - ref)
    bound = 1e-5 * max(1.0, case.K / 32) + 1e-5 * np.abs(ref)
    r_elem = float((err / bound).max())
    r_max = float(err.max() / np.abs(ref).max())
    r_comp = float((err / G.abs_product(case)).max())
    print(f"{case.name} backend {backend} kernel {plan[0]}: err/bound {r_elem:.3g}, max err / max|C| {r_max:.3g}, "
          f"componentwise {r_comp:.3g}")
    parity_record("test_gemm_matrix_gpu::test_gauss", f"{case.name}-b{backend}", kernel=plan[0], K=case.K,
                  err_over_bound=r_elem, bound=1.0, max_err_over_max_ref=r_max, componentwise=r_comp)
    assert r_elem <= 1.0, f"{case.name} backend {backend}: |C - C64| is {r_elem:.3g} x its bound"
    if backend in (2, 3):
        assert r_max <= 1e-6, f"{case.name} backend {backend}: max|C - C64| / max|C64| = {r_max:.3g} > 1e-6"
    a2, b2, factor = G.scaled_twin(case)
    twin, _ = run_case(dev, case, backend, a2, b2)
    assert_bitwise(case, backend, plan, twin, got * factor[None], "scaled twin against the scaled base result")


# ---- the minitorch layer: every branch of HipKernelOps.matrix_multiply ----------------------
def _ints(rng, *shape):
    return rng.integers(-4, 5, size=shape).astype(np.float32)


def _layer_cases():
    """name -> (a shape, b shape, how a is stored, how b is stored). 'T': the transpose is stored
    and permuted back; 'P': rows at a pitch of 3 more floats."""
    return {
        "dense2d": ((37, 29), (29, 41), "", ""),
        "pitched": ((37, 29), (29, 41), "P", "P"),
        "left_t_small": ((37, 29), (29, 41), "T", ""),
        "left_t_large": ((1030, 9), (9, 5), "T", ""),       # an output above 1024 rows: the copy
        "right_t_small": ((37, 29), (29, 41), "", "T"),
        "right_t_large": ((5, 9), (9, 1030), "", "T"),      # above 1024 columns: the copy
        "2d_3d": ((5, 7), (3, 7, 6), "", ""),
        "3d_2d": ((3, 5, 7), (7, 6), "", ""),
        "2d_t_3d": ((5, 7), (3, 7, 6), "T", ""),
        "3d_t_3d": ((3, 5, 7), (3, 7, 6), "T", ""),         # a gemm_ready 3-D view: no copy
        "4d": ((2, 3, 5, 7), (2, 3, 7, 6), "", ""),
        "4d_t": ((2, 3, 5, 7), (2, 3, 7, 6), "T", "T"),     # 4-D views: the copy
        "bcast_left": ((1, 5, 7), (3, 7, 6), "", ""),
        "bcast_right": ((3, 5, 7), (1, 7, 6), "", ""),
        "bcast_4d": ((1, 1, 5, 7), (2, 3, 7, 6), "", ""),
    }


def _tensor(minitorch, B, x, how, requires_grad=False, leaf=False):
    """The operand as matrix_multiply is to see it; with leaf also the tensor that holds .grad."""
    if how == "T":
        t = minitorch.tensor_from_numpy(np.ascontiguousarray(np.swapaxes(x, -1, -2)), B, requires_grad)
        order = list(range(x.ndim))
        order[-1], order[-2] = order[-2], order[-1]
        used = t.permute(*order)
    elif how == "P":
        assert x.ndim == 2
        flat = np.full((x.shape[0], x.shape[1] + 3), np.nan, np.float32)
        flat[:, :x.shape[1]] = x
        t = used = minitorch.Tensor(minitorch.TensorData(flat.reshape(-1), x.shape, (x.shape[1] + 3, 1)), backend=B)
    else:
        t = used = minitorch.tensor_from_numpy(x, B, requires_grad)
    return (used, t) if leaf else used


@pytest.fixture(scope="module")
def mt(dev):
    import minitorch
    return minitorch, minitorch.TensorBackend(minitorch.HipKernelOps)


@pytest.mark.parametrize("backend", (0, 2), indirect=True)
@pytest.mark.parametrize("name", list(_layer_cases()))
def test_tensor_matmul_is_exact(mt, backend, name):
    minitorch, B = mt
    sa, sb, ha, hb = _layer_cases()[name]
    rng = np.random.default_rng(len(name))
    x, w = _ints(rng, *sa), _ints(rng, *sb)
    out = (_tensor(minitorch, B, x, ha) @ _tensor(minitorch, B, w, hb)).to_numpy()
    ref = np.matmul(x.astype(np.float64), w.astype(np.float64)).astype(np.float32)
    assert out.shape == ref.shape
    bad = np.argwhere(_bits(out) != _bits(ref))
    assert bad.size == 0, f"{name}: {len(bad)} wrong, first at {tuple(bad[0])}: {out[tuple(bad[0])]} want {ref[tuple(bad[0])]}"


def test_partial_batch_broadcast_is_refused(mt):
    minitorch, B = mt
    rng = np.random.default_rng(0)
    a = minitorch.tensor_from_numpy(_ints(rng, 2, 1, 5, 7), B)
    b = minitorch.tensor_from_numpy(_ints(rng, 2, 3, 7, 6), B)
    with pytest.raises(NotImplementedError):
        a @ b


@pytest.mark.parametrize("backend", (0, 2), indirect=True)
@pytest.mark.parametrize("name", ["dense2d", "right_t_small", "4d"])
def test_matmul_backward_is_exact(mt, backend, name):
    """MatMul.backward: dA = G Bᵀ and dB = Aᵀ G with an integer upstream gradient G."""
    minitorch, B = mt
    sa, sb, ha, hb = _layer_cases()[name]
    rng = np.random.default_rng(3 + len(name))
    x, w = _ints(rng, *sa), _ints(rng, *sb)
    (ta, la), (tb, lb) = _tensor(minitorch, B, x, ha, True, True), _tensor(minitorch, B, w, hb, True, True)
    out = ta @ tb
    gup = _ints(rng, *out.shape)
    out.backward(minitorch.tensor_from_numpy(gup, B))
    g64, x64, w64 = (v.astype(np.float64) for v in (gup, x, w))
    da = np.matmul(g64, np.swapaxes(w64, -1, -2)).astype(np.float32)
    db = np.matmul(np.swapaxes(x64, -1, -2), g64).astype(np.float32)
    assert np.abs(da).max() < 2 ** 24 and np.abs(db).max() < 2 ** 24
    for what, t, how, ref in (("dA", la, ha, da), ("dB", lb, hb, db)):
        got = t.grad.to_numpy()
        if how == "T":  # the leaf holds the transpose
            got = np.swapaxes(got, -1, -2)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bad = np.argwhere(_bits(got) != _bits(ref))
        assert bad.size == 0, f"{name} {what}: {len(bad)} wrong, first at {tuple(bad[0])}"
