"""mt_matmul_f32_plan (include/minitorch_hip.h) and the GEMM exactness matrix's table and inputs
(tests/gemm_cases.py), on the CPU: the query makes no device call, so nothing is launched.

The table must reach every kernel variant the dispatch has (the coverage condition below), each
entry's plan under each backend must be the one the table states, and the exact input kinds
must be exact by construction: tests/test_gemm_matrix_gpu.py then holds the kernels to bitwise
equality with the float64 product on these inputs."""
import ctypes

import numpy as np
import pytest

import gemm_cases as G

BASE = 0x7F0000001000  # a 4 KiB-aligned stand-in for a device allocation: only its low bits count


@pytest.fixture(scope="module")
def lib():
    from minitorch import _hip
    return _hip.lib()


def plan_of(case, backend, base=(BASE, BASE, BASE)):
    from minitorch import _hip
    g = G.geometry(case)
    return _hip.matmul_plan(backend, case.batch, case.M, case.N, case.K, g["sa"], g["sb"], g["sc"],
                            base[0] + 4 * g["a_off"], base[1] + 4 * g["b_off"], base[2] + 4 * g["c_off"])


def _s3(*v):
    return (ctypes.c_int64 * 3)(*v)


def test_symbol_and_binding(lib):
    from minitorch import _hip
    assert hasattr(lib, "mt_matmul_f32_plan")
    assert "mt_matmul_f32_plan" in _hip.exported_symbols()
    assert lib.mt_abi_version() == 3


@pytest.mark.parametrize("backend,sizes,msg", [
    (0, (0, 5, 7, 9), b"bad sizes"),
    (0, (1, 0, 7, 9), b"bad sizes"),
    (2, (1, 5, 0, 9), b"bad sizes"),
    (3, (1, 5, 7, 0), b"bad sizes"),
    (1, (-1, 5, 7, 9), b"bad sizes"),
    (4, (1, 5, 7, 9), b"backend"),
    (-1, (1, 5, 7, 9), b"backend"),
    (1, (65536, 5, 7, 9), b"65535"),
])
def test_plan_rejects_bad_arguments(lib, backend, sizes, msg):
    out = (ctypes.c_int32 * 5)()
    assert lib.mt_matmul_f32_plan(backend, *sizes, _s3(63, 9, 1), _s3(63, 7, 1), _s3(35, 7, 1),
                                  None, None, None, out) < 0
    assert msg in lib.mt_last_error(), lib.mt_last_error()


@pytest.mark.parametrize("null", [0, 1, 2])
def test_plan_rejects_null_strides(lib, null):
    s = [_s3(63, 9, 1), _s3(63, 7, 1), _s3(35, 7, 1)]
    s[null] = None
    assert lib.mt_matmul_f32_plan(0, 1, 5, 7, 9, *s, None, None, None, None) < 0
    assert b"NULL" in lib.mt_last_error()


def test_plan_out_may_be_null_and_pointers_are_not_read(lib):
    """The pointers count for their alignment only: unmapped addresses give the same plan as
    NULL wherever their low four bits agree, and another one where they do not."""
    s = (_s3(0, 48, 1), _s3(0, 72, 1), _s3(0, 69, 1))
    assert lib.mt_matmul_f32_plan(2, 1, 67, 69, 45, *s, None, None, None, None) == G.X3
    out = (ctypes.c_int32 * 5)()
    for a, vec in ((0x10, 1), (0x7F0000000040, 1), (0x14, 0), (0x7F0000000044, 0)):
        assert lib.mt_matmul_f32_plan(2, 1, 67, 69, 45, *s, a, 0x20, 0x30, out) == G.X3
        assert list(out) == [1, 0, vec, 1, 45]


@pytest.mark.parametrize("backend", [0, 1, 2, 3])
@pytest.mark.parametrize("case", G.TABLE, ids=lambda c: c.name)
def test_table_entry_has_the_stated_plan(lib, case, backend):
    assert plan_of(case, backend) == G.expected(case)[backend]
    # a function of its arguments alone
    assert plan_of(case, backend) == G.expected(case)[backend]


def test_the_over_65535_batch_falls_to_the_fp32_kernel_or_is_refused(lib):
    """The own kernels put the batch in gridDim.z: the X3 plan gives way, the fp32 kernel refuses."""
    s = (_s3(63, 9, 1), _s3(63, 7, 1), _s3(35, 7, 1))
    out = (ctypes.c_int32 * 5)()
    assert lib.mt_matmul_f32_plan(0, 65536, 5, 7, 9, *s, None, None, None, out) == G.ROCBLAS
    for backend in (1, 2, 3):
        assert lib.mt_matmul_f32_plan(backend, 65536, 5, 7, 9, *s, None, None, None, out) < 0
    # (256 or more matrices fill the chip with 128-tiles, whatever their size)
    assert lib.mt_matmul_f32_plan(2, 65535, 5, 7, 9, *s, None, None, None, out) == G.X3BIG
    assert lib.mt_matmul_f32_plan(3, 65535, 5, 7, 9, *s, None, None, None, out) == G.X3


def test_table_reaches_every_kernel_variant(lib):
    """The coverage condition: kernels 3 and 4 in all eight (ak, bk, vec) forms, each unsplit and
    split; rocBLAS in its four op combinations; its split at S = 8, 4, 2 with each op on each
    operand; the fp32 kernel. From the library's own answers, not the table's expectations."""
    seen = set()
    for case in G.TABLE:
        for backend in range(4):
            kern, ak, bk, vec, S, ks = plan_of(case, backend)
            seen.add((kern, ak, bk, vec, S > 1))
            if kern == G.ROCBLAS_SPLIT:
                seen.add(("rbS", S))
                seen.add(("rbA", ak))
                seen.add(("rbB", bk))
                seen.add(("rbAB", S, ak, bk))
    want = {(kern, ak, bk, vec, split) for kern in (G.X3, G.X3BIG) for ak in (0, 1) for bk in (0, 1)
            for vec in (0, 1) for split in (False, True)}
    want |= {(G.ROCBLAS, ak, bk, -1, False) for ak in (0, 1) for bk in (0, 1)}
    want |= {("rbS", S) for S in (8, 4, 2)} | {("rbA", v) for v in (0, 1)} | {("rbB", v) for v in (0, 1)}
    want |= {("rbAB", 8, ak, bk) for ak in (0, 1) for bk in (0, 1)}
    want |= {(G.F32, -1, -1, -1, False)}
    missing = sorted(want - seen, key=str)
    assert not missing, f"the table does not reach (kernel, ak, bk, vec, split): {missing}"
    # the fp32 kernel from every backend
    for backend in range(4):
        assert any(plan_of(c, backend)[0] == G.F32 for c in G.TABLE), backend


def test_split_edges_named_by_the_issue(lib):
    """The slice counts the classes were chosen for."""
    plan = lambda name, backend: plan_of(G.BY_NAME[name], backend)  # noqa: E731
    assert {c.K: plan_of(c, 3)[4] for c in G.TABLE if c.cls == "split64"} == {511: 1, 512: 2, 1100: 4, 4100: 15}
    assert 4100 - 14 * 288 == 68  # the ragged last slice
    assert plan("bigs-kkv", 2)[4:] == (8, 1040) and 8200 - 7 * 1040 == 920
    assert plan("rb4097-nn", 0)[0] == G.ROCBLAS and plan("rb8192-coff", 0)[0] == G.ROCBLAS
    assert plan("rb8192-cpad3", 0)[0] == G.ROCBLAS and plan("rb8192-b2", 0)[0] == G.ROCBLAS
    assert G.geometry(G.BY_NAME["rb8192-nt"])["sc"][1] == 12


def _shapes():
    seen, out = set(), []
    for c in G.TABLE:
        k = G._shape_key(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


@pytest.mark.parametrize("kind", ["ints", "wide_a", "wide_b"])
@pytest.mark.parametrize("case", _shapes(), ids=lambda c: c.name)
def test_exact_kinds_are_exact(case, kind):
    a, b = G.inputs(case, kind)
    ref = G.ref64(case, kind)
    assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() < 2 ** 24
    # every partial sum, whatever the order: the sum of the terms' magnitudes stays below 2^24
    worst = np.matmul(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64)).max()
    assert worst < 2 ** 24, worst
    got32 = np.matmul(a, b)
    assert got32.dtype == np.float32 and np.array_equal(got32.astype(np.float64), ref)
    if kind == "ints":
        assert np.abs(a).max() <= 4 and np.abs(b).max() <= 4 and np.array_equal(a, np.rint(a))
        # dense: 8 of the 9 values are non-zero (a handful of elements proves nothing either way)
        assert all(x.size < 100 or (x != 0).mean() > 0.8 for x in (a, b))
        return
    wide, sparse = (a, np.swapaxes(b, 1, 2)) if kind == "wide_a" else (b, a)  # sparse: [.., lines, K]
    assert np.array_equal(np.abs(wide), np.full(wide.shape, np.float32(G.WIDE)))
    assert set(np.unique(sparse)) <= {-1.0, 0.0, 1.0}
    nz = (sparse != 0).sum(-1)
    assert nz.max() <= G.CAP
    if case.K <= G.CAP:
        assert (sparse != 0).mean() > 0.8
    else:
        assert nz.min() == G.CAP
        must = G.mandatory_k(case.K, case.M, case.N, case.batch)
        assert (sparse[..., list(must)] != 0).all()
        # the positions the issue names: slice edges of every plan of the shape, flush edges, K - 1
        assert case.K - 1 in must and 0 in must and 255 in must and (case.K <= 257 or 256 in must)
        for c in G.TABLE:
            if G._shape_key(c) == G._shape_key(case):
                for plan in G.expected(c):
                    S, ks = plan[4], plan[5]
                    for s in range(S):
                        assert s * ks in must and min(case.K, (s + 1) * ks) - 1 in must, (c.name, plan, s)


def test_wide_value_has_three_bf16_pieces():
    """65793 truncated to bf16 three times: 65536, 256, 1 (each piece exact in 8 significand bits)."""
    def bf16_trunc(x):
        u = np.array([x], np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
        return float(u.view(np.float32)[0])
    x = G.WIDE
    h = bf16_trunc(x)
    m = bf16_trunc(x - h)
    l = bf16_trunc(x - h - m)
    assert (h, m, l) == (65536.0, 256.0, 1.0)
    assert G.CAP * G.WIDE < 2 ** 24


@pytest.mark.parametrize("case", _shapes(), ids=lambda c: c.name)
def test_gauss_reference_is_scale_invariant(case):
    """NumPy's float32 product of the scaled twin is the scaled float32 product, bit for bit: the
    reference satisfies the property the kernels are held to."""
    a, b = G.inputs(case, "gauss")
    a2, b2, factor = G.scaled_twin(case)
    assert np.array_equal(np.abs(np.log2(np.abs(factor))), np.rint(np.abs(np.log2(np.abs(factor)))))
    base = np.matmul(a, b)
    twin = np.matmul(a2, b2)
    assert np.array_equal((base * factor[None]).view(np.uint32), twin.view(np.uint32))
    # and in float64 exactly
    assert np.array_equal(np.matmul(a2.astype(np.float64), b2.astype(np.float64)),
                          G.ref64(case, "gauss") * factor[None].astype(np.float64))


@pytest.mark.parametrize("case", G.TABLE, ids=lambda c: c.name)
def test_placement_is_disjoint_and_padded(case):
    """Every view lies inside its buffer, its elements are distinct (a size-1 dimension apart)
    and there is padding before or after it."""
    g = G.geometry(case)
    for key, shape in (("a", (case.batch, case.M, case.K)), ("b", (case.batch, case.K, case.N)),
                       ("c", (case.batch, case.M, case.N))):
        size, off, st = g[key + "_size"], g[key + "_off"], g["s" + key]
        nb = 1 if st[0] == 0 else shape[0]
        idx = np.arange(size, dtype=np.int64)
        v = G.view(idx, off, st, shape)
        assert v.max() <= size - 1 - G.TAIL and v.min() == off
        assert np.unique(v).size == nb * shape[1] * shape[2]
        assert G.outside_mask(size, off, st, shape).sum() == size - nb * shape[1] * shape[2] >= G.TAIL
