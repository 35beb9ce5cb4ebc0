"""The generic tensor layer of the HIP backend (csrc/combine.hip: map, zip, the six reduce
kernels, the GEMMs) on an MI355X, against plain high-precision references.

Counterpart of the reference's tests/test_tensor_general.py (every one-argument, two-argument
and reduce function, forward and gradient, on the device backend):

  A. every function id (1..18) on every map / zip dispatch path, through the C ABI on torch
     device tensors, against the formulas of minitorch/operators.py evaluated in NumPy, on
     finite inputs and on inputs spiked with +-0, +-inf, NaN, FLT_MAX, FLT_MIN and a denormal;
  B. every reduce kernel x {add, mul, max} x identity / non-identity ``start`` at the smallest
     shapes that select each kernel, against the float64 fold;
  C. every tensor Function, forward and backward, against torch float64 autograd;
  D. +-inf operands of mt_matmul_f32 on every GEMM backend.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
U = 2.0 ** -24  # fp32 unit roundoff
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MAX, FLT_MIN, 1e-40], dtype=np.float32)
SENTINEL = 12345.0

FN = {"add": 1, "mul": 2, "id": 3, "neg": 4, "lt": 5, "eq": 6, "sigmoid": 7, "relu": 8,
      "relu_back": 9, "log": 10, "log_back": 11, "exp": 12, "inv": 13, "inv_back": 14,
      "is_close": 15, "max": 16, "pow": 17, "tanh": 18}
MAP_NAMES = ["id", "neg", "sigmoid", "relu", "log", "exp", "inv", "tanh"]
ZIP_NAMES = ["add", "mul", "lt", "eq", "is_close", "relu_back", "log_back", "inv_back", "max", "pow"]
EXACT = {"add", "mul", "id", "neg", "relu", "relu_back", "lt", "eq", "is_close", "max"}
# rounded ops: (rtol, atol beyond FLT_MIN, ulp bound or None)
#   exp, sigmoid and the divisions: rtol 1e-6, tanh: rtol 1e-5 / atol 1e-6 (test_generic_ops' bounds);
#   log 3 ulp and pow 16 ulp of the fp32 result: the OpenCL full-profile fp32 bounds, which the
#   ROCm device math library is specified to meet
ROUNDED = {"exp": (1e-6, 0.0, None), "sigmoid": (1e-6, 0.0, None), "inv": (1e-6, 0.0, None),
           "log_back": (1e-6, 0.0, None), "inv_back": (1e-6, 0.0, None), "tanh": (1e-5, 1e-6, None),
           "log": (0.0, 0.0, 3.0), "pow": (0.0, 0.0, 16.0)}
_WORST_ULP = {}


@pytest.fixture(scope="module")
def mt():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from minitorch import _hip
    _hip.lib()  # fail loudly if the HIP library is missing
    return minitorch, minitorch.TensorBackend(minitorch.HipKernelOps)


# ---- device buffers with free shape / strides / base offset ----------------------------------
def _contig(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= s
    return tuple(reversed(st))


def _c64(vals):
    return (ctypes.c_int64 * max(1, len(vals)))(*[int(v) for v in vals])


class Dev:
    """A strided fp32 view (shape, element strides, base offset in floats) of a 1-D torch device
    buffer that is exactly as long as the view needs; the rest is filled with SENTINEL."""

    def __init__(self, shape, strides=None, offset=0):
        import torch
        self.shape = tuple(int(s) for s in shape)
        self.strides = tuple(int(s) for s in (strides if strides is not None else _contig(self.shape)))
        self.offset = int(offset)
        span = 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides)) if all(self.shape) else 1
        self.store = torch.full((self.offset + span,), SENTINEL, dtype=torch.float32, device="cuda")

    @classmethod
    def from_numpy(cls, arr, strides=None, offset=0):
        import torch
        d = cls(arr.shape, strides, offset)
        d.view().copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).cuda())
        return d

    @property
    def ptr(self):
        return self.store.data_ptr() + 4 * self.offset

    @property
    def dims(self):
        return len(self.shape)

    def view(self):
        import torch
        return torch.as_strided(self.store, self.shape, self.strides, self.offset)

    def numpy(self):
        return self.view().cpu().numpy()

    def gaps_untouched(self):
        """Every element of the buffer outside the view still holds SENTINEL."""
        import torch
        mask = torch.ones_like(self.store, dtype=torch.bool)
        torch.as_strided(mask, self.shape, self.strides, self.offset).fill_(False)
        return bool((self.store[mask] == SENTINEL).all())

    def tensor(self, minitorch, backend):
        from minitorch.tensor import Tensor
        from minitorch.tensor_data import TensorData
        return Tensor(TensorData(self.store[self.offset:], self.shape, self.strides), backend=backend)


def _stream():
    from minitorch import _hip
    return _hip.stream_ptr()


def _map(fn, out, a):
    from minitorch import _hip
    return _hip.lib().mt_tensor_map(fn, out.ptr, _c64(out.shape), _c64(out.strides), out.dims, a.ptr,
                                    _c64(a.shape), _c64(a.strides), a.dims, _stream())


def _zip(fn, out, a, b):
    from minitorch import _hip
    return _hip.lib().mt_tensor_zip(fn, out.ptr, _c64(out.shape), _c64(out.strides), out.dims, a.ptr,
                                    _c64(a.shape), _c64(a.strides), a.dims, b.ptr, _c64(b.shape),
                                    _c64(b.strides), b.dims, _stream())


def _reduce(fn, out, a, dim, start):
    from minitorch import _hip
    return _hip.lib().mt_tensor_reduce(fn, out.ptr, _c64(out.shape), _c64(out.strides), a.ptr, _c64(a.shape),
                                       _c64(a.strides), a.dims, int(dim), ctypes.c_float(start), _stream())


def _ok(status, what):
    from minitorch import _hip
    assert status == 0, f"{what}: {_hip.lib().mt_last_error().decode(errors='replace')}"


# ---- the reference: minitorch/operators.py in NumPy, IEEE semantics ---------------------------
def ref_fn(name, x, y=None):
    """fn(x, y) elementwise (broadcast). Every step the kernel takes in fp32 on the input side is
    taken in fp32 (x + 1e-6 before log / log_back, the two differences of is_close, x * x of
    inv_back; add, mul and the selects are single fp32 operations), the rest in float64. The
    selects keep the formulas' literal NaN behaviour: max(NaN, y) = y, max(x, NaN) = NaN,
    relu(NaN) = 0, relu_back(NaN, d) = 0, lt / eq / is_close with a NaN = 0, is_close(inf, inf) = 0."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float32)
        X = x.astype(np.float64)
        if y is not None:
            y = np.asarray(y, dtype=np.float32)
            Y = y.astype(np.float64)
        one, zero = F32(1.0), F32(0.0)
        if name == "add":
            return x + y
        if name == "mul":
            return x * y
        if name == "id":
            return x.copy()
        if name == "neg":
            return -x
        if name == "lt":
            return np.where(x < y, one, zero)
        if name == "eq":
            return np.where(x == y, one, zero)
        if name == "is_close":
            return np.where(((x - y).astype(np.float64) < 1e-2) & ((y - x).astype(np.float64) < 1e-2), one, zero)
        if name == "relu":
            return np.where(x > 0, x, zero)
        if name == "relu_back":
            return np.where(x > 0, y, zero)
        if name == "max":
            return np.where(x > y, x, y)
        if name == "sigmoid":
            e = np.exp(X)
            return np.where(X >= 0, 1.0 / (1.0 + np.exp(-X)), e / (1.0 + e))
        if name == "log":
            return np.log((x + F32(1e-6)).astype(np.float64))
        if name == "log_back":
            return Y / (x + F32(1e-6)).astype(np.float64)
        if name == "exp":
            return np.exp(X)
        if name == "inv":
            return 1.0 / X
        if name == "inv_back":
            return -(1.0 / (x * x).astype(np.float64)) * Y
        if name == "pow":
            return np.power(X, Y)
        if name == "tanh":
            return np.tanh(X)
    raise KeyError(name)


def check_fn(name, got, ref, where=""):
    """Exact ops: equal (NaN at the same places; id and neg also in the sign of zero). Rounded
    ops: the finite / +inf / -inf / NaN classes equal those of the reference rounded to fp32, and
    the finite entries within the op's bound plus FLT_MIN (a flushed denormal result passes).
    Returns the worst error of the finite entries in ulps of the fp32 result."""
    assert got.dtype == np.float32 and got.shape == ref.shape, (where, got.shape, ref.shape)
    if name in EXACT:
        ref = ref.astype(np.float32)
        np.testing.assert_array_equal(got, ref, err_msg=f"{name} {where}")
        if name in ("id", "neg"):
            keep = ~np.isnan(ref)
            np.testing.assert_array_equal(got.view(np.uint32)[keep], ref.view(np.uint32)[keep],
                                          err_msg=f"{name} {where}: sign of zero")
        return 0.0
    rtol, atol, ulps = ROUNDED[name]
    with np.errstate(all="ignore"):
        ref32 = ref.astype(np.float32)
    for cls, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        np.testing.assert_array_equal(f(got), f(ref32), err_msg=f"{name} {where}: {cls} class mask")
    fin = np.isfinite(ref32)
    if not fin.any():
        return 0.0
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    spacing = np.spacing(np.maximum(np.abs(ref32[fin]), F32(FLT_MIN))).astype(np.float64)
    bound = FLT_MIN + atol + rtol * np.abs(ref[fin]) + (ulps * spacing if ulps else 0.0)
    worst = int(np.argmax(err - bound))
    assert err[worst] <= bound[worst], (f"{name} {where}: |err| {err[worst]:.3e} > bound {bound[worst]:.3e} "
                                        f"at ref {ref[fin][worst]!r}, got {got[fin][worst]!r}")
    normal = np.abs(ref32[fin]) >= FLT_MIN
    return float((err[normal] / spacing[normal]).max()) if normal.any() else 0.0


def _note_ulp(name, ulp):
    _WORST_ULP[name] = max(_WORST_ULP.get(name, 0.0), ulp)


# ---- inputs ------------------------------------------------------------------------------------
def _logmag(rng, shape, lo, hi, signed=True):
    v = 10.0 ** rng.uniform(lo, hi, size=shape)
    if signed:
        v = v * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(np.float32)


def finite_inputs(name, xs, ys, rng, variant=0):
    """(x, y) of shapes xs, ys for fn(x, y) (y None for a map): N(0, 1) in general; |x| in
    [1e-3, 1e3] where the formula divides; small-integer grids where ties must occur (lt, eq,
    max, is_close); positive bases for fractional pow and (variant 1) negative bases with the
    exponents 2 and 3."""
    n = lambda s, k=1.0: (rng.standard_normal(s) * k).astype(np.float32)  # noqa: E731
    if name in ("lt", "eq", "max"):
        return (rng.integers(-3, 4, size=xs).astype(np.float32), rng.integers(-3, 4, size=ys).astype(np.float32))
    if name == "is_close":  # differences 0, 0.006 (close), 0.012, ... (not close)
        return ((rng.integers(-3, 4, size=xs) * 0.006).astype(np.float32),
                (rng.integers(-3, 4, size=ys) * 0.006).astype(np.float32))
    if name in ("inv", "log"):
        return _logmag(rng, xs, -3, 3, signed=name == "inv"), None
    if name in ("log_back", "inv_back"):
        return _logmag(rng, xs, -3, 3), n(ys)
    if name == "pow":
        if variant == 1:
            return _logmag(rng, xs, -1, 1), rng.choice([2.0, 3.0], size=ys).astype(np.float32)
        return _logmag(rng, xs, -1.5, 1.5, signed=False), n(ys, 2.0)
    if name == "exp":
        return n(xs, 10.0), None
    if name in ("sigmoid", "tanh"):
        return n(xs, 4.0), None
    return n(xs), (n(ys) if ys is not None else None)


def spike_positions(size):
    """The first, a middle and the last elements (C order) of an operand: up to eight places,
    which fall in both the float4 body and the scalar tail of the dense kernels."""
    pos = [0, 1, 2, size // 2, size // 2 + 1, size - 3, size - 2, size - 1]
    return sorted({p for p in pos if 0 <= p < size})


def spiked(arr, variant, shift=0):
    """arr with SPECIALS at spike_positions; `variant` walks through the specials where the operand
    has fewer than eight places, `shift` rotates them (so two spiked operands pair up differently)."""
    out = arr.copy()
    flat = out.reshape(-1)
    pos = spike_positions(flat.size)
    for i, p in enumerate(pos):
        flat[p] = SPECIALS[(variant * len(pos) + i + shift) % len(SPECIALS)]
    return out


def n_spike_variants(size):
    k = len(spike_positions(size))
    return (len(SPECIALS) + k - 1) // k


# ---- Part A: layouts ----------------------------------------------------------------------------
R8 = (2, 1, 3, 1, 2, 2, 1, 4)


def _stride2(shape):
    """Row-major strides with a last-dim stride of 2 (every other float is a gap)."""
    return tuple(2 * s for s in _contig(shape))


# name -> (shape of x (the full operand), shape of y, left (y is the left operand), layout of y:
#          None | "permuted" | "offset", strides of out: None (contiguous) | "stride2")
ZIP_LAYOUTS = {
    "same": ((6, 5, 8), (6, 5, 8), False, None, None),            # zip_dense<0,false>, float4 body
    "same_odd": ((6, 5, 7), (6, 5, 7), False, None, None),        # its n % 4 != 0 tail
    "scalar_right": ((6, 5, 8), (1,), False, None, None),         # zip_dense<1,false>
    "scalar_left": ((6, 5, 8), (1,), True, None, None),           # zip_dense<1,true>
    "scalar_right_odd": ((6, 5, 7), (1,), False, None, None),
    "scalar_left_odd": ((6, 5, 7), (1,), True, None, None),
    "row_right": ((6, 5, 8), (8,), False, None, None),            # zip_dense<2,false>
    "row_left": ((6, 5, 8), (5, 8), True, None, None),            # zip_dense<2,true>
    "row_odd": ((6, 5, 7), (7,), False, None, None),              # the odd row: scalar form
    "row_odd_left": ((6, 5, 7), (7,), True, None, None),
    "col_bcast": ((6, 5, 8), (6, 5, 1), False, None, None),       # zip_kernel<int>
    "col_bcast_left": ((6, 5, 8), (6, 5, 1), True, None, None),
    "permuted": ((6, 5, 8), (6, 5, 8), False, "permuted", None),
    "permuted_left": ((6, 5, 8), (6, 5, 8), True, "permuted", None),
    "offset_view": ((6, 5, 8), (6, 5, 8), False, "offset", None),  # a base one float off alignment
    "out_strided": ((6, 5, 8), (6, 5, 8), False, None, "stride2"),  # the out_pos path
    "rank8": (R8, (2, 1, 4), False, None, "stride2"),             # rank 8 out, rank 3 operand
    "rank8_left": (R8, (2, 1, 4), True, None, "stride2"),
    "rank8_dense": (R8, (2, 1, 4), False, None, None),            # the same through zip_dense<2>
    "lower_rank": ((5, 1), (8,), False, None, None),              # both operands broadcast
}
MAP_LAYOUTS = {k: v for k, v in ZIP_LAYOUTS.items() if not v[2] and k != "scalar_right_odd"}


def _operand(arr, how):
    if how == "permuted":  # storage in reversed dim order, seen through permuted strides
        rev = tuple(reversed(range(arr.ndim)))
        return Dev.from_numpy(arr, strides=tuple(reversed(_contig(tuple(arr.shape[i] for i in rev)))))
    if how == "offset":
        return Dev.from_numpy(arr, offset=1)
    return Dev.from_numpy(arr)


def _out_for(shape, how):
    return Dev(shape, _stride2(shape) if how == "stride2" else None)


def _variants(name, xs, ys, rng):
    """(label, x, y): the finite set(s), then the same set spiked in x, in y, and in both."""
    for fv in range(2 if name == "pow" else 1):
        x, y = finite_inputs(name, xs, ys, rng, fv)
        yield f"finite{fv}", x, y
    nx, ny = int(np.prod(xs)), (int(np.prod(ys)) if ys is not None else 0)
    for v in range(n_spike_variants(nx)):
        yield f"spike_x{v}", spiked(x, v), y
    if ys is not None:
        for v in range(n_spike_variants(ny)):
            yield f"spike_y{v}", x, spiked(y, v)
            yield f"spike_xy{v}", spiked(x, v), spiked(y, v, shift=3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("layout", list(ZIP_LAYOUTS))
@pytest.mark.parametrize("name", ZIP_NAMES)
def test_zip_matrix(mt, name, layout):
    """Every two-argument function id on every mt_tensor_zip dispatch path through the C ABI
    (dense same-shape, one-element and repeated-block operands on either side, their scalar
    tails, the strided int32 kernel with broadcast / permuted / misaligned operands, a strided
    `out`, rank 8), finite and spiked inputs, against ref_fn; where the layout can be expressed
    with minitorch Tensors, also through the backend with the _mtfast extension on and off,
    bitwise equal to the C-ABI result. The left layouts put the repeated operand first, so the
    non-commutative ids (relu_back, log_back, inv_back, pow, lt, and max through its NaN
    asymmetry) check the operand order of the SWAP kernels."""
    from minitorch import _hip
    minitorch, B = mt
    xs, ys, left, yhow, ohow = ZIP_LAYOUTS[layout]
    rng = np.random.default_rng(1000 * FN[name] + list(ZIP_LAYOUTS).index(layout))
    out_shape = np.broadcast_shapes(xs, ys)
    tname = {"pow": "pow_scalar_zip"}.get(name, f"{name}_zip")
    for label, x, y in _variants(name, xs, ys, rng):
        a_np, b_np = (y, x) if left else (x, y)
        ref = ref_fn(name, *np.broadcast_arrays(a_np, b_np))
        dx, dy = Dev.from_numpy(x), _operand(y, yhow)
        da, db = (dy, dx) if left else (dx, dy)
        out = _out_for(out_shape, ohow)
        _ok(_zip(FN[name], out, da, db), f"mt_tensor_zip {name} {layout}")
        got = out.numpy()
        _note_ulp(name, check_fn(name, got, ref, f"{layout}/{label}"))
        assert out.gaps_untouched(), f"{name} {layout}/{label}: wrote outside the output's elements"
        if ohow is None and hasattr(B, tname):
            ta, tb = da.tensor(minitorch, B), db.tensor(minitorch, B)
            assert _hip.fast is not None
            r_fast = getattr(B, tname)(ta, tb).to_numpy()
            saved, _hip.fast = _hip.fast, None
            try:
                r_ct = getattr(B, tname)(ta, tb).to_numpy()
            finally:
                _hip.fast = saved
            np.testing.assert_array_equal(_bits(r_fast), _bits(got), err_msg=f"{name} {layout}/{label}: fast")
            np.testing.assert_array_equal(_bits(r_ct), _bits(got), err_msg=f"{name} {layout}/{label}: ctypes")


@pytest.mark.parametrize("layout", list(MAP_LAYOUTS))
@pytest.mark.parametrize("name", MAP_NAMES)
def test_map_matrix(mt, name, layout):
    """Every one-argument function id on every mt_tensor_map dispatch path (map_dense_kernel's
    float4 body and scalar tail; map_kernel<int> for an input of lower rank or broadcast into
    the output, a permuted or misaligned input, a strided `out`, rank 8), as test_zip_matrix."""
    from minitorch import _hip
    minitorch, B = mt
    xs, ys, _, yhow, ohow = MAP_LAYOUTS[layout]
    rng = np.random.default_rng(2000 * FN[name] + list(MAP_LAYOUTS).index(layout))
    out_shape = np.broadcast_shapes(xs, ys)
    for label, y, _ in _variants(name, ys, None, rng):
        ref = np.broadcast_to(ref_fn(name, y), out_shape)
        dy = _operand(y, yhow)
        out = _out_for(out_shape, ohow)
        _ok(_map(FN[name], out, dy), f"mt_tensor_map {name} {layout}")
        got = out.numpy()
        _note_ulp(name, check_fn(name, got, ref, f"{layout}/{label}"))
        assert out.gaps_untouched(), f"{name} {layout}/{label}: wrote outside the output's elements"
        if ohow is None and tuple(out_shape) == tuple(ys):
            t = dy.tensor(minitorch, B)
            r_fast = getattr(B, f"{name}_map")(t).to_numpy()
            saved, _hip.fast = _hip.fast, None
            try:
                r_ct = getattr(B, f"{name}_map")(t).to_numpy()
            finally:
                _hip.fast = saved
            np.testing.assert_array_equal(_bits(r_fast), _bits(got), err_msg=f"{name} {layout}/{label}: fast")
            np.testing.assert_array_equal(_bits(r_ct), _bits(got), err_msg=f"{name} {layout}/{label}: ctypes")


def test_worst_ulp_record(mt, parity_record):
    """The worst error of each rounded function id over test_map_matrix / test_zip_matrix, in ulps
    of the fp32 result, beside the bound used (information for the parity record, not a gate:
    the gates are in check_fn)."""
    rng = np.random.default_rng(3)
    for name in sorted(set(ROUNDED) - set(_WORST_ULP)):  # run alone: the dense layout only
        x, y = finite_inputs(name, (6, 5, 8), (6, 5, 8), rng)
        out = Dev((6, 5, 8))
        if y is None:
            _ok(_map(FN[name], out, Dev.from_numpy(x)), name)
        else:
            _ok(_zip(FN[name], out, Dev.from_numpy(x), Dev.from_numpy(y)), name)
        _note_ulp(name, check_fn(name, out.numpy(), ref_fn(name, x, y), "same/finite"))
    for name in sorted(ROUNDED):
        rtol, atol, ulps = ROUNDED[name]
        bound = f"{ulps:g} ulp" if ulps else f"rtol {rtol:g}" + (f" atol {atol:g}" if atol else "")
        print(f"worst ulp {name}: {_WORST_ULP[name]:.3f} (bound {bound})")
        parity_record("test_generic_ops_gpu", f"fn_{name}", max_ulp=_WORST_ULP[name], bound=bound)


def test_empty_and_bad_rank(mt):
    """n == 0 returns 0 and writes nothing; rank 0 and rank 9 return nonzero with a message."""
    from minitorch import _hip
    lib = _hip.lib()
    a = Dev.from_numpy(np.ones((4,), np.float32))
    out = Dev((4,))
    s0, sh0 = _c64((4, 1)), _c64((0, 4))
    assert lib.mt_tensor_map(FN["neg"], out.ptr, sh0, s0, 2, a.ptr, sh0, s0, 2, _stream()) == 0
    assert lib.mt_tensor_zip(FN["add"], out.ptr, sh0, s0, 2, a.ptr, sh0, s0, 2, a.ptr, sh0, s0, 2, _stream()) == 0
    assert lib.mt_tensor_reduce(FN["add"], out.ptr, sh0, s0, a.ptr, sh0, s0, 2, 1, ctypes.c_float(0.0),
                                _stream()) == 0
    assert bool((out.store == SENTINEL).all())
    nine = _c64((1,) * 9)
    one = _c64((4,))
    for rank, shp in ((0, one), (9, nine)):
        st = lib.mt_tensor_map(FN["id"], out.ptr, shp, shp, rank, a.ptr, one, _c64((1,)), 1, _stream())
        assert st != 0 and b"rank" in lib.mt_last_error()
        st = lib.mt_tensor_zip(FN["add"], out.ptr, one, _c64((1,)), 1, a.ptr, shp, shp, rank, a.ptr, one,
                               _c64((1,)), 1, _stream())
        assert st != 0 and b"rank" in lib.mt_last_error()
        st = lib.mt_tensor_reduce(FN["add"], out.ptr, shp, shp, a.ptr, shp, shp, rank, 0, ctypes.c_float(0.0),
                                  _stream())
        assert st != 0 and b"rank" in lib.mt_last_error()
    assert bool((out.store == SENTINEL).all())


def test_int64_index_forms(mt):
    """map_kernel<int64_t> / zip_kernel<int64_t>: an operand of shape (2, 5) whose row stride is
    2^31 elements (a view of an 8 GiB buffer of which ten elements are set), map id and zip add,
    compared on the device."""
    import torch
    from minitorch import _hip
    lib = _hip.lib()
    row = 1 << 31
    try:
        big = torch.empty(row + 8, dtype=torch.float32, device="cuda")
    except torch.OutOfMemoryError:
        pytest.skip("no room for the 8 GiB buffer")
    try:
        vals = torch.arange(1, 11, dtype=torch.float32, device="cuda").view(2, 5) * 1.5
        big[0:5] = vals[0]
        big[row:row + 5] = vals[1]
        other = torch.arange(10, dtype=torch.float32, device="cuda").view(2, 5) - 3.0
        shp, sbig, sc = _c64((2, 5)), _c64((row, 1)), _c64((5, 1))
        out = torch.full((2, 5), SENTINEL, device="cuda")
        _ok(lib.mt_tensor_map(FN["id"], out.data_ptr(), shp, sc, 2, big.data_ptr(), shp, sbig, 2, _stream()),
            "map id")
        assert torch.equal(out, vals)
        for a, sa, b, sb in ((big, sbig, other, sc), (other, sc, big, sbig)):
            out.fill_(SENTINEL)
            _ok(lib.mt_tensor_zip(FN["add"], out.data_ptr(), shp, sc, 2, a.data_ptr(), shp, sa, 2, b.data_ptr(),
                                  shp, sb, 2, _stream()), "zip add")
            assert torch.equal(out, vals + other)
        torch.cuda.synchronize()
    finally:
        del big
        torch.cuda.empty_cache()


# ---- Part B: reduce -----------------------------------------------------------------------------
# (shape of a, reduced dim, layout: None | "misaligned" | "permuted" | "out_stride2"); the shapes
# follow mt_tensor_reduce's dispatch conditions, the kernel each selects is named on the right
REDUCE_CASES = [
    ((5, 128), 0, None),          # reduce_colgroup_kernel: T = 5, non-power-of-two LDS tree
    ((1025, 128), 0, None),       #   T = 1024, lane 0 holds two rows
    ((8192, 128), 0, None),       #   the upper len bound
    ((3, 7, 256), 1, None),       #   64 column groups: XCD map, outer 3
    ((40, 260), 0, None),         #   65 groups: padding workgroups
    ((100, 64), 0, None),         # reduce_cols1_kernel: R = 1
    ((300, 68), 0, None),         #   R = 4, 17 live lanes, arrival counters
    ((8200, 128), 0, None),       #   R = 127, 16 partials per wave
    ((2, 8200, 64), 1, None),     #   outer 2
    ((16, 17), 0, None),          # reduce_cols_kernel: R = 1
    ((200, 17), 0, None),         #   R = 2 (+ reduce_cols_fold)
    ((2, 200, 18), 1, None),      #   outer 2
    ((2048, 17), 0, None),        #   R = 16 = kColRMax
    ((64, 128), 0, "misaligned"),  #  rerouted here from the column-group kernel
    ((3, 2048), 1, None),         # reduce_block_kernel
    ((2, 8197), 1, None),         #   8 x 1024 loop tail
    ((3, 2048), 1, "permuted"),   #   (2048, 3) storage: stride 3 along the axis
    ((7, 64), 1, None),           # reduce_wave_kernel
    ((7, 65), 1, None),
    ((600, 100), 1, None),
    ((513, 2048), 1, None),
    ((100, 8), 0, None),          #   stride 8 along the axis
    ((17, 33), 1, None),          # reduce_thread_kernel
    ((9, 63), 1, None),
    ((40, 8), 0, None),
    ((5, 1, 128), 1, None),       #   len = 1
    ((1,), 0, None),
    ((17, 33), 1, "out_stride2"),  #  strided out
]
REDUCE_IDS = ["x".join(map(str, s)) + f"-d{d}" + (f"-{v}" if v else "") for s, d, v in REDUCE_CASES]
# fn -> [(start, what the result must be)]
STARTS = {"add": [0.0, 2.5], "mul": [1.0, 0.5], "max": [-1e9, -100.0, 100.0]}


def _from_rows(rows, shape, dim):
    """[n_out, len] rows (n_out in the output's C order) as a tensor of `shape` reduced over dim."""
    rest = tuple(s for i, s in enumerate(shape) if i != dim)
    return np.ascontiguousarray(np.moveaxis(rows.reshape(rest + (shape[dim],)), -1, dim))


@pytest.mark.parametrize("fn", ["add", "mul", "max"])
@pytest.mark.parametrize("case", REDUCE_CASES, ids=REDUCE_IDS)
def test_reduce_matrix(mt, case, fn):
    """mt_tensor_reduce on the smallest shapes that select each of its kernels, for add, mul and
    max with the identity `start` the backend passes (0, 1, -1e9) and a non-identity one (2.5,
    0.5; for max one below and one above every element: the latter must come back as `start`),
    against the float64 fold of the fp32 inputs followed by fn(start, .):

      add: |err| <= len 2^-24 (sum|x| + |start|): the any-order bound of len additions over the
           len inputs and `start` (with the identity start it is len 2^-24 sum|x|; `start` is one
           more term of the same sum, so it enters the bound as the inputs do);
      mul: relative error <= 2 len 2^-24 (len roundings plus the one for `start`), inputs uniform
           in [0.9, 1.1] so that a product of 8200 stays far inside the fp32 range;
      max: exact.

    A second launch is bitwise equal (fixed fold order; the one-pass kernel's counters reset).
    Non-finite inputs: a column holding +inf sums to +inf, one holding +inf and -inf to NaN, a mul
    column holding 0 and inf gives NaN, a max column of all -inf gives `start` (-1e9), one holding
    +inf gives +inf. (NaN in a max reduction is unspecified: include/minitorch_hip.h.)"""
    shape, dim, how = case
    ln = shape[dim]
    n_out = int(np.prod(shape)) // ln
    rng = np.random.default_rng(sum(shape) * 31 + dim + FN[fn])
    rows = (rng.uniform(0.9, 1.1, size=(n_out, ln)) if fn == "mul" else rng.standard_normal((n_out, ln)))
    rows = rows.astype(np.float32)
    out_shape = tuple(1 if i == dim else s for i, s in enumerate(shape))

    def run(rows_, start):
        x = _from_rows(rows_, shape, dim)
        if how == "permuted":
            a = _operand(x, "permuted")
        else:
            a = Dev.from_numpy(x, offset=1 if how == "misaligned" else 0)
        res = []
        for _ in range(2):
            out = Dev(out_shape, tuple(2 for _ in out_shape) if how == "out_stride2" else None)
            _ok(_reduce(FN[fn], out, a, dim, start), f"mt_tensor_reduce {fn} {case}")
            assert out.gaps_untouched()
            res.append(out.numpy().reshape(n_out))
        np.testing.assert_array_equal(_bits(res[0]), _bits(res[1]), err_msg="a second launch differs")
        return res[0]

    r64 = rows.astype(np.float64)
    for start in STARTS[fn]:
        got = run(rows, start)
        s32 = float(np.float32(start))
        if fn == "add":
            ref = r64.sum(1) + s32
            bound = ln * U * (np.abs(r64).sum(1) + abs(s32))
            assert np.all(np.abs(got - ref) <= bound), (start, float(np.max(np.abs(got - ref) / bound)))
        elif fn == "mul":
            ref = r64.prod(1) * s32
            assert np.all(np.abs(got - ref) <= 2 * ln * U * np.abs(ref)), (start, got, ref)
        else:
            ref = np.maximum(rows.max(1), np.float32(start))
            np.testing.assert_array_equal(got, ref, err_msg=f"start {start}")
            if start == 100.0:
                np.testing.assert_array_equal(got, np.full(n_out, 100.0, np.float32))

    # non-finite inputs, in the first and the last output element's columns
    o1, o2 = 0, n_out - 1
    bad = rows.copy()
    with np.errstate(all="ignore"):
        if fn == "add":
            bad[o1, ln // 2] = np.inf
            if ln >= 2 and o2 != o1:
                bad[o2, 0], bad[o2, ln - 1] = np.inf, -np.inf
            got = run(bad, 0.0)
            assert got[o1] == np.inf
            if ln >= 2 and o2 != o1:
                assert np.isnan(got[o2])
        elif fn == "mul":
            if ln >= 2:
                bad[o1, 0], bad[o1, ln - 1] = 0.0, np.inf
            else:
                bad[o1, 0] = np.inf
            got = run(bad, 1.0)
            assert np.isnan(got[o1]) if ln >= 2 else got[o1] == np.inf
        else:
            bad[o1, :] = -np.inf
            if o2 != o1:
                bad[o2, ln // 2] = np.inf
            got = run(bad, -1e9)
            assert got[o1] == np.float32(-1e9)
            if o2 != o1:
                assert got[o2] == np.inf
        # every other output element is as before
        keep = np.ones(n_out, bool)
        keep[[o1, o2]] = False
        if keep.any():
            clean = run(rows, STARTS[fn][0])
            np.testing.assert_array_equal(_bits(got[keep]), _bits(clean[keep]))


def test_tensor_level_reductions(mt):
    """Tensor.all (mul_reduce), mean, var, and max over a permuted tensor, against NumPy."""
    minitorch, B = mt
    rng = np.random.default_rng(11)
    x = rng.standard_normal((6, 40, 72)).astype(np.float32)
    t = minitorch.tensor_from_numpy(x, B)
    ones = (x > -100.0).astype(np.float32)
    assert minitorch.tensor_from_numpy(ones, B).all().to_numpy().item() == 1.0
    ones[3, 17, 5] = 0.0
    o = minitorch.tensor_from_numpy(ones, B)
    assert o.all().to_numpy().item() == 0.0
    for dim in range(3):
        np.testing.assert_array_equal(o.all(dim).to_numpy(), ones.prod(dim, keepdims=True))
        x64 = x.astype(np.float64)
        np.testing.assert_allclose(t.mean(dim).to_numpy(), x64.mean(dim, keepdims=True), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(t.var(dim).to_numpy(), x64.var(dim, keepdims=True), rtol=1e-5, atol=1e-6)
    p, xp = t.permute(2, 0, 1), x.transpose(2, 0, 1)
    for dim in range(3):
        np.testing.assert_array_equal(minitorch.max(p, dim).to_numpy(), xp.max(dim, keepdims=True))
        np.testing.assert_allclose(p.sum(dim).to_numpy(), xp.astype(np.float64).sum(dim, keepdims=True),
                                   rtol=1e-5, atol=1e-5)
    q = minitorch.tensor_from_numpy(rng.standard_normal((40, 33)).astype(np.float32), B)
    np.testing.assert_allclose(q.permute(1, 0).sum(1).to_numpy(),
                               q.to_numpy().astype(np.float64).T.sum(1, keepdims=True), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dim", [0, 1, 2])
def test_softmax_family(mt, dim):
    """nn.softmax, nn.logsoftmax and nn.logsumexp over each dim of a (3, 40, 72) tensor against
    torch float64 at rtol = atol = 1e-5."""
    import torch
    minitorch, B = mt
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((3, 40, 72)) * 3).astype(np.float32)
    t = minitorch.tensor_from_numpy(x, B)
    xt = torch.from_numpy(x).double()
    np.testing.assert_allclose(minitorch.softmax(t, dim).to_numpy(), torch.softmax(xt, dim).numpy(),
                               rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(minitorch.logsoftmax(t, dim).to_numpy(), torch.log_softmax(xt, dim).numpy(),
                               rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(minitorch.logsumexp(t, dim).to_numpy(),
                               torch.logsumexp(xt, dim, keepdim=True).numpy(), rtol=1e-5, atol=1e-5)


# ---- Part C: every tensor Function, forward and backward, against torch float64 autograd -------
def _away(rng, shape, lo, signed=True):
    """N(0, 1) pushed away from zero: |x| >= lo."""
    v = rng.standard_normal(shape)
    v = np.where(v >= 0, v + lo, v - lo)
    return (v if signed else np.abs(v)).astype(np.float32)


def _mt_fn(minitorch):
    from minitorch import tensor_functions as TF
    return TF


# name -> (minitorch f, torch f, domain: "any" | "pos" (>= 0.1) | "kink" (|x| >= 0.05))
UNARY = {
    "neg": (lambda m, a: -a, lambda a: -a, "any"),
    "inv": (lambda m, a: _mt_fn(m).Inv.apply(a), lambda a: 1.0 / a, "pos"),
    "c_over_a": (lambda m, a: 2.5 / a, lambda a: 2.5 / a, "pos"),
    "pow0": (lambda m, a: a ** 0.0, lambda a: a ** 0.0, "kink"),
    "pow1": (lambda m, a: a ** 1.0, lambda a: a ** 1.0, "kink"),
    "pow2": (lambda m, a: a ** 2.0, lambda a: a ** 2.0, "kink"),
    "pow3": (lambda m, a: a ** 3.0, lambda a: a ** 3.0, "kink"),
    "pow_half": (lambda m, a: a ** 0.5, lambda a: a ** 0.5, "pos"),
    "tanh": (lambda m, a: a.tanh(), lambda a: a.tanh(), "any"),
    "sigmoid": (lambda m, a: a.sigmoid(), lambda a: a.sigmoid(), "any"),
    "relu": (lambda m, a: a.relu(), lambda a: a.relu(), "kink"),
    "log": (lambda m, a: a.log(), lambda a: (a + 1e-6).log(), "pos"),
    "exp": (lambda m, a: a.exp(), lambda a: a.exp(), "any"),
    "sum0": (lambda m, a: a.sum(0), lambda a: a.sum(0, keepdim=True), "any"),
    "sum1": (lambda m, a: a.sum(1), lambda a: a.sum(1, keepdim=True), "any"),
    "sum2": (lambda m, a: a.sum(2), lambda a: a.sum(2, keepdim=True), "any"),
    "sum_all": (lambda m, a: a.sum(), lambda a: a.sum().view(1), "any"),
    "max0": (lambda m, a: m.max(a, 0), lambda a: a.max(0, keepdim=True).values, "any"),
    "max1": (lambda m, a: m.max(a, 1), lambda a: a.max(1, keepdim=True).values, "any"),
    "max2": (lambda m, a: m.max(a, 2), lambda a: a.max(2, keepdim=True).values, "any"),
    "permute": (lambda m, a: a.permute(2, 0, 1), lambda a: a.permute(2, 0, 1), "any"),
    "view": (lambda m, a: a.contiguous().view(30, 8), lambda a: a.reshape(30, 8), "any"),
    "copy": (lambda m, a: _mt_fn(m).Copy.apply(a), lambda a: a.clone(), "any"),
}
BINARY = {
    "add": (lambda a, b: a + b, lambda a, b: a + b, "any"),
    "mul": (lambda a, b: a * b, lambda a, b: a * b, "any"),
    "sub": (lambda a, b: a - b, lambda a, b: a - b, "any"),
    "div": (lambda a, b: a / b, lambda a, b: a / b, "pos"),
    "lt": (lambda a, b: a < b, lambda a, b: (a < b).double(), "grid"),
    "eq": (lambda a, b: a == b, lambda a, b: (a == b).double(), "grid"),
}
# (shape of a, shape of b, which operand is a permuted view: None | 0 | 1)
PAIRS = {"same": ((6, 5, 8), (6, 5, 8), None), "row": ((6, 5, 8), (8,), None),
         "col": ((6, 5, 8), (5, 1), None), "scalar_left": ((1,), (6, 5, 8), None),
         "permuted_a": ((6, 5, 8), (6, 5, 8), 0), "permuted_b": ((6, 5, 8), (5, 8), 1)}


def _draw(rng, shape, domain):
    if domain == "pos":  # >= 0.1, and no closer: 1 / x^2 in the gradients stays below 16
        return rng.uniform(0.25, 2.5, size=shape).astype(np.float32)
    if domain == "kink":
        return _away(rng, shape, 0.05)
    if domain == "grid":
        return rng.integers(-2, 3, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _leaf_pair(minitorch, B, x, permuted):
    """The minitorch and torch (float64) leaves holding x, and the operands made of them: the
    leaves themselves, or (permuted) views with reversed dims of leaves stored in reversed order."""
    import torch
    if not permuted:
        lm = minitorch.tensor_from_numpy(x, B, requires_grad=True)
        lt = torch.from_numpy(x).double().requires_grad_(True)
        return lm, lt, lm, lt
    rev = tuple(reversed(range(x.ndim)))
    xs = np.ascontiguousarray(x.transpose(rev))
    lm = minitorch.tensor_from_numpy(xs, B, requires_grad=True)
    lt = torch.from_numpy(xs).double().requires_grad_(True)
    return lm, lt, lm.permute(*rev), lt.permute(*rev)


def _fwd_bwd(minitorch, B, f_mt, f_t, arrays, permuted, rng):
    import torch
    leaves = [_leaf_pair(minitorch, B, x, p) for x, p in zip(arrays, permuted)]
    y = f_mt(*[l[2] for l in leaves])
    yt = f_t(*[l[3] for l in leaves])
    assert tuple(y.shape) == tuple(yt.shape), (y.shape, yt.shape)
    g = rng.standard_normal(tuple(yt.shape)).astype(np.float32)
    (y * minitorch.tensor_from_numpy(g, B)).sum().backward()
    np.testing.assert_allclose(y.to_numpy(), yt.detach().numpy(), rtol=1e-5, atol=1e-5, err_msg="forward")
    loss = (yt * torch.from_numpy(g).double()).sum()
    if loss.requires_grad:
        loss.backward()
    for i, (lm, lt, _, _) in enumerate(leaves):
        want = lt.grad.numpy() if lt.grad is not None else np.zeros(tuple(lt.shape))
        assert lm.grad is not None, f"operand {i} got no gradient"
        np.testing.assert_allclose(lm.grad.to_numpy(), want, rtol=1e-5, atol=1e-5, err_msg=f"grad of operand {i}")


@pytest.mark.parametrize("permuted", [False, True], ids=["dense", "permuted"])
@pytest.mark.parametrize("name", list(UNARY))
def test_unary_function_grad(mt, name, permuted):
    """y = f(a) and d((y * g).sum())/da for every one-argument tensor Function (and the scalar
    compositions c / a, a ** e) on the HIP backend against torch float64 autograd on the same
    fp32 inputs, rtol = atol = 1e-5 (sums of at most 72 terms), on a dense and on a permuted a;
    inputs kept away from the kinks (|x| >= 0.05 for ReLU and the integer powers, arguments
    >= 0.1 for Log, Inv and the square root; maxima unique)."""
    minitorch, B = mt
    f_mt, f_t, dom = UNARY[name]
    rng = np.random.default_rng(list(UNARY).index(name) * 2 + int(permuted) + 5000)
    x = _draw(rng, (6, 5, 8), dom)
    _fwd_bwd(minitorch, B, lambda a: f_mt(minitorch, a), f_t, [x], [permuted], rng)


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("name", list(BINARY))
def test_binary_function_grad(mt, name, pair):
    """y = f(a, b) and both gradients for Add, Mul, a - b, a / b, LT and EQ (zero gradients) on the
    same shape, the broadcast pairs (6,5,8)·(8,), (6,5,8)·(5,1), (1,)·(6,5,8) (the backward's
    `expand` sums run over leading and middle dims) and a permuted operand on either side, against
    torch float64 autograd, rtol = atol = 1e-5."""
    minitorch, B = mt
    f_mt, f_t, dom = BINARY[name]
    sa, sb, perm = PAIRS[pair]
    rng = np.random.default_rng(list(BINARY).index(name) * 16 + list(PAIRS).index(pair) + 7000)
    a = _draw(rng, sa, "any" if dom == "pos" else dom)
    b = _draw(rng, sb, dom)
    _fwd_bwd(minitorch, B, f_mt, f_t, [a, b], [perm == 0, perm == 1], rng)


def test_max_tie_gradient(mt):
    """Max.backward with ties, against the reference formula eq(out, input) * grad: every tied
    element receives the full gradient."""
    minitorch, B = mt
    x = np.array([[1.0, 3.0, 3.0, -2.0], [2.0, 2.0, 0.0, 2.0], [5.0, 1.0, 1.0, 1.0]], np.float32)
    g = np.array([[0.5], [-1.5], [2.0]], np.float32)
    a = minitorch.tensor_from_numpy(x, B, requires_grad=True)
    y = minitorch.max(a, 1)
    (y * minitorch.tensor_from_numpy(g, B)).sum().backward()
    np.testing.assert_array_equal(y.to_numpy(), x.max(1, keepdims=True))
    np.testing.assert_array_equal(a.grad.to_numpy(), (x == x.max(1, keepdims=True)).astype(np.float32) * g)


# ---- Part D: non-finite operands of the GEMMs ---------------------------------------------------
def _matmul_abi(a, b):
    """c[b] = a[b] @ b[b] through mt_matmul_f32 on contiguous [batch, M, K] x [batch, K, N]."""
    import torch
    from minitorch import _hip
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    batch, M, K = a.shape
    N = b.shape[2]
    c = torch.full((batch, M, N), SENTINEL, device="cuda")
    _ok(_hip.lib().mt_matmul_f32(c.data_ptr(), ta.data_ptr(), tb.data_ptr(), batch, M, N, K, _c64((M * K, K, 1)),
                                 _c64((K * N, N, 1)), _c64((M * N, N, 1)), _stream()), "mt_matmul_f32")
    torch.cuda.synchronize()
    return c.cpu().numpy()


@pytest.mark.parametrize("variant", ["finite", "a_pinf", "b_ninf"])
@pytest.mark.parametrize("shape", [(1, 70, 40, 70), (256, 16, 16, 16)], ids=["70x40x70", "256x16x16x16"])
@pytest.mark.parametrize("gemm_backend", [0, 1, 2, 3])
def test_matmul_nonfinite(mt, gemm_backend, shape, variant):
    """mt_matmul_f32 with one infinite operand on every GEMM backend: (70, 40) x (40, 70)
    (backends 2 and 3: gemm_x3_kernel) and a batch of 256 (16, 16) x (16, 16) (backend 2:
    gemm_x3_big on 256 tiles), finite, with one +inf in A (the matching row of B all positive, and
    holding 1.0 and 0.5, whose middle and low bf16 pieces are zero) and with one -inf in B. Against
    NumPy float64 matmul: the NaN / +inf / -inf masks are equal, the finite entries meet
    test_matmul's bound, and the rows (columns) the infinite entry does not touch are bitwise
    equal to the finite run on the same backend."""
    from minitorch import _hip
    batch, M, K, N = shape
    rng = np.random.default_rng(batch + M)
    a = rng.standard_normal((batch, M, K)).astype(np.float32)
    b = rng.standard_normal((batch, K, N)).astype(np.float32)
    b0, i0, k0, j0 = batch // 2, M // 3, K // 2, N - 2
    b[b0, k0, :] = np.abs(b[b0, k0, :]) + 0.5
    b[b0, k0, 0], b[b0, k0, 1] = 1.0, 0.5
    a2, b2 = a.copy(), b.copy()
    if variant == "a_pinf":
        a2[b0, i0, k0] = np.inf
    if variant == "b_ninf":
        b2[b0, k0, j0] = -np.inf
    _hip.lib().mt_set_gemm_backend(gemm_backend)
    try:
        base = _matmul_abi(a, b)
        got = _matmul_abi(a2, b2) if variant != "finite" else base
    finally:
        _hip.lib().mt_set_gemm_backend(0)
    with np.errstate(all="ignore"):
        ref = np.matmul(a2.astype(np.float64), b2.astype(np.float64))
    for cls, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        np.testing.assert_array_equal(f(got), f(ref), err_msg=f"{cls} mask")
    fin = np.isfinite(ref)
    tol = 1e-5 * max(1.0, K / 32)  # test_matmul's bound
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-5, atol=tol)
    touched = np.zeros(ref.shape, bool)
    if variant == "a_pinf":
        touched[b0, i0, :] = True
        assert np.all(np.isinf(got[b0, i0, :]))
    if variant == "b_ninf":
        touched[b0, :, j0] = True
        assert np.all(np.isinf(got[b0, :, j0]))
    np.testing.assert_array_equal(_bits(got[~touched]), _bits(base[~touched]))
