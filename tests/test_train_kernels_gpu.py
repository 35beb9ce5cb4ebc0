"""The training-step helper kernels through the C ABI, against tests/train_kernels_ref.py, at every
dispatch path, edge and write footprint:

    mt_rand_uniform, mt_dropout, mt_dropout_dseed     bit-equal to the rng.h formula
    mt_bias_gelu_fw / _bw                             float64 tanh GELU, vector / scalar / second trip
    mt_embedding_fw / _bw                             bit-equal forward, summation bound backward
    mt_adam_step / _dstep                             the float32 tensor-op restatement
    mt_softmax_xent_fw / _bw                          float64, register / online / scalar, -inf logits

Every output is a view between guard bands (tests/train_kernels_ref.py place_flat: NaN inside,
a sentinel outside); after each call nothing outside the view was written, no NaN is left inside,
and the inputs hold the bits they held. A misaligned case starts every view one float past a
16-byte boundary. The case tables and the source branch each case reaches are in
tests/train_kernels_ref.py.

Tolerances are the project's existing ones for the same kernels (tests/test_minitorch_gpu.py
test_bias_gelu_fused, tests/test_optim_gpu.py, tests/test_xent_gpu.py); the embedding backward is
held to the recursive-summation bound of its reference; everything drawn from the RNG is bit-exact.
"""
import ctypes
import zlib

import numpy as np
import pytest

import train_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    return torch, _hip, _hip.lib()


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np(v):
    return v.detach().cpu().numpy()


def _out(n, mis=False):
    p, (v,) = R.place_flat([n], DEV, True, None, mis)
    return p, v


def _in(x, mis=False):
    p, (v,) = R.place_flat([np.asarray(x).size], DEV, False, [x], mis)
    return p, v, p.bits()


def _clean(torch, outs, ins):
    """outs: (name, parent, view); ins: (name, parent, view, bits before)."""
    torch.cuda.synchronize()
    fails = R.footprint([(n, p, [v]) for n, p, v in outs], [(n, p, b) for n, p, _, b in ins])
    assert fails == [], fails


def _is_error(L, status, name):
    assert status != 0
    assert name.encode() in L.mt_last_error()


# ---- mt_rand_uniform ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.RAND_SEEDS)
@pytest.mark.parametrize("n", R.RAND_N)
def test_rand_uniform_is_the_documented_hash(hip, n, seed):
    torch, _hip, L = hip
    p, v = _out(n)
    _hip.check(L.mt_rand_uniform(v.data_ptr(), n, seed, _hip.stream_ptr()), "mt_rand_uniform")
    _clean(torch, [("out", p, v)], [])
    np.testing.assert_array_equal(_bits(_np(v)), _bits(R.uniform24_ref(seed, np.arange(n))))


@pytest.mark.parametrize("n", [257, 2_097_152 + 257])
def test_rand_uniform_misaligned(hip, n):
    torch, _hip, L = hip
    p, v = _out(n, mis=True)
    _hip.check(L.mt_rand_uniform(v.data_ptr(), n, 2 ** 63 + 11, _hip.stream_ptr()), "mt_rand_uniform")
    _clean(torch, [("out", p, v)], [])
    np.testing.assert_array_equal(_bits(_np(v)), _bits(R.uniform24_ref(2 ** 63 + 11, np.arange(n))))


def test_rand_uniform_empty_and_negative(hip):
    torch, _hip, L = hip
    p, v = _out(0)
    where = p.flat.data_ptr() + 4 * R.GUARD
    assert L.mt_rand_uniform(where, 0, 3, _hip.stream_ptr()) == 0
    _is_error(L, L.mt_rand_uniform(where, -1, 3, _hip.stream_ptr()), "mt_rand_uniform")
    _clean(torch, [("out", p, v)], [])


# ---- mt_dropout / mt_dropout_dseed -------------------------------------------------------------
def _dropout_case(n, prob):
    """(x, scale, seed); at p = 0 the seed is one whose first n draws hold an exact 0."""
    rng = _rng("dropout", n, prob)
    x = (rng.standard_normal(n) + 3).astype(np.float32)
    x[x == 0] = 1.0  # a kept element is never 0
    scale = 1.0 / (1.0 - prob) if prob < 1 else 1.0
    seed = R.DROPOUT_ZERO[n][0] if prob == 0.0 else int(rng.integers(0, 2 ** 63)) * 2 + 1
    return x, scale, seed


@pytest.mark.parametrize("prob", R.DROPOUT_P, ids=["p0", "p0.1", "p0.5", "p1-2^-24"])
@pytest.mark.parametrize("n", R.DROPOUT_N)
def test_dropout_is_the_documented_mask(hip, n, prob):
    torch, _hip, L = hip
    x, scale, seed = _dropout_case(n, prob)
    px, vx, bx = _in(x)
    p, v = _out(n)
    _hip.check(L.mt_dropout(v.data_ptr(), vx.data_ptr(), n, prob, scale, seed, _hip.stream_ptr()), "mt_dropout")
    _clean(torch, [("out", p, v)], [("x", px, vx, bx)])
    got = _np(v)
    np.testing.assert_array_equal(_bits(got), _bits(R.dropout_ref(x, prob, scale, seed)))
    u = R.uniform24_ref(seed, np.arange(n))
    if prob == 0.0:  # exactly the draws that are 0 are dropped: u > p is strict
        assert (u == 0).any()
        np.testing.assert_array_equal(np.flatnonzero(got == 0), np.flatnonzero(u == 0))
    if prob == R.DROPOUT_P[-1]:  # the largest draw is 1 - 2^-24: nothing is kept
        assert not _bits(got).any()


def test_dropout_dseed(hip):
    torch, _hip, L = hip
    n, prob = 1_048_576 + 3, 0.1
    x, scale, _ = _dropout_case(n, prob)
    seed = 2 ** 64 - 12345  # above 2^63: the whole 64-bit word is read
    px, vx, bx = _in(x)
    sd = torch.tensor([seed - 2 ** 64], dtype=torch.int64, device=DEV)
    p, v = _out(n)
    _hip.check(L.mt_dropout_dseed(v.data_ptr(), vx.data_ptr(), n, prob, scale, sd.data_ptr(), _hip.stream_ptr()),
               "mt_dropout_dseed")
    _clean(torch, [("out", p, v)], [("x", px, vx, bx)])
    p2, v2 = _out(n)
    _hip.check(L.mt_dropout(v2.data_ptr(), vx.data_ptr(), n, prob, scale, seed, _hip.stream_ptr()), "mt_dropout")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(_np(v)), _bits(_np(v2)))
    np.testing.assert_array_equal(_bits(_np(v)), _bits(R.dropout_ref(x, prob, scale, seed)))
    assert int(sd.item()) == seed - 2 ** 64
    # a NULL seed pointer is refused before any launch; n = 0 writes nothing; n < 0 is an error
    p3, v3 = _out(n)
    _is_error(L, L.mt_dropout_dseed(v3.data_ptr(), vx.data_ptr(), n, prob, scale, None, _hip.stream_ptr()),
              "mt_dropout_dseed")
    assert L.mt_dropout(v3.data_ptr(), vx.data_ptr(), 0, prob, scale, seed, _hip.stream_ptr()) == 0
    _is_error(L, L.mt_dropout(v3.data_ptr(), vx.data_ptr(), -1, prob, scale, seed, _hip.stream_ptr()), "mt_dropout")
    torch.cuda.synchronize()
    assert bool(torch.isnan(v3).all()) and R.footprint([("out", p3, [])]) == []


# ---- mt_bias_gelu_fw / _bw ---------------------------------------------------------------------
GELU_FW_TOL = dict(rtol=1e-5, atol=1e-5)   # tests/test_minitorch_gpu.py test_bias_gelu_fused
GELU_BW_TOL = dict(rtol=1e-4, atol=1e-5)


def _gelu_run(hip, x, b, dy, mis=()):
    """Forward and backward with the tensors named in `mis` one float off 16 bytes; returns
    (y, dx) after the footprint checks."""
    torch, _hip, L = hip
    rows, cols = x.shape
    px, vx, bx = _in(x, "x" in mis)
    pb, vb, bb = _in(b, "bias" in mis)
    pd, vd, bd = _in(dy, "dy" in mis)
    po, vo = _out(x.size, "out" in mis)
    _hip.check(L.mt_bias_gelu_fw(vo.data_ptr(), vx.data_ptr(), vb.data_ptr(), rows, cols, _hip.stream_ptr()),
               "mt_bias_gelu_fw")
    pg, vg = _out(x.size, "out" in mis)
    _hip.check(L.mt_bias_gelu_bw(vg.data_ptr(), vd.data_ptr(), vx.data_ptr(), vb.data_ptr(), rows, cols,
                                 _hip.stream_ptr()), "mt_bias_gelu_bw")
    _clean(torch, [("out", po, vo), ("dx", pg, vg)], [("x", px, vx, bx), ("bias", pb, vb, bb), ("dy", pd, vd, bd)])
    return _np(vo).reshape(rows, cols), _np(vg).reshape(rows, cols)


def _gelu_compare(parity_record, case, y, dx, x, b, dy):
    yr, dxr = R.bias_gelu_ref(x, b), R.bias_gelu_bw_ref(dy, x, b)
    efw, ebw = float(np.abs(y - yr).max()), float(np.abs(dx - dxr).max())
    print(f"bias_gelu {case}: max |err| forward {efw:.3g}, backward {ebw:.3g}")
    parity_record("test_train_kernels_gpu.bias_gelu", case, fw_max_abs=efw, bw_max_abs=ebw,
                  fw_atol=GELU_FW_TOL["atol"], bw_atol=GELU_BW_TOL["atol"])
    np.testing.assert_allclose(y, yr, **GELU_FW_TOL)
    np.testing.assert_allclose(dx, dxr, **GELU_BW_TOL)


@pytest.mark.parametrize("rows,cols", R.GELU_SHAPES)
def test_bias_gelu_paths(hip, parity_record, rows, cols):
    x, b, dy = R.gelu_inputs(rows, cols, _rng("gelu", rows, cols))
    y, dx = _gelu_run(hip, x, b, dy)
    _gelu_compare(parity_record, f"{rows}x{cols}", y, dx, x, b, dy)


@pytest.fixture(scope="module")
def gelu_aligned(hip):
    rows, cols = R.GELU_MISALIGNED
    x, b, dy = R.gelu_inputs(rows, cols, _rng("gelu", rows, cols))
    return (x, b, dy) + _gelu_run(hip, x, b, dy)


@pytest.mark.parametrize("which", ["out", "x", "dy", "bias"])
def test_bias_gelu_misaligned_pointer(hip, parity_record, gelu_aligned, which):
    """cols % 4 == 0 with one pointer off 16 bytes: the scalar loop, bit-equal to the vector
    loop's results on the same data (both apply the same per-element function)."""
    x, b, dy, y0, dx0 = gelu_aligned
    y, dx = _gelu_run(hip, x, b, dy, mis=(which,))
    _gelu_compare(parity_record, f"{x.shape[0]}x{x.shape[1]} {which} misaligned", y, dx, x, b, dy)
    np.testing.assert_array_equal(_bits(y), _bits(y0))
    np.testing.assert_array_equal(_bits(dx), _bits(dx0))


def test_bias_gelu_empty_and_bad_sizes(hip):
    torch, _hip, L = hip
    x, b, dy = R.gelu_inputs(4, 8, _rng("gelu-empty"))
    (px, vx, bx), (pb, vb, bb), (pd, vd, bd) = _in(x), _in(b), _in(dy)
    p, v = _out(32)
    s = _hip.stream_ptr()
    assert L.mt_bias_gelu_fw(v.data_ptr(), vx.data_ptr(), vb.data_ptr(), 0, 8, s) == 0
    assert L.mt_bias_gelu_bw(v.data_ptr(), vd.data_ptr(), vx.data_ptr(), vb.data_ptr(), 0, 8, s) == 0
    _is_error(L, L.mt_bias_gelu_fw(v.data_ptr(), vx.data_ptr(), vb.data_ptr(), 4, 0, s), "mt_bias_gelu_fw")
    _is_error(L, L.mt_bias_gelu_bw(v.data_ptr(), vd.data_ptr(), vx.data_ptr(), vb.data_ptr(), 4, 0, s), "mt_bias_gelu_bw")
    _is_error(L, L.mt_bias_gelu_fw(v.data_ptr(), vx.data_ptr(), vb.data_ptr(), -1, 8, s), "mt_bias_gelu_fw")
    torch.cuda.synchronize()
    assert bool(torch.isnan(v).all()) and R.footprint([("out", p, [])]) == []


# ---- mt_embedding_fw / _bw ---------------------------------------------------------------------
def _embed_run(hip, ids, W, dy, launches=1):
    """Forward, then `launches` backward launches into fresh buffers; footprint-checked."""
    torch, _hip, L = hip
    ntok, (V, E) = len(ids), W.shape
    (pi, vi, bi), (pw, vw, bw), (pd, vd, bd) = _in(ids), _in(W), _in(dy)
    s = _hip.stream_ptr()
    po, vo = _out(ntok * E)
    _hip.check(L.mt_embedding_fw(vo.data_ptr(), vi.data_ptr(), vw.data_ptr(), ntok, V, E, s), "mt_embedding_fw")
    outs, dws = [("out", po, vo)] if ntok else [], []
    for k in range(launches):
        pg, vg = _out(V * E)
        _hip.check(L.mt_embedding_bw(vg.data_ptr(), vd.data_ptr(), vi.data_ptr(), ntok, V, E, s), "mt_embedding_bw")
        outs.append((f"dW{k}", pg, vg))
        dws.append(vg)
    _clean(torch, outs, [("ids", pi, vi, bi), ("W", pw, vw, bw), ("dy", pd, vd, bd)])
    return (po, vo), [_np(g).reshape(V, E) for g in dws]


def _embed_check_bw(parity_record, case, dw, dy, ids, V):
    """dW against float64 within cnt 2^-24 sum |g| per element; exact where cnt <= 1; +0.0 rows
    for ids never seen."""
    ref, cnt, sabs = R.embed_bw_ref(dy, ids, V)
    few = cnt <= 1
    np.testing.assert_array_equal(_bits(dw[few]), _bits(ref[few].astype(np.float32)))
    assert not _bits(dw[cnt == 0]).any()
    bound = cnt[:, None] * 2.0 ** -24 * sabs
    err = np.abs(dw.astype(np.float64) - ref)
    frac = float((err[~few] / bound[~few]).max()) if (~few).any() and bound[~few].min() > 0 else 0.0
    print(f"embedding_bw {case}: worst error {frac:.3g} of its bound (largest count {int(cnt.max())})")
    parity_record("test_train_kernels_gpu.embedding_bw", case, max_frac_of_bound=frac, max_count=int(cnt.max()))
    assert (err <= bound).all(), f"worst error {frac:.3g} of the bound"


@pytest.mark.parametrize("V,E,ntok", R.EMBED_CASES)
def test_embedding_edges(hip, parity_record, V, E, ntok):
    rng = _rng("embed", V, E, ntok)
    ids, planted = R.embed_ids(V, ntok, rng)
    W = rng.standard_normal((V, E)).astype(np.float32)
    dy = rng.standard_normal((ntok, E)).astype(np.float32)
    (po, vo), dws = _embed_run(hip, ids, W, dy, launches=2)
    out = _np(vo).reshape(ntok, E)
    np.testing.assert_array_equal(_bits(out), _bits(R.embed_fw_ref(ids, W)))
    for pos, row in planted.items():  # stated here too, not only through the reference
        want = W[row] if row is not None else np.zeros(E, np.float32)
        np.testing.assert_array_equal(_bits(out[pos]), _bits(want), err_msg=f"id {ids[pos]}")
    _embed_check_bw(parity_record, f"V{V} E{E} ntok{ntok}", dws[0], dy, ids, V)
    np.testing.assert_array_equal(_bits(dws[0]), _bits(dws[1]))  # fixed order: deterministic


def test_embedding_bw_hot_id_every_chunk(hip, parity_record):
    """All 4097 tokens on one id: 128 matches in every wave of the two full chunks (four batches
    of 32 each), one match in the third chunk, and the four groups' fold."""
    V, E, ntok = 9, 257, 4097
    rng = _rng("embed-hot")
    ids = np.full(ntok, 5.0, dtype=np.float32)
    W = rng.standard_normal((V, E)).astype(np.float32)
    dy = rng.standard_normal((ntok, E)).astype(np.float32)
    _, dws = _embed_run(hip, ids, W, dy, launches=2)
    _embed_check_bw(parity_record, "one id x 4097", dws[0], dy, ids, V)
    np.testing.assert_array_equal(_bits(dws[0]), _bits(dws[1]))


def test_embedding_bw_41_hits_in_one_wave(hip, parity_record):
    """Id 3 exactly 41 times among wave 1's 128 tokens, whose other tokens name rows of the next
    vocabulary block or none: that wave's list for block 0 holds 41 entries, added as one batch
    of 32, one of 8 and a single."""
    V, E, ntok = 17, 33, 300
    rng = _rng("embed-41")
    ids = rng.integers(0, V, ntok).astype(np.float32)
    ids[128:256] = rng.choice([8.0, 9.0, 16.0, 17.0, -1.0], 128)
    hot = 128 + rng.choice(128, 41, replace=False)
    ids[hot] = 3.0
    valid, row = R.embed_rows(ids[128:256], V)
    assert int((valid & (row < 8)).sum()) == 41
    W = rng.standard_normal((V, E)).astype(np.float32)
    dy = rng.standard_normal((ntok, E)).astype(np.float32)
    _, dws = _embed_run(hip, ids, W, dy, launches=2)
    _embed_check_bw(parity_record, "41 hits in one wave", dws[0], dy, ids, V)
    np.testing.assert_array_equal(_bits(dws[0]), _bits(dws[1]))


def test_embedding_no_tokens(hip):
    """ntok = 0: the backward still writes every row of dW (zeros), the forward writes nothing."""
    torch, _hip, L = hip
    V, E = 9, 257
    W = _rng("embed-0").standard_normal((V, E)).astype(np.float32)
    (pw, vw, bw), (pi, vi, bi) = _in(W), _in(np.zeros(4, np.float32))
    s = _hip.stream_ptr()
    po, vo = _out(E)
    assert L.mt_embedding_fw(vo.data_ptr(), vi.data_ptr(), vw.data_ptr(), 0, V, E, s) == 0
    pg, vg = _out(V * E)
    _hip.check(L.mt_embedding_bw(vg.data_ptr(), vi.data_ptr(), vi.data_ptr(), 0, V, E, s), "mt_embedding_bw")
    _clean(torch, [("dW", pg, vg)], [("W", pw, vw, bw), ("ids", pi, vi, bi)])
    assert not _bits(_np(vg)).any()
    assert bool(torch.isnan(vo).all()) and R.footprint([("out", po, [])]) == []
    _is_error(L, L.mt_embedding_fw(vo.data_ptr(), vi.data_ptr(), vw.data_ptr(), 1, 0, E, s), "mt_embedding_fw")
    _is_error(L, L.mt_embedding_bw(vg.data_ptr(), vi.data_ptr(), vi.data_ptr(), -1, V, E, s), "mt_embedding_bw")


# ---- mt_adam_step / _dstep ---------------------------------------------------------------------
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _ptrs(views):
    return (ctypes.c_void_p * max(1, len(views)))(*[v.data_ptr() if v.numel() else None for v in views])


def _adam_run(hip, count, mis=False, dstep=False, steps=2):
    """`steps` Adam steps over the list of `count` tensors; returns the NumPy (p, m, v) lists of
    the kernel and of the reference, footprints checked after every step."""
    torch, _hip, L = hip
    sizes = R.adam_sizes(count, 12 if count == 25 else None)
    rng = _rng("adam", count)
    ps = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    ms = [np.zeros(n, np.float32) for n in sizes]
    vs = [np.zeros(n, np.float32) for n in sizes]
    pp, vp = R.place_flat(sizes, DEV, True, ps, mis)
    pm, vm = R.place_flat(sizes, DEV, True, ms, mis)
    pv, vv = R.place_flat(sizes, DEV, True, vs, mis)
    numels = (ctypes.c_int64 * count)(*sizes)
    for t in range(1, steps + 1):
        gs = [(rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2)).astype(np.float32) for n in sizes]
        pg, vg = R.place_flat(sizes, DEV, False, gs, mis)
        before = pg.bits()
        step = LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
        args = (count, _ptrs(vp), _ptrs(vg), _ptrs(vm), _ptrs(vv), numels, B1, B2, EPS)
        if dstep:
            sd = torch.tensor([step], dtype=torch.float32, device=DEV)
            _hip.check(L.mt_adam_step_dstep(*args, sd.data_ptr(), _hip.stream_ptr()), "mt_adam_step_dstep")
        else:
            _hip.check(L.mt_adam_step(*args, step, _hip.stream_ptr()), "mt_adam_step")
        torch.cuda.synchronize()
        fails = R.footprint([("p", pp, vp), ("m", pm, vm), ("v", pv, vv)], [("g", pg, before)])
        assert fails == [], fails
        for i in range(count):
            ps[i], ms[i], vs[i] = R.adam_ref(ps[i], gs[i], ms[i], vs[i], t, LR, B1, B2, EPS)
    return ([_np(x) for x in vp], [_np(x) for x in vm], [_np(x) for x in vv]), (ps, ms, vs)


def _adam_compare(got, ref):
    for (p, m, v), (pr, mr, vr) in zip(zip(*got), zip(*ref)):
        if not p.size:
            continue
        np.testing.assert_allclose(m, mr, rtol=1e-6, atol=0)   # tests/test_optim_gpu.py's tolerances
        np.testing.assert_allclose(v, vr, rtol=1e-6, atol=0)
        np.testing.assert_allclose(p, pr, rtol=0, atol=1e-7 * max(1.0, np.abs(pr).max()))


@pytest.mark.parametrize("count", R.ADAM_COUNTS)
def test_adam_launch_groups(hip, count):
    """24 / 25 / 48 / 49 tensors: one full launch, a launch of one tensor after it, two full
    ones, and three; the list of 25 has a zero-numel entry (NULL pointers) in the first group."""
    got, ref = _adam_run(hip, count)
    _adam_compare(got, ref)


@pytest.fixture(scope="module")
def adam_aligned(hip):
    return _adam_run(hip, 25)


def test_adam_misaligned_is_the_scalar_path(hip, adam_aligned):
    """Every P / G / M / V one float off 16 bytes: vec == false with n >= 4, bit-equal to the
    aligned run (the same adam_elem per element)."""
    got, ref = _adam_run(hip, 25, mis=True)
    _adam_compare(got, ref)
    for a, b in zip(got, adam_aligned[0]):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(_bits(x), _bits(y))


def test_adam_dstep_equals_host_step(hip, adam_aligned):
    got, ref = _adam_run(hip, 25, dstep=True)
    _adam_compare(got, ref)
    for a, b in zip(got, adam_aligned[0]):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(_bits(x), _bits(y))


def test_adam_bad_arguments(hip):
    torch, _hip, L = hip
    pp, vp = R.place_flat([5], DEV, True, [np.ones(5, np.float32)])
    one = _ptrs(vp)
    null = (ctypes.c_void_p * 1)(None)
    n5 = (ctypes.c_int64 * 1)(5)
    s = _hip.stream_ptr()
    assert L.mt_adam_step(0, one, one, one, one, n5, B1, B2, EPS, 1e-3, s) == 0
    _is_error(L, L.mt_adam_step(-1, one, one, one, one, n5, B1, B2, EPS, 1e-3, s), "mt_adam_step")
    for k in range(4):
        args = [one] * 4
        args[k] = null
        _is_error(L, L.mt_adam_step(1, *args, n5, B1, B2, EPS, 1e-3, s), "mt_adam_step")
    _is_error(L, L.mt_adam_step_dstep(1, one, one, one, one, n5, B1, B2, EPS, None, s), "mt_adam_step_dstep")
    torch.cuda.synchronize()
    assert R.footprint([("p", pp, vp)]) == [] and bool((vp[0] == 1).all())


# ---- mt_softmax_xent_fw / _bw ------------------------------------------------------------------
XENT_LOSS_TOL = dict(rtol=1e-5, atol=1e-4)  # tests/test_xent_gpu.py; lse is held to the same
XENT_DX_TOL = dict(rtol=1e-4, atol=1e-6)


def _xent_run(hip, x, t, g, mis_x=False, mis_dx=False):
    """Forward then backward (reading the forward's lse); returns (loss, lse, dx)."""
    torch, _hip, L = hip
    rows, C = x.shape
    (px, vx, bx), (pt, vt, bt), (pg, vg, bg) = _in(x, mis_x), _in(t), _in(g)
    s = _hip.stream_ptr()
    pl, (vloss, vlse) = R.place_flat([rows, rows], DEV, True)
    _hip.check(L.mt_softmax_xent_fw(vloss.data_ptr(), vlse.data_ptr(), vx.data_ptr(), vt.data_ptr(), rows, C, s),
               "mt_softmax_xent_fw")
    torch.cuda.synchronize()
    after_fw = pl.bits()
    pd, vd = _out(rows * C, mis_dx)
    _hip.check(L.mt_softmax_xent_bw(vd.data_ptr(), vg.data_ptr(), vx.data_ptr(), vt.data_ptr(), vlse.data_ptr(),
                                    rows, C, s), "mt_softmax_xent_bw")
    torch.cuda.synchronize()
    fails = R.footprint([("loss+lse", pl, [vloss, vlse]), ("dx", pd, [vd])],
                        [("x", px, bx), ("target", pt, bt), ("g", pg, bg), ("loss+lse (backward)", pl, after_fw)])
    assert fails == [], fails
    return _np(vloss), _np(vlse), _np(vd).reshape(rows, C)


def _xent_compare(parity_record, case, got, x, t, g):
    loss, lse, dx = got
    lser, lossr, dxr = R.xent_ref(x, t, g)
    el, ed = float(np.abs(loss - lossr).max()), float(np.abs(dx - dxr).max())
    print(f"softmax_xent {case}: max |err| loss {el:.3g}, lse {float(np.abs(lse - lser).max()):.3g}, dx {ed:.3g}")
    parity_record("test_train_kernels_gpu.softmax_xent", case, loss_max_abs=el, dx_max_abs=ed,
                  loss_atol=XENT_LOSS_TOL["atol"], dx_atol=XENT_DX_TOL["atol"])
    np.testing.assert_allclose(loss, lossr, **XENT_LOSS_TOL)
    np.testing.assert_allclose(lse, lser, **XENT_LOSS_TOL)
    np.testing.assert_allclose(dx, dxr, **XENT_DX_TOL)


def _xent_inputs(rows, C, rng):
    x = (rng.standard_normal((rows, C)) * 3).astype(np.float32)
    x[0, :] += 60.0                # a row far from zero
    x[-1, min(1, C - 1)] = 80.0    # a spike
    return x, rng.standard_normal(rows).astype(np.float32)


@pytest.mark.parametrize("rows,C", R.XENT_SHAPES)
def test_xent_paths(hip, parity_record, rows, C):
    rng = _rng("xent", rows, C)
    x, g = _xent_inputs(rows, C, rng)
    for k, t in enumerate(R.xent_targets(rows, C, rng)):
        _xent_compare(parity_record, f"{rows}x{C} targets {k}", _xent_run(hip, x, t, g), x, t, g)


@pytest.mark.parametrize("which", ["logits", "dlogits"])
def test_xent_misaligned_pointer(hip, parity_record, which):
    """An aligned class count with logits off 16 bytes (online scalar forward, scalar backward),
    then with only dlogits off (register forward, scalar backward)."""
    rows, C = R.XENT_MISALIGNED
    rng = _rng("xent-mis")
    x, g = _xent_inputs(rows, C, rng)
    t = R.xent_targets(rows, C, rng)[0]
    got = _xent_run(hip, x, t, g, mis_x=which == "logits", mis_dx=which == "dlogits")
    _xent_compare(parity_record, f"{rows}x{C} {which} misaligned", got, x, t, g)


@pytest.mark.parametrize("C,mis", R.XENT_NEGINF, ids=[f"C{c}{'-misaligned' if m else ''}" for c, m in R.XENT_NEGINF])
def test_xent_neginf_logits(hip, parity_record, C, mis):
    """-inf logits weigh zero in every forward kernel: finite loss and lse equal to the reference,
    dx exactly 0 at those columns. In the online kernel (C = 1023, 16388 and the misaligned 1024)
    a thread whose first value is -inf holds a NaN partial sum for a while; its max is still -inf
    then, and every later use drops the sum of such a pair, so the NaN never reaches lse."""
    x, t = R.xent_neginf_rows(C, _rng("xent-neginf", C))
    g = np.array([1.0, -2.0, 0.5, 1.5], dtype=np.float32)
    loss, lse, dx = got = _xent_run(hip, x, t, g, mis_x=mis)
    print(f"softmax_xent -inf C={C} misaligned={mis}: loss {loss}, lse {lse}")
    assert np.isfinite(loss).all() and np.isfinite(lse).all(), (loss, lse)
    _xent_compare(parity_record, f"-inf logits C{C}{' misaligned' if mis else ''}", got, x, t, g)
    assert not dx[np.isneginf(x)].any()


def test_xent_bad_sizes(hip):
    torch, _hip, L = hip
    p, v = _out(8)
    s = _hip.stream_ptr()
    a = v.data_ptr()
    for rows, C in ((2, 0), (-1, 4), (2, -4)):
        _is_error(L, L.mt_softmax_xent_fw(a, a, a, a, rows, C, s), "mt_softmax_xent_fw")
        _is_error(L, L.mt_softmax_xent_bw(a, a, a, a, a, rows, C, s), "mt_softmax_xent_bw")
    torch.cuda.synchronize()
    assert bool(torch.isnan(v).all()) and R.footprint([("out", p, [])]) == []
