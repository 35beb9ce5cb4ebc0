"""Inputs and the case table of the GEMM exactness matrix (test infrastructure; modelled on
tests/decode_cases.py). tests/test_gemm_plan.py checks the table and the inputs on the CPU,
tests/test_gemm_matrix_gpu.py runs mt_matmul_f32 on them.

Exact input kinds: every partial sum of the product is an integer below 2^24 in magnitude, so
any summation order in any binary format with 24 significand bits gives the float64 product
bit for bit, and a wrong index, tail, slice or bf16 plane shows as a wrong integer.

  ints    A, B integers in [-4, 4], dense: |sum| <= 16 K. Every (m, n, k) counts once. In the
          three-piece bf16 GEMM (X3) only the high plane is non-zero.
  wide_a  A = +-65793 = 2^16 + 2^8 + 1, whose X3 pieces are 65536, 256 and 1: all three planes
          carry data. B in {-1, 0, 1} with at most 255 non-zeros per column (255 * 65793 < 2^24).
          K <= 255: dense. Above: random positions plus, in every column, the k a kernel could
          drop or double: the first and last k of every split-K slice any backend's plan for the
          shape has, the last k of a slice's first 256-k flush group and the first of its second,
          and K - 1.
  wide_b  the same with the roles swapped (A sparse per row, B = +-65793).

Floating kind `gauss`: N(0,1) and a twin with row i of A times 2^e_i and column j of B times
2^f_j (e, f integers in [-20, 20]). A power of two commutes with every rounding and with the X3
truncation, so the twin's product must be the base product times 2^(e_i + f_j) bit for bit.

Placement: each operand and C is a view inside a larger flat buffer; operand padding (before,
between rows, between batches, after) is NaN, C's is the SENTINEL bit pattern. A layout is
Lay(unit, pad, off, bs, strides): unit 'k' / 'm' / 'n' names the unit-stride dimension ('x':
none, both strides even), pad the leading dimension's excess over the extent (AL4: up to the
next multiple of 4 floats and at least 1; ODD: to an odd leading dimension), off the view's
offset in floats, bs the batch stride (None: the matrix's span rounded up to 4 floats plus 4;
0: broadcast), strides an explicit (row, col) pair for the size-1 cases.
"""
import collections
import functools
import itertools

import numpy as np

WIDE = 65793.0
CAP = 255
SENTINEL = 0xDEADBEEF
AL4, ODD = -1, -2
TAIL = 5  # floats after the last element

Lay = collections.namedtuple("Lay", "unit pad off bs strides", defaults=(0, 0, None, None))
Case = collections.namedtuple("Case", "name cls batch M N K la lb lc")

# kernel ids of mt_matmul_f32_plan
ROCBLAS, ROCBLAS_SPLIT, F32, X3, X3BIG = range(5)


def V(unit, bs=None):
    """A layout the 16-B kernels take: 16-B aligned base (4 NaN floats before it), leading
    dimension a multiple of 4 above the extent."""
    return Lay(unit, AL4, 4, bs)


def NVOFF(unit, bs=None):
    """As V but one float further: misaligned base."""
    return Lay(unit, AL4, 1, bs)


def NVODD(unit, bs=None):
    """Aligned base, odd leading dimension."""
    return Lay(unit, ODD, 4, bs)


def _operand(ak, vec, which, how):
    unit = "k" if ak else which
    return V(unit) if vec else (NVOFF(unit) if how == 0 else NVODD(unit))


# C layouts: tight, padded row, batch gap, transposed (scm = 1), misaligned base
C_TIGHT = Lay("n", 0, 0)
C_PAD = Lay("n", 3, 4)
C_PAD4 = Lay("n", 4, 4)
C_GAP = Lay("n", 0, 4, -7)  # bs < 0: the span plus that many floats
C_T = Lay("m", 2, 4)
C_OFF1 = Lay("n", 0, 1)
C_CYCLE = (C_TIGHT, C_PAD, C_GAP, C_T, C_OFF1, C_PAD4, C_TIGHT, C_PAD)

VARIANTS = tuple(itertools.product((True, False), (True, False), (True, False)))  # (ak, bk, vec)


def _variants(cls, tag, batch, M, N, K, which=VARIANTS, c_cycle=C_CYCLE, a_bs=None, b_bs=None):
    out = []
    for i, (ak, bk, vec) in enumerate(which):
        # non-VEC: one operand alone breaks the 16-B form (A's base, or B's leading dimension)
        la = _operand(ak, vec or ak != bk, "m", 0)
        lb = _operand(bk, vec or ak == bk, "n", 1)
        if a_bs is not None and i == a_bs:
            la = la._replace(bs=0)
        if b_bs is not None and i == b_bs:
            lb = lb._replace(bs=0)
        name = f"{tag}-{'k' if ak else 'm'}{'k' if bk else 'n'}{'v' if vec else 's'}"
        out.append(Case(name, cls, batch, M, N, K, la, lb, c_cycle[i % len(c_cycle)]))
    return out


def _table():
    t = []
    # unit dimensions with odd free strides: rocBLAS's stride normalisation, X3's K / M / N == 1
    S_ = lambda sr, sc, off=0: Lay("s", 0, off, None, (sr, sc))  # noqa: E731
    t += [
        Case("unit-m1", "unit", 1, 1, 5, 7, S_(3, 1), Lay("n", 2, 1), S_(13, 1)),
        Case("unit-m1-t", "unit", 1, 1, 5, 7, S_(11, 3), Lay("k", 1, 0), S_(1, 1, 3)),
        Case("unit-n1", "unit", 1, 5, 1, 7, Lay("k", 2, 1), S_(1, 9), S_(3, 5)),
        Case("unit-n1-t", "unit", 1, 5, 1, 7, Lay("m", 0, 0), S_(3, 5), S_(1, 7, 1)),
        Case("unit-k1", "unit", 1, 5, 7, 1, S_(3, 5), S_(11, 1), Lay("n", 1, 1)),
        Case("unit-k1-t", "unit", 1, 5, 7, 1, S_(1, 9), S_(3, 1), C_T),
        Case("unit-m1n1", "unit", 1, 1, 1, 9, S_(5, 1), S_(1, 11), S_(7, 3)),
        Case("unit-m1n1-x", "unit", 1, 1, 1, 9, S_(5, 3), S_(3, 11), S_(7, 3, 1)),
    ]
    # every tile edge of the 64-tile kernels and of gemm_f32_kernel
    t += _variants("ragged", "ragged1", 1, 67, 69, 45)
    t += _variants("ragged", "ragged3", 3, 67, 69, 45, which=((True, False, True), (False, True, False),
                                                             (True, True, True), (False, False, False),
                                                             (True, False, False)),
                   c_cycle=(C_GAP, C_PAD, C_TIGHT, C_OFF1, C_T), a_bs=1, b_bs=2)
    # k edges: 1 / 2 / 3 ring stages, the 256-k flush, BK = 16 of the fp32 kernel
    for i, K in enumerate((15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)):
        which = (VARIANTS[(2 * i) % 8], VARIANTS[(2 * i + 5) % 8])
        t += _variants("kedge", f"k{K}", 1, 33, 35, K, which=which, c_cycle=C_CYCLE[i % 5:])
    # 64-tile split-K: S = 1, 2, 4, 15 (ragged last slice)
    for i, K in enumerate((511, 512, 4100)):
        which = (VARIANTS[(3 * i) % 8], VARIANTS[(3 * i + 5) % 8])
        t += _variants("split64", f"s{K}", 1, 67, 69, K, which=which, c_cycle=C_CYCLE[i + 1:])
    t += _variants("split64", "s1100", 1, 67, 69, 1100)
    # gemm_x3_big: ragged M, N, K against 128 / 16, batched and split
    t += _variants("big", "big64", 64, 130, 140, 21, a_bs=2, b_bs=5)
    t += _variants("bigsplit", "bigs", 1, 763, 765, 8200)
    # rocBLAS's own split-K: S = 8, 4, 2, none; both ops on both operands; the gating conditions
    AN, AT, BN, BT = V("k"), V("m"), V("n"), V("k")
    t += [
        Case("rb8192-nn", "rbsplit", 1, 5, 8, 8192, AN, BN, C_TIGHT),
        Case("rb8192-nt", "rbsplit", 1, 5, 8, 8192, AN, BT, C_PAD4),     # scm = 12
        Case("rb8192-tn", "rbsplit", 1, 5, 8, 8192, AT, BN, C_PAD4),
        Case("rb8192-tt", "rbsplit", 1, 5, 8, 8192, AT, BT, C_TIGHT),
        Case("rb8192-coff", "rbsplit", 1, 5, 8, 8192, AN, BN, C_OFF1),   # C misaligned: no split
        Case("rb8192-cpad3", "rbsplit", 1, 5, 8, 8192, AN, BN, C_PAD),   # scm = 11: no split
        Case("rb4100-nn", "rbsplit", 1, 5, 8, 4100, AN, BN, C_PAD4),
        Case("rb4100-tt", "rbsplit", 1, 5, 8, 4100, AT, BT, C_TIGHT),
        Case("rb4098-nt", "rbsplit", 1, 5, 8, 4098, NVOFF("k"), BT, C_TIGHT),
        Case("rb4098-tn", "rbsplit", 1, 5, 8, 4098, AT, NVODD("n"), C_PAD4),
        Case("rb4097-nn", "rbsplit", 1, 5, 8, 4097, AN, BN, C_TIGHT),    # no S divides K
        Case("rb8192-b2", "rbsplit", 2, 5, 8, 8192, AN, BN, C_TIGHT),    # batch 2: no split
        Case("rb300-nn", "rbsplit", 1, 300, 64, 8192, AN, BN, C_TIGHT),
        Case("rb300-tt", "rbsplit", 1, 300, 64, 8192, AT, BT, C_PAD4),
    ]
    # no unit stride in an operand; C transposed
    t += [
        Case("fb-ax", "fallback", 1, 67, 69, 45, Lay("x", 1, 1), V("n"), C_PAD),
        Case("fb-bx", "fallback", 3, 67, 69, 45, V("k"), Lay("x", 0, 0), C_GAP),
        Case("fb-ct", "fallback", 1, 67, 69, 45, V("k"), V("n"), C_T),
        Case("fb-ct3", "fallback", 3, 67, 69, 45, NVOFF("m"), V("k"), C_T),
    ]
    names = [c.name for c in t]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(t)


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}

# The plan mt_matmul_f32_plan must give for each entry under backends 0..3:
# (kernel, ak, bk, vec, S, ks). A change of the dispatch shows here before it moves a case of
# the GPU matrix to another kernel. Entries of one class differ in layout only, so most of a
# class shares its plans but for (ak, bk, vec).
def _x(kern, c, S=1, ks=None):
    ak, bk, vec = _abv(c)
    return (kern, ak, bk, vec, S, c.K if ks is None else ks)


def _abv(c):
    """(ak, bk, vec) the X3 dispatch must see for the entry's layouts."""
    ak = int(c.la.unit == "k" or c.K == 1 or (c.la.strides is not None and c.la.strides[1] == 1))
    bk = int(c.lb.unit == "k" or c.K == 1 or (c.lb.strides is not None and c.lb.strides[0] == 1))
    g = geometry(c)
    sa, sb = list(g["sa"]), list(g["sb"])
    if c.K == 1:
        sa[2], sb[1] = 1, 1
    if c.M == 1:
        sa[1] = 1
    if c.N == 1:
        sb[2] = 1
    oa, ob = (sa[1] if ak else sa[2]), (sb[2] if bk else sb[1])
    vec = int(g["a_off"] % 4 == 0 and g["b_off"] % 4 == 0 and oa % 4 == 0 and ob % 4 == 0 and
              (c.batch == 1 or (sa[0] % 4 == 0 and sb[0] % 4 == 0)))
    return ak, bk, vec


def _rb(c, S=1, ks=None, kern=None):
    """rocBLAS: ak / bk = op N on A / B."""
    an = int(c.la.unit == "k" or (c.la.strides is not None and (c.la.strides[1] == 1 or c.K == 1)))
    bn = int(c.lb.unit == "n" or (c.lb.strides is not None and (c.lb.strides[1] == 1 or c.K == 1)))
    if kern is None:
        kern = ROCBLAS_SPLIT if S > 1 else ROCBLAS
    return (kern, an, bn, -1, S, c.K if ks is None else ks)


F32PLAN = lambda c: (F32, -1, -1, -1, 1, c.K)  # noqa: E731


def expected(c):
    """The four plans (backends 0..3) of a table entry, from its class."""
    f = F32PLAN(c)
    if c.cls == "unit":
        x = _x(X3, c)
        per = {  # backend 0: which unit-dimension layouts rocBLAS takes after normalisation
            "unit-m1": _rb(c), "unit-m1-t": f, "unit-n1": _rb(c), "unit-n1-t": f,
            "unit-k1": _rb(c), "unit-k1-t": f, "unit-m1n1": _rb(c), "unit-m1n1-x": f,
        }[c.name]
        # X3 takes them all: a size-1 dimension's stride is rewritten to 1 (unit-m1n1-x then
        # reads A along m and B along n)
        return (per, f, x, x)
    if c.cls in ("ragged", "kedge"):
        r = f if c.lc.unit == "m" else _rb(c)
        return (r, f, _x(X3, c), _x(X3, c))
    if c.cls == "split64":
        S, ks = {511: (1, 511), 512: (2, 256), 1100: (4, 288), 4100: (15, 288)}[c.K]
        r = f if c.lc.unit == "m" else _rb(c)
        return (r, f, _x(X3, c, S, ks), _x(X3, c, S, ks))
    if c.cls == "big":
        r = f if c.lc.unit == "m" else _rb(c)
        return (r, f, _x(X3BIG, c), _x(X3, c))
    if c.cls == "bigsplit":
        r = f if c.lc.unit == "m" else _rb(c)
        return (r, f, _x(X3BIG, c, 8, 1040), _x(X3, c))
    if c.cls == "rbsplit":
        split = {"rb8192-nn": 8, "rb8192-nt": 8, "rb8192-tn": 8, "rb8192-tt": 8, "rb8192-coff": 1,
                 "rb8192-cpad3": 1, "rb4100-nn": 4, "rb4100-tt": 4, "rb4098-nt": 2, "rb4098-tn": 2,
                 "rb4097-nn": 1, "rb8192-b2": 1, "rb300-nn": 8, "rb300-tt": 8}[c.name]
        r = _rb(c, split, c.K // split)
        if c.M == 300:   # 5 x 1 tiles of 64: 16 slices wanted, K / 256 = 32 allows them
            x = _x(X3, c, 16, 512)
        elif c.batch > 1:
            x = _x(X3, c)
        else:            # one 64-tile: 16 slices of ceil32(K / 16)
            ks = -(-(-(-c.K // 16)) // 32) * 32
            x = _x(X3, c, -(-c.K // ks), ks)
        return (r, f, x, x)
    if c.cls == "fallback":
        if c.name in ("fb-ax", "fb-bx"):
            return (f, f, f, f)
        return (f, f, _x(X3, c), _x(X3, c))  # the X3 kernels write any C strides themselves
    raise KeyError(c.cls)


# ---- geometry ------------------------------------------------------------------------------
def _pad(pad, ext):
    if pad == AL4:
        return (-ext) % 4 or 4
    if pad == ODD:
        return 0 if ext % 2 else 1
    return pad


def _matrix(lay, rows, cols, first, second):
    """(row stride, col stride, span) of a logical [rows, cols] matrix whose dimensions are
    named `first` / `second` ('m','k' for A; 'k','n' for B; 'm','n' for C)."""
    if lay.strides is not None:
        sr, sc = lay.strides
        return sr, sc, (rows - 1) * sr + (cols - 1) * sc + 1
    if lay.unit == second:
        ld = cols + _pad(lay.pad, cols)
        return ld, 1, rows * ld
    if lay.unit == first:
        ld = rows + _pad(lay.pad, rows)
        return 1, ld, cols * ld
    assert lay.unit == "x", lay
    ld = cols + _pad(lay.pad, cols)
    return 2 * ld, 2, 2 * rows * ld


def _batch_stride(lay, span):
    if lay.bs is None:
        return (span + 3) // 4 * 4 + 4
    if lay.bs < 0:
        return span - lay.bs
    return lay.bs


@functools.lru_cache(maxsize=None)
def geometry(c):
    """Strides (batch, row, col), offsets and buffer sizes (floats) of a table entry."""
    g = {}
    for key, lay, rows, cols, d0, d1 in (("a", c.la, c.M, c.K, "m", "k"), ("b", c.lb, c.K, c.N, "k", "n"),
                                         ("c", c.lc, c.M, c.N, "m", "n")):
        sr, sc, span = _matrix(lay, rows, cols, d0, d1)
        bs = _batch_stride(lay, span)
        nb = 1 if bs == 0 else c.batch
        g["s" + key] = (bs, sr, sc)
        g[key + "_off"] = lay.off
        g[key + "_size"] = lay.off + (nb - 1) * bs + span + TAIL
    return g


def view(buf, off, strides, shape):
    """The [batch, rows, cols] view of a flat buffer (a broadcast batch shows its one matrix)."""
    nb = 1 if strides[0] == 0 else shape[0]
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(nb,) + tuple(shape[1:]),
                                           strides=tuple(int(s) * buf.itemsize for s in strides))


def place(vals, off, strides, size, fill):
    """A flat fp32 buffer of `size` floats holding `fill` bits/values everywhere but the view."""
    buf = np.empty(size, np.float32)
    if isinstance(fill, int):
        buf.view(np.uint32)[:] = fill
    else:
        buf[:] = fill
    if vals is not None:
        view(buf, off, strides, vals.shape)[...] = vals if strides[0] else vals[:1]
    return buf


def outside_mask(size, off, strides, shape):
    """True for every float of the buffer that is not an element of the view."""
    m = np.ones(size, bool)
    view(m, off, strides, shape)[...] = False
    return m


# ---- inputs --------------------------------------------------------------------------------
def _shape_key(c):
    return (c.batch, c.M, c.N, c.K, geometry(c)["sa"][0] == 0, geometry(c)["sb"][0] == 0)


@functools.lru_cache(maxsize=None)
def mandatory_k(K, M=None, N=None, batch=None):
    """The k positions every sparse column (row) must hold for a [.., K] reduction: slice and
    flush-group edges of every split plan the table expects for the shape, and K - 1."""
    plans = {(1, K)}
    for c in TABLE:
        if (c.M, c.N, c.K, c.batch) == (M, N, K, batch):
            plans.update((p[4], p[5]) for p in expected(c))
    ks_ = {K - 1}
    for S, ks in plans:
        for s in range(S):
            beg, end = s * ks, min(K, (s + 1) * ks)
            ks_.update((beg, end - 1))
            if beg + 256 < end:
                ks_.update((beg + 255, beg + 256))
    return tuple(sorted(k for k in ks_ if 0 <= k < K))


def _sparse_ternary(rng, lines, K, must):
    """[lines, K] in {-1, 0, 1}: dense for K <= CAP, else CAP non-zeros per line, `must` among them."""
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=(lines, K))
    if K <= CAP:
        sign[rng.random((lines, K)) < 0.1] = 0.0
        return sign
    assert len(must) <= CAP, len(must)
    keep = np.zeros((lines, K), bool)
    keep[:, list(must)] = True
    free = np.setdiff1d(np.arange(K), np.array(must, np.int64))
    n = CAP - len(must)
    for i in range(lines):
        keep[i, rng.choice(free, size=n, replace=False)] = True
    return np.where(keep, sign, np.float32(0.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(key, kind):
    batch, M, N, K, a0, b0 = key
    rng = np.random.default_rng([batch, M, N, K, int(a0), int(b0), len(kind), ord(kind[-1])])
    na, nb = (1 if a0 else batch), (1 if b0 else batch)
    if kind == "ints":
        a = rng.integers(-4, 5, size=(na, M, K)).astype(np.float32)
        b = rng.integers(-4, 5, size=(nb, K, N)).astype(np.float32)
    elif kind in ("wide_a", "wide_b"):
        must = mandatory_k(K, M, N, batch)
        if kind == "wide_a":
            a = (rng.choice(np.array([-WIDE, WIDE]), size=(na, M, K))).astype(np.float32)
            b = _sparse_ternary(rng, nb * N, K, must).reshape(nb, N, K).transpose(0, 2, 1).copy()
        else:
            a = _sparse_ternary(rng, na * M, K, must).reshape(na, M, K)
            b = (rng.choice(np.array([-WIDE, WIDE]), size=(nb, K, N))).astype(np.float32)
    elif kind == "gauss":
        a = rng.standard_normal((na, M, K)).astype(np.float32)
        b = rng.standard_normal((nb, K, N)).astype(np.float32)
    else:
        raise KeyError(kind)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def inputs(c, kind):
    """Logical (A [batch or 1, M, K], B [batch or 1, K, N]) fp32, read-only, shared by every
    entry of the same shape (a broadcast operand has one matrix)."""
    return _inputs(_shape_key(c), kind)


@functools.lru_cache(maxsize=None)
def _ref64(key, kind):
    a, b = _inputs(key, kind)
    r = np.matmul(a.astype(np.float64), b.astype(np.float64))
    r.setflags(write=False)
    return r


def ref64(c, kind):
    """The float64 product [batch, M, N], computed once per shape and kind."""
    return _ref64(_shape_key(c), kind)


@functools.lru_cache(maxsize=None)
def _abs_product(key):
    a, b = _inputs(key, "gauss")
    r = np.matmul(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64))
    r.setflags(write=False)
    return r


def abs_product(c):
    """|A||B| of the gauss inputs in float64 (the componentwise error's denominator)."""
    return _abs_product(_shape_key(c))


@functools.lru_cache(maxsize=None)
def _scales(key):
    batch, M, N, K, a0, b0 = key
    rng = np.random.default_rng([7, M, N, K])
    e = rng.integers(-20, 21, size=M)
    f = rng.integers(-20, 21, size=N)
    return e, f


def scaled_twin(c):
    """(A', B', factor): A' = 2^e_i A, B' = 2^f_j B of the gauss inputs and factor[i, j] =
    2^(e_i + f_j) (fp32, exact)."""
    a, b = inputs(c, "gauss")
    e, f = _scales(_shape_key(c))
    a2 = np.ldexp(a, e[None, :, None]).astype(np.float32)
    b2 = np.ldexp(b, f[None, None, :]).astype(np.float32)
    factor = np.ldexp(np.float32(1.0), e[:, None] + f[None, :]).astype(np.float32)
    return a2, b2, factor


def locate(c, plan, b, m, n):
    """Where output (b, m, n) lies for a plan (kernel, ak, bk, vec, S, ks): a failure message's
    tile and slice description."""
    kern, S, ks = plan[0], plan[4], plan[5]
    t = 128 if kern == X3BIG else 64
    s = f"tile (m {m // t}, n {n // t}) of {t}x{t}, in-tile ({m % t}, {n % t})"
    if S > 1:
        s += f"; {S} k-slices of {ks} (last {c.K - (S - 1) * ks})"
    return s
