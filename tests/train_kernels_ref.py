"""References and case tables for the training-step helper kernels (csrc/combine.hip,
csrc/softmax_layernorm.hip, csrc/rng.h): mt_rand_uniform, mt_dropout, mt_bias_gelu_fw / _bw,
mt_embedding_fw / _bw, mt_adam_step and mt_softmax_xent_fw / _bw.

No GPU; NumPy only, but for the two guard-band helpers (place_flat, footprint), which hand out
torch views of tests/flash_layouts.py's Parent on the device asked for. tests/test_train_kernels.py checks these references against published
vectors and torch's float64 forms; tests/test_train_kernels_gpu.py runs the kernels against them
over the case tables at the end of this file.

Each reference restates the contract in include/minitorch_hip.h, not the kernel's code:

    uniform24_ref     rng.h: u[i] = top 24 bits of splitmix64(seed + golden (i + 1)) / 2^24
    dropout_ref       out = u > p ? x * scale : 0 (float32, exact)
    bias_gelu_ref     0.5 u (1 + tanh(sqrt(2/pi) (u + 0.044715 u^3))), u = x + bias, float64
    embed_*_ref       a float id f names row trunc(f) iff f >= 0 and trunc(f) < V, else a zero row
    adam_ref          the optimizer's tensor-op arithmetic in float32
    xent_ref          lse, lse - x[target], g (softmax - onehot) in float64
"""
import numpy as np

# ---- the counter-based RNG ---------------------------------------------------------------------
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64_ref(seed, idx):
    """Output number idx (from 0) of the splitmix64 stream seeded with `seed`, as np.uint64:
    mix64(seed + GOLDEN (idx + 1)) in wrapping 64-bit arithmetic."""
    i = np.atleast_1d(np.asarray(idx)).astype(np.uint64)
    s = np.full(1, int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = s + np.uint64(GOLDEN) * (i + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform24_ref(seed, idx):
    """The float32 mt_rand_uniform(out, n, seed) writes at out[idx]: exact, (h >> 40) < 2^24."""
    h = splitmix64_ref(seed, idx)
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_ref(x, p, scale, seed):
    """mt_dropout over the flat float32 x: bit-exact (one float32 product per kept element)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    u = uniform24_ref(seed, np.arange(x.size, dtype=np.int64))
    return np.where(u > np.float32(p), x * np.float32(scale), np.float32(0.0)).astype(np.float32)


# ---- bias + GELU (tanh form) -------------------------------------------------------------------
_K = np.sqrt(2.0 / np.pi)
_C = 0.044715


def bias_gelu_ref(x, b):
    u = np.asarray(x, dtype=np.float64) + np.asarray(b, dtype=np.float64)
    return 0.5 * u * (1.0 + np.tanh(_K * (u + _C * u ** 3)))


def bias_gelu_bw_ref(dy, x, b):
    u = np.asarray(x, dtype=np.float64) + np.asarray(b, dtype=np.float64)
    t = np.tanh(_K * (u + _C * u ** 3))
    return np.asarray(dy, dtype=np.float64) * (0.5 * (1.0 + t) + 0.5 * u * (1.0 - t * t) * _K * (1.0 + 3.0 * _C * u * u))


# ---- embedding ---------------------------------------------------------------------------------
def embed_rows(ids, V):
    """(valid, row) of float token ids: valid iff f >= 0 and trunc(f) < V (NaN, +-inf, negative
    and too-large ids name no row); row is 0 where invalid."""
    f = np.asarray(ids, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = (f >= 0) & (np.trunc(f) < V)
    return valid, np.where(valid, np.trunc(np.where(valid, f, 0.0)), 0.0).astype(np.int64)


def embed_fw_ref(ids, W):
    """out[t] = W[ids[t]] or a row of +0.0: bit-exact."""
    W = np.asarray(W, dtype=np.float32)
    valid, row = embed_rows(ids, W.shape[0])
    return np.where(valid[:, None], W[row], np.float32(0.0)).astype(np.float32)


def embed_bw_ref(dy, ids, V):
    """(dW float64 [V, E], cnt int64 [V], sabs float64 [V, E]): the sum of the dy rows of each id,
    how many there are, and the sum of their magnitudes. A float32 sum of cnt terms in any fixed
    order is within cnt 2^-24 sabs of dW (recursive-summation bound, (cnt - 1) u / (1 - (cnt - 1) u)
    <= cnt u for cnt < 2^12); with cnt <= 1 it is exact."""
    dy = np.asarray(dy, dtype=np.float32).astype(np.float64)
    valid, row = embed_rows(ids, V)
    dW = np.zeros((V, dy.shape[1]))
    sabs = np.zeros((V, dy.shape[1]))
    cnt = np.zeros(V, dtype=np.int64)
    np.add.at(dW, row[valid], dy[valid])
    np.add.at(sabs, row[valid], np.abs(dy[valid]))
    np.add.at(cnt, row[valid], 1)
    return dW, cnt, sabs


# ---- Adam --------------------------------------------------------------------------------------
# One step of minitorch.optim.Adam's tensor-op arithmetic in float32 (second moment on
# (1 - beta2)), (p, g, m, v, t, lr, b1, b2, eps) -> (p, m, v): the restatement the existing Adam
# test already holds the kernel to, imported so that there is one copy of it
from test_optim_gpu import _np_adam as adam_ref  # noqa: E402


# ---- softmax cross-entropy ---------------------------------------------------------------------
def xent_ref(x, t, g):
    """(lse, loss, dx) in float64 of rows x [rows, C], float targets t and upstream g [rows].
    A target outside [0, C) picks nothing: loss = lse, dx = g softmax. -inf logits weigh zero."""
    x = np.asarray(x, dtype=np.float64)
    rows, C = x.shape
    ti = np.trunc(np.asarray(t, dtype=np.float64)).astype(np.int64)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
    inr = (ti >= 0) & (ti < C)
    r = np.arange(rows)
    pick = np.where(inr, x[r, np.where(inr, ti, 0)], 0.0)
    sm = np.exp(x - lse[:, None])
    sm[r[inr], ti[inr]] -= 1.0
    return lse, lse - pick, sm * np.asarray(g, dtype=np.float64)[:, None]


# ---- guard-banded buffers (tests/flash_layouts.py's Parent and checks; torch from here on) -----
GUARD = 64  # floats of guard band on each side of every view


def place_flat(sizes, device, output, xs=None, mis=False):
    """One float32 Parent holding a flat view per entry of `sizes`, GUARD floats of band before the
    first, between neighbours and after the last. Each view starts on a 16-byte boundary, or one
    float past it (mis). An output parent holds the sentinel outside the views and NaN inside
    (xs[i] instead where xs is given: a tensor updated in place); an input parent holds NaN
    outside and xs[i] inside. Returns (parent, views)."""
    import torch
    import flash_layouts as FL
    offs, off = [], GUARD
    for n in sizes:
        offs.append(off + int(mis))
        off += (n + 1 + 3) // 4 * 4 + GUARD
    p = FL.Parent(off, torch.float32, device, output)
    assert p.flat.data_ptr() % 16 == 0
    views = []
    for i, (n, o) in enumerate(zip(sizes, offs)):
        x = None if xs is None else np.asarray(xs[i], dtype=np.float32).reshape(-1)
        assert x is None or x.size == n
        v = p.view((n,), (1,), o, x)
        assert n == 0 or v.data_ptr() % 16 == (4 if mis else 0)
        views.append(v)
    return p, views


def footprint(outs=(), ins=()):
    """Failure strings of one call. outs: (name, parent, views): nothing outside the views was
    written and no NaN is left inside. ins: (name, parent, bits before): nothing changed."""
    import flash_layouts as FL
    fails = []
    for name, p, views in outs:
        fails += FL.untouched(p, what=f"{name} parent")
        for i, v in enumerate(views):
            fails += FL.all_written(v, f"{name}[{i}]")
    for name, p, before in ins:
        fails += FL.unchanged(before, p, f"{name} parent")
    return fails


# ---- case tables -------------------------------------------------------------------------------

# mt_rand_uniform: 256 threads a workgroup, at most 8192 workgroups: index 2,097,152 is the first
# of the second grid-stride trip
RAND_N = (1, 255, 256, 257, 2_097_152, 2_097_152 + 257)
RAND_SEEDS = (0, 1, 2 ** 63, 2 ** 64 - 1)

# mt_dropout: grid_for caps at 4096 workgroups: index 1,048,576 is the second trip
DROPOUT_N = (1, 1023, 1_048_576 + 3)
DROPOUT_P = (0.0, 0.1, 0.5, 1.0 - 2.0 ** -24)
# a draw is exactly 0 once in 2^24: seeds (found by search with uniform24_ref) whose first n draws
# hold one, and where, so that p = 0 has something to drop (tests/test_train_kernels.py checks them)
DROPOUT_ZERO = {1: (5618432, 0), 1023: (2296, 356), 1_048_576 + 3: (49, 330783)}

# mt_bias_gelu (rows, cols) and the source branch each reaches
GELU_SHAPES = (
    (1, 1),         # scalar, one element
    (3, 4),         # vector, bias index wraps every float4
    (5, 8),         # vector
    (33, 7),        # scalar (cols % 4)
    (7, 1028),      # vector, 257 float4 a row: more than one workgroup
    (4100, 1028),   # vector, n / 4 = 1,053,700 > 1,048,576: the second grid-stride trip
    (1025, 1027),   # scalar, n = 1,052,675: the second trip
)
GELU_MISALIGNED = (64, 256)  # cols % 4 == 0 with one pointer off 16 bytes: the scalar fallback
GELU_PLANTED = (0.0, 1e-8, -1e-8, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0, 30.0, -30.0, 1e4, -1e4)


def gelu_inputs(rows, cols, rng):
    """(x, bias, dy) float32: x ~ N(0, 2), bias ~ N(0, 1) with every third column 0, dy ~ N(0, 1);
    GELU_PLANTED (saturation both ways, the 1 + tanh cancellation for negative u, tiny values)
    written into x at spread positions of the zero-bias columns, so u = x + bias is the planted
    value itself (as many as there are positions)."""
    x = (rng.standard_normal((rows, cols)) * 2).astype(np.float32)
    b = rng.standard_normal(cols).astype(np.float32)
    b[::3] = 0.0
    dy = rng.standard_normal((rows, cols)).astype(np.float32)
    r, c = np.meshgrid(np.arange(rows), np.arange(0, cols, 3), indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    k = min(len(GELU_PLANTED), r.size)
    for n in range(k):
        j = (n * r.size) // k
        x[r[j], c[j]] = GELU_PLANTED[n]
    return x, b, dy

# mt_embedding: V at the kEmbVB = 8 edges, E at the 256-column passes, ntok at the wave (128
# tokens) and chunk (2048 tokens) edges. Every (V, E) pair once, ntok chosen so that every value
# appears at least twice, every V meets four ntok and every E five (all 40 (E, ntok) pairs
# would need 40 cases); (9, 257, 2049) and (17, 513, 4097) are in it.
EMBED_V = (1, 7, 8, 9, 17)
EMBED_E = (1, 255, 256, 257, 513)
EMBED_NTOK = (1, 127, 128, 129, 2047, 2048, 2049, 4097)
EMBED_CASES = tuple((V, E, EMBED_NTOK[(3 * i + 6 * j + 3) % 8])
                    for i, V in enumerate(EMBED_V) for j, E in enumerate(EMBED_E))


def embed_special_ids(V):
    """Ids planted among the random ones, with the row each must select (None: a zero row)."""
    sp = [(float(V), None), (float(V + 3), None), (-1.0, None), (-0.0, 0), (4294967298.0, None),
          (1e30, None), (float("inf"), None), (float("-inf"), None), (float("nan"), None)]
    if V > 2:
        sp.append((2.7, 2))
    return sp


def embed_ids(V, ntok, rng):
    """Random ids in [0, V) as float32 with the specials planted at spread positions (as many as
    fit); returns (ids, {position: expected row or None})."""
    ids = rng.integers(0, V, ntok).astype(np.float32)
    sp = embed_special_ids(V)
    planted = {}
    if ntok >= 2:
        k = min(len(sp), ntok - 1)  # leave at least one plain id
        for n, (f, row) in enumerate(sp[:k]):
            pos = 1 + (n * (ntok - 1)) // k
            ids[pos] = f
            planted[pos] = row
    return ids, planted


# mt_adam_step: kAdamMax = 24 tensors a launch
ADAM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4097)
ADAM_COUNTS = (24, 25, 48, 49)


def adam_sizes(count, zero_at=None):
    """`count` sizes cycling through ADAM_SIZES from an offset that depends on count, with a
    zero-numel entry at index zero_at."""
    s = [ADAM_SIZES[(i + count) % len(ADAM_SIZES)] for i in range(count)]
    if zero_at is not None:
        s[zero_at] = 0
    return s


# mt_softmax_xent (rows, C) and the forward kernel each reaches (the backward has one kernel with a
# vector and a scalar loop)
XENT_SHAPES = (
    (3, 1),           # online, scalar
    (5, 3),           # online, scalar
    (5, 4),           # register kernel, nk = 1, one lane live
    (4, 1020),        # register, nk = 1, last lane idle
    (4, 1024),        # register, nk = 1 exactly
    (4, 1028),        # register, nk = 2, one float4 in the second piece
    (3, 16380),       # register, nk = 16, last piece partial
    (3, 16384),       # register, nk = 16 exactly (the largest)
    (3, 16388),       # online, vector
    (3, 16387),       # online, scalar
    (65536 + 5, 5),   # the row grid-stride (65536 workgroups)
)
XENT_MISALIGNED = (8, 1024)
XENT_NEGINF = ((1023, False), (1024, False), (16388, False), (1024, True))  # (C, misaligned)


def xent_targets(rows, C, rng):
    """Float target vectors of length `rows` that between them hold column 0, column C - 1, -1, C
    (both pick nothing), a column inside the last float4, and random columns."""
    special = [0, C - 1, -1, C, max(C - 2, 0)]
    n = -(-(len(special) + 1) // rows) * rows
    t = np.concatenate([special, rng.integers(0, C, n - len(special))]).astype(np.float32)
    return [t[i:i + rows] for i in range(0, len(t), rows)]


def xent_neginf_rows(C, rng):
    """(x [4, C] float32, t [4]): row 0 with -inf at column 0; row 1 with -inf at every column some
    thread reads first in any path (columns 0 .. 255 of the scalar loops, every fourth column
    below 1024 of the float4 loops), so every online (max, sum) pair starts from -inf; row 2 with
    -inf at a random third of the columns; row 3 without (the control). The target sits on a
    finite column."""
    x = (rng.standard_normal((4, C)) * 3).astype(np.float32)
    x[0, 0] = -np.inf
    first = np.union1d(np.arange(min(256, C)), np.arange(0, min(1024, C), 4))
    x[1, first] = -np.inf
    x[2, rng.random(C) < 1.0 / 3.0] = -np.inf
    t = np.array([rng.choice(np.flatnonzero(np.isfinite(x[r]))) for r in range(4)], dtype=np.float32)
    return x, t
