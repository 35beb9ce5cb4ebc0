"""Boundary-sensitive key-padding (kv_len) inputs (test infrastructure; tests/test_varlen_edges.py
runs the oracle side on the CPU, tests/test_varlen_matrix_gpu.py the kernels).

One case is a (B, H, N, d) batch with N = 300 and one batch row per kv_len of KV_LEN: every
key-block edge of the kernels that take kv_len, each with the value below and above it, a full
row and a row with no valid key. The edges, read from the kernels:

    32    the ring kernels' 32-key slots (fa_fwd_ring<.., 32, ..>, the X3 forms, fa_bwd_ring's
          BK = 32 dQ tiles) and one 32x32 MFMA tile of keys everywhere else
    64    the 64-key slots / tiles (KB = 2: fa_fwd_generic, fa_fwd_ring<bf16, 64>, fa_bwd_dq)
    128   the generic and ring dK/dV passes' key blocks (BKV = 128)
    256   the fused backwards' key blocks (fa_bwd_fused.hip kKB, fa_bwd_ring.hip kFrBKV), also
          the unit the paired grids count in; 300 = 256 + 44 leaves a ragged second block
    1, 299, 300, 0   one key, one padding key, no padding, no key

Every larger tile is a multiple of a listed one, so the list needs no further edge.

Values: N(0,1) (rounded to bf16 for the bf16 cases); then per row with n = kv_len[b] the last
valid key K[b,:,n-1] x4, the padding keys K[b,:,n:] x4 and the padding values V[b,:,n:] = 64:
all finite and still bf16-exact (the contract is the reference's additive -inf mask, so a
masked key contributes exactly 0 whatever it holds). The last query of every head is
(K[n-1] + K[n]) / sqrt(d), logits of about 16 on the two keys at the boundary: under the
causal mask it is the only query that sees the keys at 298 / 299, and with a random query a
head's off-by-one there moved nothing by its bound in about one head in three. On plain
N(0,1) inputs a kernel that admits the first padding key, or drops the last valid one, moves
a row by about 1/kv_len and stays inside the bf16 bounds from kv_len ~ 100 on; with these
inputs either mistake moves some output by many times its bound (tests/test_varlen_edges.py
asserts at least 3x on every head, oracle only).
"""
import numpy as np

from oracle import attention as A

N = 300
KV_EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 299)
KV_LEN = KV_EDGES + (300, 0)   # 16 batch rows
H_PAIRED = 19                  # 16 x 19 = 304 heads: ceil(300 / 256) x 304 = 608 >= 512 (paired grids)

SPIKE = 4.0      # the last valid key and the padding keys
PAD_V = 64.0     # the padding values


def make_inputs(d, H, bf16, kv=KV_LEN, n=N, seed=0):
    """(q, k, v, do) fp32 arrays (len(kv), H, n, d) of one case (bf16-exact when bf16)."""
    rng = np.random.default_rng([seed, d, H, int(bf16)])
    q, k, v, do = (rng.standard_normal((len(kv), H, n, d)).astype(np.float32) for _ in range(4))
    if bf16:
        q, k, v, do = (A.bf16_round(x) for x in (q, k, v, do))
    for b, nk in enumerate(kv):
        if nk > 0:
            k[b, :, nk - 1] *= np.float32(SPIKE)
        k[b, :, nk:] *= np.float32(SPIKE)
        v[b, :, nk:] = np.float32(PAD_V)
        edge = (k[b, :, nk - 1] if nk > 0 else 0) + (k[b, :, nk] if nk < n else 0)
        last = edge / np.float32(np.sqrt(d))
        q[b, :, n - 1] = A.bf16_round(last) if bf16 else last
    return q, k, v, do


def zero_padding(k, v, kv):
    """Copies of k, v with the padding rows zeroed."""
    k, v = k.copy(), v.copy()
    for b, nk in enumerate(kv):
        k[b, :, nk:] = 0
        v[b, :, nk:] = 0
    return k, v


def oracle_numpy(q, k, v, do, causal, kv):
    """(o, m, l, dq, dk, dv) of the NumPy oracle."""
    o, m, l = A.attention_fwd(q, k, v, causal, kv)
    return (o, m, l) + tuple(A.attention_bwd(q, k, v, o, do, m, l, causal, kv))


def oracle_c(q, k, v, do, causal, kv):
    """(o, m, l, dq, dk, dv) of the C oracle (the same restatement, OpenMP over heads)."""
    from oracle import cref
    o, m, l = cref.attn_fwd(q, k, v, causal, kv_len=kv)
    return (o, m, l) + tuple(cref.attn_bwd(q, k, v, do, m, l, causal, kv_len=kv))


def bf16_bounds(q, k, v, do, causal, kv, p_abs):
    """The elementwise bf16 bounds of tests/bounds.py for a whole case: (O, dQ, dK, dV) arrays
    (B, H, N, d). p_abs: the oracle's P|V| (its forward run on |V|)."""
    from bounds import R_BF16, grad_bounds
    out = [1e-3 + R_BF16 * np.asarray(p_abs, np.float64)] + [np.empty(q.shape) for _ in range(3)]
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            for dst, bnd in zip(out[1:], grad_bounds(q[b, h], k[b, h], v[b, h], do[b, h], causal, kv=kv[b])):
                dst[b, h] = bnd
    return tuple(out)


def bf16_bounds_torch(q, k, v, do, causal, kv, p_abs, device):
    """bf16_bounds with the gradient bounds formed by bounds.grad_bounds_torch on `device` (the
    same arithmetic over all heads at once; tests/test_varlen_edges.py holds the two together)."""
    import torch
    from bounds import R_BF16, grad_bounds_torch
    B, H, n, d = q.shape
    heads = [torch.from_numpy(np.ascontiguousarray(x)).to(device).reshape(B * H, n, d) for x in (q, k, v, do)]
    grads = grad_bounds_torch(*heads, causal, kv=np.repeat(np.asarray(kv, np.int64), H))
    return (1e-3 + R_BF16 * np.asarray(p_abs, np.float64),) + tuple(g.reshape(q.shape).cpu().numpy() for g in grads)


def ref64(q, k, v, do, causal, kv):
    """Plain float64 softmax attention with the key-padding mask, forward and backward
    (o, dq, dk, dv): the yardstick the fp32 oracle's own error is measured against."""
    q, k, v, do = (np.asarray(a, np.float64) for a in (q, k, v, do))
    B, H, n, d = q.shape
    outs = [np.zeros(q.shape) for _ in range(4)]
    tri = np.triu(np.ones((n, n), bool), 1)
    for b in range(B):
        s = q[b] @ np.swapaxes(k[b], -1, -2) / np.sqrt(d)
        if causal:
            s[:, tri] = -np.inf
        s[:, :, int(kv[b]):] = -np.inf
        mx = s.max(-1, keepdims=True)
        p = np.exp(s - np.where(np.isneginf(mx), 0.0, mx))
        tot = p.sum(-1, keepdims=True)
        p = np.where(tot > 0, p / np.where(tot > 0, tot, 1.0), 0.0)
        dp = do[b] @ np.swapaxes(v[b], -1, -2)
        ds = p * (dp - (dp * p).sum(-1, keepdims=True))
        outs[0][b] = p @ v[b]
        outs[1][b] = ds @ k[b] / np.sqrt(d)
        outs[2][b] = np.swapaxes(ds, -1, -2) @ q[b] / np.sqrt(d)
        outs[3][b] = np.swapaxes(p, -1, -2) @ do[b]
    return tuple(outs)


def fp32_bounds(ref, r64):
    """The project's fp32 bounds for one case: 1e-5 max-abs on O and 2e-5 x max(1, max|ref|)
    on the gradients (tests/test_flash_gpu.py). The spiked keys make the logits ~4x those of
    the other fp32 tests, and the fp32 oracle rounds them to fp32 between its ops; where its own
    distance from float64 exceeds a tenth of a bound, that measured distance is added to the
    bound (the kernel is not asked to be closer to the oracle than the oracle is to the truth).
    Returns ({name: bound}, {name: oracle error}) for o, dq, dk, dv."""
    o, _, _, dq, dk, dv = ref
    scale = max(1.0, *(float(np.abs(g).max()) for g in (dq, dk, dv)))
    base = {"o": 1e-5, "dq": 2e-5 * scale, "dk": 2e-5 * scale, "dv": 2e-5 * scale}
    own = {n: float(np.abs(a - b).max()) for n, a, b in zip(("o", "dq", "dk", "dv"), (o, dq, dk, dv), r64)}
    return {n: base[n] + (own[n] if own[n] > 0.1 * base[n] else 0.0) for n in base}, own
