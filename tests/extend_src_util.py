"""Helpers shared by tests/test_extend_paged_gpu.py and tests/test_extend_kvq_gpu.py (test
infrastructure): the inputs of tests/extend_cases.py on the device, output buffers between sentinel
bands, and the byte comparison of (O, m, l)."""
import functools

import numpy as np

import extend_cases as EC

CODES = {"f32": 0, "bf16": 1, "bf16_f32o": 2}
SENT = 768.0  # exact in bf16
PAD = 64


@functools.lru_cache(maxsize=None)
def inputs(bf16, d, kv_heads, rows):
    """(q, k, v) of extend_cases.make_inputs for these rows, computed once, read-only."""
    q, k, v = EC.make_inputs(d, EC.NQ, bf16, rows, heads=EC.H, kv_heads=kv_heads)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def counts(torch, rows):
    """Device int32 (kv_len, q_len) of the rows, as given (unclamped)."""
    kv = torch.tensor([L for L, _ in rows], dtype=torch.int32, device="cuda")
    ql = torch.tensor([t for _, t in rows], dtype=torch.int32, device="cuda")
    return kv, ql


def bnhd(t):
    """The same [B,H,N,d] values on [B,N,H,d] storage."""
    return t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)


class Outputs:
    """O [B,H,Nq,d] (optionally on [B,Nq,H,d] storage), m and l [B,H,Nq], each inside a buffer with
    PAD sentinel elements on either side."""

    def __init__(self, torch, B, H, nq, d, tout, strided=False):
        self.torch, self.n = torch, (B * H * nq * d, B * H * nq, B * H * nq)
        self.obuf = torch.full((self.n[0] + 2 * PAD,), SENT, dtype=tout, device="cuda")
        o = self.obuf[PAD:PAD + self.n[0]].view((B, nq, H, d) if strided else (B, H, nq, d))
        self.o = o.permute(0, 2, 1, 3) if strided else o
        self.mbuf = torch.full((self.n[1] + 2 * PAD,), SENT, dtype=torch.float32, device="cuda")
        self.lbuf = torch.full((self.n[2] + 2 * PAD,), SENT, dtype=torch.float32, device="cuda")
        self.m = self.mbuf[PAD:PAD + self.n[1]].view(B, H, nq)
        self.l = self.lbuf[PAD:PAD + self.n[2]].view(B, H, nq)

    def check_bands(self):
        for buf, n in zip((self.obuf, self.mbuf, self.lbuf), self.n):
            assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all()), "wrote outside O / m / l"

    def check_all_written(self):
        """The contract writes every (b, h, query) row of O, m and l (a padding query gets (0, -inf, 0)),
        and no sentinel survives inside them."""
        for t in (self.o, self.m, self.l):
            assert not bool((t == SENT).any()), "a row of O / m / l was not written"

    def result(self):
        return self.o.contiguous(), self.m.clone(), self.l.clone()


def same_bits(torch, got, want, what):
    for x, y, nm in zip(got, want, "Oml"):
        assert x.dtype == y.dtype and x.shape == y.shape
        ity = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(x.contiguous().view(ity), y.contiguous().view(ity)), f"{nm} differs: {what}"


def all_finite_or_none(torch, res, rows, nq):
    """O and l finite everywhere; m finite for a query that sees a key and -inf for the others."""
    o, m, l = res
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(l).all())
    assert not bool(torch.isnan(m).any()) and not bool((m == float("inf")).any())
    for b, (L, t) in enumerate(rows):
        n, t = EC.visible(L), EC.real(t, nq)
        if n > 0 and t > 0:
            assert bool(torch.isfinite(m[b, :, t - 1]).all())
        assert bool((m[b, :, t:] == float("-inf")).all()) and not bool(l[b, :, t:].any())
