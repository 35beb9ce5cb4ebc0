"""Extend attention on a quantised cache read in place (csrc/fa_extend.hip on ExtKvqSrc, through
mt_flash_attn_extend_kvq) on the GPU.

The yardstick is exact: mt_kv_cache_dequant followed by mt_flash_attn_extend(MT_F32) on the fp32
copy must give the same bytes of O, m and l, because the kernel stages the same fp32 values in its
ring. Inputs and ragged rows: tests/extend_cases.py (H = 2, a cache of 448 rows, 168 new queries,
the rows of gpu_rows(bq, bk) of the fp32 plan), quantised by mt_kv_cache_append_quant."""
import numpy as np
import pytest

import extend_cases as EC
import extend_src_util as U

pytestmark = pytest.mark.gpu

KV = {"bf16": 1, "fp8": 2}
DS = (32, 64, 72, 128, 256)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def _rows(_hip, kv, d, kv_heads):
    kid, bq, bk = _hip.extend_kvq_plan(KV[kv], 27, EC.H, EC.NQ, EC.NMAX, d, Hkv=kv_heads)
    assert (kid, bq, bk) == _hip.extend_plan(0, 27, EC.H, EC.NQ, EC.NMAX, d, Hkv=kv_heads)
    return EC.gpu_rows(bq, bk)


def _quantise(hip, kv, tk, tv, strided=False):
    """Caches [B,Hkv,N,d] (on [B,N,Hkv,d] storage when strided) and fp8 scales holding the rows of
    the fp32 tk / tv, written by one mt_kv_cache_append_quant of all N rows at row 0."""
    torch, _hip = hip
    B, Hkv, N, d = tk.shape
    dt = torch.bfloat16 if kv == "bf16" else torch.uint8

    def one():
        t = torch.zeros((B, N, Hkv, d) if strided else (B, Hkv, N, d), dtype=dt, device="cuda")
        return t.permute(0, 2, 1, 3) if strided else t
    kc, vc = one(), one()
    ks = vs = None
    if kv == "fp8":
        ks, vs = (torch.zeros((B, Hkv, N), dtype=torch.float32, device="cuda") for _ in range(2))
    _hip.kv_cache_append_quant(tk, tv, kc, vc, torch.zeros(B, dtype=torch.int32, device="cuda"), ks, vs)
    torch.cuda.synchronize()
    return kc, vc, ks, vs


def _two_launches(hip, tq, caches, rows, causal):
    """The yardstick: dequantise the visible rows into an fp32 pair, then the plain fp32 kernel."""
    torch, _hip = hip
    kv, ql = U.counts(torch, rows)
    kc, vc, ks, vs = caches
    B, H, nq, d = tq.shape
    kf, vf = (torch.full(tuple(kc.shape), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    _hip.kv_cache_dequant(kc, vc, ks, vs, kv_len=kv, k_out=kf, v_out=vf)
    out = U.Outputs(torch, B, H, nq, d, torch.float32)
    _hip.flash_extend(tq, kf, vf, kv_len=kv, q_len=ql, causal=causal, out=out.o, m=out.m, l=out.l)
    torch.cuda.synchronize()
    return out.result()


def _direct(hip, tq, caches, rows, causal, strided_o=False, footprint=False):
    torch, _hip = hip
    kv, ql = U.counts(torch, rows)
    kc, vc, ks, vs = caches
    B, H, nq, d = tq.shape
    out = U.Outputs(torch, B, H, nq, d, torch.float32, strided=strided_o)
    ins = [t for t in (tq, kc, vc, ks, vs) if t is not None]
    before = [t.clone() for t in ins]
    _hip.flash_extend_kvq(tq, kc, vc, ks, vs, kv_len=kv, q_len=ql, causal=causal, out=out.o, m=out.m, l=out.l)
    torch.cuda.synchronize()
    if footprint:
        out.check_bands()
        out.check_all_written()
        for t, t0 in zip(ins, before):
            ity = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
            assert torch.equal(t.contiguous().view(ity), t0.contiguous().view(ity)), "inputs changed"
    return out.result()


def _device_inputs(torch, d, kv_heads, rows):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in U.inputs(False, d, kv_heads, rows))


def _poison_tail(torch, kv, caches, rows):
    """Copies of the caches with NaN patterns in every code and scale of a row >= n."""
    kc, vc, ks, vs = (None if t is None else t.clone() for t in caches)
    for b, (L, _) in enumerate(rows):
        n = EC.visible(L)
        for c in (kc, vc):
            if kv == "bf16":
                c[b, :, n:] = float("nan")
            else:
                c[b, :, n:] = 0x7F
        for s in (ks, vs):
            if s is not None:
                s[b, :, n:] = float("nan")
    return kc, vc, ks, vs


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("kv_heads", [EC.H, 1], ids=["mha", "hkv1"])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_bits_of_dequant_then_extend_and_stale_tail(hip, kv, d, kv_heads, causal):
    """O, m and l are byte-equal to mt_kv_cache_dequant followed by mt_flash_attn_extend(MT_F32). Then
    the same call with NaN patterns in the codes and scales of every row >= n: the same bytes, finite."""
    torch, _hip = hip
    rows = _rows(_hip, kv, d, kv_heads)
    tq, tk, tv = _device_inputs(torch, d, kv_heads, rows)
    caches = _quantise(hip, kv, tk, tv)
    want = _two_launches(hip, tq, caches, rows, causal)
    got = _direct(hip, tq, caches, rows, causal, footprint=True)
    U.same_bits(torch, got, want, "direct against dequant + extend")
    stale = _direct(hip, tq, _poison_tail(torch, kv, caches, rows), rows, causal, footprint=True)
    U.all_finite_or_none(torch, stale, rows, EC.NQ)
    U.same_bits(torch, stale, want, "NaN codes and scales in the rows >= n")


@pytest.mark.parametrize("kv,d,kv_heads", [("bf16", 64, 2), ("fp8", 64, 1), ("fp8", 256, 2), ("bf16", 32, 1)])
def test_footprint_with_strided_layouts(hip, kv, d, kv_heads):
    """Q and O on [B,Nq,H,d] storage and the caches on [B,N,Hkv,d] storage: the same bytes, nothing
    written outside O, m and l, the inputs untouched."""
    torch, _hip = hip
    rows = _rows(_hip, kv, d, kv_heads)
    tq, tk, tv = _device_inputs(torch, d, kv_heads, rows)
    dense = _direct(hip, tq, _quantise(hip, kv, tk, tv), rows, True, footprint=True)
    caches = _quantise(hip, kv, tk, tv, strided=True)
    assert kv_heads == 1 or not caches[0].is_contiguous()
    strided = _direct(hip, U.bnhd(tq), caches, rows, True, strided_o=True, footprint=True)
    U.same_bits(torch, strided, dense, "strided q / o / caches")


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_graph_replay_with_changing_lengths(hip, kv):
    """append_quant + extend captured once, replayed after kv_len and q_len were rewritten in place:
    each replay is bit-equal to the eager call on the same state."""
    torch, _hip = hip
    B, H, nq, d, nmax = 3, 2, EC.NQ, 64, EC.NMAX
    _, bq, bk = _hip.extend_kvq_plan(KV[kv], B, H, nq, nmax, d)
    rng = np.random.default_rng(13)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    base = [dev(rng.standard_normal((B, H, nmax, d)).astype(np.float32)) for _ in range(2)]
    kc, vc, ks, vs = _quantise(hip, kv, *base, strided=True)
    T = np.array([[bq - 1, 5, 0], [bq, 5, nq], [bq + 1, 5, 1]], np.int32)             # real new tokens
    N = np.array([[bq + 9, bk - 1, 50], [bq + 10, bk, 300], [bq + 11, bk + 1, 1]], np.int32)  # keys held after
    steps = [[dev(rng.standard_normal((B, H, nq, d)).astype(np.float32)) for _ in range(3)] for _ in range(3)]
    q, kn, vn = (torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda") for _ in range(3))
    pos, kvl, qln = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    o = torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda")
    m, l = (torch.empty((B, H, nq), dtype=torch.float32, device="cuda") for _ in range(2))
    eager = [None if t is None else t.clone() for t in (kc, vc, ks, vs)]  # clone keeps the strides

    def step():
        _hip.kv_cache_append_quant(kn, vn, kc, vc, pos, ks, vs)
        _hip.flash_extend_kvq(q, kc, vc, ks, vs, kv_len=kvl, q_len=qln, causal=True, out=o, m=m, l=l)

    def load(i):
        for dst, src in zip((q, kn, vn), steps[i]):
            dst.copy_(src)
        pos.copy_(dev(N[i] - T[i]))
        kvl.copy_(dev(N[i]))
        qln.copy_(dev(T[i]))
    side = torch.cuda.Stream()
    load(0)
    saved = [None if t is None else t.clone() for t in (kc, vc, ks, vs)]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, t0 in zip((kc, vc, ks, vs), saved):
        if t is not None:
            t.copy_(t0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in range(3):
        load(i)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in (o, m, l)]
        _hip.kv_cache_append_quant(steps[i][1], steps[i][2], eager[0], eager[1], dev(N[i] - T[i]), eager[2], eager[3])
        ref = _hip.flash_extend_kvq(steps[i][0], *eager, kv_len=dev(N[i]), q_len=dev(T[i]), causal=True)
        torch.cuda.synchronize()
        U.same_bits(torch, got, ref, f"replay {i} against the eager call")
        assert bool((got[2][0, :, :int(T[i][0])] > 0).all()) and not bool(got[2][0, :, int(T[i][0]):].any())
