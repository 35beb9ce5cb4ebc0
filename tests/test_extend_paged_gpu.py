"""Extend attention on a paged cache read in place (csrc/fa_extend.hip on ExtPagedSrc, through
mt_flash_attn_extend_paged) on the GPU.

The yardstick is exact: mt_flash_attn_extend on the contiguous cache that holds the same rows must
give the same bytes of O, m and l, so parity with the float64 oracle is inherited from
tests/test_extend_gpu.py. Inputs and ragged rows: tests/extend_cases.py (H = 2, a cache of 448
rows, 168 new queries, the rows of gpu_rows(bq, bk) on the block and tile edges of the library's own
plan). A pool holds more pages than the tables use, and the tables are one shuffled permutation of
them; P = 16 is below every key tile (32 / 64), P = 64 at or above it."""
import numpy as np
import pytest

import extend_cases as EC
import extend_src_util as U

pytestmark = pytest.mark.gpu

CASES = [("f32", d) for d in (16, 64, 68, 128, 256)] + [("bf16", d) for d in (32, 64, 128, 256)] + [("bf16_f32o", 64)]
IDS = [f"{n}-d{d}" for n, d in CASES]
SPARE = 5  # pool pages no table names


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from minitorch import _hip
    _hip.lib()
    return torch, _hip


def _rows(_hip, name, d, P, kv_heads):
    kid, bq, bk = _hip.extend_paged_plan(U.CODES[name], 27, EC.H, EC.NQ, EC.NMAX // P, P, d, Hkv=kv_heads)
    assert (kid, bq, bk) == _hip.extend_plan(U.CODES[name], 27, EC.H, EC.NQ, EC.NMAX, d, Hkv=kv_heads)
    return EC.gpu_rows(bq, bk)


def _dtypes(torch, name):
    return (torch.float32 if name == "f32" else torch.bfloat16), (torch.bfloat16 if name == "bf16" else torch.float32)


def _pools(torch, tk, tv, P, seed, strided=False, fill=None):
    """Page pools holding the rows of the contiguous caches tk / tv [B,Hkv,Nmax,d] behind a shuffled
    table: (k_pool, v_pool [n_pages,Hkv,P,d], table int32 [B,W], used-page mask). strided: the pools
    on [n_pages,P,Hkv,d] storage. fill: the value of the pages no table names."""
    B, Hkv, nmax, d = tk.shape
    W = nmax // P
    assert W * P == nmax
    n_pages = B * W + SPARE
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_pages, generator=g)
    table = perm[:B * W].view(B, W).to(torch.int32)
    assert not torch.equal(table.flatten(), torch.arange(B * W, dtype=torch.int32))
    pools = []
    for t in (tk, tv):
        pool = torch.zeros((n_pages, P, Hkv, d) if strided else (n_pages, Hkv, P, d), dtype=t.dtype, device="cuda")
        if strided:
            pool = pool.permute(0, 2, 1, 3)
        if fill is not None:
            pool.fill_(fill)
        # [B,Hkv,W,P,d] -> [B*W,Hkv,P,d], scattered to the table's pages
        src = t.reshape(B, Hkv, W, P, d).permute(0, 2, 1, 3, 4).reshape(B * W, Hkv, P, d)
        pool[table.flatten().long().cuda()] = src
        pools.append(pool)
    return pools[0], pools[1], table.cuda()


def _plain(hip, name, tq, tk, tv, rows, causal):
    torch, _hip = hip
    kv, ql = U.counts(torch, rows)
    B, H, nq, d = tq.shape
    out = U.Outputs(torch, B, H, nq, d, _dtypes(torch, name)[1])
    _hip.flash_extend(tq, tk, tv, kv_len=kv, q_len=ql, causal=causal, out=out.o, m=out.m, l=out.l)
    torch.cuda.synchronize()
    return out.result()


def _paged(hip, name, tq, kp, vp, table, rows, causal, strided_o=False, footprint=False):
    torch, _hip = hip
    kv, ql = U.counts(torch, rows)
    B, H, nq, d = tq.shape
    out = U.Outputs(torch, B, H, nq, d, _dtypes(torch, name)[1], strided=strided_o)
    before = [t.clone() for t in (tq, kp, vp, table)]
    _hip.flash_extend_paged(tq, kp, vp, table, kv_len=kv, q_len=ql, causal=causal, out=out.o, m=out.m, l=out.l)
    torch.cuda.synchronize()
    if footprint:
        out.check_bands()
        out.check_all_written()
        for t, t0 in zip((tq, kp, vp, table), before):
            ity = {2: torch.int16, 4: torch.int32}[t.element_size()]
            assert torch.equal(t.contiguous().view(ity), t0.contiguous().view(ity)), "inputs changed"
    return out.result()


def _device_inputs(torch, name, d, kv_heads, rows):
    tin = _dtypes(torch, name)[0]
    return tuple(torch.from_numpy(np.array(a)).cuda().to(tin) for a in U.inputs(name != "f32", d, kv_heads, rows))


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("kv_heads", [EC.H, 1], ids=["mha", "hkv1"])
@pytest.mark.parametrize("P", [16, 64])
@pytest.mark.parametrize("name,d", CASES, ids=IDS)
def test_bits_of_the_plain_kernel_and_stale_content(hip, name, d, P, kv_heads, causal):
    """O, m and l are byte-equal to mt_flash_attn_extend on the contiguous cache. Then the same call
    with NaN in every pool page no table entry below ceil(n / P) names and in the rows >= n of a
    row's last page, and -1 in the table entries at index >= ceil(n / P): the same bytes, all finite."""
    torch, _hip = hip
    rows = _rows(_hip, name, d, P, kv_heads)
    tq, tk, tv = _device_inputs(torch, name, d, kv_heads, rows)
    want = _plain(hip, name, tq, tk, tv, rows, causal)
    kp, vp, table = _pools(torch, tk, tv, P, seed=d + P)
    got = _paged(hip, name, tq, kp, vp, table, rows, causal, footprint=True)
    U.same_bits(torch, got, want, "paged against the contiguous cache")

    nk, nv = tk.clone(), tv.clone()
    ntable = table.clone()
    for b, (L, _) in enumerate(rows):
        n = EC.visible(L)
        nk[b, :, n:] = float("nan")
        nv[b, :, n:] = float("nan")
        ntable[b, -(-n // P):] = -1
    kp2, vp2, table2 = _pools(torch, nk, nv, P, seed=d + P, fill=float("nan"))
    assert torch.equal(table2, table)
    stale = _paged(hip, name, tq, kp2, vp2, ntable, rows, causal, footprint=True)
    U.all_finite_or_none(torch, stale, rows, EC.NQ)
    U.same_bits(torch, stale, want, "NaN in the stale pages and rows, -1 past the row's pages")


@pytest.mark.parametrize("name,d,P", [("f32", 64, 16), ("f32", 128, 64), ("bf16", 128, 16)])
def test_shared_prefix_pages(hip, name, d, P):
    """Two batch rows whose tables name the same pages for a common prefix give the bits of two
    private copies of it."""
    torch, _hip = hip
    _, bq, bk = _hip.extend_paged_plan(U.CODES[name], 2, EC.H, EC.NQ, EC.NMAX // P, P, d)
    shared = 2 * P + 2 * 64  # whole pages, past the first key tiles
    assert shared % P == 0 and shared + bq + 1 <= EC.NMAX
    rows = ((shared + 37, 37), (shared + bq + 1, bq + 1))
    tq, tk, tv = _device_inputs(torch, name, d, EC.H, rows)
    tk, tv = tk.clone(), tv.clone()
    tk[1, :, :shared] = tk[0, :, :shared]
    tv[1, :, :shared] = tv[0, :, :shared]
    want = _plain(hip, name, tq, tk, tv, rows, True)
    kp, vp, table = _pools(torch, tk, tv, P, seed=3, fill=float("nan"))
    private = _paged(hip, name, tq, kp, vp, table, rows, True)
    # row 1 reads row 0's pages for the prefix; its own copies of them become stale
    for pool in (kp, vp):
        pool[table[1, :shared // P].long()] = float("nan")
    table[1, :shared // P] = table[0, :shared // P]
    both = _paged(hip, name, tq, kp, vp, table, rows, True, footprint=True)
    U.same_bits(torch, private, want, "private pages against the contiguous cache")
    U.same_bits(torch, both, private, "shared prefix pages against private copies")


@pytest.mark.parametrize("name,d,P,kv_heads", [("f32", 64, 16, 2), ("f32", 256, 64, 1), ("bf16", 64, 16, 1),
                                               ("bf16_f32o", 64, 64, 2)])
def test_footprint_with_strided_layouts(hip, name, d, P, kv_heads):
    """Q and O on [B,Nq,H,d] storage and the pools on [n_pages,P,Hkv,d] storage: the same bytes,
    nothing written outside O, m and l, the inputs untouched."""
    torch, _hip = hip
    rows = _rows(_hip, name, d, P, kv_heads)
    tq, tk, tv = _device_inputs(torch, name, d, kv_heads, rows)
    kp, vp, table = _pools(torch, tk, tv, P, seed=1)
    dense = _paged(hip, name, tq, kp, vp, table, rows, True, footprint=True)
    kps, vps, table_s = _pools(torch, tk, tv, P, seed=1, strided=True)
    assert (kv_heads == 1 or not kps.is_contiguous()) and torch.equal(table_s, table)
    strided = _paged(hip, name, U.bnhd(tq), kps, vps, table, rows, True, strided_o=True, footprint=True)
    U.same_bits(torch, strided, dense, "strided q / o / pools")


def test_graph_replay_with_changing_lengths_and_table(hip):
    """append + extend captured once, replayed after kv_len, q_len and the table were rewritten in
    place: each replay is bit-equal to the eager call on the same state."""
    torch, _hip = hip
    B, H, nq, d, P = 3, 2, EC.NQ, 64, 16
    W = EC.NMAX // P
    _, bq, bk = _hip.extend_paged_plan(0, B, H, nq, W, P, d)
    n_pages = B * W + SPARE
    g = torch.Generator().manual_seed(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rng = np.random.default_rng(12)
    kp, vp = (dev(rng.standard_normal((n_pages, H, P, d)).astype(np.float32)) for _ in range(2))
    T = np.array([[bq - 1, 5, 0], [bq, 5, nq], [bq + 1, 5, 1]], np.int32)             # real new tokens
    N = np.array([[bq + 9, bk - 1, 50], [bq + 10, bk, 300], [bq + 11, bk + 1, 1]], np.int32)  # keys held after
    tables = [torch.randperm(n_pages, generator=g)[:B * W].view(B, W).to(torch.int32).cuda() for _ in range(3)]
    steps = [[dev(rng.standard_normal((B, H, nq, d)).astype(np.float32)) for _ in range(3)] for _ in range(3)]
    q, kn, vn = (torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda") for _ in range(3))
    pos, kvl, qln = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    table = tables[0].clone()
    o = torch.empty((B, H, nq, d), dtype=torch.float32, device="cuda")
    m, l = (torch.empty((B, H, nq), dtype=torch.float32, device="cuda") for _ in range(2))
    kp_e, vp_e = kp.clone(), vp.clone()  # the eager leg's pools

    def step():
        _hip.kv_cache_append_paged(kn, vn, kp, vp, table, pos, qln)
        _hip.flash_extend_paged(q, kp, vp, table, kv_len=kvl, q_len=qln, causal=True, out=o, m=m, l=l)

    def load(i):
        for dst, src in zip((q, kn, vn), steps[i]):
            dst.copy_(src)
        pos.copy_(dev(N[i] - T[i]))
        kvl.copy_(dev(N[i]))
        qln.copy_(dev(T[i]))
        table.copy_(tables[i])
    side = torch.cuda.Stream()
    load(0)
    kp0, vp0 = kp.clone(), vp.clone()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kp.copy_(kp0)
    vp.copy_(vp0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for i in range(3):
        load(i)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in (o, m, l)]
        _hip.kv_cache_append_paged(steps[i][1], steps[i][2], kp_e, vp_e, tables[i], dev(N[i] - T[i]), dev(T[i]))
        ref = _hip.flash_extend_paged(steps[i][0], kp_e, vp_e, tables[i], kv_len=dev(N[i]), q_len=dev(T[i]), causal=True)
        torch.cuda.synchronize()
        U.same_bits(torch, got, ref, f"replay {i} against the eager call")
        assert bool((got[2][0, :, :int(T[i][0])] > 0).all()) and not bool(got[2][0, :, int(T[i][0]):].any())
        assert torch.equal(kp.view(torch.int32), kp_e.view(torch.int32))
        assert torch.equal(vp.view(torch.int32), vp_e.view(torch.int32))
