"""Key padding (kv_len) through every kernel family that takes it, at the key-block edges.

With kv_len set the bf16 MFMA fast paths are off and the call runs the generic / ring kernels
and the fused backwards (key padding: the (dtype, d, layout, policy) -> kernel
table). Every case here is the batch of tests/varlen_cases.py: N = 300, one batch row per
kv_len in {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 299, 300, 0}, the last
valid key and the padding keys x4, the padding values 64, so that a mask off by one key moves
an output by many times its bound (tests/test_varlen_edges.py shows that with the oracle alone).
H = 1 or 2 for the small grids, H = 19 (304 heads, ceil(300 / 256) x 304 = 608 >= 512) for the
paired / chip-filling forms. Forward then backward through _hip.flash_fwd / _hip.flash_bwd,
every head checked:

  * O, dQ, dK, dV against the C oracle; (m, l) through _check_ml;
  * dK = dV = 0 exactly past kv_len; the kv_len = 0 row O = 0, dQ = 0, m = -inf, l = 0;
  * the outputs are filled with NaN before the call (an element a kernel skips fails).

Tolerances: bf16 the elementwise bounds of tests/bounds.py; fp32 1e-5 max-abs on O and
2e-5 x max(1, max|ref|) on the gradients, plus the fp32 oracle's own measured distance from a
float64 reference where that exceeds a tenth of the bound (varlen_cases.fp32_bounds).
"""
import ctypes

import numpy as np
import pytest

import varlen_cases as VC
from test_flash_gpu import _check_ml, _use_policy

pytestmark = pytest.mark.gpu

N = VC.N
KV = VC.KV_LEN


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch


_INPUTS, _REFS = {}, {}


def _inputs(bf16, d, H, kv=KV):
    key = (bf16, d, H, kv)
    if key not in _INPUTS:
        _INPUTS[key] = VC.make_inputs(d, H, bf16, kv=kv)
    return _INPUTS[key]


def _reference(bf16, d, H, causal):
    """The oracle's (o, m, l, dq, dk, dv) and the case's bounds, computed once per case (the
    304-head cases are used by one test each and not kept)."""
    key = (bf16, d, H, causal)
    if key in _REFS:
        return _REFS[key]
    q, k, v, do = _inputs(bf16, d, H)
    ref = VC.oracle_c(q, k, v, do, causal, KV)
    if bf16:
        from oracle import cref
        p_abs = cref.attn_fwd(q, k, np.abs(v), causal, kv_len=KV)[0]
        bounds = VC.bf16_bounds_torch(q, k, v, do, causal, KV, p_abs, "cuda")
        own = None
    else:
        bounds, own = VC.fp32_bounds(ref, VC.ref64(q, k, v, do, causal, KV))
    if H <= 2:
        _REFS[key] = (ref, bounds, own)
    return ref, bounds, own


def _place(torch, shape, dtype, x=None, layout="bhnd", offset=0):
    """A device tensor seen as [B, H, N, d]: contiguous, or a permuted view of a [B, N, H, d]
    buffer (what minitorch's MHA hands over), its base `offset` elements into its allocation;
    filled with x, or with NaN (an output)."""
    B, H, n, d = shape
    flat = torch.full((B * H * n * d + offset,), float("nan"), dtype=dtype, device="cuda")
    t = flat[offset:].view((B, n, H, d) if layout == "bnhd" else shape)
    if layout == "bnhd":
        t = t.permute(0, 2, 1, 3)
    if x is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(x)).to("cuda").to(dtype))
    return t


def _run(torch, inputs, bf16, causal, kv=KV, layout="bhnd", offset=0, o_f32=False, bwd=True):
    """Forward (and backward) on the device; returns (o, m, l, dq, dk, dv) torch tensors."""
    from minitorch import _hip
    tdt = torch.bfloat16 if bf16 else torch.float32
    shape = inputs[0].shape
    tq, tk, tv, tdo = (_place(torch, shape, tdt, x, layout, offset) for x in inputs)
    o = _place(torch, shape, torch.float32 if o_f32 else tdt, None, layout, offset)
    m, l = (torch.full(shape[:3], float("nan"), device="cuda") for _ in range(2))
    _hip.flash_fwd(tq, tk, tv, causal, out=o, m=m, l=l, kv_len=kv)
    if not bwd:
        torch.cuda.synchronize()
        return o, m, l
    dq, dk, dv = (_place(torch, shape, tdt, None, layout, offset) for _ in range(3))
    _hip.flash_bwd(tq, tk, tv, o, tdo, m, l, causal, dq=dq, dk=dk, dv=dv, kv_len=kv)
    torch.cuda.synchronize()
    return o, m, l, dq, dk, dv


def _np(t):
    return t.float().cpu().numpy()


def _check_structure(o, m, l, dq, dk, dv, kv=KV):
    """What key padding fixes exactly: zero dK / dV past kv_len, and the row with no key."""
    for b, n in enumerate(kv):
        assert not dk[b, :, n:].any(), f"dK past kv_len = {n} is not zero"
        assert not dv[b, :, n:].any(), f"dV past kv_len = {n} is not zero"
        if n == 0:
            assert not o[b].any() and not dq[b].any(), "kv_len = 0: O / dQ not zero"
            assert np.isneginf(m[b]).all() and not l[b].any(), "kv_len = 0: (m, l) != (-inf, 0)"


def _check(got, bf16, d, H, causal, family, record, only=("o", "ml", "dq", "dk", "dv")):
    """Outputs (torch) of one case against its reference, every head; records the worst
    error / bound per output under `family`."""
    (o_ref, m_ref, l_ref, *g_ref), bounds, own = _reference(bf16, d, H, causal)
    o, m, l = (_np(t) for t in got[:3])
    grads = [_np(t) for t in got[3:]]
    if grads:
        _check_structure(o, m, l, *grads)
    live = [b for b, n in enumerate(KV) if n > 0]
    if "ml" in only:
        _check_ml(m[live], l[live], m_ref[live], l_ref[live], exact=not bf16)
    names = ("o", "dq", "dk", "dv")
    worst, fails = {}, []
    for name, x, ref in zip(names, [o] + grads, [o_ref] + g_ref):
        if name not in only:
            continue
        bnd = bounds[names.index(name)] if bf16 else bounds[name]
        err = np.abs(x - ref)  # NaN (an element never written) fails the comparison below
        ratio = err / bnd
        worst[name] = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("nan")
        bad = ~(ratio <= 1.0)
        if bad.any():
            b, h, i, j = (int(t) for t in np.argwhere(bad)[0])
            fails.append(f"{name}: {int(bad.sum())} elements over the bound, first at (b,h,n,c)=({b},{h},{i},{j}) "
                         f"kv_len {KV[b]}: |err| {err[b, h, i, j]:.3e}, worst error/bound {worst[name]:.3f}")
    print(f"{family} causal={causal}: error/bound " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items())
          + ("" if own is None else f"; fp32 oracle vs float64 {own}"), flush=True)
    rec = {f"{n}_err_over_bound": r for n, r in worst.items()}
    if own is not None:
        rec.update({f"{n}_bound": bounds[n] for n in worst}, **{f"{n}_oracle_vs_f64": own[n] for n in worst})
    record("test_varlen_matrix_gpu", f"{family} ({len(KV)},{H},{N},{d}) causal={causal}",
           bound="tests/bounds.py elementwise" if bf16 else "1e-5 (O), 2e-5 x max|ref| (grads) + oracle's own error",
           **rec)
    assert not fails, f"{family} causal={causal}: " + "; ".join(fails)


# (id, bf16, d, H, layout, offset): the kernels each case reaches are listed in DESIGN.md
MATRIX = [
    ("bf16-d128", True, 128, 2, "bhnd", 0),          # fa_fwd_generic<bf16,128,2>, dispatch_bwd<bf16,128,1,1>
    ("bf16-d128-grid304", True, 128, 19, "bhnd", 0),  # the same, the causal backward paired
    ("bf16-d96", True, 96, 2, "bhnd", 0),            # 64 < d < 128: the 128-wide generic kernels
    ("bf16-d64", True, 64, 2, "bhnd", 0),            # ring forward, fused backward (small grid)
    ("bf16-d64-grid304", True, 64, 19, "bhnd", 0),   # paired ring forward; fused R3 full grid / causal paired
    ("bf16-d48", True, 48, 2, "bhnd", 0),            # fa_fwd_generic_ring<bf16,64>, the bf16 ring backward
    ("bf16-d32", True, 32, 2, "bhnd", 0),            # fa_fwd_generic_ring<bf16,32>
    ("bf16-d32-grid304", True, 32, 19, "bhnd", 0),   # the 32-column ring forward and backward, paired
    ("bf16-d20", True, 20, 2, "bhnd", 0),            # d % 8 != 0: VEC = false generic
    ("bf16-d64-offset1", True, 64, 2, "bhnd", 1),    # misaligned base: VEC = false generic
    ("bf16-d64-bnhd", True, 64, 2, "bnhd", 0),       # permuted views, inputs and outputs
    ("fp32-d64", False, 64, 2, "bhnd", 0),           # X3 ring forward, split ring backward
    ("fp32-d64-grid304", False, 64, 19, "bhnd", 0),  # X3 ring paired; fused ring backward (causal: paired)
    ("fp32-d128", False, 128, 2, "bhnd", 0),         # fa_fwd_generic_ring<float,128,1>, dispatch_bwd<float,64,1,1> x 2 chunks
    ("fp32-d200", False, 200, 1, "bhnd", 0),         # fa_fwd_generic<float,128,1>, two d-chunks
    ("fp32-d20", False, 20, 2, "bhnd", 0),           # 16-B rows: the 32-column X3 ring, ring backward
    ("fp32-d20-grid304", False, 20, 19, "bhnd", 0),  # the same, paired
    ("fp32-d18", False, 18, 2, "bhnd", 0),           # d % 4 != 0: VEC = false generic
    ("fp32-d64-offset1", False, 64, 2, "bhnd", 1),   # misaligned base: VEC = false generic
    ("fp32-d64-bnhd", False, 64, 2, "bnhd", 0),      # permuted views
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("name,bf16,d,H,layout,offset", MATRIX, ids=[c[0] for c in MATRIX])
def test_varlen_edges_vs_oracle(torch_dev, name, bf16, d, H, layout, offset, causal, parity_record):
    got = _run(torch_dev, _inputs(bf16, d, H), bf16, causal, layout=layout, offset=offset)
    if layout == "bnhd":
        assert not got[0].is_contiguous() and not got[3].is_contiguous()
    if offset:
        assert got[0].data_ptr() % 16 and got[4].data_ptr() % 16
    _check(got, bf16, d, H, causal, name, parity_record)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("policy,H", [(121, 2), (1, 2), (121, 19)])
def test_varlen_edges_product_policies(torch_dev, policy, H, causal, parity_record):
    """bf16 d = 64 under the product library's other policies: 121 (split backward) keeps the
    ring forward and runs the generic backward dispatch_bwd<bf16,64,2,2> (the split bf16
    kernels have no key bound), on the 304-head grid its causal paired form; 1 (generic only)
    also the non-ring fa_fwd_generic<bf16,64,2>."""
    from minitorch import _hip
    try:
        _use_policy(_hip, policy)
        got = _run(torch_dev, _inputs(True, 64, H), True, causal)
    finally:
        _hip.set_policy(0)
    _check(got, True, 64, H, causal, f"bf16-d64-policy{policy}" + ("-grid304" if H > 2 else ""), parity_record)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_varlen_edges_fp32_out(torch_dev, d, causal, parity_record):
    """MT_BF16_F32OUT with kv_len (the f32o stores of fa_fwd_generic_ring at d = 64 and fa_fwd_generic
    at d = 128): the fp32 O within the bf16-O bound of the oracle, (m, l) as the bf16-O run's,
    and, the same kernel running either way, the fp32 O rounded to bf16 equal to the bf16 O."""
    torch = torch_dev
    inputs = _inputs(True, d, 2)
    o, m, l = _run(torch, inputs, True, causal, bwd=False)
    o32, m32, l32 = _run(torch, inputs, True, causal, o_f32=True, bwd=False)
    assert o32.dtype == torch.float32
    assert torch.equal(o32.to(torch.bfloat16), o)
    assert torch.equal(m32, m) and torch.equal(l32, l)
    b0 = KV.index(0)
    assert not o32[b0].any() and torch.isneginf(m32[b0]).all() and not l32[b0].any()
    _check((o32, m32, l32), True, d, 2, causal, f"bf16-d{d}-f32out", parity_record, only=("o", "ml"))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("bf16,d", [(True, 64), (False, 64), (True, 128)])
def test_varlen_kv_len_clamped(torch_dev, bf16, d, causal):
    """kv_len is clamped to [0, N] (fa_common.h kv_keys): N + 5 and 2^31 - 1 act as N, -1 and
    -2^31 as 0, to the bit, in every output."""
    torch = torch_dev
    kv_in = KV + (N, 0)
    kv_out = KV[:-2] + (N + 5, -1, 2 ** 31 - 1, -2 ** 31)
    assert [min(max(x, 0), N) for x in kv_out] == list(kv_in)
    inputs = _inputs(bf16, d, 2, kv_in)
    a = _run(torch, inputs, bf16, causal, kv=kv_in)
    b = _run(torch, inputs, bf16, causal, kv=kv_out)
    _check_structure(*(_np(t) for t in a), kv=kv_in)
    for x, y, name in zip(a, b, ("o", "m", "l", "dq", "dk", "dv")):
        assert not torch.isnan(x).any(), name
        assert torch.equal(x, y), f"{name} differs with out-of-range kv_len"


@pytest.mark.parametrize("causal", [False, True])
def test_varlen_legacy_bwd_entry(torch_dev, causal, parity_record):
    """mt_flash_attn_bwd_varlen (the entry without a workspace size, which _hip.flash_bwd no
    longer calls) on bf16 d = 64 with a workspace of mt_flash_attn_bwd_workspace_bytes.

    It cannot equal mt_flash_attn_bwd_v3 under the default policy to the bit: an unchecked
    caller may hold a workspace of the ABI-2 size, which has no room for the fused backward's
    arrival counters unless the heads run in several groups (a slab over 1 GiB), so at every
    size a test can afford the legacy entry runs the generic backward dispatch_bwd<bf16,64,2,2>
    where _v3 runs fa_bwd_fused_bf16 (capi_flash.hip, flash_attn_bwd_impl: slab_ok). The two
    entries are compared to the bit where they dispatch alike, under policy 121 (the split
    backward, which with kv_len is that generic backward), and the legacy entry's gradients
    under the default policy are held to the oracle like every other case."""
    from minitorch import _hip
    torch = torch_dev
    B, H, d = len(KV), 2, 64
    inputs = _inputs(True, d, H)
    tq, tk, tv, tdo = (_place(torch, inputs[0].shape, torch.bfloat16, x) for x in inputs)
    o, m, l = _hip.flash_fwd(tq, tk, tv, causal, kv_len=KV)
    kv = torch.tensor(KV, dtype=torch.int32, device="cuda")
    lib = _hip.lib()
    ws = torch.empty(lib.mt_flash_attn_bwd_workspace_bytes(B, H, N, d) // 4, dtype=torch.float32, device="cuda")

    def legacy():
        grads = [_place(torch, inputs[0].shape, torch.bfloat16) for _ in range(3)]
        strides = (ctypes.c_int64 * 24)()
        for i, t in enumerate((tq, tk, tv, o, tdo, *grads)):
            strides[3 * i:3 * i + 3] = list(_hip.strides3(t))
        _hip.check(lib.mt_flash_attn_bwd_varlen(
            _hip.MT_BF16, int(causal), tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), o.data_ptr(), tdo.data_ptr(),
            m.data_ptr(), l.data_ptr(), *(g.data_ptr() for g in grads), B, H, N, d, strides, kv.data_ptr(),
            ws.data_ptr(), _hip.stream_ptr(tq.device)), "mt_flash_attn_bwd_varlen")
        torch.cuda.synchronize()
        return grads

    try:
        _use_policy(_hip, 121)
        old = legacy()
        new = _hip.flash_bwd(tq, tk, tv, o, tdo, m, l, causal, kv_len=KV)
        torch.cuda.synchronize()
    finally:
        _hip.set_policy(0)
    for x, y, name in zip(old, new, ("dq", "dk", "dv")):
        assert torch.equal(x, y), f"{name}: the legacy entry and _v3 differ under policy 121"
    _check((o, m, l, *legacy()), True, d, H, causal, "bf16-d64-legacy-entry", parity_record)


def test_varlen_bf16_bwd_fused_head_groups(torch_dev, parity_record):
    """kv_len with the fused backward's head groups (bh0 + bhl in fa_bwd_dq_reduce, one launch
    per group): the shape of test_bf16_bwd_fused_head_groups, (2,72,4096,64) non-causal, two
    launches (heads 0-127, 128-143) over one slab, kv_len = (4096, 1000); the same four heads,
    on both sides of the seam, against the C oracle under the bounds of tests/bounds.py taken
    with kv_len, and zero dK / dV past 1000 on every head of the second row."""
    from bounds import grad_bounds
    from minitorch import _hip
    from oracle import cref
    torch = torch_dev
    kv = (4096, 1000)
    g = torch.Generator(device="cuda").manual_seed(72 + 2)
    q, k, v, do = (torch.randn((2, 72, 4096, 64), device="cuda", generator=g).to(torch.bfloat16)
                   for _ in range(4))
    o, m, l = _hip.flash_fwd(q, k, v, False, kv_len=kv)
    dq, dk, dv = _hip.flash_bwd(q, k, v, o, do, m, l, False, kv_len=kv)
    torch.cuda.synchronize()
    for b, n in enumerate(kv):
        assert not dk[b, :, n:].any() and not dv[b, :, n:].any()
    heads = [(0, 0), (1, 55), (1, 56), (1, 71)]
    kvh = [kv[b] for b, _ in heads]
    qs, ks, vs, dos = (np.stack([_np(t[b, h]) for (b, h) in heads]) for t in (q, k, v, do))
    _, m_ref, l_ref = cref.attn_fwd(qs, ks, vs, False, kv_len=kvh)
    g_ref = cref.attn_bwd(qs, ks, vs, dos, m_ref, l_ref, False, kv_len=kvh)
    worst = {}
    for x, (b, h) in enumerate(heads):
        bnds = grad_bounds(qs[x], ks[x], vs[x], dos[x], False, kv=kv[b])
        for got, ref, bnd, name in zip((dq, dk, dv), g_ref, bnds, ("dq", "dk", "dv")):
            ratio = float((np.abs(_np(got[b, h]) - ref[x]) / bnd).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ratio <= 1.0, f"{name} (b,h)=({b},{h}) worst error/bound {ratio:.3f}"
    parity_record("test_varlen_bf16_bwd_fused_head_groups", "(2,72,4096,64) kv=(4096,1000) non-causal",
                  bound="tests/bounds.py", **{f"{n}_err_over_bound": r for n, r in worst.items()})
