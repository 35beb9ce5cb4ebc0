"""The default dispatch (no kv_len, policy 0) on tensors that are not contiguous [B,H,N,d]
allocations of their own, with the write footprint of every kernel checked.

Every tensor of a call is placed by tests/flash_layouts.py: permuted [B,N,H,d] views, slices of
a larger parent (row pad, foreign rows and heads around the view, a base aligned to 16 bytes
only), the fused-QKV packing, and three mixes that give the eight tensors of a call different
strides. Inputs are N(0,1) (rounded to bf16 for the bf16 cases), NaN around the views; outputs
are NaN inside the views and a sentinel around them; (m, l) and the backward workspace (exactly
mt_flash_attn_bwd_workspace_bytes) lie between guard bands. Forward then backward through
_hip.flash_fwd / _hip.flash_bwd, and on every test:

  * values, every head: O, dQ, dK, dV against the C oracle under the project's bounds (bf16:
    tests/bounds.py, 1e-3 + 2^-7 (P|V|) on O, 2^-8 on an fp32 O; fp32: varlen_cases.fp32_bounds),
    (m, l) through _check_ml;
  * footprint: no NaN left in any output view, the sentinel intact around every output, around
    m, l and the workspace, every input parent (and O, m, l across the backward) unchanged;
  * layout independence: every output equal to the bit to the contiguous run of the same case
    (strides change addresses, not arithmetic).

tests/test_flash_layouts.py shows on the CPU that each of these checks can fail. The kernels
each case reaches: the comments of CASES (thresholds from capi_flash.hip fwd_bf16_dispatch /
flash_attn_bwd_impl, fa_bwd_fused.hip launch_bwd_fused, fa_bwd_d128.hip launch_bwd_d128_passes),
DESIGN.md and profiles/flash_layouts_kernels.txt.
"""
from collections import OrderedDict

import numpy as np
import pytest

import flash_layouts as FL
import varlen_cases as VC
from test_flash_gpu import _check_ml, _use_policy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch


# id: (bf16, (B, H, N, d)). bh = B*H; non-causal / causal forward, then the backward.
CASES = OrderedDict([
    # d = 64, bh = 2, N < 128: v6 declines (N < 2 kBK) -> v4 / v4 paired (pair = 2). Backward: slab -> variant 20,
    # fused; nkb = 1 partial key block, N % 64 != 0 -> <false,false,R3>; causal (1+1)/2*2 < 256 -> unpaired
    ("a", (True, (1, 2, 100, 64))),
    # N % 64 != 0, ceil(N/512)*bh = 2 < 256 and <18> declines a ragged N -> v4 both ways; fused R3, nkb = 2
    ("b", (True, (1, 2, 333, 64))),
    # N % 128 == 0, ceil(N/256)*bh = 4 < 512, ceil(N/512)*bh = 2 < 256 -> v6 split-key <18>; causal
    # w4grid = 2 < 256 -> v4 paired. Backward: N % 64 == 0 -> <false,false,Rot>; causal unpaired
    ("c", (True, (1, 2, 512, 64))),
    # bh = 256: ceil(N/256)*bh = 256 < 512, ceil(N/512)*bh = 256 >= 256 -> 8-wave <66>; causal w4grid =
    # (1+1)/2*256 = 256 -> <16482>, one 256-query block. Backward: Rot; causal (nkb+1)/2*256 >= 256 -> paired, nkb = 1
    ("d", (True, (2, 128, 192, 64))),
    # ceil(N/256)*bh = 512 -> W4 <16450>; causal <16482>, nqb = 2: one light / heavy pair. Backward: Rot;
    # causal paired (nkb = 2, one pair) + fa_bwd_dq_reduce
    ("e", (True, (2, 128, 512, 64))),
    # N % 64 = 1: ceil(N/512)*bh = 512 >= 256 -> <66|65536> = <65602>; causal w4grid = (3+1)/2*256 -> <82018>.
    # Backward: R3 ragged, nkb = 3; causal paired, the middle block alone
    ("f", (True, (2, 128, 577, 64))),
    # d = 128, N < 128: d128v2 declines -> fa_fwd_d128 (8 waves; causal paired). Backward: nbh = 1 partial block,
    # 4-wave dQ (nbh8*bh = 2 < 256), unpaired
    ("g", (True, (1, 2, 100, 128))),
    # N % 64 == 0, N >= 128 -> d128v2 <8,0> / <8,32>; backward the 4-wave passes, nbh = 2
    ("h", (True, (1, 2, 256, 128))),
    # ragged N -> fa_fwd_d128; backward with a ragged last block (nbh = 3)
    ("i", (True, (1, 2, 333, 128))),
    # bh = 128, ragged -> fa_fwd_d128. Backward: nbh8*bh = 2*128 >= 256 -> dQ 8-wave (<1,false,false,true,0,3,8,true>);
    # causal (nbh+1)/2*bh = 2*128 -> dK/dV paired, (nbh8+1)/2*bh = 128 < 256 -> dQ 4-wave paired
    ("j", (True, (2, 64, 300, 128))),
    # bh = 256, N % 64 == 0 -> d128v2; causal (nbh8+1)/2*bh = 256 -> dQ 8-wave paired (<1,true,true,true,0,2,8,true>)
    ("k", (True, (2, 128, 320, 128))),
    # pad_dim: 48 -> 64 (v4 / fused on the padded copies), 96 -> 128 (fa_fwd_d128 / d128 passes): pad_rows and
    # unpad_rows read and write with the caller's strides
    ("l48", (True, (2, 3, 333, 48))),
    ("l96", (True, (2, 3, 333, 96))),
    # d % 8 != 0: no 16-B rows, the generic kernels without vectors
    ("m20", (True, (1, 2, 100, 20))),
    # d = 32: no bf16 MFMA kernel -> the 32-column ring forward, the ring backward
    ("m32", (True, (1, 2, 300, 32))),
    # fp32 d = 64: the X3 ring forward; the split ring backward (fa_bwd_dkv_ring / fa_bwd_dq_ring), the fused
    # pass needing ceil(N/256)*bh >= 256 (fa_bwd.hip launch_bwd_generic)
    ("n2", (False, (1, 2, 300, 64))),
    # 304 heads (ceil(300/256)*304 = 608 >= 512): the paired X3 ring, the fused ring backward (causal paired)
    ("n304", (False, (16, 19, 300, 64))),
    # fp32 d = 200: the generic kernels in two d-chunks (a chunk overrun lands in the slice's row pad)
    ("o", (False, (1, 1, 130, 200))),
])
# every case runs every layout (bhnd is the control each is compared with): the 128- to 304-head
# cases take about a second each, every head checked
LAYOUTS = ("bnhd", "slice", "packed", "mixedA", "mixedB", "mixedC")
MATRIX = [(c, causal, lay) for c in CASES for causal in (False, True) for lay in LAYOUTS]
# bf16 inputs, fp32 O (MT_BF16_F32OUT), forward only
F32OUT = [
    ("e", True),    # w8grid = (1+1)/2*256 >= 256, N % 64 == 0 -> the fp16-PV form <610>
    ("e", False),   # <16450>, the p.o_f32 stores
    ("f", False),   # <65602>, the p.o_f32 stores
    ("f", True),    # ragged: no <610> -> v4
    ("g", False), ("g", True),  # d128v2 declines N < 128, fa_fwd_d128 an fp32 O -> fa_fwd_fast<128>
    ("i", False), ("i", True),  # the same, ragged
    ("h", False), ("h", True),  # d128v2
]
# (case, policy): 121 the split bf16 backward (dK/dV variant 5 non-causal; causal 0 at c, 18 at e where
# ceil(N/256)*bh = 512; and its dQ kernels), 1 the generic kernels only
POLICIES = [("c", 121), ("e", 121), ("b", 1)]
OTHER_LAYOUTS = ("slice", "mixedA")

_REF = OrderedDict()    # (case, causal) -> reference (the two latest)
_BASE = OrderedDict()   # (case, causal, o_f32, policy) -> the contiguous run's outputs (the two latest)


def _cached(store, key, make, keep=2):
    if key not in store:
        while len(store) >= keep:
            store.popitem(last=False)
        store[key] = make()
    return store[key]


def _inputs(case):
    bf16, shape = CASES[case]
    rng = np.random.default_rng([20, list(CASES).index(case), *shape])
    xs = [rng.standard_normal(shape).astype(np.float32) for _ in range(4)]
    return [VC.A.bf16_round(x) for x in xs] if bf16 else xs


def _reference(torch, case, causal):
    """Inputs, the C oracle's outputs on every head and the case's bounds, once per (case, causal)."""
    def make():
        from bounds import R_BF16, grad_bounds_torch
        from oracle import cref
        bf16, shape = CASES[case]
        B, H, N, d = shape
        q, k, v, do = inputs = _inputs(case)
        o, m, l = cref.attn_fwd(q, k, v, causal)
        ref = (o, m, l) + tuple(cref.attn_bwd(q, k, v, do, m, l, causal))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
        out = {"inputs": inputs, "m": m, "l": l,
               "ref": {n: dev(a) for n, a in zip(("o", "dq", "dk", "dv"), (o,) + ref[3:])}}
        if bf16:
            pabs = dev(cref.attn_fwd(q, k, np.abs(v), causal)[0]).double()
            flat = [dev(x).reshape(B * H, N, d) for x in inputs]
            groups = [grad_bounds_torch(*(t[h:h + 8] for t in flat), causal) for h in range(0, B * H, 8)]
            grads = [torch.cat([g[i] for g in groups]).reshape(shape) for i in range(3)]
            out["bounds"] = dict(zip(("dq", "dk", "dv"), grads), o=1e-3 + R_BF16 * pabs,
                                 o_f32=1e-3 + 2.0 ** -8 * pabs)
            out["own"] = None
        else:
            out["bounds"], out["own"] = VC.fp32_bounds(ref, VC.ref64(q, k, v, do, causal, [N] * B))
        return out
    return _cached(_REF, (case, causal), make)


WRITTEN_FWD, WRITTEN_ALL = ("o", "m", "l"), ("o", "m", "l", "dq", "dk", "dv")


def _run(torch, case, causal, layout, o_f32=False, bwd=True):
    """Forward (and backward) of a case with every tensor placed under `layout`; returns the
    outputs {name: view} and the footprint failures."""
    from minitorch import _hip
    bf16, shape = CASES[case]
    tdt = torch.bfloat16 if bf16 else torch.float32
    ws = _hip.lib().mt_flash_attn_bwd_workspace_bytes(*shape) if bwd else None
    call = FL.Call(shape, tdt, layout, _reference(torch, case, causal)["inputs"], "cuda",
                   o_dtype=torch.float32 if o_f32 else None, ws_bytes=ws)
    q, k, v, o, do, dq, dk, dv = call.views(*FL.ROLES)
    call.snapshot("q", "k", "v", "do")
    _hip.flash_fwd(q, k, v, causal, out=o, m=call.m.view, l=call.l.view)
    torch.cuda.synchronize()
    if bwd:
        assert call.ws.view.numel() == ws and call.ws.view.data_ptr() % 256 == 0
        call.snapshot("o", "m", "l")
        _hip.flash_bwd(q, k, v, o, do, call.m.view, call.l.view, causal, dq=dq, dk=dk, dv=dv, workspace=call.ws.view)
        torch.cuda.synchronize()
    names = WRITTEN_ALL if bwd else WRITTEN_FWD
    got = {n: (call.m.view if n == "m" else call.l.view if n == "l" else call.t[n].view) for n in names}
    return got, call.failures(names)


def _check(torch, case, causal, layout, record, family, o_f32=False, bwd=True, policy=0, bit_equal=True):
    """One placed run against the oracle, its footprint, and the contiguous run of the same
    case; every finding is collected before the assertion."""
    bf16, shape = CASES[case]
    ref = _reference(torch, case, causal)
    got, fails = _run(torch, case, causal, layout, o_f32, bwd)
    worst = {}
    for name in ("o", "dq", "dk", "dv")[:4 if bwd else 1]:
        bnd = ref["bounds"]["o_f32" if (name == "o" and o_f32) else name]
        err = (got[name].double() - ref["ref"][name].double()).abs()  # NaN fails the comparison below
        ratio = err / bnd
        bad = ~(ratio <= 1.0)
        worst[name] = float(torch.nan_to_num(ratio, nan=float("inf")).max())
        if bool(bad.any()):
            b, h, i, j = (int(t) for t in bad.nonzero()[0])
            fails.append(f"{name}: {int(bad.sum())} elements over the bound, first at (b,h,n,c)=({b},{h},{i},{j}): "
                         f"|err| {float(err[b, h, i, j]):.3e}, worst error/bound {worst[name]:.3f}")
    print(f"{family} {case} {shape} causal={causal} {layout}: error/bound "
          + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()), flush=True)
    rec = {f"{n}_err_over_bound": r for n, r in worst.items()}
    if ref["own"] is not None:
        rec.update({f"{n}_bound": ref["bounds"][n] for n in worst}, **{f"{n}_oracle_vs_f64": ref["own"][n] for n in worst})
    record("test_flash_layouts_gpu", f"{family} {case} {shape} causal={causal} {layout}",
           bound="tests/bounds.py elementwise" if bf16 else "1e-5 (O), 2e-5 x max|ref| (grads) + oracle's own error", **rec)
    if layout != "bhnd" and bit_equal:
        base = _cached(_BASE, (case, causal, o_f32, policy), lambda: {
            n: t.clone() for n, t in _run(torch, case, causal, "bhnd", o_f32, bwd)[0].items()})
        for n, t in got.items():
            if not FL.same_bits(t, base[n]):
                diff = (t.float() != base[n].float()) | (torch.isnan(t) != torch.isnan(base[n]))
                fails.append(f"{n}: {int(diff.sum())} elements differ from the contiguous run's")
    assert not fails, f"{family} {case} causal={causal} {layout}: " + "; ".join(fails)
    if not torch.isnan(got["m"]).any():
        _check_ml(got["m"].cpu().numpy(), got["l"].cpu().numpy(), ref["m"], ref["l"], exact=not bf16)


@pytest.mark.parametrize("case,causal,layout", MATRIX, ids=[f"{c}-{'causal' if z else 'full'}-{lay}" for c, z, lay in MATRIX])
def test_layouts_default_dispatch(torch_dev, case, causal, layout, parity_record):
    _check(torch_dev, case, causal, layout, parity_record, "default")


@pytest.mark.parametrize("layout", OTHER_LAYOUTS)
@pytest.mark.parametrize("case,causal", F32OUT, ids=[f"{c}-{'causal' if z else 'full'}" for c, z in F32OUT])
def test_layouts_fp32_out(torch_dev, case, causal, layout, parity_record):
    """MT_BF16_F32OUT, O placed as fp32: the forward alone, O under 1e-3 + 2^-8 (P|V|)."""
    _check(torch_dev, case, causal, layout, parity_record, "fp32-O", o_f32=True, bwd=False)


@pytest.mark.parametrize("layout", OTHER_LAYOUTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case,policy", POLICIES, ids=[f"{c}-policy{p}" for c, p in POLICIES])
def test_layouts_product_policies(torch_dev, case, policy, causal, layout, parity_record):
    """The product library's other policies: 121 the split bf16 backward, 1 the generic kernels."""
    from minitorch import _hip
    try:
        _use_policy(_hip, policy)
        _check(torch_dev, case, causal, layout, parity_record, f"policy{policy}", policy=policy)
    finally:
        _hip.set_policy(0)
