"""The placements and footprint checks of tests/flash_layouts.py can fail.

Oracle only (no GPU): oracle.attention stands in for a kernel and writes its results through
the placed views on the CPU. The unmutated stand-in passes every check in every layout; each
mutation (a kernel mistake the GPU tests in tests/test_flash_layouts_gpu.py are there to catch)
is reported, and by the check named:

    one extra row N, 8 elements past a row's end, head H      untouched
    the last row skipped                                      all_written
    4 bytes past the workspace, one float past m              untouched
    an input modified                                         unchanged
    dO read with Q's strides, dK written with K's (mixedA)    NaN left, or an output moved by
                                                              3x its tests/bounds.py bound

The 3x is a condition on the inputs, as in tests/test_varlen_edges.py.
"""
import numpy as np
import pytest
import torch

import flash_layouts as FL
import varlen_cases as VC
from oracle import attention as A

SHAPES = [(1, 2, 37, 16), (1, 2, 37, 64)]
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
WS_BYTES = 1000  # any size: the stand-in only fills it


def _inputs(shape, bf16, seed=0):
    rng = np.random.default_rng([seed, *shape, int(bf16)])
    xs = [rng.standard_normal(shape).astype(np.float32) for _ in range(4)]
    return [A.bf16_round(x) for x in xs] if bf16 else xs


def _strided(p, like, size=None, extra=0):
    """Elements of p's parent at p's base (+ extra) with the strides of `like`, on a copy padded
    with NaN (what a read past the allocation finds is not the test's to say); returns the view
    and the padded copy."""
    size = tuple(like.view.shape) if size is None else size
    off = p.view.storage_offset() + extra
    need = off + sum((n - 1) * s for n, s in zip(size, like.view.stride())) + 1
    flat = p.parent.flat
    pad = torch.full((max(need, flat.numel()),), float("nan"), dtype=flat.dtype)
    pad[:flat.numel()] = flat
    return pad.as_strided(size, like.view.stride(), off), pad


def _store(p, like, x, size=None, extra=0, rows=None):
    """Write x through p's base with like's strides (stores past the allocation are dropped)."""
    v, pad = _strided(p, like, size, extra)
    x = torch.as_tensor(x).to(pad.dtype)
    if rows is not None:
        v, x = v[:, :, :rows], x[:, :, :rows]
    v.copy_(x)
    p.parent.flat.copy_(pad[:p.parent.flat.numel()])


def standin(call, causal, mut=None, role="o"):
    """Forward then backward of oracle.attention through the views of `call`; mut: the kernel
    mistake to make, on the output `role` where it names none."""
    B, H, N, d = call.shape
    t = call.t

    def stray(p):  # the stores of an output that do not belong to it
        s1, s2 = p.view.stride(1), p.view.stride(2)
        if mut == "extra_row":      # row N of head 0
            _store(p, p, torch.zeros(B, 1, 1, d), (B, 1, 1, d), N * s2)
        elif mut == "row_overrun":  # 8 elements past the end of every row
            _store(p, p, torch.zeros(B, H, N, 8), (B, H, N, 8), d)
        elif mut == "head_H":       # a head past the last
            _store(p, p, torch.zeros(B, 1, N, d), (B, 1, N, d), H * s1)

    call.snapshot("q", "k", "v", "do")
    q, k, v = (t[r].view.float().numpy() for r in ("q", "k", "v"))
    o, m, l = A.attention_fwd(q, k, v, causal)
    outs = {"o": o}
    call.m.view.copy_(torch.from_numpy(m))
    call.l.view.copy_(torch.from_numpy(l))
    if mut == "m_overrun":
        call.m.parent.flat[FL.ROW_GUARD + B * H * N] = 0.0
    _store(t["o"], t["o"], o, rows=N - 1 if (mut == "skip_last_row" and role == "o") else None)
    if role == "o":
        stray(t["o"])
    call.snapshot("o", "m", "l")
    do = (_strided(t["do"], t["q"])[0] if mut == "strides" else t["do"].view).float().numpy()
    o_read = t["o"].view.float().numpy()
    outs.update(zip(("dq", "dk", "dv"), A.attention_bwd(q, k, v, o_read, do, m, l, causal)))
    for r in ("dq", "dk", "dv"):
        like = t["k"] if (mut == "strides" and r == "dk") else t[r]
        _store(t[r], like, outs[r], rows=N - 1 if (mut == "skip_last_row" and r == role) else None)
    if call.ws is not None:
        call.ws.view.fill_(0)
        if mut == "ws_overrun":
            call.ws.parent.flat[FL.WS_GUARD + WS_BYTES:FL.WS_GUARD + WS_BYTES + 4] = 0
    if role != "o":
        stray(t[role])
    if mut == "touch_input":
        t["q"].view[0, 0, 0, 0] += 1.0
    elif mut == "touch_o":      # O modified by the backward
        t["o"].view[0, H - 1, N - 1, d - 1] += 1.0
    return outs


def _call(shape, dtype, layout, seed=0):
    bf16 = dtype == "bf16"
    inputs = _inputs(shape, bf16, seed)
    return FL.Call(shape, DTYPES[dtype], layout, inputs, ws_bytes=WS_BYTES), inputs


WRITTEN = ("o", "m", "l", "dq", "dk", "dv")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout", FL.LAYOUTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_standin_passes_every_layout(shape, dtype, layout, causal):
    """The unmutated stand-in: no footprint failure, and the values read back through the views
    are the oracle's on the plain arrays (rounded to the dtype)."""
    call, inputs = _call(shape, dtype, layout)
    outs = standin(call, causal)
    assert call.failures(WRITTEN) == []
    q, k, v, do = inputs
    o, m, l = A.attention_fwd(q, k, v, causal)
    o_used = A.bf16_round(o) if dtype == "bf16" else o
    ref = dict(zip(("dq", "dk", "dv"), A.attention_bwd(q, k, v, o_used, do, m, l, causal)), o=o)
    for r in FL.OUTPUTS:
        got = call.t[r].view.float().numpy()
        want = A.bf16_round(ref[r]) if dtype == "bf16" else ref[r]
        np.testing.assert_array_equal(got, want, err_msg=r)
        np.testing.assert_array_equal(want, A.bf16_round(outs[r]) if dtype == "bf16" else outs[r])
    if layout != "bhnd":
        assert not all(call.t[r].view.is_contiguous() for r in FL.ROLES)


def test_layout_tables():
    """What the layouts promise: mixedA gives every tensor pair one kernel reads with adjacent
    arguments different strides; all eight roles differ in packed / mixed from bhnd somewhere;
    the slice view is 16-byte aligned and no more, with every stride a multiple of 16 bytes."""
    shape = (1, 2, 37, 64)
    call, _ = _call(shape, "bf16", "mixedA")
    st = {r: call.t[r].view.stride() for r in FL.ROLES}
    for a, b in (("q", "do"), ("k", "v"), ("dq", "q"), ("dk", "k")):
        assert st[a] != st[b], (a, b)
    call, _ = _call(shape, "bf16", "mixedC")
    st = {r: call.t[r].view.stride() for r in FL.ROLES}
    for a, b in (("q", "do"), ("k", "v"), ("dq", "q"), ("dk", "k"), ("dv", "v")):
        assert st[a] != st[b], (a, b)
    for lay in FL.MIXED:
        assert sorted(set(FL.MIXED[lay].values())) == ["bhnd", "bnhd", "slice"]
        assert set(FL.MIXED[lay]) == set(FL.ROLES)
    assert all(FL.MIXED["mixedA"][r] != FL.MIXED["mixedB"][r] for r in FL.ROLES)
    for dtype, epc in (("bf16", 8), ("fp32", 4)):
        for shp in SHAPES + [(2, 3, 100, 64), (2, 3, 333, 128)]:
            call, _ = _call(shp, dtype, "slice")
            for r in FL.ROLES:
                v = call.t[r].view
                assert v.data_ptr() % 32 == 16 and all(s % epc == 0 for s in v.stride()[:3])
                assert v.stride(2) == shp[3] + 8
    call, _ = _call(shape, "bf16", "packed")
    assert call.t["q"].parent is call.t["k"].parent is call.t["v"].parent
    assert call.t["dq"].parent is call.t["dk"].parent is call.t["dv"].parent
    assert call.t["q"].view.stride(2) == 3 * 3 * 64
    assert int((~call.t["q"].parent.mask).sum()) == 1 * 37 * 3 * 64  # head slot H of q, k, v


def _only(fails, check_word, role):
    """Every failure names `role` and the check's wording, and there is one."""
    assert fails, "the mutation went unreported"
    for f in fails:
        names = f.split("] ", 1)[1].split(":")[0].replace(" parent", "").split("+")
        assert check_word in f and role in names, fails


@pytest.mark.parametrize("role", FL.OUTPUTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_overruns_reported_by_untouched(shape, dtype, role):
    """Row N, 8 elements past a row's end (slice) and head H (slice, packed) of every output."""
    cases = [("extra_row", "slice"), ("row_overrun", "slice"), ("head_H", "slice")]
    if role != "o":
        cases.append(("head_H", "packed"))  # O is bnhd there
    for mut, layout in cases:
        call, _ = _call(shape, dtype, layout)
        standin(call, False, mut, role)
        _only(call.failures(WRITTEN), "outside the view were written", role)


@pytest.mark.parametrize("role", FL.OUTPUTS)
@pytest.mark.parametrize("layout", FL.LAYOUTS)
def test_skipped_row_reported_by_all_written(layout, role):
    for shape in SHAPES:
        call, _ = _call(shape, "bf16", layout)
        standin(call, True, "skip_last_row", role)
        _only(call.failures(WRITTEN), "are NaN", role)


@pytest.mark.parametrize("layout", ["bhnd", "slice", "mixedA"])
def test_workspace_and_row_guards(layout):
    for mut, role in (("ws_overrun", "ws"), ("m_overrun", "m")):
        call, _ = _call(SHAPES[1], "bf16", layout)
        standin(call, False, mut)
        fails = call.failures(WRITTEN)
        _only(fails, "outside the view were written", role)
        assert len(fails) == 1


@pytest.mark.parametrize("layout", FL.LAYOUTS)
def test_modified_input_reported_by_unchanged(layout):
    for mut, role in (("touch_input", "q"), ("touch_o", "o")):
        call, _ = _call(SHAPES[0], "fp32", layout)
        standin(call, False, mut)
        fails = call.failures(WRITTEN)
        _only(fails, "elements changed", role)
        assert len(fails) == 1


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mixed_strides_confusion_is_seen(shape, causal):
    """mixedA, dO read with Q's strides and dK written with K's: NaN left in an output (reported
    by all_written), or some output at least 3x its tests/bounds.py bound from the oracle; and
    the stray dK stores land outside the view (untouched)."""
    call, (q, k, v, do) = _call(shape, "bf16", "mixedA")
    standin(call, causal, "strides")
    fails = call.failures(WRITTEN)
    assert any("dk parent" in f and "outside the view" in f for f in fails), fails
    kv = [shape[2]] * shape[0]
    ref = VC.oracle_numpy(q, k, v, do, causal, kv)
    bounds = VC.bf16_bounds(q, k, v, do, causal, kv, A.attention_fwd(q, k, np.abs(v), causal)[0])
    for r, want, bnd in zip(("dq", "dk", "dv"), ref[3:], bounds[1:]):
        got = call.t[r].view.float().numpy()
        nan = bool(np.isnan(got).any())
        moved = float(np.nanmax(np.abs(got - want) / bnd))
        assert nan == any(f"] {r}:" in f and "are NaN" in f for f in fails)
        print(f"{shape} causal={causal} {r}: NaN left {nan}, moved {moved:.1f}x its bound")
        assert nan or moved >= 3.0, f"{r}: the confusion moves it by {moved:.2f}x its bound and leaves no NaN"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_strides_confusion_moves_values(shape, causal, monkeypatch):
    """The same confusion between dense layouts of one size (q, dk bhnd; k, do bnhd), where no
    store leaves a view and no read meets a NaN: the footprint checks have nothing to report,
    and the values do: dQ, dK and dV each end at least 3x their bound from the oracle."""
    monkeypatch.setitem(FL.MIXED, "dense", dict(q="bhnd", k="bnhd", v="bhnd", o="bnhd", do="bnhd",
                                                dq="bhnd", dk="bhnd", dv="bnhd"))
    call, (q, k, v, do) = _call(shape, "bf16", "dense")
    standin(call, causal, "strides")
    assert call.failures(WRITTEN) == []
    kv = [shape[2]] * shape[0]
    ref = VC.oracle_numpy(q, k, v, do, causal, kv)
    bounds = VC.bf16_bounds(q, k, v, do, causal, kv, A.attention_fwd(q, k, np.abs(v), causal)[0])
    for r, want, bnd in zip(("dq", "dk", "dv"), ref[3:], bounds[1:]):
        moved = float((np.abs(call.t[r].view.float().numpy() - want) / bnd).max())
        print(f"{shape} causal={causal} {r}: moved {moved:.1f}x its bound")
        assert moved >= 3.0, f"{r}: the confusion moves it by only {moved:.2f}x its bound"
