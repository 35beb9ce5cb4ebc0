"""Tensor placements and write-footprint checks for the flash-attention entry points (test
infrastructure; tests/test_flash_layouts.py runs it on the CPU with the oracle as a stand-in
kernel, tests/test_flash_layouts_gpu.py on the kernels).

Every tensor of a call is a [B, H, N, d] view of a larger parent allocation:

    bhnd     contiguous (the control)
    bnhd     a [B, N, H, d] parent permuted to [B, H, N, d] (what minitorch's MHA hands over)
    slice    parent [B, H+2, N+3, d+8] behind a 16-byte lead, the view [:, 1:H+1, 2:N+2, :d]:
             a base aligned to 16 bytes and no more (where (N+5)(d+8) elements are an odd number
             of 16-byte units a 16-byte lead would leave the view 32-byte aligned, and the lead
             is 32 bytes instead), 8 foreign elements after every row,
             foreign rows before row 0 and after row N-1 of every head, foreign heads before
             head 0 and after head H-1
    packed   Q, K, V in one [B, N, 3, H+1, d] parent (a fused QKV projection with one head slot
             that is never viewed), dQ, dK, dV in a second one, O and dO bnhd
    mixedA / mixedB / mixedC   a different layout per tensor (MIXED)

Input parents hold NaN outside the view, output parents NaN inside it (an element a kernel
skips fails) and SENTINEL outside (an element a kernel must not write). (m, l) are the interior
of a buffer with a 64-float guard band on each side, the backward workspace a uint8 slice of
exactly the advertised size between two 4096-byte bands.

The checks return lists of failure strings (empty: passed) and compare bit patterns, so a NaN
is equal to itself and -0.0 differs from 0.0.
"""
import numpy as np
import torch

SENTINEL = 12288.0      # 1.5 x 2^13: exact in bf16
WS_SENTINEL = 0x5A      # the workspace guard bands' byte
ROW_GUARD = 64          # floats on each side of m / l
WS_GUARD = 4096         # bytes on each side of the workspace

LAYOUTS = ("bhnd", "bnhd", "slice", "packed", "mixedA", "mixedB", "mixedC")
ROLES = ("q", "k", "v", "o", "do", "dq", "dk", "dv")
INPUTS, OUTPUTS = ("q", "k", "v", "do"), ("o", "dq", "dk", "dv")
MIXED = {
    # mixedA: no two tensors one kernel reads with adjacent arguments (q/do, k/v, dq/q, dk/k)
    # alike; dv and v are alike in mixedA and mixedB, so mixedC sets those two apart as well
    "mixedA": dict(q="slice", k="bnhd", v="bhnd", o="bnhd", do="bhnd", dq="bnhd", dk="slice", dv="bhnd"),
    "mixedB": dict(q="bhnd", k="slice", v="bnhd", o="slice", do="slice", dq="slice", dk="bhnd", dv="bnhd"),
    "mixedC": dict(q="bnhd", k="bhnd", v="slice", o="bhnd", do="slice", dq="bhnd", dk="bnhd", dv="bnhd"),
}
_PACK_SLOT = dict(q=0, k=1, v=2, dq=0, dk=1, dv=2)


def layout_of(layout, role):
    """The placement of one tensor under a case layout."""
    if layout in MIXED:
        return MIXED[layout][role]
    if layout == "packed":
        return "packed" if role in _PACK_SLOT else "bnhd"
    assert layout in ("bhnd", "bnhd", "slice"), layout
    return layout


def _bits(t):
    """The tensor's bit patterns as integers of its element size."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Parent:
    """One allocation: `flat` (1-D, the whole of it), `mask` (True where some view handed out
    covers it), `output`, and the sentinel its uncovered elements hold (outputs only)."""

    def __init__(self, numel, dtype, device, output, sentinel=SENTINEL):
        fill = sentinel if output else float("nan")
        self.flat = torch.full((numel,), fill, dtype=dtype, device=device)
        self.mask = torch.zeros(numel, dtype=torch.bool, device=device)
        self.output = output
        self.sentinel = torch.full((1,), fill, dtype=dtype, device=device)

    def view(self, size, stride, offset, x=None):
        v = self.flat.as_strided(size, stride, offset)
        self.mask.as_strided(size, stride, offset).fill_(True)
        if x is not None:
            v.copy_(torch.as_tensor(np.ascontiguousarray(x)).to(self.flat.device).to(self.flat.dtype))
        elif self.output:
            v.fill_(float("nan")) if self.flat.dtype.is_floating_point else v.fill_(0xFF)
        return v

    def bits(self):
        return _bits(self.flat).clone()


class Placed:
    """A view with its parent allocation."""

    def __init__(self, view, parent, layout):
        self.view, self.parent, self.layout = view, parent, layout


def place(shape, dtype, layout, role, x=None, device="cpu", shared=None):
    """The tensor `role` of a call under `layout`: a [B, H, N, d] view (filled with x, an
    input; or with NaN, an output) and its parent. shared: a dict the tensors of one call pass
    along, which holds the two parents of `packed`."""
    B, H, N, d = shape
    output = x is None
    es = torch.empty((), dtype=dtype).element_size()
    epc = 16 // es
    how = layout_of(layout, role)
    if how == "bhnd":
        p = Parent(B * H * N * d, dtype, device, output)
        v = p.view(shape, (H * N * d, N * d, d, 1), 0, x)
    elif how == "bnhd":
        p = Parent(B * H * N * d, dtype, device, output)
        v = p.view(shape, (N * H * d, d, H * d, 1), 0, x)
    elif how == "slice":
        Hp, Np, dp = H + 2, N + 3, d + 8
        inner = Np * dp + 2 * dp  # head 1, row 2 of the parent
        lead = epc if (epc + inner) % (2 * epc) else 2 * epc
        p = Parent(lead + B * Hp * Np * dp, dtype, device, output)
        v = p.view(shape, (Hp * Np * dp, Np * dp, dp, 1), lead + inner, x)
        if d % epc == 0:
            assert v.data_ptr() % 32 == 16
    else:
        assert how == "packed"
        key = "packed_out" if output else "packed_in"
        shared = {} if shared is None else shared
        if key not in shared:
            shared[key] = Parent(B * N * 3 * (H + 1) * d, dtype, device, output)
        p = shared[key]
        row = 3 * (H + 1) * d
        v = p.view(shape, (N * row, d, row, 1), _PACK_SLOT[role] * (H + 1) * d, x)
    assert v.stride(3) == 1 and v.data_ptr() == p.flat.data_ptr() + v.storage_offset() * es
    if d % epc == 0:  # the library's vec_ok: the 16-B paths are still taken
        assert all(s % epc == 0 for s in v.stride()[:3]) and v.data_ptr() % 16 == 0, (how, v.stride())
    return Placed(v, p, how)


def place_rows(B, H, N, device="cpu"):
    """m or l: the interior [B, H, N] of a buffer of B*H*N + 2*ROW_GUARD floats."""
    p = Parent(B * H * N + 2 * ROW_GUARD, torch.float32, device, True)
    return Placed(p.view((B, H, N), (H * N, N, 1), ROW_GUARD), p, "rows")


def place_workspace(nbytes, device="cpu"):
    """The backward workspace: exactly nbytes (uint8) between two WS_GUARD-byte bands."""
    p = Parent(nbytes + 2 * WS_GUARD, torch.uint8, device, True, sentinel=WS_SENTINEL)
    return Placed(p.view((nbytes,), (1,), WS_GUARD), p, "workspace")


def same_bits(a, b):
    """Two tensors of one shape and dtype hold the same bit patterns."""
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


# ---- the checks ------------------------------------------------------------------------------
def untouched(parent, view_mask=None, what="parent"):
    """Every element outside the views still holds the sentinel, to the bit."""
    mask = parent.mask if view_mask is None else view_mask
    bad = (_bits(parent.flat) != _bits(parent.sentinel)) & ~mask
    n = int(bad.sum())
    if not n:
        return []
    first = int(bad.nonzero()[0])
    return [f"{what}: {n} elements outside the view were written, first at flat index {first} "
            f"(value {parent.flat[first].item()})"]


def all_written(view, what="view"):
    """No NaN is left inside the view."""
    nan = torch.isnan(view)
    n = int(nan.sum())
    if not n:
        return []
    first = tuple(int(i) for i in nan.nonzero()[0])
    return [f"{what}: {n} elements are NaN (never written, or made of foreign data), first at {first}"]


def unchanged(before_bits, parent, what="parent"):
    """The whole allocation holds the bits it held before."""
    diff = _bits(parent.flat) != before_bits
    n = int(diff.sum())
    if not n:
        return []
    return [f"{what}: {n} elements changed, first at flat index {int(diff.nonzero()[0])}"]


# ---- one call's tensors ----------------------------------------------------------------------
class Call:
    """The tensors of one forward + backward: t[role] (Placed) for ROLES, m, l, ws; and the
    footprint checks over them."""

    def __init__(self, shape, dtype, layout, inputs, device="cpu", o_dtype=None, ws_bytes=None):
        B, H, N, d = shape
        self.shape, self.layout = shape, layout
        shared = {}
        self.t = {}
        for role, x in zip(INPUTS, inputs):
            self.t[role] = place(shape, dtype, layout, role, x, device, shared)
        for role in OUTPUTS:
            self.t[role] = place(shape, o_dtype if role == "o" and o_dtype is not None else dtype, layout, role,
                                 None, device, shared)
        self.m, self.l = place_rows(B, H, N, device), place_rows(B, H, N, device)
        self.ws = None if ws_bytes is None else place_workspace(ws_bytes, device)
        self._before = {}

    def views(self, *roles):
        return tuple(self.t[r].view for r in roles)

    def _named_parents(self, roles):
        seen, out = {}, []
        for r in roles:
            p = {"m": self.m, "l": self.l, "ws": self.ws}[r].parent if r in ("m", "l", "ws") else self.t[r].parent
            if id(p) not in seen:
                seen[id(p)] = len(out)
                out.append((r, p))
            else:  # a shared parent is named after every tensor in it
                i = seen[id(p)]
                out[i] = (out[i][0] + "+" + r, p)
        return out

    def snapshot(self, *roles):
        """Remember the bits of the parents of `roles` (for unchanged)."""
        for r, p in self._named_parents(roles):
            self._before[r] = (p, p.bits())

    def failures(self, written):
        """all_written on the views of `written`, untouched on their parents (each once) and on
        the workspace's, unchanged on everything snapshotted."""
        fails = []
        for r in written:
            v = {"m": self.m, "l": self.l}[r].view if r in ("m", "l") else self.t[r].view
            fails += all_written(v, r)
        guards = tuple(written) + (("ws",) if self.ws is not None else ())
        for r, p in self._named_parents(guards):
            fails += untouched(p, what=f"{r} parent")
        for r, (p, before) in self._before.items():
            fails += unchanged(before, p, f"{r} parent")
        return [f"[{self.layout}] {f}" for f in fails]
