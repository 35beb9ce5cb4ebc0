"""mt_rope on the device against a float64 NumPy rotation of the same fp32 inputs and tables.

The bound, per output element: 2^-23 (|a cos| + |b sin|), a and b the two inputs of the pair.
The kernel forms two rounded products and one rounded sum, 2^-24 relative each (the sum's
magnitude is at most |a cos| + |b sin|); a fused multiply-add only drops one of the roundings.
Nothing is measured to set it. Inputs are N(0, 1).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, H, H2 = 2, 3, 1
N_POS = 136  # the longest T below is 130
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from minitorch import _hip
    _hip.lib()
    tables = {}

    def table(n_pos, d):
        if (n_pos, d) not in tables:
            tab = minitorch.RotaryTable(n_pos, d)
            tables[n_pos, d] = (tab, torch.from_numpy(tab.cos_host).cuda(), torch.from_numpy(tab.sin_host).cuda())
        return tables[n_pos, d]
    return dict(torch=torch, hip=_hip, minitorch=minitorch, table=table)


def positions(pos0, n_rows, T, n_pos):
    start = np.zeros(n_rows, np.int64) if pos0 is None else np.maximum(np.asarray(pos0, np.int64), 0)
    return np.minimum(start[:, None] + np.arange(T)[None, :], n_pos - 1)


def rotate64(x, tab, pos, inverse=False):
    """(reference, bound) of x [B,h,T,d] fp32 rotated at the table rows pos [B,T]."""
    h = x.shape[-1] // 2
    c = tab.cos_host.astype(np.float64)[pos][:, None]
    s = tab.sin_host.astype(np.float64)[pos][:, None] * (-1.0 if inverse else 1.0)
    a, b = x[..., :h].astype(np.float64), x[..., h:].astype(np.float64)
    ref = np.concatenate([a * c - b * s, b * c + a * s], axis=-1)
    bound = EPS * np.concatenate([np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)], axis=-1)
    return ref, bound


def inputs(torch, d, T, layout, seed):
    """(q, k) device tensors [B,H,T,d] / [B,H2,T,d] in the layout, and their host values."""
    rng = np.random.default_rng(seed)
    out = []
    for heads in (H, H2):
        x = rng.standard_normal((B, heads, T, d)).astype(np.float32)
        if layout == "dense":
            t = torch.from_numpy(x).cuda()
        else:  # the model's [B,T,H,d] projection storage seen as [B,H,T,d]
            t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1, 3))).cuda().permute(0, 2, 1, 3)
            assert not t.is_contiguous() or heads == 1 or T == 1
        out.append((t, x))
    return out


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def check(got, x, tab, pos, what, inverse=False):
    ref, bound = rotate64(x, tab, pos, inverse)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), f"{what}: worst error / bound {worst:.3f}"
    return worst


@pytest.mark.parametrize("layout", ["dense", "permuted"])
@pytest.mark.parametrize("T", [1, 5, 130])
@pytest.mark.parametrize("d", [2, 6, 8, 72, 256])
def test_rotation_meets_the_bound(dev, d, T, layout, parity_record):
    """Both bodies (d = 2, 6: one pair per thread; d = 8, 72, 256: 16-B chunks), one to many
    workgroups with a ragged tail, dense and permuted strides: the two-tensor launch meets the
    bound on Q and K, equals two one-tensor launches bit for bit, and in place equals out of
    place bit for bit."""
    torch, hip = dev["torch"], dev["hip"]
    tab, cos, sin = dev["table"](N_POS, d)
    (q, qh), (k, kh) = inputs(torch, d, T, layout, seed=d * 1000 + T)
    pos = positions(None, B, T, N_POS)
    oq, ok = hip.rope(q, cos, sin, x2=k)
    assert oq.shape == q.shape and ok.shape == k.shape
    worst = max(check(oq, qh, tab, pos, "Q"), check(ok, kh, tab, pos, "K"))
    parity_record("test_rotation_meets_the_bound", f"d={d} T={T} {layout}", max_ratio=worst, bound=1.0)
    # the inputs are untouched by the out-of-place launch
    assert np.array_equal(q.cpu().numpy(), qh) and np.array_equal(k.cpu().numpy(), kh)
    # one tensor at a time
    assert np.array_equal(bits(hip.rope(q, cos, sin)), bits(oq))
    assert np.array_equal(bits(hip.rope(k, cos, sin)), bits(ok))
    # in place, in the inputs' own layout
    q2, k2 = q.clone(memory_format=torch.preserve_format), k.clone(memory_format=torch.preserve_format)
    rq, rk = hip.rope(q2, cos, sin, out=q2, x2=k2, out2=k2)
    assert rq is q2 and rk is k2
    assert np.array_equal(bits(q2), bits(oq)) and np.array_equal(bits(k2), bits(ok))


def test_misaligned_view_takes_the_scalar_body(dev):
    """A view offset by one element at d = 8: no 16-B alignment, so the pair-per-thread body
    runs; it meets the same bound."""
    torch, hip = dev["torch"], dev["hip"]
    d, T = 8, 5
    tab, cos, sin = dev["table"](N_POS, d)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, H, T, d)).astype(np.float32)
    buf = torch.zeros(x.size + 1, device="cuda")
    buf[1:] = torch.from_numpy(x.reshape(-1)).cuda()
    view = buf[1:].view(B, H, T, d)
    assert view.data_ptr() % 16 == 4
    obuf = torch.zeros(x.size + 1, device="cuda")
    out = hip.rope(view, cos, sin, out=obuf[1:].view(B, H, T, d))
    check(out, x, tab, positions(None, B, T, N_POS), "offset view")
    assert float(obuf[0]) == 0.0


@pytest.mark.parametrize("d", [6, 8])
def test_positions_and_both_clamps(dev, d):
    """pos0 = [-3, n_pos - 2] with n_pos = 16, T = 5: row 0 starts at the negative clamp (0),
    row 1 runs into the top clamp (14, 15, 15, 15, 15). The reference applies the same formula."""
    torch, hip = dev["torch"], dev["hip"]
    n_pos, T = 16, 5
    tab, cos, sin = dev["table"](n_pos, d)
    pos0 = np.array([-3, n_pos - 2], np.int32)
    pos = positions(pos0, B, T, n_pos)
    assert list(pos[0]) == [0, 1, 2, 3, 4] and list(pos[1]) == [14, 15, 15, 15, 15]
    (q, qh), (k, kh) = inputs(torch, d, T, "permuted", seed=11 + d)
    oq, ok = hip.rope(q, cos, sin, pos0=torch.from_numpy(pos0).cuda(), x2=k)
    check(oq, qh, tab, pos, "Q")
    check(ok, kh, tab, pos, "K")
    # a host vector is converted; the result is the same
    assert np.array_equal(bits(hip.rope(q, cos, sin, pos0=[-3, n_pos - 2])), bits(oq))


@pytest.mark.parametrize("d", [6, 72])
def test_inverse(dev, d, parity_record):
    """inverse alone meets the bound against the transposed reference. inverse(forward(x))
    returns x within twice the bound, 2 * 2^-23 (|a cos| + |b sin|) with a and b the inputs of
    the inverse step, y = forward(x). Also recorded, not asserted: the error against the looser
    derived form, the inverse step's bound plus the forward step's bound carried through the
    inverse rotation (|cos| of the element's own forward bound and |sin| of its partner's)."""
    torch, hip = dev["torch"], dev["hip"]
    T = 5
    tab, cos, sin = dev["table"](N_POS, d)
    pos0 = np.array([7, 100], np.int32)
    pos = positions(pos0, B, T, N_POS)
    p0 = torch.from_numpy(pos0).cuda()
    (q, qh), _ = inputs(torch, d, T, "dense", seed=21 + d)
    check(hip.rope(q, cos, sin, pos0=p0, inverse=True), qh, tab, pos, "inverse", inverse=True)
    y = hip.rope(q, cos, sin, pos0=p0)
    back = hip.rope(y, cos, sin, pos0=p0, inverse=True).cpu().numpy().astype(np.float64)
    _, b_fwd = rotate64(qh, tab, pos)
    _, b_inv = rotate64(y.cpu().numpy(), tab, pos, inverse=True)
    h = d // 2
    c = np.abs(tab.cos_host.astype(np.float64)[pos][:, None])
    s = np.abs(tab.sin_host.astype(np.float64)[pos][:, None])
    carried = np.concatenate([c * b_fwd[..., :h] + s * b_fwd[..., h:], c * b_fwd[..., h:] + s * b_fwd[..., :h]], -1)
    err = np.abs(back - qh.astype(np.float64))
    tol = 2.0 * b_inv
    worst = float((err / np.maximum(tol, 1e-300)).max())
    derived = float((err / np.maximum(b_inv + carried, 1e-300)).max())
    print(f"round trip d={d}: worst error / (2 bound) {worst:.3f}; / (inverse bound + carried forward bound) {derived:.3f}")
    parity_record("test_inverse", f"round trip d={d}", max_ratio=worst, bound=1.0, ratio_to_derived_form=derived)
    assert (err <= tol).all(), f"round trip: worst error / (2 bound) {worst:.3f}"


@pytest.mark.parametrize("d", [6, 8, 72])
def test_write_footprint(dev, d):
    """Outputs with row stride d + 4 and a tail guard, pre-filled with a NaN pattern: every slack
    and guard word is bit-identical afterwards, the rows hold the rotation, the inputs are
    unchanged."""
    torch, hip = dev["torch"], dev["hip"]
    T, pad, guard = 5, 4, 64
    tab, cos, sin = dev["table"](N_POS, d)
    (q, qh), (k, kh) = inputs(torch, d, T, "dense", seed=31 + d)
    pattern = np.uint32(0x7FC0BEEF)
    outs, raws = [], []
    for heads in (H, H2):
        rows = B * heads * T
        raw = torch.from_numpy(np.full(rows * (d + pad) + guard, pattern, np.uint32).view(np.float32)).cuda()
        raws.append(raw)
        outs.append(torch.as_strided(raw, (B, heads, T, d), (heads * T * (d + pad), T * (d + pad), d + pad, 1)))
    q_before, k_before = bits(q).copy(), bits(k).copy()
    hip.rope(q, cos, sin, out=outs[0], x2=k, out2=outs[1])
    pos = positions(None, B, T, N_POS)
    check(outs[0], qh, tab, pos, "Q")
    check(outs[1], kh, tab, pos, "K")
    for raw, heads in zip(raws, (H, H2)):
        rows = B * heads * T
        words = raw.cpu().numpy().view(np.uint32)
        body = words[:rows * (d + pad)].reshape(rows, d + pad)
        assert (body[:, d:] == pattern).all(), "a slack word changed"
        assert (words[rows * (d + pad):] == pattern).all(), "a guard word changed"
        assert not (body[:, :d] == pattern).any()
    assert np.array_equal(bits(q), q_before) and np.array_equal(bits(k), k_before)


def test_relative_position_property(dev):
    """<R_p q, R_p' k> depends on p - p' alone: shifting both positions by s leaves it within
    1e-5 |q||k|. This pins the convention and the table (a wrong pairing or a wrong frequency
    breaks it), not only agreement with a reference that shares the formula."""
    torch, hip = dev["torch"], dev["hip"]
    d, n_pos = 8, 64
    tab, cos, sin = dev["table"](n_pos, d)
    rng = np.random.default_rng(7)
    cases = [(0, 0, 5), (3, 1, 20), (1, 17, 40), (30, 2, 33), (9, 9, 54), (0, 41, 22)]
    n = len(cases)
    qv = rng.standard_normal((n, 1, 1, d)).astype(np.float32)
    kv = rng.standard_normal((n, 1, 1, d)).astype(np.float32)

    def dots(pq, pk):
        rq = hip.rope(torch.from_numpy(qv).cuda(), cos, sin, pos0=torch.tensor(pq, dtype=torch.int32, device="cuda"))
        rk = hip.rope(torch.from_numpy(kv).cuda(), cos, sin, pos0=torch.tensor(pk, dtype=torch.int32, device="cuda"))
        return (rq.cpu().numpy().astype(np.float64) * rk.cpu().numpy().astype(np.float64)).sum(-1).reshape(n)
    assert all(p + s < n_pos and pp + s < n_pos for p, pp, s in cases)
    base = dots([p for p, _, _ in cases], [pp for _, pp, _ in cases])
    moved = dots([p + s for p, _, s in cases], [pp + s for _, pp, s in cases])
    scale = np.linalg.norm(qv.reshape(n, d), axis=1) * np.linalg.norm(kv.reshape(n, d), axis=1)
    assert (np.abs(base - moved) <= 1e-5 * scale).all(), (base, moved)
    # and the rotation is not the identity: the product moves when only one side does
    other = dots([p + s for p, _, s in cases], [pp for _, pp, _ in cases])
    assert (np.abs(base - other) > 1e-3 * scale).any()


@pytest.mark.parametrize("with_pos", [False, True])
def test_rope_function_backward(dev, with_pos):
    """d/dx sum(rope(x) * g) = R^T g: the Rope Function's backward (the kernel with inverse = 1)
    against the transposed float64 rotation of g, within the bound; x arrives as the model's
    permuted projection view."""
    mt = dev["minitorch"]
    hipb = mt.TensorBackend(mt.HipKernelOps)
    d, T, n_pos = 8, 5, 16
    tab = mt.RotaryTable(n_pos, d, backend=hipb)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((B, T, H, d)).astype(np.float32)
    g = rng.standard_normal((B, H, T, d)).astype(np.float32)
    pos0 = [-3, n_pos - 2] if with_pos else None
    pos = positions(pos0, B, T, n_pos)
    xt = mt.tensor_from_numpy(x, hipb, requires_grad=True)
    out = xt.permute(0, 2, 1, 3).rope(tab, pos0)
    xh = x.transpose(0, 2, 1, 3)
    ref, bound = rotate64(xh, tab, pos)
    assert (np.abs(out.to_numpy().astype(np.float64) - ref) <= bound).all()
    (out * mt.tensor_from_numpy(g, hipb)).sum().backward()
    want, gbound = rotate64(g, tab, pos, inverse=True)
    got = xt.grad.to_numpy().transpose(0, 2, 1, 3).astype(np.float64)
    assert (np.abs(got - want) <= gbound).all()
