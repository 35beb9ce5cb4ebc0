"""mt_rope's argument validation and the host side of rotary position embedding (CPU: every
refusal precedes the first device call, so dummy pointers are enough and nothing is launched; the
table, the model wiring and the tensor-op form run on the NumPy test backend)."""
import ctypes
import math

import numpy as np
import pytest

DUMMY = ctypes.c_void_p(256)
MT_F32 = 0


def _call(lib, **kw):
    a = dict(dtype=MT_F32, inverse=0, x=DUMMY, out=DUMMY, H=3, x_strides=None, out_strides=None,
             x2=None, out2=None, H2=0, x2_strides=None, out2_strides=None, B=2, T=5, d=8,
             cos=DUMMY, sin=DUMMY, n_pos=16, pos0=None, stream=None)
    a.update(kw)
    return lib.mt_rope(a["dtype"], a["inverse"], a["x"], a["out"], a["H"], a["x_strides"], a["out_strides"],
                       a["x2"], a["out2"], a["H2"], a["x2_strides"], a["out2_strides"], a["B"], a["T"], a["d"],
                       a["cos"], a["sin"], a["n_pos"], a["pos0"], a["stream"])


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), b"bad sizes"),
    (dict(B=-2), b"bad sizes"),
    (dict(T=0), b"bad sizes"),
    (dict(T=-1), b"bad sizes"),
    (dict(H=0), b"bad sizes"),
    (dict(H=-1), b"bad sizes"),
    (dict(d=0), b"bad sizes"),
    (dict(d=-8), b"bad sizes"),
    (dict(n_pos=0), b"bad sizes"),
    (dict(n_pos=-4), b"bad sizes"),
    (dict(d=7), b"odd"),
    (dict(d=258), b"limit of 256"),
    (dict(dtype=1), b"dtype"),
    (dict(dtype=2), b"dtype"),
    (dict(x=None), b"x is NULL"),
    (dict(out=None), b"out is NULL"),
    (dict(cos=None), b"table is NULL"),
    (dict(sin=None), b"table is NULL"),
    (dict(x2=DUMMY, out2=None, H2=1), b"out2 is NULL"),
    (dict(x2=DUMMY, out2=DUMMY, H2=0), b"H2"),
    (dict(x2=DUMMY, out2=DUMMY, H2=-1), b"H2"),
    # 2^31 pairs in one launch: the kernels index them in 32 bits
    (dict(B=1 << 10, H=1 << 10, T=1 << 9, d=8), b"out of range"),
    (dict(B=1 << 10, H=1 << 9, x2=DUMMY, out2=DUMMY, H2=1 << 9, T=1 << 9, d=8), b"out of range"),
])
def test_refusals(kw, msg):
    from minitorch import _hip
    lib = _hip.lib()
    assert _call(lib, **kw) != 0
    err = lib.mt_last_error()
    assert b"mt_rope" in err and msg in err, err


def test_abi_version_and_binding():
    from minitorch import _hip
    lib = _hip.lib()
    assert lib.mt_abi_version() == 3
    assert "mt_rope" in _hip.exported_symbols()
    assert callable(_hip.rope)


def test_backend_binds_rope_optionally():
    import minitorch
    from cpu_backend import NumpyOps
    assert minitorch.TensorBackend(NumpyOps).rope is None
    assert minitorch.TensorBackend(minitorch.HipKernelOps).rope is not None


@pytest.mark.parametrize("n_positions,d", [(64, 8), (7, 2)])
def test_table_is_the_float64_angles_rounded_once(n_positions, d):
    """cos_host / sin_host against an independent float64 computation (Python's math, element
    by element) of the angle p * theta ** (-2j / d), rounded to fp32: bit for bit."""
    import minitorch
    theta = 10000.0
    tab = minitorch.RotaryTable(n_positions, d, theta)
    assert tab.cos_host.shape == tab.sin_host.shape == (n_positions, d // 2)
    assert tab.cos_host.dtype == tab.sin_host.dtype == np.float32
    want_c = np.empty((n_positions, d // 2), np.float32)
    want_s = np.empty((n_positions, d // 2), np.float32)
    for p in range(n_positions):
        for j in range(d // 2):
            angle = float(p) * theta ** (-2.0 * j / d)
            want_c[p, j] = np.float32(math.cos(angle))
            want_s[p, j] = np.float32(math.sin(angle))
    assert np.array_equal(tab.cos_host.view(np.uint32), want_c.view(np.uint32))
    assert np.array_equal(tab.sin_host.view(np.uint32), want_s.view(np.uint32))
    with pytest.raises(ValueError, match="head_dim"):
        minitorch.RotaryTable(8, 3)
    with pytest.raises(ValueError, match="n_positions"):
        minitorch.RotaryTable(0, 4)


def test_decoder_lm_pos_encoding():
    import minitorch
    from cpu_backend import NumpyOps
    cpu = minitorch.TensorBackend(NumpyOps)
    kw = dict(n_vocab=11, n_embd=8, n_head=2, n_positions=8, p_dropout=0.0, backend=cpu, n_layer=1)
    np.random.seed(0)
    learned = [n for n, _ in minitorch.DecoderLM(**kw).named_parameters()]
    np.random.seed(0)
    explicit = [n for n, _ in minitorch.DecoderLM(pos_encoding="learned", **kw).named_parameters()]
    rope_lm = minitorch.DecoderLM(pos_encoding="rope", **kw)
    rope = [n for n, _ in rope_lm.named_parameters()]
    assert learned == explicit
    # the default model's names and order, as they were before the rotary option existed
    layer = [f"t_layer_1.{m}.{p}" for m in ("attention.q_projection", "attention.k_projection",
                                            "attention.v_projection", "attention.out_projection",
                                            "ff.linear_in", "ff.linear_out", "ln_1", "ln_2")
             for p in ("weights", "bias")]
    assert learned == (["token_embeddings.weights", "position_embeddings.weights"] + layer
                       + ["lm_head.weights", "lm_head.bias", "ln.weights", "ln.bias"])
    assert not any("position_embeddings" in n for n in rope)
    assert [n for n in learned if "position_embeddings" not in n] == rope
    # one table, shared by every layer, sized by the model
    tab = rope_lm.rope
    assert isinstance(tab, minitorch.RotaryTable) and rope_lm.t_layer_1.attention.rope is tab
    assert (tab.n_positions, tab.head_dim, tab.theta) == (8, 4, 10000.0)
    assert minitorch.DecoderLM(pos_encoding="rope", rope_theta=500.0, **kw).rope.theta == 500.0
    with pytest.raises(ValueError, match="pos_encoding"):
        minitorch.DecoderLM(pos_encoding="alibi", **kw)
    # the rotary model runs end to end on the CPU backend, and the positions matter: the last
    # token's logits change when a token is put in front of the same suffix
    rope_lm.eval()
    a = rope_lm(minitorch.tensor_from_numpy(np.array([[1, 2, 3]], np.float32), cpu)).to_numpy()
    b = rope_lm(minitorch.tensor_from_numpy(np.array([[3]], np.float32), cpu)).to_numpy()
    assert a.shape == (1, 3, 11) and np.isfinite(a).all()
    assert np.abs(a[0, 2] - b[0, 0]).max() > 0
    assert len(rope_lm.generate([[1, 2]], 3, use_cache=False)[0]) == 3


def _rotate64(x, cos, sin, pos):
    """The rotation in float64 NumPy: x [B,H,T,d], pos [B,T] table rows."""
    h = x.shape[-1] // 2
    c = cos.astype(np.float64)[pos][:, None]
    s = sin.astype(np.float64)[pos][:, None]
    a, b = x[..., :h].astype(np.float64), x[..., h:].astype(np.float64)
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


@pytest.mark.parametrize("pos0", [None, [-3, 14]])
def test_tensor_op_form_matches_a_direct_rotation(pos0):
    """x * C + (x @ P) * S on the CPU backend (fp32 NumPy: a few ulp) against the float64
    rotation, within 1e-6 max|x|; with pos0 the negative and the top clamp are hit. Its
    autodiff backward is the transposed rotation."""
    import minitorch
    from cpu_backend import NumpyOps
    cpu = minitorch.TensorBackend(NumpyOps)
    B, H, T, d, n_pos = 2, 3, 5, 8, 16
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, H, T, d)).astype(np.float32)
    g = rng.standard_normal((B, H, T, d)).astype(np.float32)
    tab = minitorch.RotaryTable(n_pos, d, backend=cpu)
    start = np.zeros(B, np.int64) if pos0 is None else np.maximum(np.asarray(pos0), 0)
    pos = np.minimum(start[:, None] + np.arange(T)[None, :], n_pos - 1)
    if pos0 is not None:
        assert pos[0, 0] == 0 and (pos[1] == n_pos - 1).sum() > 1, "both clamps are exercised"
    xt = minitorch.tensor_from_numpy(x, cpu, requires_grad=True)
    out = xt.rope(tab, pos0)
    want = _rotate64(x, tab.cos_host, tab.sin_host, pos)
    tol = 1e-6 * float(np.abs(x).max())
    assert float(np.abs(out.to_numpy() - want).max()) <= tol
    (out * minitorch.tensor_from_numpy(g, cpu)).sum().backward()
    want_g = _rotate64(g, tab.cos_host, -tab.sin_host, pos)
    assert float(np.abs(xt.grad.to_numpy() - want_g).max()) <= 1e-6 * float(np.abs(g).max())
    # the kernel path is refused by name on a backend without the kernel
    with pytest.raises(NotImplementedError, match="rope"):
        minitorch.apply_rope(xt, tab, fused=True)
