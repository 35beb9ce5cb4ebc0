"""The storage formats of the weight-only quantised linear: what mt_weight_quant stores, read back
through mt_weight_dequant (W' and the codes), against the fp32 input and each format's rule."""
import numpy as np
import pytest

import kvq_cases as Q

pytestmark = pytest.mark.gpu

SHAPES = ((128, 63, False), (256, 256, True), (1024, 200, False))
CODE_DTYPE = {"bf16": np.uint16, "fp8": np.uint8, "int4": np.int8}


def weight(K, N, glu, seed=0):
    """Uniform in +-K^-1/2 (test_fused_linear_gpu._inputs' draw), column 1 all zero, column 2 x 100."""
    w = np.random.default_rng(seed + K + N).uniform(-K ** -0.5, K ** -0.5, (K, 2 * N if glu else N)).astype(np.float32)
    w[:, 1] = 0.0
    w[:, 2] *= 100.0
    return w


def roundtrip(w, fmt, glu):
    """(W', codes, scales) as numpy arrays."""
    import torch
    from minitorch import QuantizedWeight
    q = QuantizedWeight.from_tensor(torch.from_numpy(w).cuda(), fmt, glu)
    codes = torch.empty(w.shape, dtype={"bf16": torch.uint16, "fp8": torch.uint8, "int4": torch.int8}[fmt], device="cuda")
    wd = q.dequantize(codes_out=codes)
    assert (q.K, q.ncols, q.glu, q.fmt) == (*w.shape, glu, fmt)
    return wd.cpu().numpy(), codes.cpu().numpy().view(CODE_DTYPE[fmt]), None if q.scales is None else q.scales.cpu().numpy()


@pytest.mark.parametrize("K,N,glu", SHAPES)
def test_bf16(K, N, glu):
    w = weight(K, N, glu)
    wd, codes, _ = roundtrip(w, "bf16", glu)
    u = w.view(np.uint32).astype(np.uint64)
    want = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)  # round to nearest even
    assert np.array_equal(codes, want)
    assert np.array_equal(wd.view(np.uint32), codes.astype(np.uint32) << 16)


@pytest.mark.parametrize("K,N,glu", SHAPES)
def test_fp8(K, N, glu):
    w = weight(K, N, glu)
    wd, codes, scales = roundtrip(w, "fp8", glu)
    assert scales.shape == (w.shape[1],) and len(np.unique(scales)) > 2
    print("worst half-spacings off:", Q.check_fp8_rows(w.T, codes.T, scales))
    assert np.array_equal(wd.view(np.uint32), (Q.E4M3_F32[codes] * scales[None, :]).view(np.uint32))


@pytest.mark.parametrize("K,N,glu", SHAPES)
def test_int4(K, N, glu):
    w = weight(K, N, glu)
    wd, codes, scales = roundtrip(w, "int4", glu)
    assert scales.shape == (K // 32, w.shape[1])
    grouped = w.reshape(K // 32, 32, -1)
    cg = codes.reshape(K // 32, 32, -1).astype(np.float64)
    amax = np.abs(grouped).max(1)
    zero = amax == 0
    assert zero[:, 1].all() and (scales[zero] == 1.0).all() and not cg.transpose(0, 2, 1)[zero].any()
    want = (amax / np.float32(7.0)).astype(np.float32)
    assert (np.abs(scales.astype(np.float64) - want)[~zero] <= 2 * np.spacing(want)[~zero]).all(), "scale != amax / 7"
    y = grouped.astype(np.float64) / scales.astype(np.float64)[:, None, :]
    err = np.abs(cg - y)
    print("worst |code - W / s|:", float(err.max()))
    assert (err <= 0.5 * (1 + 2.0 ** -20)).all()
    assert (np.abs(cg) <= 7).all() and (np.abs(cg).max(1)[~zero] == 7).all()
    sfull = np.repeat(scales, 32, axis=0)
    assert np.array_equal(wd.view(np.uint32), (codes.astype(np.float32) * sfull).view(np.uint32))
