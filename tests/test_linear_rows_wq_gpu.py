"""mt_linear_rows_wq (through _hip.fused_linear on QuantizedWeights) against the fp32 kernel on the
dequantised weights W', bit for bit, and against the float64 restatements of
tests/test_fused_linear_gpu.py and tests/test_fused_linear_glu_gpu.py on W' (imported, with their
bounds: (K + 8) 2^-24 (|xh| @ |W'| + |bias| + |residual|), the gated rule of the second file for
the gate, and the first file's ATOL where a norm, GELU or the gate is on). Row independence is
the fp32 kernel's, inherited through the bit equality."""
import numpy as np
import pytest

import test_fused_linear_glu_gpu as G
from test_fused_linear_gpu import ATOL, ref64 as ref_plain

pytestmark = pytest.mark.gpu

FORMATS = ("bf16", "fp8", "int4")
MS = (1, 17, 64)
KNS = ((128, 63), (256, 256), (1024, 200))
FUSIONS = ("ln+bias", "rms+glu", "bias+gelu", "bias+residual")
CASES = [(f, m, kn, FUSIONS[(a + i + j) % 4]) for a, f in enumerate(FORMATS) for i, m in enumerate(MS)
         for j, kn in enumerate(KNS)]


def _both(d, fmt, fusion):
    """(outputs on the QuantizedWeights, outputs of the fp32 kernel on W', the W' as numpy) for all of d's groups."""
    import torch
    from minitorch import QuantizedWeight, _hip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    glu, groups = "glu" in fusion, range(len(d["W"]))
    half = lambda a: a if glu else a[..., :a.shape[-1] // 2]  # noqa: E731
    qs = [QuantizedWeight.from_tensor(dev(half(d["W"][g])), fmt, glu) for g in groups]
    wd = [q.dequantize() for q in qs]
    kw = dict(biases=[dev(half(d["bias"][g])) for g in groups] if "bias" in fusion else None,
              residuals=[dev(d["res"][g]) for g in groups] if "residual" in fusion else None,
              gelu="gelu" in fusion, glu=glu)
    if "ln" in fusion:
        kw.update(gamma=dev(d["gamma"]), beta=dev(d["beta"]))
    if "rms" in fusion:
        kw.update(gamma=dev(d["gamma"]), norm="rms", eps=G.EPS)
    x = dev(d["x"])
    calls = _hip.fused_linear_calls
    got = [o.cpu().numpy() for o in _hip.fused_linear(x, qs, **kw)]
    assert _hip.fused_linear_calls == calls + 1
    return got, [o.cpu().numpy() for o in _hip.fused_linear(x, wd, **kw)], [w.cpu().numpy() for w in wd]


def _check(d, fmt, fusion):
    got, fp32, wd = _both(d, fmt, fusion)
    K = d["x"].shape[1]
    for g in range(len(wd)):
        assert np.array_equal(got[g].view(np.uint32), fp32[g].view(np.uint32)), "not the fp32 kernel's bits on W'"
        if "glu" in fusion:
            want, bound = G.ref64(dict(d, W=wd), g, fusion)
        else:
            n = wd[g].shape[1]
            want, mag = ref_plain(d["x"], wd[g], d["bias"][g][:n] if "bias" in fusion else None,
                                  d["res"][g] if "residual" in fusion else None,
                                  (d["gamma"], d["beta"]) if "ln" in fusion else None, "gelu" in fusion)
            bound = (K + 8) * 2.0 ** -24 * mag
        if fusion != "bias+residual":
            bound = bound + ATOL
        err = np.abs(got[g] - want)
        print(f"{fmt} {fusion} group {g}: max err {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f}")
        assert got[g].shape == want.shape and (err <= bound).all()


@pytest.mark.parametrize("fmt,M,kn,fusion", CASES)
def test_parity(fmt, M, kn, fusion):
    _check(G._inputs(M, kn[0], [kn[1]], seed=M * 4099 + kn[0] + kn[1]), fmt, fusion)


@pytest.mark.parametrize("fmt", FORMATS)
def test_parity_grouped_gqa_projection(fmt):
    """G = 3 with N_g = (64, 16, 16): the Q / K / V launch of a width-128 model with one kv head."""
    _check(G._inputs(5, 128, [64, 16, 16], seed=7), fmt, "ln+bias")
