"""Host side of the quantised KV cache tests (test infrastructure; tests/test_kvq_cases.py runs
it on the CPU, tests/test_kvq_gpu.py holds the kernels to it).

Formats, from their definitions: OCP e4m3 ("e4m3fn"): 1 sign, 4 exponent (bias 7), 3 mantissa
bits; exponent 0 is subnormal (m / 8 * 2^-6); no infinities; exponent 15 with mantissa 7 is NaN
(0x7F, 0xFF), so the largest value is 1.75 * 2^8 = 448. bf16: the upper 16 bits of an fp32.

An fp8 cache row holds codes and one fp32 scale s: its values are fp32(e4m3(code) * s). The
append's rule for a row x of d elements: amax = max |x|, s = amax / 448 (1 for an all-zero row),
code = e4m3 round-to-nearest of x / s.

The inputs are those of tests/decode_cases.py (imported, not copied).
"""
import numpy as np

from decode_cases import EDGE_LENGTHS, H, NMAX, bound, limits, make_inputs, ref64, visible  # noqa: F401

KV_BF16, KV_FP8 = 1, 2
E4M3_MAX = 448.0


def _e4m3_table():
    t = np.empty(256, np.float64)
    for code in range(256):
        sign = -1.0 if code & 0x80 else 1.0
        e, m = (code >> 3) & 0xF, code & 0x7
        if e == 15 and m == 7:
            t[code] = np.nan
        elif e == 0:
            t[code] = sign * (m / 8.0) * 2.0 ** -6
        else:
            t[code] = sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return t


E4M3 = _e4m3_table()            # float64 value of every code (exact: 4 significant bits)
E4M3.setflags(write=False)
E4M3_F32 = E4M3.astype(np.float32)
E4M3_F32.setflags(write=False)
NAN_CODES = (0x7F, 0xFF)


def e4m3_spacing(y):
    """The distance between neighbouring e4m3 values around |y| (float64 array): 2^-9 below the
    smallest normal 2^-6, else 2^(floor(log2 |y|) - 3), the last binade's (2^5) from 256 up."""
    a = np.abs(np.asarray(y, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))
    return 2.0 ** (np.minimum(e, 8.0) - 3.0)


def bf16_decode(u16):
    """uint16 bf16 bit patterns -> float32, by shift."""
    return (np.asarray(u16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def dequant(kv_dtype, cache, scales=None):
    """The fp32 values of a cache read back from the device: bf16 bit patterns (uint16 [..., d])
    widened, or e4m3 codes (uint8 [..., d]) times the row scales (float32 [...]): one fp32
    product, what mt_kv_cache_dequant computes."""
    if kv_dtype == KV_BF16:
        return bf16_decode(cache)
    return E4M3_F32[np.asarray(cache, np.uint8)] * np.asarray(scales, np.float32)[..., None]


def quantise_fp8(x):
    """(codes uint8 [..., d], scales float32 [...]) of fp32 rows x [..., d] by the append's rule,
    on the host: x / s in fp32, the nearest e4m3 value (ties to the even code)."""
    x = np.asarray(x, np.float32)
    amax = np.abs(x).max(-1)
    s = np.where(amax > 0, amax / np.float32(E4M3_MAX), np.float32(1.0)).astype(np.float32)
    y = (x / s[..., None]).astype(np.float32).astype(np.float64)
    pos = E4M3[:0x7F]                                    # the 127 non-negative values, ascending
    i = np.clip(np.searchsorted(pos, np.abs(y)), 1, 126)
    lo, hi = pos[i - 1], pos[i]
    up = (np.abs(y) - lo > hi - np.abs(y)) | ((np.abs(y) - lo == hi - np.abs(y)) & (i % 2 == 0))
    code = np.where(up, i, i - 1).astype(np.uint8)
    return code | np.where(np.signbit(y), 0x80, 0).astype(np.uint8), s


def check_fp8_rows(x, codes, scales):
    """The append's contract on fp32 rows x [..., d] and what was stored for them. Returns the
    worst |value - y| / (half spacing) over the elements (<= 1 + 2^-20 asserted here)."""
    x = np.asarray(x, np.float32)
    codes, scales = np.asarray(codes, np.uint8), np.asarray(scales, np.float32)
    assert not np.isin(codes, NAN_CODES).any(), "a NaN code for a finite row"
    amax = np.abs(x).max(-1)
    zero = amax == 0
    assert (scales[zero] == 1.0).all() and not codes[zero].any(), "an all-zero row: scale 1, codes 0"
    want = (amax / np.float32(E4M3_MAX)).astype(np.float32)
    ulp = np.spacing(want)
    assert (np.abs(scales[~zero].astype(np.float64) - want[~zero]) <= 2 * ulp[~zero]).all(), "scale != amax / 448"
    y = x.astype(np.float64) / scales.astype(np.float64)[..., None]
    val = E4M3[codes]
    ratio = np.abs(val - y) / (0.5 * e4m3_spacing(y))
    assert (ratio <= 1.0 + 2.0 ** -20).all(), f"not the nearest e4m3 value: {float(ratio.max())} half-spacings off"
    assert (np.abs(val).max(-1)[~zero] == E4M3_MAX).all(), "the largest element of a row must land on 448"
    return float(ratio.max())
