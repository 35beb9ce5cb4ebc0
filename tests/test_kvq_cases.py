"""The host helpers of the quantised KV cache tests (tests/kvq_cases.py), on the CPU: the e4m3
table against torch's float8_e4m3fn, the bf16 decode, and the host quantiser against the rule
the GPU test holds mt_kv_cache_append_quant to (so that rule is one a correct quantiser meets)."""
import numpy as np
import pytest

import kvq_cases as KC


def test_e4m3_table_is_torchs_e4m3fn():
    import torch
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    nan = np.isnan(KC.E4M3)
    assert sorted(np.flatnonzero(nan)) == sorted(KC.NAN_CODES)
    assert np.isnan(ref[nan]).all()
    assert np.array_equal(KC.E4M3_F32[~nan].view(np.uint32), ref[~nan].view(np.uint32))
    assert KC.E4M3[0x7E] == 448.0 and KC.E4M3[0xFE] == -448.0 and KC.E4M3[1] == 2.0 ** -9
    # torch's own conversion: 0.3 -> 0.3125 (code 42), -448 -> code 254
    got = torch.tensor([0.3, -448.0]).to(torch.float8_e4m3fn).view(torch.uint8).tolist()
    assert got == [42, 254] and KC.E4M3[42] == 0.3125


def test_spacing_is_the_gap_between_neighbouring_codes():
    pos = KC.E4M3[:0x7F]
    gaps = np.diff(pos)
    mid = (pos[1:] + pos[:-1]) / 2
    assert np.array_equal(KC.e4m3_spacing(mid), gaps)
    assert KC.e4m3_spacing(np.array([0.0, 448.0, 449.0])).tolist() == [2.0 ** -9, 32.0, 32.0]


def test_bf16_decode_by_shift():
    import torch
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1)).bfloat16()
    assert np.array_equal(KC.bf16_decode(x.view(torch.int16).numpy().view(np.uint16)), x.float().numpy())


@pytest.mark.parametrize("d", [8, 40, 64, 256])
def test_host_quantiser_meets_the_round_to_nearest_rule(d):
    lengths = (1, 257, 1100)
    _, k, v = KC.make_inputs(d, 3, False, lengths)
    for x in (k, v):
        x = x.copy()
        x[0, 0, 7] = 0.0  # an all-zero row
        codes, scales = KC.quantise_fp8(x)
        worst = KC.check_fp8_rows(x, codes, scales)
        assert worst <= 1.0 + 2.0 ** -20
        dq = KC.dequant(KC.KV_FP8, codes, scales)
        # a round trip moves an element by at most half a spacing of its row: amax / 448 * 16
        assert (np.abs(dq - x) <= np.abs(x).max(-1, keepdims=True) / 448.0 * 16.0 * (1 + 1e-6)).all()


def test_rule_rejects_a_truncating_quantiser():
    """The rule is not vacuous: codes rounded toward zero break it."""
    x = KC.make_inputs(64, 1, False, (5,))[1][0, 0, :64]
    codes, scales = KC.quantise_fp8(x)
    y = np.abs(x.astype(np.float64) / scales.astype(np.float64)[:, None])
    down = (np.searchsorted(KC.E4M3[:0x7F], y, side="right") - 1).astype(np.uint8) | (codes & 0x80)
    assert (down != codes).any()
    with pytest.raises(AssertionError):
        KC.check_fp8_rows(x, down, scales)
