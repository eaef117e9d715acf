"""Time stretch and pitch shift without a GPU: the pure host functions of the library."""
from fractions import Fraction

import pytest

from demucs_cpp_amd import binding as dmx


def test_check_names_the_field_and_the_workspace_refuses_a_bad_spec():
    S = dmx.StretchSpec
    dmx.stretch_check(S(), 8, 2, 2049)
    dmx.stretch_check(S(1, 4, 196, 185), 1, 1, 5000)
    for field, args in (("num", (S(0, 1), 2, 2, 5000)), ("den", (S(1, (1 << 20) + 1), 2, 2, 5000)), ("pitch_num", (S(1, 1, 0, 1), 2, 2, 5000)),
                        ("pitch_den", (S(1, 1, 1, -3), 2, 2, 5000)), ("num / den", (S(9, 2), 2, 2, 5000)), ("num / den", (S(2, 9), 2, 2, 5000)),
                        ("n_sources", (S(), 9, 2, 5000)), ("channels", (S(), 2, 3, 5000)), ("n 2048", (S(), 2, 2, 2048)),
                        ("stretched length", (S(4, 1), 2, 2, 8192)), ("stretched length", (S(1, 4), 2, 2, 1 << 30)),
                        ("pitch_num / pitch_den = 1000000 / 999983: resample", (S(1, 1, 1000000, 999983), 2, 2, 5000))):
        with pytest.raises(dmx.DmxError) as e:
            dmx.stretch_check(*args)
        assert e.value.code == 5 and field in str(e.value)
        assert dmx.stretch_workspace_bytes(*args) == -1
    with pytest.raises(dmx.DmxError, match="null spec"):
        dmx.stretch_check(None, 2, 2, 5000)


def test_length_and_workspace_follow_the_plan():
    S = dmx.StretchSpec
    assert dmx.stretch_length(S(4, 5), 41083) == -(-41083 * 5 // 4) == 51354
    assert dmx.stretch_length(S(185, 196, 196, 185), 65537) == -(-(-(-65537 * 196 // 185)) * 185 // 196) == 65538
    assert dmx.stretch_length(S(9, 2), 5000) == -1 and dmx.stretch_length(S(), -1) == -1
    # stretch_plan.h on 4 minutes a semitone up: the tables, the flags of the all-zero frames, D, a complex128 row per plane and
    # chunk of 12 output frames, the planes ahead of the converter
    J, C, n = 4, 2, 240 * 44100
    n2 = -(-n * 196 // 185)
    T, chunks = 1 + n // 1024, -(-(1 + n2 // 1024) // 12)
    parts = [2048 * 8, 4096 * 4, T * 8, J * C * T * 4, J * C * T * 2064 * 8, J * C * chunks * 2064 * 16, J * C * ((n2 + 63) // 64 * 64) * 4]
    assert dmx.stretch_workspace_bytes(S(185, 196, 196, 185), J, C, n) == sum((p + 255) // 256 * 256 for p in parts)
    assert dmx.stretch_workspace_bytes(S(185, 196), J, C, n) == sum((p + 255) // 256 * 256 for p in parts[:6])


@pytest.mark.parametrize("value,max_den", [(2.0 ** (s / 12.0), 512) for s in range(-12, 13) if s] +
                         [(0.25, 4096), (0.9, 4096), (1.0, 4096), (4.0, 4096), (1.0 / 3.0, 2), (2.5, 1), (44100.0 / 48000.0, 100)])
def test_ratio_is_the_nearest_fraction_with_the_smaller_denominator_on_ties(value, max_den):
    v = Fraction(value)  # exact
    want = min(((abs(v - Fraction(max(1, round(v * d)), d)), d, max(1, round(v * d))) for d in range(1, max_den + 1)))
    num, den = dmx.stretch_ratio(value, max_den)
    assert abs(v - Fraction(num, den)) == want[0] and den == want[1] and Fraction(num, den).denominator == den
