"""Time stretch and pitch shift on the GPU (csrc/stretch.hip): binding.stretch against the complex128
mode of tests/stretch_spec.py by max |out - ref| / max |ref|, within 8 x the distance of the specification's own float32 mode
(STFT and inverse in single precision through pocketfft) from its complex128 mode. Those distances, measured on the CPU with
the committed specification, are the constants D below. The phase of a weak bin is ill-conditioned, so the inputs are broadband:
every bin of every non-zero frame stays far above the transform's rounding floor."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stretch_spec  # noqa: E402
import wiener_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402

pytestmark = pytest.mark.gpu

N = 40 * 1024 + 123
# name: J, C, n, num, den, semitones up, D
CASES = {
    "slow": (2, 2, N, 4, 5, 0, 8.39063611655441e-06),
    "fast": (2, 2, N, 5, 4, 0, 1.2153441053809146e-06),
    "identity": (2, 2, N, 1, 1, 0, 2.41899557885016e-07),
    "mono": (1, 1, 7 * 1024 + 5, 3, 2, 0, 3.219125830928807e-07),
    "zeros": (2, 2, N, 4, 5, 0, 3.117602089233044e-06),
    "semitone": (1, 2, 64 * 1024 + 1, 0, 0, 1, 8.735386996736913e-06),
    "coprime": (1, 2, N, 185, 196, 0, 7.21958936991812e-06),
}


def spec_of(name):
    """the StretchSpec of a case; a pitch change at the tempo 1: the converter p -> q with p / q ~ 2^(s / 12) behind the rate q / p"""
    num, den, semis = CASES[name][3:6]
    if not semis:
        return dmx.StretchSpec(num, den)
    p, q = dmx.stretch_ratio(2.0 ** (semis / 12.0), 512)
    return dmx.StretchSpec(q, p, p, q)


def stems(name):
    """seeded Gaussian noise and two tones per plane; `zeros`: stem 0 is all zero and 14000 samples of stem 1's first channel are"""
    J, C, n = CASES[name][:3]
    rng = np.random.default_rng(sorted(CASES).index(name))
    t = np.arange(n)
    x = 0.2 * rng.standard_normal((J, C, n)) + 0.3 * np.sin(2 * np.pi * 440.0 / 44100.0 * t) + 0.2 * np.sin(2 * np.pi * 0.31 * t)
    if name == "zeros":
        x[0] = 0.0
        x[1, 0, 6000:20000] = 0.0
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, dtype=np.float64):
    """the input and the reference, computed once"""
    s = spec_of(name)
    x = stems(name)
    taps = dmx.resample_filter(s.pitch_num, s.pitch_den)[2] if s.pitch_num != s.pitch_den else None
    ref = stretch_spec.stretch(x, s.num, s.den, s.pitch_num, s.pitch_den, taps, dtype)
    for a in (x, ref):
        a.setflags(write=False)
    return x, ref


def distance(out, ref):
    return float(np.abs(out.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_stretch_equals_the_specification(name):
    J, C, n = CASES[name][:3]
    D = CASES[name][6]
    x, ref = case(name)
    s = spec_of(name)
    out = dmx.stretch(x, s)
    err = distance(out, ref)
    print(name, "max error / max |ref|", err, "bound", 8 * D)
    assert out.shape == ref.shape == (J, C, dmx.stretch_length(s, n)) and out.dtype == np.float32
    assert err <= 8 * D
    if name == "identity":  # the product telescopes: ph[t] = unit(D[t]), Y = D
        assert out.shape == x.shape and distance(out, wiener_spec.istft(wiener_spec.stft(x), n)) <= 8 * D
    if name == "zeros":
        assert not out[0].any() and out[1].any()
    if name == "semitone":
        assert abs(out.shape[-1] - n) <= 1


def test_equal_bits_on_a_stream_of_the_caller_and_in_the_timed_call():
    import torch
    name = "semitone"
    J, C, n = CASES[name][:3]
    x, _ = case(name)
    s = spec_of(name)
    first, again = dmx.stretch(x, s), dmx.stretch(x, s)
    assert first.tobytes() == again.tobytes()
    nbytes, m = dmx.stretch_workspace_bytes(s, J, C, n), dmx.stretch_length(s, n)
    d_x = torch.tensor(x).cuda()
    d_out, d_work = torch.empty((J, C, m), device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    args = [0, d_x.data_ptr(), J, C, n, n, ctypes.byref(s), d_out.data_ptr(), m, d_work.data_ptr()]
    with pytest.raises(dmx.DmxError, match="work_bytes"):
        dmx._chk(dmx.lib().dmx_stretch_device(*args, nbytes - 1, stream.cuda_stream))
    dmx._chk(dmx.lib().dmx_stretch_device(*args, nbytes, stream.cuda_stream))
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == first.tobytes()
    d_out.zero_()
    ms = (ctypes.c_float * 5)(*([-1.0] * 5))
    dmx._chk(dmx.lib().dmx_stretch_device_timed(*args, nbytes, None, ms))
    got = list(ms)
    assert all(np.isfinite(v) and v >= 0.0 for v in got[:4]) and got[4] == -1.0
    assert d_out.cpu().numpy().tobytes() == first.tobytes()
    with pytest.raises(dmx.DmxError, match="null ms pointer") as e:
        dmx._chk(dmx.lib().dmx_stretch_device_timed(*args, nbytes, None, None))
    assert e.value.code == 5  # DMX_ERR_ARG
