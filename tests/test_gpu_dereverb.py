"""WPE de-reverberation on the GPU (csrc/dereverb.hip): binding.dereverb against the complex128 mode of
tests/dereverb_spec.py by max |out - ref| / max |ref|, within 8 x the distance of the specification's own float32 mode (STFT
and inverse in single precision through pocketfft) from its complex128 mode. Those distances, measured on the CPU with the
committed specification, are the constants D below."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import scipy.signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dereverb_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402

pytestmark = pytest.mark.gpu

# name: J, C, N, taps, delay, iterations, zero stem, D
CASES = {
    "small": (2, 2, 40 * 1024 + 123, 3, 2, 2, False, 5.004051661486218e-07),
    "defaults": (1, 2, 64 * 1024 + 1, 10, 3, 2, False, 1.0594214902808344e-06),
    "mono": (2, 1, 48 * 1024, 4, 1, 1, False, 2.595271329129282e-07),
    "widest": (1, 2, 48 * 1024, 16, 8, 1, False, 4.153266816349317e-07),
    "short": (1, 2, 7 * 1024 + 5, 10, 3, 2, False, 1.7691035094502414e-07),
    "silent_stem": (2, 2, 40 * 1024 + 123, 3, 2, 2, True, 2.389487212061813e-07),
}


def stems(name):
    """seeded Gaussian sources, each channel convolved with its own exponentially decaying 6000-tap impulse response; the last
    stem's source is silent on 6000 .. 30000, so its frames between the tail and the restart are exact zeros (the floor is
    reached); with `zero stem` stem 0 is all zeros"""
    J, C, N, _, _, _, zero, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    src = 0.3 * rng.standard_normal((J, N))
    src[J - 1, 6000:30000] = 0.0
    h = rng.standard_normal((J, C, 6000)) * np.exp(-np.arange(6000) / 1500.0) * 0.2
    h[:, :, 0] = 1.0
    x = np.stack([[scipy.signal.fftconvolve(src[j], h[j, c])[:N] for c in range(C)] for j in range(J)])
    if zero:
        x[0] = 0.0
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """the input and the reference, computed once"""
    taps, delay, it = CASES[name][3:6]
    x = stems(name)
    ref = dereverb_spec.dereverb(x, taps, delay, it)
    for a in (x, ref):
        a.setflags(write=False)
    return x, ref


def distance(out, ref):
    return float(np.abs(out.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_dereverb_equals_the_specification(name):
    J, C, N, taps, delay, it, zero, D = CASES[name]
    x, ref = case(name)
    out = dmx.dereverb(x, dmx.DereverbSpec(taps, delay, it))
    err = distance(out, ref)
    print(name, "max error / max |ref|", err, "bound", 8 * D)
    assert out.shape == (J, C, N) and out.dtype == np.float32
    assert err <= 8 * D
    if zero:
        assert not out[0].any() and out[1].any()


def test_equal_bits_twice_and_on_a_stream_of_the_caller():
    import torch
    name = "small"
    J, C, N, taps, delay, it = CASES[name][:6]
    x, _ = case(name)
    spec = dmx.DereverbSpec(taps, delay, it)
    first, again = dmx.dereverb(x, spec), dmx.dereverb(x, spec)
    assert first.tobytes() == again.tobytes()
    nbytes = dmx.dereverb_workspace_bytes(spec, J, C, N)
    d_x = torch.tensor(x).cuda()
    d_out, d_work = torch.empty_like(d_x), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    args = [0, d_x.data_ptr(), J, C, N, N, ctypes.byref(spec), d_out.data_ptr(), d_work.data_ptr()]
    with pytest.raises(dmx.DmxError, match="work_bytes"):
        dmx._chk(dmx.lib().dmx_dereverb_device(*args, nbytes - 1, stream.cuda_stream))
    dmx._chk(dmx.lib().dmx_dereverb_device(*args, nbytes, stream.cuda_stream))
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == first.tobytes()


def test_timed_call_fills_its_entries_and_keeps_the_bits():
    import torch
    name = "small"
    J, C, N, taps, delay, it = CASES[name][:6]
    x, _ = case(name)
    spec = dmx.DereverbSpec(taps, delay, it)
    nbytes = dmx.dereverb_workspace_bytes(spec, J, C, N)
    d_x = torch.tensor(x).cuda()
    d_out, d_work = torch.empty_like(d_x), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    args = [0, d_x.data_ptr(), J, C, N, N, ctypes.byref(spec), d_out.data_ptr(), d_work.data_ptr(), nbytes, None]
    ms = (ctypes.c_float * (it + 3))(*([-1.0] * (it + 3)))
    dmx._chk(dmx.lib().dmx_dereverb_device_timed(*args, ms))
    got = list(ms)
    assert all(np.isfinite(v) and v >= 0.0 for v in got[:it + 2]) and got[it + 2] == -1.0
    assert d_out.cpu().numpy().tobytes() == dmx.dereverb(x, spec).tobytes()
    with pytest.raises(dmx.DmxError, match="null ms pointer") as e:
        dmx._chk(dmx.lib().dmx_dereverb_device_timed(*args, None))
    assert e.value.code == 5  # DMX_ERR_ARG
