"""The Wiener post-filter on the GPU (csrc/wiener.hip): binding.wiener against the complex128 mode of
tests/wiener_spec.py by max |out - ref| / max |ref|, within 8 x the distance of the specification's own float32 mode (STFT and
inverse in single precision through pocketfft) from its complex128 mode. Those distances, measured on the CPU with the
committed specification, are the constants D below."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wiener_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402

pytestmark = pytest.mark.gpu

# name: J, C, N, iterations, residual, win_len, amplitude, zero head, D
CASES = {
    "two_blocks": (2, 2, 7 * 1024 + 123, 1, 0, 5, 0.3, 0, 1.2096986156868878e-06),
    "nine_sources": (5, 2, 7 * 1024 + 123, 3, 1, 5, 0.3, 0, 9.555844354407155e-07),
    "mono_quiet": (3, 1, 9 * 1024 + 1, 2, 0, 4, 1e-3, 0, 2.2813993556111473e-07),
    "short_block": (4, 2, 12 * 1024, 2, 0, 300, 0.3, 0, 4.813636531676039e-07),
    "zero_head": (2, 2, 7 * 1024 + 123, 1, 0, 5, 0.3, 6000, 2.7415250019160215e-07),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """seeded Gaussian sources, their sum as the mixture, estimates = sources + 30 % noise; source 0 silent on 2000 .. 5000,
    source 1's right channel 0.7 x its left (a rank-one R); the reference, computed once"""
    J, C, N, it, res, wl, amp, head, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    src = amp * rng.standard_normal((J, C, N))
    est = src + 0.3 * amp * rng.standard_normal((J, C, N))
    src[:, :, :head] = 0.0  # zero_head: the mixture is zero there, X = 0 in the first frames
    for a in (src, est):
        a[0, :, 2000:5000] = 0.0
        if C == 2 and J > 1:
            a[1, 1] = 0.7 * a[1, 0]
    mix, est = src.sum(axis=0).astype(np.float32), est.astype(np.float32)
    ref = wiener_spec.wiener(mix, est, it, bool(res), wl)
    for a in (mix, est, ref):
        a.setflags(write=False)
    return mix, est, ref


def distance(out, ref):
    return float(np.abs(out.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_wiener_equals_the_specification(name):
    J, C, N, it, res, wl, _, _, D = CASES[name]
    mix, est, ref = case(name)
    out = dmx.wiener(mix, est, it, bool(res), wl)
    err = distance(out, ref)
    print(name, "max error / max |ref|", err, "bound", 8 * D)
    assert out.shape == (J, C, N) and out.dtype == np.float32
    assert err <= 8 * D


def test_equal_bits_twice_and_on_a_stream_of_the_caller():
    import torch
    name = "nine_sources"
    J, C, N, it, res, wl = CASES[name][:6]
    mix, est, _ = case(name)
    first, again = dmx.wiener(mix, est, it, bool(res), wl), dmx.wiener(mix, est, it, bool(res), wl)
    assert first.tobytes() == again.tobytes()
    spec = dmx.WienerSpec(it, res, wl)
    nbytes = dmx.wiener_workspace_bytes(spec, J, C, N)
    d_mix, d_est = torch.tensor(mix).cuda(), torch.tensor(est).cuda()
    d_out, d_work = torch.empty_like(d_est), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    args = [0, d_mix.data_ptr(), d_est.data_ptr(), J, C, N, N, ctypes.byref(spec), d_out.data_ptr(), d_work.data_ptr()]
    with pytest.raises(dmx.DmxError, match="work_bytes"):
        dmx._chk(dmx.lib().dmx_wiener_device(*args, nbytes - 1, stream.cuda_stream))
    dmx._chk(dmx.lib().dmx_wiener_device(*args, nbytes, stream.cuda_stream))
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == first.tobytes()
