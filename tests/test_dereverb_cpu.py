"""WPE de-reverberation without a GPU: a property of the specification tests/dereverb_spec.py, and
the pure host functions of the library."""
import os
import sys

import numpy as np
import pytest
import scipy.signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dereverb_spec  # noqa: E402


def test_a_known_late_tail_on_white_noise_is_taken_out():
    rng = np.random.default_rng(0)
    n = 100 * 1024
    dry = rng.standard_normal((2, n))
    tail = np.zeros((2, 14000))  # late reflections only, behind the prediction delay of 3 hops and the window
    tail[:, 6000:] = 0.5 * rng.standard_normal((2, 8000)) * np.exp(-np.arange(8000) / 3000.0)
    wet = np.stack([dry[c] + scipy.signal.fftconvolve(dry[c], tail[c])[:n] for c in range(2)]).astype(np.float32)
    out = dereverb_spec.dereverb(wet[None], 10, 3, 3)[0]
    before, after = np.sqrt(((wet - dry) ** 2).mean()), np.sqrt(((out - dry) ** 2).mean())
    print("rms distance from the dry signal: in", before, "out", after)
    assert after < before


def test_host_functions_check_the_arguments_and_size_the_workspace():
    from demucs_cpp_amd import binding as dmx
    ok = dmx.DereverbSpec()
    dmx.dereverb_check(ok, 4, 2, 2049)
    for field, args in (("taps", (dmx.DereverbSpec(0), 2, 2, 5000)), ("taps", (dmx.DereverbSpec(17), 2, 2, 5000)),
                        ("delay", (dmx.DereverbSpec(10, 0), 2, 2, 5000)), ("delay", (dmx.DereverbSpec(10, 9), 2, 2, 5000)),
                        ("iterations", (dmx.DereverbSpec(10, 3, 0), 2, 2, 5000)), ("iterations", (dmx.DereverbSpec(10, 3, 9), 2, 2, 5000)),
                        ("eps", (dmx.DereverbSpec(10, 3, 3, 0.0), 2, 2, 5000)), ("reg", (dmx.DereverbSpec(10, 3, 3, 1e-10, -1.0), 2, 2, 5000)),
                        ("n_sources", (ok, 9, 2, 5000)), ("n 2048", (ok, 2, 2, 2048)), ("channels", (ok, 2, 3, 5000))):
        with pytest.raises(dmx.DmxError) as e:
            dmx.dereverb_check(*args)
        assert e.value.code == 5 and field in str(e.value)
        assert dmx.dereverb_workspace_bytes(*args) == -1
    # dereverb_plan.h at the defaults on 4 minutes: 4 ranges of frames, 3 row tiles -> 6 tiles of 256 doubles per partial
    J, C, n = 4, 2, 240 * 44100
    T = 1 + n // 1024
    parts = [2048 * 8, 4096 * 4, J * T * 8, J * 8, J * C * T * 2064 * 8, J * C * T * 2064 * 8, J * T * 2064 * 8,
             J * 2049 * 4 * 6 * 256 * 8, J * 2049 * 20 * C * 16]
    assert dmx.dereverb_workspace_bytes(ok, J, C, n) == sum((p + 255) // 256 * 256 for p in parts)
