"""The Wiener post-filter without a GPU: two properties of the specification tests/wiener_spec.py,
and the pure host functions of the library."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wiener_spec  # noqa: E402


def test_one_source_returns_the_mixture_and_the_stems_sum_to_it():
    rng = np.random.default_rng(0)
    mix = rng.standard_normal((2, 5000)).astype(np.float32)  # loud: s > 1
    peak = float(np.abs(mix).max())
    one = wiener_spec.wiener(mix, (0.5 * mix + 0.1 * rng.standard_normal(mix.shape))[None].astype(np.float32), 2, False, 3)
    assert np.abs(one[0] - mix).max() <= 1e-4 * peak
    ests = rng.standard_normal((3, 2, 5000)).astype(np.float32)
    out = wiener_spec.wiener(mix, ests, 2, False, 3)
    # Cxx^-1 x is x up to the sqrt(eps) regularisation; a draft gave 8e-6 of the peak on loud noise
    assert np.abs(out.sum(axis=0) - mix).max() <= 1e-4 * peak
    assert np.abs(out[0] - ests[0]).max() > 0.1 * peak  # not the identity


def test_host_functions_check_the_arguments_and_size_the_workspace():
    from demucs_cpp_amd import binding as dmx
    ok = dmx.WienerSpec(1, False, 300)
    dmx.wiener_check(ok, 4, 2, 2049)
    for field, args in (("iterations", (dmx.WienerSpec(0), 2, 2, 5000)), ("iterations", (dmx.WienerSpec(9), 2, 2, 5000)),
                        ("win_len", (dmx.WienerSpec(1, False, 0), 2, 2, 5000)), ("n_sources", (ok, 9, 2, 5000)),
                        ("n 2048", (ok, 2, 2, 2048)), ("channels", (ok, 2, 3, 5000))):
        with pytest.raises(dmx.DmxError) as e:
            dmx.wiener_check(*args)
        assert e.value.code == 5 and field in str(e.value)
        assert dmx.wiener_workspace_bytes(*args) == -1
    # wiener_plan.h: the twiddles, the window, max |X|^2 per frame, (1 + J + residual) C planes of T rows of 2064 complex64
    for J, C, n, res in ((4, 2, 240 * 44100, 0), (3, 1, 9 * 1024 + 1, 1)):
        T = 1 + n // 1024
        parts = [2048 * 8, 4096 * 4, T * 8, (1 + J + res) * C * T * 2064 * 8]
        assert dmx.wiener_workspace_bytes(dmx.WienerSpec(1, res, 300), J, C, n) == sum((p + 255) // 256 * 256 for p in parts)
