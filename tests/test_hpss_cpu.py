"""Harmonic/percussive split without a GPU: the pure host functions of the library, and the
specification's medians against SciPy's median filter."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpss_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402


def test_check_names_the_field_and_the_workspace_follows_the_plan():
    S = dmx.HpssSpec
    dmx.hpss_check(S(), 8, 2, 2049)
    dmx.hpss_check(S(3, 17, 8, 100.0, 1.0, 1), 1, 1, 5000)
    for field, args in (("kernel_h", (S(kernel_h=33), 2, 2, 5000)), ("kernel_h", (S(kernel_h=4), 2, 2, 5000)), ("kernel_p", (S(kernel_p=1), 2, 2, 5000)),
                        ("power", (S(power=0), 2, 2, 5000)), ("power", (S(power=9), 2, 2, 5000)), ("margin_h", (S(margin_h=0.5), 2, 2, 5000)),
                        ("margin_p", (S(margin_p=float("nan")), 2, 2, 5000)), ("residual", (S(residual=2), 2, 2, 5000)),
                        ("n_sources", (S(), 9, 2, 5000)), ("channels", (S(), 2, 3, 5000)), ("n 2048", (S(), 2, 2, 2048))):
        with pytest.raises(dmx.DmxError) as e:
            dmx.hpss_check(*args)
        assert e.value.code == 5 and field in str(e.value)
        assert dmx.hpss_workspace_bytes(*args) == -1
    with pytest.raises(dmx.DmxError, match="null spec"):
        dmx.hpss_check(None, 2, 2, 5000)
    # hpss_plan.h on 4 minutes: the tables, the forward kernel's by-product, D and two fp32 mask planes
    J, C, n = 4, 2, 240 * 44100
    T = 1 + n // 1024
    parts = [2048 * 8, 4096 * 4, T * 8, J * C * T * 2064 * 8, J * C * T * 2064 * 4, J * C * T * 2064 * 4]
    assert dmx.hpss_workspace_bytes(S(), J, C, n) == sum((p + 255) // 256 * 256 for p in parts)
    assert dmx.hpss_workspace_bytes(S(), J, C, 2 * n) > dmx.hpss_workspace_bytes(S(), J, C, n) > dmx.hpss_workspace_bytes(S(), 1, 1, n)
    assert dmx.hpss_geometry() == (32, 64)


def test_the_medians_of_the_specification_are_scipys_reflect_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for shape, kh, kp in (((40, 50), 31, 31), ((5, 7), 31, 31), ((9, 33), 17, 3)):
        S = np.abs(rng.standard_normal(shape)).astype(np.float32)
        H, P = hpss_spec.medians(S, kh, kp)
        assert np.array_equal(H, ndimage.median_filter(S, size=(kh, 1), mode="reflect"))
        assert np.array_equal(P, ndimage.median_filter(S, size=(1, kp), mode="reflect"))
