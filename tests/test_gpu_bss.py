"""BSS Eval v4 on the GPU (csrc/bss.hip): binding.bss_eval against route A of tests/bss_spec.py on the
cases of tests/bss_cases.py, within max(16 d, 1e-9 dB) for the metrics and 16 dx relative for the filters, d and dx the case's
committed distances between route B and route A; masks, infinities and status exactly."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bss_cases  # noqa: E402
import bss_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402

pytestmark = pytest.mark.gpu
METRICS = ("sdr", "isr", "sir", "sar")


@pytest.mark.parametrize("name", bss_cases.NAMES)
def test_bss_eval_equals_route_a(name):
    _, J, C, L, N, W, H, _, d, dx = bss_cases.case(name)
    refs, ests = bss_cases.signals(name)
    want = bss_cases.reference(name)
    got = dmx.bss_eval(refs, ests, W, H, L, filters=True)
    again = dmx.bss_eval(refs, ests, W, H, L, filters=True)
    assert got["status"] == want["status"]
    for k in METRICS:
        fin = np.isfinite(want[k])
        err = float(np.abs(got[k][fin] - want[k][fin]).max()) if fin.any() else 0.0
        print(name, k, "max error", err, "dB, bound", max(16 * d, 1e-9))
        assert got[k].shape == (J, len(bss_spec.windows(N, W, H)))
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.array_equal(got[k][~fin], want[k][~fin], equal_nan=True)
        assert err <= max(16 * d, 1e-9)
        assert got[k].tobytes() == again[k].tobytes()
    assert got["X"].tobytes() == again["X"].tobytes()
    if want["status"] == bss_spec.OK:
        err = float(np.abs(got["X"] - want["X"]).max() / np.abs(want["X"]).max())
        print(name, "X max relative error", err, "bound", 16 * dx)
        assert err <= 16 * dx


def test_two_identical_references_are_singular():
    """rank deficient by construction: with one tap and an energy of 16 per reference G is [[16, 16], [16, 16]], whose factor
    is exact in binary64 and whose second pivot is exactly zero"""
    r = np.full((1, 1, 64), 0.5, np.float32)
    refs = np.concatenate([r, r])
    ests = np.random.default_rng(6).standard_normal(refs.shape).astype(np.float32)
    got = dmx.bss_eval(refs, ests, 16, 16, 1)
    assert got["status"] == dmx.BSS_SINGULAR
    assert all(np.isnan(got[k]).all() and got[k].shape == (2, 4) for k in METRICS)
