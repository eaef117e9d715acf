"""BSS Eval v4 without a GPU: the two routes of tests/bss_spec.py agree within the distances committed
in tests/bss_cases.py, the decomposition adds up, the SDR is tools/eval_sdr.py's, and the pure host functions of the library
give the specification's values."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bss_cases  # noqa: E402
import bss_spec  # noqa: E402
import eval_sdr  # noqa: E402


@pytest.mark.parametrize("name", bss_cases.NAMES)
def test_route_b_is_within_the_committed_distance_of_route_a(name):
    _, J, C, L, N, W, H, _, d, dx = bss_cases.case(name)
    refs, ests = bss_cases.signals(name)
    a, b = bss_cases.reference(name), bss_cases.route_b(name)
    got_d, got_dx, same = bss_spec.distance(a, b)
    print(name, got_d, got_dx)
    assert same and got_d <= d and got_dx <= dx
    # the four parts add up to the estimate, and the SDR is the one tools/eval_sdr.py prints
    assert np.allclose(a["parts"].sum(axis=0), ests.astype(np.float64), rtol=0, atol=1e-12)
    for j in bss_spec.kept_sources(refs):
        f = eval_sdr.sdr_framewise(refs[j].T, ests[j].T, W, H)
        both = np.isfinite(f) & np.isfinite(a["sdr"][j])
        assert f.shape == a["sdr"][j].shape and np.allclose(f[both], a["sdr"][j][both], rtol=0, atol=1e-9)


def test_host_functions_give_the_specifications_values():
    from demucs_cpp_amd import binding as dmx
    for n, W, H in ((100, 50, 50), (1000, 256, 128), (40, 44100, 44100), (4097, 1024, 1024), (44100, 44100, 44100), (44099, 44100, 1)):
        assert dmx.bss_windows(n, W, H) == len(bss_spec.windows(n, W, H))
    assert dmx.bss_windows(0, 1, 1) == -1 and dmx.bss_windows(10, 0, 1) == -1 and dmx.bss_windows(10, 1, 0) == -1
    dmx.bss_check(dmx.BssSpec())
    for field, spec in (("window", dmx.BssSpec(0, 1, 1)), ("hop", dmx.BssSpec(1, 0, 1)), ("filters_len", dmx.BssSpec(1, 1, 0)),
                        ("filters_len", dmx.BssSpec(1, 1, 513))):
        with pytest.raises(dmx.DmxError) as e:
            dmx.bss_check(spec)
        assert e.value.code == 5 and field in str(e.value)
    # the workspace: G, the own-source blocks, two projections in binary64 and the partial correlations of every chunk
    for J, C, n, L in ((1, 1, 100, 1), (4, 2, 240 * 44100, 512), (6, 2, 3001, 37), (2, 1, bss_cases.GRAM_CHUNK + 1, 8)):
        M, Lp, chunks = J * C, (L + 15) // 16 * 16, -(-n // bss_cases.GRAM_CHUNK)
        parts = [chunks * 2 * M * 16 * Lp * 8, 2 * M * 16 * Lp * 8, (M * L) ** 2 * 8, J * (C * L) ** 2 * 8, M * L * 16 * 8, M * L * 16 * 8,
                 2 * M * n * 8, J * n * 4]
        assert dmx.bss_eval_workspace_bytes(J, C, n, L) == sum((p + 255) // 256 * 256 for p in parts)
    for bad in ((0, 2, 100, 8), (9, 2, 100, 8), (2, 3, 100, 8), (2, 2, 0, 8), (2, 2, 100, 0), (2, 2, 100, 513), (7, 2, 100, 512)):
        assert dmx.bss_eval_workspace_bytes(*bad) == -1
