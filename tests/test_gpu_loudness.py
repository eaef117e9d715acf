"""The loudness stage on the GPU (csrc/loudness.hip) against tests/loudness_spec.py: the measurement
over rates x lengths x signals within the bounds of test_loudness_cpu.py (|L - L_spec| <= 1e-6 LU, lufs_c equal, hop energies
within 1e-9 of the channel's largest), and the applied gain, whose bytes, peaks and lufs_c must EQUAL the specification
composed with remix_spec and pcm_spec. The stage alone, without a model."""
import math

import numpy as np
import pytest

import loudness_cases as lc
import loudness_spec as ls
import remix_spec as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dmx():
    from demucs_cpp_amd import binding
    if binding.device_count() < 1:
        pytest.fail("no HIP device")
    return binding


def _device_measure(dmx, x, rate, interleaved, offset):
    """dmx_loudness_device on a signal that starts `offset` floats into a device buffer (an odd 4-byte alignment); planar
    planes lie plane_stride = n + 1 apart, so the second one has another alignment than the first"""
    import torch
    n = x.shape[1]
    stride = 0 if interleaved else n + 1
    host = np.zeros(offset + 2 * n + 8, np.float32)
    if interleaved:
        host[offset:offset + 2 * n] = np.ascontiguousarray(x.T).ravel()
    else:
        host[offset:offset + n] = x[0]
        host[offset + stride:offset + stride + n] = x[1]
    d = torch.from_numpy(host).cuda()
    H = n // ls.hop(rate)
    work = torch.zeros(dmx.loudness_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    res = torch.zeros(16, dtype=torch.uint8, device="cuda")
    e = torch.zeros(max(2 * H, 1), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = dmx.lib().dmx_loudness_device(0, d.data_ptr() + 4 * offset, n, stride, rate, res.data_ptr(), e.data_ptr(), work.data_ptr(), None)
    assert rc == 0, dmx.lib().dmx_last_error()
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(dmx.LOUDNESS_DTYPE)[0]
    return float(r["lufs"]), int(r["lufs_c"]), e.cpu().numpy()[:2 * H].reshape(2, H)


@pytest.mark.parametrize("kind", lc.SIGNALS)
@pytest.mark.parametrize("rate", lc.RATES)
def test_measure_against_the_spec(dmx, rate, kind):
    for name, n, x in lc.cases(rate, kind):
        lc.check_fixture(x, rate)
        if kind == "interleaved":
            lc.compare_with_spec(*_device_measure(dmx, x, rate, True, 1), x, rate)
            lc.compare_with_spec(*_device_measure(dmx, x, rate, False, 3), x, rate)
            continue
        res, e = dmx.loudness(x, rate)
        assert res.gain == 0.0
        lc.compare_with_spec(res.lufs, res.lufs_c, e, x, rate)
        if n < 4 * ls.hop(rate) or kind == "nan":
            assert res.lufs_c == dmx.LUFS_UNMEASURABLE and math.isnan(res.lufs), name


def test_measure_units_of_several_tiles_and_interleaved_host_form(dmx):
    fs, n = 8000, 64 * lc.TILE + 5  # 65 tiles: the second-level scan's lanes take 2 tiles each
    x = lc.signal(fs, "65 tiles", n, "down15")
    lc.check_fixture(x, fs)
    a, ea = dmx.loudness(x, fs)
    lc.compare_with_spec(a.lufs, a.lufs_c, ea, x, fs)
    b, eb = dmx.loudness(np.ascontiguousarray(x.T), fs, interleaved=True)
    assert (a.lufs_c, a.lufs) == (b.lufs_c, b.lufs) and ea.tobytes() == eb.tobytes()  # fixed order: the same bits


# ------------------------------------------------------------------------------------------------ apply
FS = 8000
N = lc.TILE + 3 + 2 * ls.hop(FS)  # two tiles, an odd length, 7 hops: 4 blocks


def _stems(S, seed=0, n=N):
    rng = np.random.default_rng([S, seed, n])
    level = np.array([0.2, 0.05, 0.1, 0.02, 0.15, 0.08], np.float32)[:S]
    v = (level[:, None, None] * rng.standard_normal((S, 2, n))).astype(np.float32)
    mix = (v.sum(axis=0) + 0.01 * rng.standard_normal((2, n))).astype(np.float32)
    return v, mix


def _rows(S):
    """stem 0, stem 1, the two-stems 'other' row of stem 0 (the other stems added), mixture - stem 0"""
    g = np.zeros((4, S + 1), np.float32)
    g[0, 0] = 1
    g[1, 1] = 1
    g[2, 1:S] = 1
    g[3, 0], g[3, S] = -1, 1
    return g


@pytest.fixture(scope="module")
def checked_stems():
    """the stems, once per S, with the fixtures' condition asserted on every signal that is measured"""
    got = {}
    for S in (4, 6):
        v, mix = _stems(S)
        for o in rs.outputs(v, mix, _rows(S)):
            lc.check_fixture(o, FS)
        lc.check_fixture(mix, FS)
        got[S] = (v, mix)
    return got


def _same(got, want):
    return all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(got, want)) and len(got) == len(want)


@pytest.mark.parametrize("S", (4, 6))
@pytest.mark.parametrize("clip", (0, 1, 2))
@pytest.mark.parametrize("encoding", (0, 1, 2))
@pytest.mark.parametrize("mode", (ls.MEASURE, ls.MIXTURE, ls.EACH))
def test_apply_equals_the_spec(dmx, checked_stems, mode, encoding, clip, S):
    v, mix = checked_stems[S]
    g = _rows(S)
    target, ceiling = -16.0, 0.9
    want, wpeaks, wlufs, wgain = ls.apply(v, mix, g, encoding, clip, mode, target, ceiling, FS)
    spec = dmx.RemixSpec(g, encoding, clip)
    outs, peaks, report = dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(mode, target, ceiling), FS)
    assert list(report["lufs_c"]) == list(wlufs)
    assert report["gain"][:-1].tobytes() == wgain.tobytes() and report["gain"][-1] == 0.0
    assert peaks.tobytes() == wpeaks.tobytes()
    assert _same(outs, want)
    if mode == ls.MEASURE:
        plain, ppeaks = dmx.remix_encode(v, mix, spec)
        assert _same(outs, plain) and peaks.tobytes() == ppeaks.tobytes()
    if mode == ls.MIXTURE:
        assert len(set(report["gain"][:-1].tolist())) == 1  # one gain: the outputs keep their balance
    outs2, peaks2, report2 = dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(mode, target, ceiling), FS)
    assert _same(outs, outs2) and peaks.tobytes() == peaks2.tobytes() and report.tobytes() == report2.tobytes()  # run to run


@pytest.mark.parametrize("mode", (ls.MIXTURE, ls.EACH))
def test_apply_ceiling_engages(dmx, checked_stems, mode):
    v, mix = checked_stems[4]
    g = _rows(4)
    want, wpeaks, wlufs, wgain = ls.apply(v, mix, g, 1, 0, mode, 0.0, 0.5, FS)
    outs, peaks, report = dmx.loud_encode(v, mix, dmx.RemixSpec(g, 1, 0), dmx.LoudnessSpec(mode, 0.0, 0.5), FS)
    assert _same(outs, want) and peaks.tobytes() == wpeaks.tobytes() and report["gain"][:-1].tobytes() == wgain.tobytes()
    # the ceiling, not the table, set the gain: the largest peak lands on max_peak to within the division's rounding
    assert abs(float(peaks.max()) - 0.5) <= 2.0 ** -23
    free = ls.apply(v, mix, g, 1, 0, mode, 0.0, math.inf, FS)[3]
    assert (wgain < free).all()


def test_apply_unmeasurable_signal_keeps_its_bytes(dmx):
    n = 4 * ls.hop(FS) - 1
    v, mix = _stems(4, 1, n)
    g = _rows(4)
    spec = dmx.RemixSpec(g, 2, 1)
    for mode in (ls.MIXTURE, ls.EACH):
        outs, peaks, report = dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(mode, -14.0, 0.5), FS)
        plain, ppeaks = dmx.remix_encode(v, mix, spec)
        assert (report["lufs_c"] == dmx.LUFS_UNMEASURABLE).all() and np.isnan(report["lufs"]).all()
        assert (report["gain"][:-1] == 1.0).all()
        assert _same(outs, plain) and peaks.tobytes() == ppeaks.tobytes()


def test_a_nan_in_a_stem_nobody_reads_does_not_spread(dmx, checked_stems):
    v, mix = checked_stems[4]
    g = _rows(4)
    g[2, 3] = 0  # no row reads stem 3
    bad = v.copy()
    bad[3, 1, N // 2] = np.nan
    spec = dmx.RemixSpec(g, 1, 1)
    loud = dmx.LoudnessSpec(ls.EACH, -20.0, 0.9)
    a = dmx.loud_encode(v, mix, spec, loud, FS)
    b = dmx.loud_encode(bad, mix, spec, loud, FS)
    assert _same(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert (b[2]["lufs_c"] != dmx.LUFS_UNMEASURABLE).all()
