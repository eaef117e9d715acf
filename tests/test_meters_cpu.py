"""The meters without a GPU: the specification against the EBU Tech 3341 true-peak tones and the
Tech 3342 loudness-range tones, the library's host functions against the specification, and the kernel text of
csrc/meters.hip compiled as host code (tests/meters_host_main.cpp: the staged tiles with their halo, the lane's window,
the integer histogram and its walk) against it, plain and under ASan/UBSan as a stand-alone program.

The kernel text against the specification: TP equal as bits (fp32 in a fixed order; a maximum has no order), the three
integers equal (the fixtures keep every quantised value 0.001 from a tie, tests/meters_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

import loudness_cases as lc
import loudness_spec as ls
import meters_cases as mc
import meters_spec as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dmx():
    so = os.path.join(ROOT, "demucs_cpp_amd", "lib", "libdemucs_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", ROOT, "demucs_cpp_amd/lib/libdemucs_hip.so"], stdout=subprocess.DEVNULL)
    from demucs_cpp_amd import binding
    return binding


@pytest.fixture(scope="module")
def host_exes():
    subprocess.check_call(["make", "-C", ROOT, "meters_host", "meters_host_asan"], stdout=subprocess.DEVNULL)
    return {k: os.path.join(ROOT, "tests", "_build", v) for k, v in (("plain", "meters_host_main"), ("asan", "meters_host_main_asan"))}


# ------------------------------------------------------------------------------------------------ EBU Tech 3341: true peak
def _faded_tone(fs, period, phase_deg, amp, seconds=0.5):
    """in-phase stereo sine at fs / period with a 10 ms raised-cosine fade at both ends"""
    n = int(seconds * fs)
    t = np.arange(n)
    x = amp * np.sin(2 * np.pi * t / period + np.deg2rad(phase_deg))
    k = int(0.010 * fs)
    ramp = 0.5 * (1.0 - np.cos(np.pi * (np.arange(k) + 0.5) / k))
    x[:k] *= ramp
    x[n - k:] *= ramp[::-1]
    x = x.astype(np.float32)
    return np.stack([x, x])


TECH_3341 = {15: (4, 0.0, 0.5), 16: (4, 45.0, 0.5), 17: (6, 60.0, 0.5), 18: (8, 67.5, 0.5), 19: (4, 45.0, 1.41)}


@pytest.mark.parametrize("fs", (48000, 96000))
@pytest.mark.parametrize("case", sorted(TECH_3341))
def test_ebu_tech_3341_true_peak_tones(case, fs):
    period, phase, amp = TECH_3341[case]
    x = _faded_tone(fs, period, phase, amp)
    tp, _ = ms.true_peak(x, fs)
    d = 20 * np.log10(float(tp)) - 20 * np.log10(amp)
    assert -0.4 <= d <= 0.2, d  # the tolerance of Tech 3341
    assert abs(d) <= 0.035, d   # where this filter lands (F = 4 at 48 kHz, F = 2 at 96 kHz)
    assert tp >= ms.sample_peak(x)
    if case == 16:
        assert abs(20 * np.log10(float(ms.sample_peak(x))) + 9.03) < 0.01  # the sample peak misses 3 dB


def test_a_hard_start_overshoots_and_that_is_the_signal():
    period, phase, amp = TECH_3341[18]
    fs = 48000
    t = np.arange(fs // 2)
    x = (amp * np.sin(2 * np.pi * t / period + np.deg2rad(phase))).astype(np.float32)
    d = 20 * np.log10(float(ms.true_peak(np.stack([x, x]), fs)[0]) / amp)
    assert 0.3 < d < 1.0, d


def test_true_peak_edges_of_the_spec():
    fs = 48000
    assert ms.true_peak(np.zeros((2, 100), np.float32), fs) == (0.0, 0)
    x = np.zeros((2, 50), np.float32)
    x[0, 20] = np.nan
    assert ms.true_peak(x, fs)[0] == 0.0  # every value the NaN reaches is ignored, nothing else is left but zeros
    x[1, 3] = -0.25
    assert ms.true_peak(x, fs)[0] == np.float32(0.25)
    y = mc.tp_signal(fs, 300, "lowpass")
    assert ms.true_peak(y, 192000)[0] == ms.sample_peak(y) and ms.factor(191999) == 2 and ms.factor(95999) == 4


# ------------------------------------------------------------------------------------------------ EBU Tech 3342: loudness range
def _tone(fs, parts):
    n = [int(round(s * fs)) for _, s in parts]
    t = np.arange(sum(n)) / fs
    amp = np.concatenate([np.full(k, 10.0 ** (d / 20.0)) for (d, _), k in zip(parts, n)])
    x = (amp * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    return np.stack([x, x])


TECH_3342 = {1: ((-20, -30), 1000), 2: ((-20, -15), 500), 3: ((-40, -20), 2000), 4: ((-50, -35, -20, -35, -50), 1500)}


@pytest.mark.parametrize("case", sorted(TECH_3342))
def test_ebu_tech_3342_loudness_range_tones(case):
    levels, want = TECH_3342[case]
    fs = 48000
    x = _tone(fs, [(d, 20) for d in levels])
    lra = ms.hop_meters(ls.hop_energies(x, fs), ls.hop(fs))[0]
    assert abs(lra - want) <= 100, lra  # the document's +- 1 LU
    assert lra == want, lra             # the value recorded with the specification


def test_hop_meter_edges_of_the_spec():
    fs, h = 8000, 800
    U = ms.UNMEASURABLE
    x = mc.hop_signal(fs, "30h", 30 * h, "noise")
    e = ls.hop_energies(x, fs)
    assert ms.hop_meters(e[:, :3], h) == (U, U, U)
    lra, m, s = ms.hop_meters(e[:, :29], h)
    assert lra == U and s == U and m != U
    lra, m, s = ms.hop_meters(e, h)
    assert lra == 0 and s != U  # one block: a range of nothing
    z = np.zeros((2, 40))
    assert ms.hop_meters(z, h) == (U, U, U)  # all blocks silent
    z[0, 5] = np.nan
    assert ms.hop_meters(z, h) == (U, U, U)
    # the top bin clamps: blocks at +25 and +30 LUFS both count as +20
    big = np.full((2, 60), 10.0 ** ((25.0 + 0.691) / 10.0) * h / 2)
    big[:, 30:] *= 10.0 ** 0.5
    lra, m, s = ms.hop_meters(big, h)
    assert lra == 0 and s == 3000


# ------------------------------------------------------------------------------------------------ host functions of the library
@pytest.mark.parametrize("rate", lc.RATES + (192000,))
def test_library_filter_equals_the_spec_bit_for_bit(dmx, rate):
    F, taps = dmx.true_peak_filter(rate)
    assert F == ms.factor(rate) and taps.size == 12 * F + 1
    assert taps.tobytes() == ms.taps(rate).tobytes()
    # phase 0 is the unit tap: the centre is exactly 1, and what the rounded sine leaves at the other multiples of F (which the
    # kernel never reads: phase 0 is the sample itself) is below 1e-16
    assert taps[6 * F] == 1.0 and taps[0] == 0.0
    others = np.delete(taps[::F], 6)
    assert np.abs(others).max() < 1e-16


def test_host_program_filter_equals_the_spec_bit_for_bit(host_exes):
    for rate in lc.RATES + (192000,):
        out = subprocess.run([host_exes["plain"], "filter", str(rate)], capture_output=True, text=True, check=True).stdout.split()
        assert int(out[0]) == ms.factor(rate)
        assert np.array([float.fromhex(v) for v in out[1:]], np.float32).tobytes() == ms.taps(rate).tobytes()


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_loudness_check_accepts_the_flag_on_the_three_modes(dmx, mode):
    assert ms.check_spec(mode | 0x100, -14.0, 0.9, 44100) is None
    dmx.loudness_check(dmx.LoudnessSpec(mode | 0x100, -14.0, 0.9), 44100)
    assert dmx.LoudnessSpec(mode, -14.0, 0.9, true_peak=True).mode == mode | dmx.LOUD_TRUE_PEAK


@pytest.mark.parametrize("mode", (3, 7, -1, 0x100 | 3, 0x200, 0x300 | 1))
def test_loudness_check_still_names_the_mode(dmx, mode):
    assert ms.check_spec(mode, -14.0, 0.9, 44100) == "mode"
    with pytest.raises(dmx.DmxError) as e:
        dmx.loudness_check(dmx.LoudnessSpec(mode, -14.0, 0.9), 44100)
    assert e.value.code == 5 and "mode" in str(e.value), str(e.value)


def test_workspace_bytes(dmx):
    assert dmx.meters_workspace_bytes(0) == -1
    for n in (1, 63, 4096, 44100 * 240):
        b = dmx.meters_workspace_bytes(n)
        assert b > 0 and b % 16 == 0 and (dmx.loudness_workspace_bytes(n) + b) % 16 == 0


def test_entry_points_refuse_bad_arguments_before_any_gpu_work(dmx):
    v = np.zeros((4, 2, 100), np.float32)
    mix = np.zeros((2, 100), np.float32)
    spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32))
    with pytest.raises(dmx.DmxError) as e:
        dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(0x100 | 3, -14.0), 44100, meters=True)
    assert e.value.code == 5 and "mode" in str(e.value)
    with pytest.raises(dmx.DmxError) as e:
        dmx.meters(mix, 3000)
    assert e.value.code == 5 and "rate" in str(e.value)
    with pytest.raises(dmx.DmxError):
        dmx.true_peak_filter(0)


# ------------------------------------------------------------------------------------------------ the kernel text as host code
def _write(x, interleaved, tmp_path):
    p = tmp_path / "x.f32"
    (np.ascontiguousarray(x.T) if interleaved else x).tofile(p)
    return str(p)


def _host_tp(exe, path, fs, interleaved, cut):
    r = subprocess.run([exe, "tp", path, str(fs), "1" if interleaved else "0", str(cut)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout, 16)


def _host_meters(exe, path, fs, interleaved):
    r = subprocess.run([exe, "meters", path, str(fs), "1" if interleaved else "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    w = r.stdout.split()
    return int(w[1]), int(w[3]), int(w[5])


@pytest.mark.parametrize("form", ("plain", "asan"))
@pytest.mark.parametrize("kind", mc.TP_SIGNALS)
@pytest.mark.parametrize("rate", mc.TP_RATES)
def test_host_compiled_true_peak_against_the_spec(host_exes, tmp_path, rate, kind, form):
    """whole, and cut into two pieces at a multiple of 4: the halo makes the cut invisible"""
    for name, n, x in mc.tp_cases(rate, kind):
        want, phase = ms.true_peak(x, rate)
        if kind == "lowpass" and n >= 12:
            assert phase != 0, f"bad fixture: the largest value of {name} lies on a sample"
        il = kind == "interleaved"
        path = _write(x, il, tmp_path)
        cuts = (0, (n // 2) & ~3) if form == "plain" or n <= 2 * mc.T + 3 else (0,)
        for cut in cuts:
            assert _host_tp(host_exes[form], path, rate, il, cut) == int(np.float32(want).view(np.uint32)), (name, cut)


@pytest.mark.parametrize("form", ("plain", "asan"))
@pytest.mark.parametrize("kind", mc.HOP_SIGNALS)
@pytest.mark.parametrize("rate", mc.HOP_RATES)
def test_host_compiled_hop_meters_against_the_spec(host_exes, tmp_path, rate, kind, form):
    for name, n, x in mc.hop_cases(rate, kind):
        mc.check_fixture(x, rate)
        il = kind == "interleaved"
        got = _host_meters(host_exes[form], _write(x, il, tmp_path), rate, il)
        assert got == ms.hop_meters(ls.hop_energies(x, rate), ls.hop(rate)), name


def test_stage_fixture_meets_its_conditions():
    v, mix = mc.stage_inputs()
    mc.check_stage_fixture(v, mix, mc.stage_rows(), mc.STAGE_FS)


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_parses_true_peak_and_meters(tmp_path):
    """bad combinations print the usage and exit 1 before anything is loaded; good ones get as far as the (missing) model file"""
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    subprocess.check_call(["make", "-C", ROOT, "cli"], stdout=subprocess.DEVNULL)

    def run(flags):
        return subprocess.run([batch] + flags + [str(tmp_path / "no_model.bin"), str(tmp_path / "out"), str(tmp_path / "x.wav")],
                              capture_output=True, text=True, timeout=120)

    for bad in (["--true-peak"], ["--true-peak", "--loudness"], ["--meters"], ["--true-peak", "--max-peak", "-1"], ["--true-peak", "1"],
                ["--meters", "--two-stems", "vocals"]):
        r = run(bad)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--true-peak" in r.stderr, (bad, r.stderr[-300:])
    for good in (["--loudnorm", "-14", "--true-peak"], ["--true-peak", "--loudnorm-each", "-23", "--max-peak", "-2"], ["--loudness", "--meters"],
                 ["--loudnorm", "-14", "--max-peak", "-1", "--true-peak", "--meters", "--flac"]):
        r = run(good)
        assert r.returncode == 1 and "Usage:" not in r.stderr and "failed to open" in r.stderr, (good, r.stderr[-300:])
