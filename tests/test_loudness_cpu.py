"""The loudness stage without a GPU: the specification against the EBU Tech 3341 tones and the BS.1770
table, the library's host functions against the specification, and the kernel text of csrc/loudness.hip compiled as host
code (tests/loudness_host_main.cpp: the chunked scan, the hop straddle, the fixed-order sums) against it, plain and under
ASan/UBSan as a stand-alone program.

Bounds of the kernel text against the specification: |L - L_spec| <= 1e-6 LU, lufs_c equal, every hop energy within
1e-9 of the channel's largest. A binary64 sum of up to 2^27 terms is off by at most about n 2^-53 relative (6e-8 dB), and
the chunked evaluation, with its matrix powers formed by stepping the filter, differs from the sequential one by 4e-13 relative
in energy and 1.4e-12 LU (measured on the EBU tone of case 1): the bounds lie three orders above the arithmetic and four under
the quantum."""
import math
import os
import subprocess

import numpy as np
import pytest

import loudness_cases as lc
import loudness_spec as ls

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
    subprocess.check_call(["make", "-C", ROOT, "loudness_host", "loudness_host_asan"], stdout=subprocess.DEVNULL)
    return {k: os.path.join(ROOT, "tests", "_build", v) for k, v in (("plain", "loudness_host_main"), ("asan", "loudness_host_main_asan"))}


# ------------------------------------------------------------------------------------------------ coefficients
def test_coefficients_at_48k_are_the_bs1770_table():
    k = ls.coefficients(48000)
    want = {0: 1.53512485958697, 1: -2.69169618940638, 2: 1.19839281085285, 3: -1.69065929318241, 4: 0.73248077421585,
            8: -1.99004745483398, 9: 0.99007225036621}
    for i, v in want.items():
        assert abs(k[i] - v) <= 1e-13, (i, k[i], v)
    assert list(k[5:8]) == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("rate", lc.RATES)
def test_library_coefficients_equal_the_spec_bit_for_bit(dmx, rate):
    assert dmx.loudness_coefficients(rate).tobytes() == ls.coefficients(rate).tobytes()


def test_host_program_coefficients_equal_the_spec_bit_for_bit(host_exes):
    for rate in lc.RATES:
        out = subprocess.run([host_exes["plain"], "coef", str(rate)], capture_output=True, text=True, check=True).stdout.split()
        assert [float.fromhex(v) for v in out] == list(ls.coefficients(rate))


# ------------------------------------------------------------------------------------------------ EBU Tech 3341 through the spec
def _tone(fs, parts):
    """in-phase stereo 1 kHz sine, parts = [(dBFS, seconds), ...]"""
    n = [int(round(s * fs)) for _, s in parts]
    t = np.arange(sum(n)) / fs
    amp = np.concatenate([np.full(k, 10.0 ** (d / 20.0)) for (d, _), k in zip(parts, n)])
    x = (amp * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    return np.stack([x, x])


EBU = {
    1: ([(-23, 20)], -23.0, -22.993),
    2: ([(-33, 20)], -33.0, -32.993),
    3: ([(-36, 10), (-23, 60), (-36, 10)], -23.0, -23.014),
    4: ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0, -23.014),
    5: ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0, -22.979),
}


@pytest.mark.parametrize("case", sorted(EBU))
def test_ebu_tech_3341_tones(case):
    parts, target, computed = EBU[case]
    L, c, _ = ls.measure(_tone(48000, parts), 48000)
    assert abs(L - target) <= 0.1, L
    assert abs(L - computed) <= 0.0015, L  # the value recorded with the specification, to its three printed decimals
    assert c == int(np.rint(100 * L))


@pytest.mark.parametrize("fs,computed", [(44100, -22.991), (96000, -23.011), (22050, -22.964), (8000, -22.980)])
def test_ebu_case_1_at_other_rates(fs, computed):
    L, _, _ = ls.measure(_tone(fs, EBU[1][0]), fs)
    assert abs(L + 23.0) <= 0.1 and abs(L - computed) <= 0.0015, L


def test_spec_unmeasurable_and_gates():
    fs = 8000
    h = ls.hop(fs)
    x = lc.signal(fs, "4h", 4 * h, "noise")
    assert ls.measure(x[:, :4 * h - 1], fs)[1] == ls.UNMEASURABLE  # H < 4
    assert ls.measure(np.zeros((2, 8 * h), np.float32), fs)[1] == ls.UNMEASURABLE  # no block passes
    assert math.isnan(ls.measure(np.zeros((2, 8 * h), np.float32), fs)[0])
    y = lc.signal(fs, "3s", 3 * fs, "nan")
    assert ls.measure(y, fs)[1] == ls.UNMEASURABLE and math.isnan(ls.measure(y, fs)[0])
    # the gates: a third of digital silence would pull an ungated mean down by 10 log10(3/2) = 1.76 LU; the all-silent blocks
    # are dropped, and what is left of the drop comes from the blocks that straddle the edges
    z = lc.signal(fs, "3s", 3 * fs, "silence")
    full = ls.measure(lc.signal(fs, "3s", 3 * fs, "noise"), fs)[0]
    assert 0.0 < full - ls.measure(z, fs)[0] < 1.0


# ------------------------------------------------------------------------------------------------ the kernel text as host code
def _run_host(exe, x, fs, interleaved, tmp_path):
    p = tmp_path / "x.f32"
    (np.ascontiguousarray(x.T) if interleaved else x).tofile(p)
    r = subprocess.run([exe, "measure", str(p), str(fs), "1" if interleaved else "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    head = lines[0].split()
    e = np.array([float.fromhex(v) for v in lines[1:] if v], np.float64).reshape(2, -1)
    assert int(head[5]) == e.shape[1]
    return float.fromhex(head[1]), int(head[3]), e


@pytest.mark.parametrize("kind", lc.SIGNALS)
@pytest.mark.parametrize("rate", lc.RATES)
def test_host_compiled_kernel_text_against_the_spec(host_exes, tmp_path, rate, kind):
    for name, n, x in lc.cases(rate, kind):
        lc.check_fixture(x, rate)
        L, c, e = _run_host(host_exes["plain"], x, rate, kind == "interleaved", tmp_path)
        lc.compare_with_spec(L, c, e, x, rate)
        if kind == "nan" and n >= 4 * ls.hop(rate):
            assert c == ls.UNMEASURABLE, name


@pytest.mark.parametrize("kind", lc.SIGNALS)
@pytest.mark.parametrize("rate", lc.RATES)
def test_host_compiled_kernel_text_under_asan_and_ubsan(host_exes, tmp_path, rate, kind):
    """the same shapes - every rate, length and signal - clean under the sanitizers (a stand-alone CPU program)"""
    for name, n, x in lc.cases(rate, kind):
        L, c, e = _run_host(host_exes["asan"], x, rate, kind == "interleaved", tmp_path)
        lc.compare_with_spec(L, c, e, x, rate)


def test_units_of_several_tiles_in_the_second_level_scan(host_exes, tmp_path):
    """more than 64 tiles: the scan's lanes take units of 2 tiles (3 s at 96 kHz is 71 tiles; this is the smallest such case
    at a low rate, 65 tiles)"""
    fs, n = 8000, 64 * lc.TILE + 5
    x = lc.signal(fs, "65 tiles", n, "down15")
    lc.check_fixture(x, fs)
    lc.compare_with_spec(*_run_host(host_exes["plain"], x, fs, False, tmp_path), x, fs)


# ------------------------------------------------------------------------------------------------ host-side checks of the library
def test_gain_table_entry_for_entry(dmx, host_exes, tmp_path):
    want = np.array([np.float32(math.pow(10.0, (i - 6000) / 2000.0)) for i in range(12001)], np.float32)
    assert dmx.loudness_gain_table().tobytes() == want.tobytes()
    assert ls.gain_table().tobytes() == want.tobytes()
    subprocess.run([host_exes["plain"], "table", str(tmp_path / "t.bin")], check=True)
    assert np.fromfile(tmp_path / "t.bin", np.float32).tobytes() == want.tobytes()


def test_workspace_is_under_a_byte_per_frame(dmx):
    """64 bytes of result, 256 per tile of 4096 frames (states and hop partials) and 16 per 400 frames (hop energies): about n / 10.
    The first tile's 320 bytes are a constant: a signal of fewer than 320 frames needs more than one byte per frame, every
    longer one less."""
    assert dmx.loudness_workspace_bytes(0) == -1
    for n in (1, 63, 319, 320, 4095, 4096, 4097, 44100 * 240, 96000 * 3600):
        b = dmx.loudness_workspace_bytes(n)
        assert b == 64 + 256 * -(-n // 4096) + 16 * (n // 400) and b % 16 == 0, (n, b)
        assert (b <= n) == (n >= 320), (n, b)
    assert dmx.loudness_workspace_bytes(48000 * 240) <= 48000 * 240 // 9


@pytest.mark.parametrize("mode,target,peak,rate,word", [
    (3, -14.0, 0.9, 44100, "mode"), (-1, -14.0, 0.9, 44100, "mode"),
    (1, 0.5, 0.9, 44100, "target_lufs"), (1, -70.5, 0.9, 44100, "target_lufs"), (1, float("nan"), 0.9, 44100, "target_lufs"),
    (1, float("-inf"), 0.9, 44100, "target_lufs"),
    (1, -14.0, 0.0, 44100, "max_peak"), (1, -14.0, -1.0, 44100, "max_peak"), (1, -14.0, float("nan"), 44100, "max_peak"),
    (1, -14.0, 0.9, 3999, "rate"),
])
def test_argument_checks_name_the_field(dmx, mode, target, peak, rate, word):
    assert ls.check_spec(mode, target, peak, rate) == word
    with pytest.raises(dmx.DmxError) as e:
        dmx.loudness_check(dmx.LoudnessSpec(mode, target, peak), rate)
    assert e.value.code == 5 and word in str(e.value), str(e.value)


def test_argument_checks_accept_the_edges(dmx):
    for mode in (dmx.LOUD_MEASURE, dmx.LOUD_MIXTURE, dmx.LOUD_EACH):
        for target in (-70.0, -23.0, 0.0):
            for peak in (1e-6, 1.0, float("inf")):
                assert ls.check_spec(mode, target, peak, 4000) is None
                dmx.loudness_check(dmx.LoudnessSpec(mode, target, peak), 4000)
    with pytest.raises(dmx.DmxError) as e:
        dmx.loudness_check(None, 44100)
    assert "null loudness spec" in str(e.value)
    with pytest.raises(dmx.DmxError) as e:
        dmx.loudness_coefficients(3999)
    assert "rate" in str(e.value)


def test_entry_points_refuse_bad_arguments_before_any_gpu_work(dmx):
    """no device is needed to be told that an argument is wrong"""
    v = np.zeros((4, 2, 100), np.float32)
    mix = np.zeros((2, 100), np.float32)
    spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32))
    for loud, rate, word in ((dmx.LoudnessSpec(7, -14.0), 44100, "mode"), (dmx.LoudnessSpec(1, 1.0), 44100, "target_lufs"),
                             (dmx.LoudnessSpec(1, -14.0, 0.0), 44100, "max_peak"), (dmx.LoudnessSpec(1, -14.0), 2000, "rate")):
        with pytest.raises(dmx.DmxError) as e:
            dmx.loud_encode(v, mix, spec, loud, rate)
        assert e.value.code == 5 and word in str(e.value), str(e.value)
    with pytest.raises(dmx.DmxError) as e:
        dmx.loudness(mix, 3000)
    assert e.value.code == 5 and "rate" in str(e.value)


def test_cli_parses_the_four_flags_and_rejects_bad_values(tmp_path):
    """bad values print the usage and exit 1 before anything is loaded; good ones get as far as the (missing) model file"""
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    if not os.path.exists(batch):
        subprocess.check_call(["make", "-C", ROOT, "cli"], stdout=subprocess.DEVNULL)

    def run(flags):
        return subprocess.run([batch] + flags + [str(tmp_path / "no_model.bin"), str(tmp_path / "out"), str(tmp_path / "x.wav")],
                              capture_output=True, text=True, timeout=120)

    for bad in (["--loudnorm", "abc"], ["--loudnorm", "1"], ["--loudnorm", "-70.5"], ["--loudnorm", "nan"], ["--loudnorm", ""],
                ["--loudnorm-each", "-14x"], ["--loudnorm-each", "0.01"], ["--max-peak", "loud"], ["--max-peak", "inf"], ["--loudnorm"]):
        r = run(bad)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--loudnorm LUFS" in r.stderr, (bad, r.stderr[-300:])
    for good in (["--loudnorm", "-14"], ["--loudnorm-each", "-23", "--max-peak", "-2"], ["--loudness"], ["--loudnorm", "0", "--max-peak", "3"],
                 ["--loudness", "--flac", "--int24"], ["--two-stems", "vocals", "--loudnorm", "-16"]):
        r = run(good)
        assert r.returncode == 1 and "Usage:" not in r.stderr and "failed to open" in r.stderr, (good, r.stderr[-300:])


def _flac_image(rate, n=600, seed=0):
    """a small stereo 16-bit FLAC file at `rate` Hz (the writer of tests/flac_in_spec.py)"""
    import flac_in_spec as fs
    rng = np.random.default_rng(seed)
    x = rng.integers(-2000, 2000, (n, 2))
    return np.frombuffer(fs.write([fs.frame(x)], 2, 16, rate=rate)[0], np.uint8)


def test_track_calls_refuse_a_rate_below_4000_naming_the_track_before_any_gpu_work(dmx):
    """no context and no device: the refusal comes from the numbers alone. The track's number must be the one of the track
    whose rate is too low, in the rates form and in the form whose rates come from the files."""
    import ctypes
    L = dmx.lib()
    spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32))
    loud = dmx.LoudnessSpec(dmx.LOUD_MIXTURE, -14.0)
    for bad in (0, 1, 2):
        rates = [44100, 48000, 44100]
        rates[bad] = 3000
        ra = (ctypes.c_int * 3)(*rates)
        na = (ctypes.c_int64 * 3)(30000, 30000, 30000)
        rc = L.dmx_tracks_infer_loud(None, None, 0, None, 3, None, na, ra, 1, 0.25, None, ctypes.byref(spec.c), 0, None, None, None,
                                     dmx.LAYOUT_PLANAR, None, None, ctypes.byref(loud), None)
        msg = L.dmx_last_error().decode()
        assert rc == 5 and f"track {bad}:" in msg and "rate 3000" in msg and "4000" in msg, msg
        imgs = [_flac_image(r, seed=t) for t, r in enumerate(rates)]
        assert dmx.flac_probe(imgs[bad]).sample_rate == 3000
        fb = (ctypes.c_int64 * 3)(*[f.size for f in imgs])
        ptrs = (ctypes.c_void_p * 3)(*[f.ctypes.data for f in imgs])
        status = np.zeros(6, np.int64)
        rc = L.dmx_tracks_infer_from_flac_loud(None, None, 0, None, 3, ptrs, fb, 1, 0.25, None, ctypes.byref(spec.c), 0, None, None, None,
                                               status.ctypes.data, None, None, ctypes.byref(loud), None)
        msg = L.dmx_last_error().decode()
        assert rc == 5 and f"track {bad}:" in msg and "rate 3000" in msg and "4000" in msg, msg
    # the fields of the spec come first, and without a track
    rc = L.dmx_tracks_infer_loud(None, None, 0, None, 3, None, na, ra, 1, 0.25, None, ctypes.byref(spec.c), 0, None, None, None,
                                 dmx.LAYOUT_PLANAR, None, None, ctypes.byref(dmx.LoudnessSpec(1, 5.0)), None)
    assert rc == 5 and "target_lufs" in L.dmx_last_error().decode()
