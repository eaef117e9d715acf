"""The meters on the GPU (csrc/meters.hip) against tests/meters_spec.py: true peak equal as bits, the
loudness range and the momentary and short-term maxima equal as integers, the ceiling by true peak through the stage
(loud_encode) and through the track path, where a call must equal the stage alone on the call's own fp32 stems.

The lengths sit where the true-peak kernel can go wrong - at its halo of 6 frames, at the edge of its tile of T = 2048
frames and just past it, over several tiles - and at the first block of 4 and of 30 hops (tests/meters_cases.py)."""
import numpy as np
import pytest

import loudness_spec as ls
import meters_cases as mc
import meters_spec as ms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dmx():
    from demucs_cpp_amd import binding
    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


def _bits(v) -> int:
    return int(np.float32(v).view(np.uint32))


def _same(got, want):
    return len(got) == len(want) and all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------ true peak
@pytest.mark.parametrize("kind", mc.TP_SIGNALS)
@pytest.mark.parametrize("rate", mc.TP_RATES)
def test_true_peak_equals_the_spec_as_bits(dmx, rate, kind):
    for name, n, x in mc.tp_cases(rate, kind):
        want, phase = ms.true_peak(x, rate)
        if kind == "lowpass" and n >= 12:
            assert phase != 0, f"bad fixture: the largest value of {name} lies on a sample"
        il = kind == "interleaved"
        res, e, m = dmx.meters(np.ascontiguousarray(x.T) if il else x, rate, interleaved=il)
        assert _bits(m.true_peak) == _bits(want), (name, m.true_peak, want)
        assert m.true_peak >= ms.sample_peak(x), name
        if kind == "silence":
            assert m.true_peak == 0.0
        if kind == "tone45" and n >= mc.T:  # the samples sit 3 dB under the crest (the hard start overshoots it a little)
            assert m.true_peak >= 0.499 and abs(20 * np.log10(ms.sample_peak(x) / 0.5) + 3.01) < 0.01


def test_true_peak_above_96_khz(dmx):
    """F = 2 from 96 kHz on, and from 192 kHz on the sample peak"""
    x = mc.tp_signal(48000, mc.T + 7, "lowpass")
    for rate in (100000, 192000):
        m = dmx.meters(x, rate)[2]
        assert _bits(m.true_peak) == _bits(ms.true_peak(x, rate)[0])
    assert _bits(dmx.meters(x, 192000)[2].true_peak) == _bits(ms.sample_peak(x))


# ------------------------------------------------------------------------------------------------ the hop meters
@pytest.mark.parametrize("kind", mc.HOP_SIGNALS)
@pytest.mark.parametrize("rate", mc.HOP_RATES)
def test_hop_meters_equal_the_spec(dmx, rate, kind):
    h = ls.hop(rate)
    for name, n, x in mc.hop_cases(rate, kind):
        mc.check_fixture(x, rate)
        il = kind == "interleaved"
        xin = np.ascontiguousarray(x.T) if il else x
        res, e, m = dmx.meters(xin, rate, interleaved=il)
        want = ms.hop_meters(ls.hop_energies(x, rate), h)
        assert (m.lra_c, m.max_momentary_c, m.max_short_c) == want, (name, (m.lra_c, m.max_momentary_c, m.max_short_c), want)
        base, be = dmx.loudness(xin, rate, interleaved=il)  # the loudness result is dmx_loudness's, bit for bit
        assert bytes(res) == bytes(base) and e.tobytes() == be.tobytes(), name
        U = dmx.LUFS_UNMEASURABLE
        if n < 4 * h or kind == "nan":
            assert m.max_momentary_c == U, name
        if n < 30 * h or kind == "nan":
            assert m.max_short_c == U and m.lra_c == U, name
        if kind == "amp1e-5" and n >= 30 * h:  # everything under the absolute gate: no range, but maxima
            assert m.lra_c == U and m.max_short_c != U and m.max_momentary_c != U, name
        if kind == "amp100" and n >= 30 * h:
            assert m.max_short_c > 2000 and m.lra_c != U, name
        if kind == "step15" and name == "6s":
            assert 1000 <= m.lra_c <= 1500, m.lra_c


# ------------------------------------------------------------------------------------------------ the stage
@pytest.fixture(scope="module")
def stage():
    v, mix = mc.stage_inputs()
    g = mc.stage_rows()
    mc.check_stage_fixture(v, mix, g, mc.STAGE_FS)
    return v, mix, g


def _meters_rows(meters):
    return [(_bits(r["true_peak"]), int(r["lra_c"]), int(r["max_momentary_c"]), int(r["max_short_c"])) for r in meters]


@pytest.mark.parametrize("encoding", (0, 1, 2))
@pytest.mark.parametrize("mode", (ls.MEASURE, ls.MIXTURE, ls.EACH))
def test_stage_with_the_true_peak_ceiling_equals_the_spec(dmx, stage, mode, encoding):
    v, mix, g = stage
    fs, clip, target, ceiling = mc.STAGE_FS, (0, 2, 1)[encoding], -10.0, 0.3
    want, wpeaks, wlufs, wgain, wmeters = ms.apply(v, mix, g, encoding, clip, mode | ms.TRUE_PEAK, target, ceiling, fs)
    spec = dmx.RemixSpec(g, encoding, clip)
    loud = dmx.LoudnessSpec(mode, target, ceiling, true_peak=True)
    assert loud.mode == mode | 0x100
    outs, peaks, report, meters = dmx.loud_encode(v, mix, spec, loud, fs, meters=True)
    assert list(report["lufs_c"]) == list(wlufs)
    assert report["gain"][:-1].tobytes() == wgain.tobytes() and report["gain"][-1] == 0.0
    assert peaks.tobytes() == wpeaks.tobytes()
    assert _same(outs, want)
    assert _meters_rows(meters) == [(_bits(m[0]),) + tuple(m[1:]) for m in wmeters]
    assert all(m["true_peak"] >= p for m, p in zip(meters, np.array([ms.sample_peak(x) for x in mc.stage_signals(v, mix, g)])))
    # the entry point without a meters report honours the flag with the same bytes
    outs1, peaks1, report1 = dmx.loud_encode(v, mix, spec, loud, fs)
    assert _same(outs, outs1) and peaks.tobytes() == peaks1.tobytes() and report.tobytes() == report1.tobytes()
    # without the flag: the bytes of the call as it was, with or without a meters report
    plain = dmx.LoudnessSpec(mode, target, ceiling)
    a = dmx.loud_encode(v, mix, spec, plain, fs)
    b = dmx.loud_encode(v, mix, spec, plain, fs, meters=True)
    want0 = ls.apply(v, mix, g, encoding, clip, mode, target, ceiling, fs)
    assert _same(a[0], want0[0]) and a[1].tobytes() == want0[1].tobytes()
    assert _same(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert _meters_rows(b[3]) == _meters_rows(meters)  # the meters are of the signals as measured, whatever the gain
    if mode != ls.MEASURE:  # the ceiling engaged, and the two ceilings differ
        assert (report["gain"][:-1] <= a[2]["gain"][:-1]).all() and report["gain"][0] < a[2]["gain"][0]
        assert all(np.float32(r["gain"] * m["true_peak"]) <= np.float32(ceiling) * np.float32(1 + 2.0 ** -23)
                   for r, m in zip(report[:-1], meters[:-1]))


def test_the_two_ceilings_differ_on_the_tone_sampled_at_45_degrees(dmx):
    """the fs/4 tone at 45 degrees as a stem: its samples lie 3 dB under its crest, and a ceiling between g P and g TP lets
    the sample-peak rule pass what the true-peak rule holds back"""
    fs, n = mc.STAGE_FS, mc.STAGE_N
    t = np.arange(n)
    tone = (0.5 * np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0)).astype(np.float32)
    v = np.zeros((4, 2, n), np.float32)
    v[0] = tone
    v[1:] = mc.stage_inputs()[0][1:] * np.float32(0.01)
    mix = v.sum(axis=0).astype(np.float32)
    g = np.zeros((1, 5), np.float32)
    g[0, 0] = 1
    P, TP = float(ms.sample_peak(v[0])), float(ms.true_peak(v[0], fs)[0])
    assert TP > 1.3 * P
    g0 = float(ls.gain(ls.measure(v[0], fs)[1], -12.0, 0.0, np.inf))  # the table's gain, no ceiling
    ceiling = g0 * 0.5 * (P + TP)
    spec = dmx.RemixSpec(g, 1, 0)
    a = dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(ls.EACH, -12.0, ceiling), fs, meters=True)
    b = dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(ls.EACH, -12.0, ceiling, true_peak=True), fs, meters=True)
    ga, gb = a[2]["gain"][0], b[2]["gain"][0]
    assert ga == np.float32(g0) and gb < ga
    assert np.float32(gb * b[3]["true_peak"][0]) <= np.float32(ceiling)
    assert np.float32(ga * a[3]["true_peak"][0]) > np.float32(ceiling)  # what the sample-peak ceiling lets through
    assert b[1][0] == np.float32(gb * np.float32(P))  # the peak returned stays the gained sample peak


def test_the_same_call_twice_gives_identical_reports(dmx, stage):
    v, mix, g = stage
    spec = dmx.RemixSpec(g, 1, 1)
    loud = dmx.LoudnessSpec(ls.MIXTURE, -14.0, 0.5, true_peak=True)
    a = dmx.loud_encode(v, mix, spec, loud, mc.STAGE_FS, meters=True)
    b = dmx.loud_encode(v, mix, spec, loud, mc.STAGE_FS, meters=True)
    assert _same(a[0], b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    x = mc.hop_signal(48000, "6s", 6 * 48000, "step15")
    r1, e1, m1 = dmx.meters(x, 48000)
    r2, e2, m2 = dmx.meters(x, 48000)
    assert bytes(r1) == bytes(r2) and bytes(m1) == bytes(m2) and e1.tobytes() == e2.tobytes()


# ------------------------------------------------------------------------------------------------ the track path
@pytest.fixture(scope="module")
def run(dmx, tmp_models):
    import test_gpu_loudness_tracks as lt
    m = dmx.Model(tmp_models[4])
    ctx = dmx.Context(m, lt.SEG, 3)
    audios, pcm = lt._audios()
    stems = ctx.tracks_rates(audios, lt.RATES, None, shift_offsets=lt.OFFS)
    yield dmx, m, ctx, audios, pcm, stems, lt
    ctx.close()
    m.close()


def _track_equals_stage(dmx, got, t, stems, audio, spec, loud, rate):
    want = dmx.loud_encode(stems, audio, spec, loud, rate, meters=True)
    outs, peaks, report, meters = got
    assert _same(outs[t], want[0]), t
    assert peaks[t].tobytes() == want[1].tobytes() and report[t].tobytes() == want[2].tobytes(), (t, report[t], want[2])
    assert meters[t].tobytes() == want[3].tobytes(), (t, meters[t], want[3])


def test_tracks_with_meters_equal_the_stage_alone_on_the_fp32_stems(run):
    dmx, m, ctx, audios, pcm, stems, lt = run
    spec = dmx.RemixSpec(lt._gains(), 1, 1)
    loud = dmx.LoudnessSpec(ls.MIXTURE, -18.0, 0.25, true_peak=True)
    # the any-rate call: a track at 44.1 kHz, one at 48 kHz, one of 0.3 s - three lengths in one call
    got = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud, meters=True)
    assert got[3].shape == (3, 4)
    for t in range(3):
        _track_equals_stage(dmx, got, t, stems[t], audios[t], spec, loud, lt.RATES[t])
    assert (got[3]["true_peak"] > 0).all() and (got[3][2]["max_short_c"] == dmx.LUFS_UNMEASURABLE).all()
    # tracks of different length in one call equal their single calls
    for t in (0, 2):
        one = ctx.tracks_rates(audios[t:t + 1], lt.RATES[t:t + 1], spec, shift_offsets=lt.OFFS[t:t + 1], loudness=loud, meters=True)
        assert _same(one[0][0], got[0][t]) and all(one[k][0].tobytes() == got[k][t].tobytes() for k in (1, 2, 3))
    # the tracks as FLAC files, each at its own rate
    imgs = [dmx.flac_encode(p, 16, r) for p, r in zip(pcm, lt.RATES)]
    fo, fp, status, fr, fm = ctx.tracks_from_flac(imgs, spec, shift_offsets=lt.OFFS, any_rate=True, loudness=loud, meters=True)
    assert (status[:, 0] == 0).all() and fr.tobytes() == got[2].tobytes() and fm.tobytes() == got[3].tobytes()
    assert all(_same(a, b) for a, b in zip(fo, got[0])) and all(a.tobytes() == b.tobytes() for a, b in zip(fp, got[1]))
    # the flag without a meters report: the same bytes, peaks and loudness report
    bare = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud)
    assert len(bare) == 3 and all(_same(a, b) for a, b in zip(bare[0], got[0])) and bare[2].tobytes() == got[2].tobytes()
    # the same call twice
    again = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud, meters=True)
    assert again[2].tobytes() == got[2].tobytes() and again[3].tobytes() == got[3].tobytes()


@pytest.mark.parametrize("mode", (ls.MEASURE, ls.EACH))
def test_meters_without_the_flag_leave_the_bytes_of_the_loud_call(run, mode):
    dmx, m, ctx, audios, pcm, stems, lt = run
    spec = dmx.RemixSpec(lt._gains(), 2, 0)
    loud = dmx.LoudnessSpec(mode, -18.0, 0.8)
    a = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud)
    b = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud, meters=True)
    assert all(_same(x, y) for x, y in zip(a[0], b[0]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2].tobytes() == b[2].tobytes()
    for t in range(3):
        _track_equals_stage(dmx, b, t, stems[t], audios[t], spec, loud, lt.RATES[t])


def test_cli_true_peak_and_meters_write_the_bytes_of_the_call_and_print_the_line(run, tmp_models, golden_dir, tmp_path):
    """the starting of a further process is what this test is about: the shim's marshalling and the printed line"""
    import os
    import re
    import subprocess

    from test_gpu_pcm_output import _read
    from wavio import read_wav

    dmx, m, ctx, audios, pcm, stems, lt = run
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    batch = os.path.join(root, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    wav = os.path.join(golden_dir, "gspi_stereo_short.wav")
    _, audio = read_wav(wav)
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033", DMX_BATCH="2")
    full = dmx.Context(m, 0, 2)
    loud = dmx.LoudnessSpec(ls.MIXTURE, -20.0, np.float32(10.0 ** (-12.0 / 20.0)), true_peak=True)
    out = tmp_path / "tp"
    r = subprocess.run([batch, "--two-stems", "vocals", "--loudnorm", "-20", "--max-peak", "-12", "--true-peak", "--meters", tmp_models[4], str(out), wav],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    spec = dmx.RemixSpec(dmx.remix_two_stems(4, 3, dmx.OTHER_ADD), 1, 1)
    want, _, report, meters = full.tracks_remix([audio], spec, shift_offsets=[[4033]], loudness=loud, meters=True)
    full.close()
    for o, f in enumerate(("target_0_vocals.wav", "target_1_no_vocals.wav")):
        assert _read(out / "gspi_stereo_short" / f)[4] == want[0][o].tobytes(), f

    def lu(c):
        return "n/a" if c == dmx.LUFS_UNMEASURABLE else f"{c / 100:.2f}"

    for o, name in enumerate(("vocals", "no_vocals", "mixture")):
        line = re.search(rf"^{name}: .* TP (-?\d+\.\d\d|-inf) dBTP, LRA (\S+)( LU)?, max M (\S+), max S (\S+)$", r.stdout, re.M)
        assert line, r.stdout[-1500:]
        rep, mt = report[0][o], meters[0][o]
        tp = np.float32(rep["gain"] * mt["true_peak"]) if o < 2 else mt["true_peak"]
        assert line.group(1) == f"{20 * np.log10(float(tp)):.2f}", (line.group(0), tp)
        assert (line.group(2), line.group(4), line.group(5)) == (lu(mt["lra_c"]), lu(mt["max_momentary_c"]), lu(mt["max_short_c"])), line.group(0)
        if o < 2:
            assert float(line.group(1)) <= -12.0 + 0.005  # what leaves stays under the dBTP ceiling
