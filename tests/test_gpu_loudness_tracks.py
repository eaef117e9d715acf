"""The loudness stage on the track path (dmx_tracks_infer_loud / dmx_tracks_infer_from_flac_loud; Context.tracks_* with
loudness=): one call with a track at 44.1 kHz, one at 48 kHz and one of 0.3 s, which is unmeasurable. What the call returns must
EQUAL the stage alone (loud_encode, itself held to the specification by test_gpu_loudness.py) applied to the fp32 stems of
the same call without a spec and to the caller's audio; max_batch and the order of the tracks change no byte; the FLAC form
decodes to the PCM form's bytes; tracks given as FLAC files equal the audio form on the decoded tracks."""
import numpy as np
import pytest

import loudness_spec as ls

pytestmark = pytest.mark.gpu
SEG = 8000
RATES = [44100, 48000, 44100]
OFFS = [[0], [4033], [7]]


@pytest.fixture(scope="module")
def dmx():
    from demucs_cpp_amd import binding
    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


def _audios():
    """16-bit values, so that a FLAC file holds them exactly: (2, n) float32 per track, and the (n, 2) int16 behind them"""
    rng = np.random.default_rng(77)
    pcm = [np.clip(np.rint(a * 32768 * rng.standard_normal((n, 2))), -32768, 32767).astype(np.int16)
           for n, a in ((26411, 0.05), (30003, 0.2), (13230, 0.1))]  # 0.6 s, 0.625 s, 0.3 s < 4 hops of 100 ms
    return [np.ascontiguousarray(p.T.astype(np.float32) / np.float32(32768)) for p in pcm], pcm


def _gains():
    g = np.zeros((3, 5), np.float32)
    g[0, 3] = 1            # a stem
    g[1, :3] = 1           # the other stems added
    g[2, 3], g[2, 4] = -1, 1  # mixture - stem
    return g


@pytest.fixture(scope="module")
def run(dmx, tmp_models):
    m = dmx.Model(tmp_models[4])
    ctx = dmx.Context(m, SEG, 3)
    audios, pcm = _audios()
    stems = ctx.tracks_rates(audios, RATES, None, shift_offsets=OFFS)
    yield dmx, m, ctx, audios, pcm, stems
    ctx.close()
    m.close()


def _same(a, b):
    return len(a) == len(b) and all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("enc,clip", [(1, 1), (2, 0), (0, 2)])
@pytest.mark.parametrize("mode", (ls.MEASURE, ls.MIXTURE, ls.EACH))
def test_tracks_equal_the_stage_alone_on_the_fp32_stems(run, mode, enc, clip):
    dmx, m, ctx, audios, pcm, stems = run
    spec = dmx.RemixSpec(_gains(), enc, clip)
    loud = dmx.LoudnessSpec(mode, -18.0, 0.8)
    seen = []
    outs, peaks, report = ctx.tracks_rates(audios, RATES, spec, shift_offsets=OFFS, loudness=loud,
                                           progress=lambda f, msg: seen.append(f))
    assert seen and seen[-1] == 1.0 and all(b >= a for a, b in zip(seen, seen[1:]))
    assert report.shape == (3, 4)
    for t in range(3):
        want, wpeaks, wreport = dmx.loud_encode(stems[t], audios[t], spec, loud, RATES[t])
        assert _same(outs[t], want), (t, mode)
        assert peaks[t].tobytes() == wpeaks.tobytes() and report[t].tobytes() == wreport.tobytes(), (t, report[t], wreport)
    assert (report[2]["lufs_c"] == dmx.LUFS_UNMEASURABLE).all() and (report[2]["gain"][:-1] == 1.0).all()
    assert (report[:2]["lufs_c"] != dmx.LUFS_UNMEASURABLE).all()
    if mode == ls.MEASURE:  # the bytes of the call without loudness
        plain, ppeaks = ctx.tracks_rates(audios, RATES, spec, shift_offsets=OFFS)
        assert all(_same(a, b) for a, b in zip(outs, plain)) and all(a.tobytes() == b.tobytes() for a, b in zip(peaks, ppeaks))
    if mode == ls.MIXTURE:
        assert all(len(set(report[t]["gain"][:-1].tolist())) == 1 for t in range(3))


def test_max_batch_and_track_order_do_not_change_a_byte(run):
    dmx, m, ctx, audios, pcm, stems = run
    spec = dmx.RemixSpec(_gains(), 1, 1)
    loud = dmx.LoudnessSpec(ls.MIXTURE, -16.0)
    a = ctx.tracks_rates(audios, RATES, spec, shift_offsets=OFFS, loudness=loud)
    ctx1 = dmx.Context(m, SEG, 1)
    b = ctx1.tracks_rates(audios[::-1], RATES[::-1], spec, shift_offsets=OFFS[::-1], loudness=loud)
    ctx1.close()
    for t in range(3):
        assert _same(a[0][t], b[0][2 - t]) and a[1][t].tobytes() == b[1][2 - t].tobytes() and a[2][t].tobytes() == b[2][2 - t].tobytes()


def test_flac_form_and_tracks_from_flac_and_the_44100_entry_points(run):
    dmx, m, ctx, audios, pcm, stems = run
    spec = dmx.RemixSpec(_gains(), 1, 0)
    loud = dmx.LoudnessSpec(ls.EACH, -20.0, 0.7)
    outs, peaks, report = ctx.tracks_rates(audios, RATES, spec, shift_offsets=OFFS, loudness=loud)
    files, fpeaks, freport = ctx.tracks_rates(audios, RATES, spec, flac=True, shift_offsets=OFFS, loudness=loud)
    assert report.tobytes() == freport.tobytes()
    for t in range(3):
        for o in range(3):
            dec, status, good, info = dmx.flac_decode(files[t][o], dmx.PCM_S16)
            assert status == 0 and info.sample_rate == RATES[t] and dec.tobytes() == outs[t][o].tobytes(), (t, o)
    # the tracks as FLAC files, each at its own rate
    imgs = [dmx.flac_encode(p, 16, r) for p, r in zip(pcm, RATES)]
    got, gpeaks, status, greport = ctx.tracks_from_flac(imgs, spec, shift_offsets=OFFS, any_rate=True, loudness=loud)
    assert (status[:, 0] == 0).all() and greport.tobytes() == report.tobytes()
    assert all(_same(a, b) for a, b in zip(got, outs)) and all(a.tobytes() == b.tobytes() for a, b in zip(gpeaks, peaks))
    # rates None means 44100 for all tracks: tracks_remix and tracks_pcm with loudness= take that way
    one = ctx.tracks_remix(audios[:1], spec, shift_offsets=OFFS[:1], loudness=loud)
    assert _same(one[0][0], outs[0]) and one[2][0].tobytes() == report[0].tobytes()
    fl = ctx.tracks_flac(audios[:1], spec, shift_offsets=OFFS[:1], loudness=loud)
    assert [bytes(f) for f in fl[0][0]] == [bytes(f) for f in files[0]] and fl[2][0].tobytes() == report[0].tobytes()
    ident = ctx.tracks_pcm(audios[:1], dmx.OutputSpec(1, 0, -1), shift_offsets=OFFS[:1], loudness=dmx.LoudnessSpec(ls.MEASURE))
    plain = ctx.tracks_pcm(audios[:1], dmx.OutputSpec(1, 0, -1), shift_offsets=OFFS[:1])
    assert _same(ident[0][0], plain[0][0]) and ident[2].shape == (1, 5)


def test_errors_name_the_field_and_the_track(run):
    dmx, m, ctx, audios, pcm, stems = run
    spec = dmx.RemixSpec(_gains(), 1, 0)
    for loud, word in ((dmx.LoudnessSpec(5, -14.0), "mode"), (dmx.LoudnessSpec(1, 2.0), "target_lufs"), (dmx.LoudnessSpec(1, -14.0, -0.5), "max_peak")):
        with pytest.raises(dmx.DmxError) as e:
            ctx.tracks_rates(audios, RATES, spec, shift_offsets=OFFS, loudness=loud)
        assert e.value.code == 5 and word in str(e.value)
    with pytest.raises(dmx.DmxError) as e:
        ctx.tracks_rates(audios, RATES, None, shift_offsets=OFFS, loudness=dmx.LoudnessSpec())
    assert "remix spec" in str(e.value)


def test_cli_loudnorm_writes_the_bytes_of_the_call_and_prints_the_report(run, tmp_models, golden_dir, tmp_path):
    import os
    import re
    import subprocess

    from test_gpu_pcm_output import _read
    from wavio import read_wav

    dmx, m, ctx, audios, pcm, stems = run
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    batch = os.path.join(root, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    wav = os.path.join(golden_dir, "gspi_stereo_short.wav")
    _, audio = read_wav(wav)
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033", DMX_BATCH="2")
    full = dmx.Context(m, 0, 2)
    for flags, loud in ((["--loudnorm", "-20", "--max-peak", "-3"], dmx.LoudnessSpec(ls.MIXTURE, -20.0, np.float32(10.0 ** (-3.0 / 20.0)))),
                        (["--loudnorm-each", "-23"], dmx.LoudnessSpec(ls.EACH, -23.0, np.float32(10.0 ** (-1.0 / 20.0)))),
                        (["--loudness"], dmx.LoudnessSpec(ls.MEASURE, -14.0, np.float32(10.0 ** (-1.0 / 20.0))))):
        out = tmp_path / flags[0].strip("-")
        r = subprocess.run([batch, "--two-stems", "vocals"] + flags + [tmp_models[4], str(out), wav], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        spec = dmx.RemixSpec(dmx.remix_two_stems(4, 3, dmx.OTHER_ADD), 1, 1)
        want, _, report = full.tracks_remix([audio], spec, shift_offsets=[[4033]], loudness=loud)
        for o, f in enumerate(("target_0_vocals.wav", "target_1_no_vocals.wav")):
            assert _read(out / "gspi_stereo_short" / f)[4] == want[0][o].tobytes(), (flags, f)
        for o, name in enumerate(("vocals", "no_vocals")):
            line = re.search(rf"^{name}: (-?\d+\.\d\d) LUFS, gain ([+-]\d+\.\d\d) dB$", r.stdout, re.M)
            assert line, r.stdout[-1500:]
            assert line.group(1) == f"{report[0]['lufs_c'][o] / 100:.2f}"
            assert line.group(2) == f"{20 * np.log10(float(report[0]['gain'][o])):+.2f}"
        assert re.search(rf"^mixture: {report[0]['lufs_c'][2] / 100:.2f} LUFS$", r.stdout, re.M), r.stdout[-1500:]
    full.close()


def test_a_rate_below_4000_is_refused_naming_the_track_and_nothing_runs(run):
    """through the context's calls: the rates form, and the form whose rates come from the files"""
    dmx, m, ctx, audios, pcm, stems = run
    spec = dmx.RemixSpec(_gains(), 1, 0)
    loud = dmx.LoudnessSpec(ls.MIXTURE, -14.0)
    seen = []
    with pytest.raises(dmx.DmxError) as e:
        ctx.tracks_rates(audios, [44100, 3000, 44100], spec, shift_offsets=OFFS, loudness=loud, progress=lambda f, msg: seen.append(f))
    assert e.value.code == 5 and "track 1:" in str(e.value) and "rate 3000" in str(e.value) and not seen, str(e.value)
    with pytest.raises(dmx.DmxError) as e:
        ctx.tracks_rates(audios, [44100, 48000, 2000], spec, shift_offsets=OFFS, loudness=loud)
    assert e.value.code == 5 and "track 2:" in str(e.value) and "rate 2000" in str(e.value), str(e.value)
    imgs = [dmx.flac_encode(p, 16, r) for p, r in zip(pcm, (3999, 48000, 44100))]
    with pytest.raises(dmx.DmxError) as e:
        ctx.tracks_from_flac(imgs, spec, shift_offsets=OFFS, any_rate=True, loudness=loud, progress=lambda f, msg: seen.append(f))
    assert e.value.code == 5 and "track 0:" in str(e.value) and "rate 3999" in str(e.value) and not seen, str(e.value)
    with pytest.raises(dmx.DmxError) as e:  # without any_rate a file at another rate is refused as it is without loudness
        ctx.tracks_from_flac([dmx.flac_encode(pcm[1], 16, 48000)], spec, shift_offsets=OFFS[:1], loudness=loud)
    assert e.value.code == 5 and "track 0" in str(e.value) and "48000" in str(e.value)
