"""Tracks at their own sample rates on the multi-track path (dmx_tracks_infer_rates, dmx_tracks_infer_from_flac_rates; DESIGN.md
section 2.13). The specification is a composition of public calls, and every comparison is by equality:
    x44 = resample(x, r -> 44100);  v44 = tracks_opts / tracks_bag (x44);  v = resample(v44, 44100 -> r)[:, :m]
    outputs = remix_encode(v, x, spec) (the CALLER's track as the mixture);  files = flac_encode(outputs, rate r)
Reduced segment (8000), the synthetic 4-source model and max_batch 2, so that pieces end inside tracks; tracks of 0.4, 1 and 3.3
segments after conversion at 48000, 22050 and 96000 Hz, and one at 44100 Hz in the same call. The composed stems are made once
per configuration and shared. The conversion does not depend on the GEMM arithmetic: the process default alone."""
import functools
import os
import subprocess
import wave

import numpy as np
import pytest

import flac_in_spec as fis
import flac_spec as fs
import remix_spec as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 8000
RATES = [48000, 22050, 44100, 96000]
FRAMES = [int(0.4 * SEG * 48000 / 44100), SEG // 2, int(0.7 * SEG), int(3.3 * SEG * 96000 / 44100)]
OFFS = [[4033], [12436], [7], [21999]]


class Stage:
    pass


@pytest.fixture(scope="module")
def st(tmp_models):
    from demucs_cpp_amd import binding as dmx

    assert dmx.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    s = Stage()
    s.dmx = dmx
    s.model = dmx.Model(tmp_models[4])
    s.ctx = dmx.Context(s.model, SEG, 2)
    rng = np.random.default_rng(2718)
    # smooth and loud enough to clip now and then, with content near the native Nyquist that 44.1 kHz cannot carry
    s.x = []
    for m in FRAMES:
        t = np.arange(m)
        s.x.append((0.5 * np.sin(2 * np.pi * t[None] / np.array([[37.0], [2.1]])) + 0.2 * rng.standard_normal((2, m))).astype(np.float32))
    s.cache = {}
    yield s
    s.ctx.close()
    s.model.close()


def compose(s, sel=(0, 1, 2, 3), N=1, offs=None, models=None, weights=None):
    """the stems of the specification for the tracks `sel`: [(S, 2, m_t)]"""
    key = (tuple(sel), N, models is not None)
    if key in s.cache:
        return s.cache[key]
    dmx = s.dmx
    offs = offs if offs is not None else [OFFS[t] for t in sel]
    x44 = [s.x[t] if RATES[t] == 44100 else dmx.resample(s.x[t], RATES[t], 44100) for t in sel]
    for t, a in zip(sel, x44):
        assert a.shape[1] == dmx.resample_length(FRAMES[t], RATES[t], 44100)
    if models is None:
        v44 = s.ctx.tracks_opts(x44, n_shifts=N, shift_offsets=offs)
    else:
        v44 = s.ctx.tracks_bag(models, x44, weights=weights, n_shifts=N, shift_offsets=offs)
    out = []
    for t, v in zip(sel, v44):
        if RATES[t] == 44100:
            out.append(v)
            continue
        S, _, n44 = v.shape
        y = dmx.resample(v.reshape(2 * S, n44), 44100, RATES[t])
        assert y.shape[1] >= FRAMES[t]
        out.append(np.ascontiguousarray(y[:, :FRAMES[t]]).reshape(S, 2, FRAMES[t]))
    s.cache[key] = out
    return out


def encoded(s, v, sel, spec):
    """[(outputs, peaks)] of the specification's output stage on the composed stems"""
    return [s.dmx.remix_encode(vt, s.x[t], spec) for vt, t in zip(v, sel)]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_outputs(s, got, gpeaks, v, sel, spec):
    want = encoded(s, v, sel, spec)
    assert len(got) == len(want)
    for i, (g, gp, (w, wp)) in enumerate(zip(got, gpeaks, want)):
        assert len(g) == len(w) == spec.n_out
        for o in range(spec.n_out):
            assert same(g[o], w[o]), (sel[i], o)
        assert same(gp, wp), (sel[i], gp, wp)


def test_fp32_stems_in_both_layouts(st):
    v = compose(st)
    assert [a.shape for a in v] == [(4, 2, m) for m in FRAMES]
    for layout in (st.dmx.LAYOUT_PLANAR, st.dmx.LAYOUT_EIGEN):
        got = st.ctx.tracks_rates(st.x, RATES, shift_offsets=OFFS, layout=layout)
        for t in range(4):
            assert same(got[t], v[t]), (layout, t)
    # the track at 44100 Hz in that call: the bits of the existing entry point
    alone = st.ctx.tracks_opts([st.x[2]], shift_offsets=[OFFS[2]])
    assert same(v[2], alone[0])


@pytest.mark.parametrize("clip", ["CLIP_RESCALE", "CLIP_CLAMP"])
@pytest.mark.parametrize("enc", ["PCM_S16", "PCM_S24"])
def test_pcm_of_every_stem(enc, clip, st):
    dmx = st.dmx
    spec = dmx.RemixSpec(rs.identity(4), getattr(dmx, enc), getattr(dmx, clip))
    for layout in (dmx.LAYOUT_PLANAR, dmx.LAYOUT_EIGEN):
        got, peaks = st.ctx.tracks_rates(st.x, RATES, spec, shift_offsets=OFFS, layout=layout)
        check_outputs(st, got, peaks, compose(st), (0, 1, 2, 3), spec)
    # the same bytes as the PCM stage of an output spec writes for these stems
    ospec = dmx.OutputSpec(getattr(dmx, enc), getattr(dmx, clip))
    for t in (0, 3):
        w, wp = dmx.pcm_encode(compose(st)[t], ospec)
        assert all(same(a, b) for a, b in zip(got[t], w)) and same(peaks[t], wp)


def test_two_stems_minus_takes_the_mixture_at_the_native_rate(st):
    dmx = st.dmx
    g = dmx.remix_two_stems(4, 0, dmx.OTHER_MINUS)
    assert np.array_equal(g, rs.two_stems(4, 0, rs.OTHER_MINUS))
    for enc, clip in ((dmx.PCM_S16, dmx.CLIP_RESCALE), (dmx.PCM_F32, dmx.CLIP_NONE)):
        spec = dmx.RemixSpec(g, enc, clip)
        got, peaks = st.ctx.tracks_rates(st.x, RATES, spec, shift_offsets=OFFS)
        check_outputs(st, got, peaks, compose(st), (0, 1, 2, 3), spec)
    # fp32: no_vocals + vocals gives back the caller's track, not its round trip through 44.1 kHz
    v = compose(st)
    for t in (0, 3):
        back = np.asarray(got[t][0]) + np.asarray(got[t][1])
        trip = dmx.resample(dmx.resample(st.x[t], RATES[t], 44100), 44100, RATES[t])[:, :FRAMES[t]].T
        assert np.abs(back - st.x[t].T).max() <= 4 * np.finfo(np.float32).eps * (1.0 + float(np.abs(v[t][0]).max()))
        assert np.abs(trip - st.x[t].T).max() > 0.05  # what the round trip loses is not small


def test_eight_output_remix(st):
    rng = np.random.default_rng(8)
    g = rng.uniform(-1, 1, (8, 5)).astype(np.float32)
    g[1, 4] = 0  # a row without the mixture
    g[5, :4] = 0  # and one of the mixture alone
    spec = st.dmx.RemixSpec(g, st.dmx.PCM_S24, st.dmx.CLIP_CLAMP)
    got, peaks = st.ctx.tracks_rates(st.x, RATES, spec, shift_offsets=OFFS)
    check_outputs(st, got, peaks, compose(st), (0, 1, 2, 3), spec)


@pytest.mark.parametrize("level", [0, 2])
def test_flac_files_carry_the_rate_of_their_track(level, st):
    dmx = st.dmx
    v = compose(st)
    old = st.ctx.flac_level
    st.ctx.flac_level = level
    try:
        for enc, bits, clip in ((dmx.PCM_S16, 16, dmx.CLIP_RESCALE), (dmx.PCM_S24, 24, dmx.CLIP_CLAMP)):
            spec = dmx.RemixSpec(rs.fractional(4)[:2], enc, clip)
            files, peaks = st.ctx.tracks_rates(st.x, RATES, spec, flac=True, shift_offsets=OFFS)
            want = encoded(st, v, (0, 1, 2, 3), spec)
            for t in range(4):
                for o in range(2):
                    assert files[t][o] == dmx.flac_encode(want[t][0][o], bits, RATES[t], level=level), (bits, t, o)
                assert same(peaks[t], want[t][1])
            for t in (0, 1):
                ints = fs.pcm_ints(np.asarray(want[t][0][0]).view(np.uint8).ravel(), bits)
                ref = fis.decode(files[t][0])  # (checks every frame header's rate against the stream's)
                assert (ref["status"], ref["good"], ref["info"]["rate"], ref["info"]["bits"]) == (fis.OK, FRAMES[t], RATES[t], bits)
                assert np.array_equal(ref["samples"], ints)
                if level == 0:  # flac_spec's decoder reads the FIXED predictors only
                    pcm, b, rate = fs.decode(files[t][0])
                    assert (b, rate) == (bits, RATES[t]) and np.array_equal(pcm, ints)
    finally:
        st.ctx.flac_level = old


def test_two_shifts(st):
    dmx = st.dmx
    offs = [[(4033 * (t + 1) + 311 * k) % 22050 for k in range(2)] for t in range(4)]
    v = compose(st, N=2, offs=offs)
    got = st.ctx.tracks_rates(st.x, RATES, n_shifts=2, shift_offsets=offs)
    assert all(same(a, b) for a, b in zip(got, v))
    spec = dmx.RemixSpec(rs.fractional(4), dmx.PCM_S16, dmx.CLIP_RESCALE)
    got, peaks = st.ctx.tracks_rates(st.x, RATES, spec, n_shifts=2, shift_offsets=offs)
    check_outputs(st, got, peaks, v, (0, 1, 2, 3), spec)


def test_the_diagonal_bag(st, tmp_path):
    from demucs_cpp_amd.weights import write_synthetic_model

    dmx = st.dmx
    paths = [str(tmp_path / f"ggml-model-htdemucs_bag_{i}-4s-f16.bin") for i in range(4)]
    for i, p in enumerate(paths):
        write_synthetic_model(p, 4, 80 + i)
    models = [dmx.Model(p) for p in paths]
    try:
        offs = np.array([[[(4033 * (t + 1) + 977 * q) % 22050] for q in range(4)] for t in range(4)])
        v = compose(st, offs=offs, models=models)
        got = st.ctx.tracks_rates(st.x, RATES, models=models, shift_offsets=offs, layout=dmx.LAYOUT_EIGEN)
        assert all(same(a, b) for a, b in zip(got, v))
        spec = dmx.RemixSpec(rs.two_stems(4, 3, rs.OTHER_MINUS), dmx.PCM_S16, dmx.CLIP_RESCALE)
        got, peaks = st.ctx.tracks_rates(st.x, RATES, spec, models=models, shift_offsets=offs)
        check_outputs(st, got, peaks, v, (0, 1, 2, 3), spec)
    finally:
        for m in models:
            m.close()


@pytest.mark.parametrize("max_batch", [1, 5])
def test_results_do_not_depend_on_max_batch(max_batch, st):
    dmx = st.dmx
    v = compose(st)
    ctx = dmx.Context(st.model, SEG, max_batch)
    try:
        got = ctx.tracks_rates(st.x, RATES, shift_offsets=OFFS, layout=dmx.LAYOUT_EIGEN)
        assert all(same(a, b) for a, b in zip(got, v))
        spec = dmx.RemixSpec(rs.fractional(4), dmx.PCM_S16, dmx.CLIP_CLAMP)
        got, peaks = ctx.tracks_rates(st.x, RATES, spec, shift_offsets=OFFS)
        check_outputs(st, got, peaks, v, (0, 1, 2, 3), spec)
    finally:
        ctx.close()


def test_results_do_not_depend_on_the_other_tracks_of_the_call(st):
    dmx = st.dmx
    v = compose(st)
    spec = dmx.RemixSpec(rs.fractional(4), dmx.PCM_S24, dmx.CLIP_RESCALE)
    for sel in ((3,), (1, 0), (3, 3, 0)):
        xs, rates, offs = [st.x[t] for t in sel], [RATES[t] for t in sel], [OFFS[t] for t in sel]
        got = st.ctx.tracks_rates(xs, rates, shift_offsets=offs)
        assert all(same(a, v[t]) for a, t in zip(got, sel)), sel
        got, peaks = st.ctx.tracks_rates(xs, rates, spec, shift_offsets=offs)
        check_outputs(st, got, peaks, [v[t] for t in sel], sel, spec)


def test_all_rates_44100_is_the_existing_path(st):
    dmx = st.dmx
    xs = [st.x[0], st.x[2], st.x[3][:, :int(2.2 * SEG)]]
    offs = [[4033], [12436], [7]]
    spec = dmx.RemixSpec(rs.fractional(4), dmx.PCM_S16, dmx.CLIP_RESCALE)
    want, wpeaks = st.ctx.tracks_remix(xs, spec, shift_offsets=offs)
    got, peaks = st.ctx.tracks_rates(xs, [44100] * 3, spec, shift_offsets=offs)
    assert all(same(a, b) for g, w in zip(got, want) for a, b in zip(g, w)) and all(same(a, b) for a, b in zip(peaks, wpeaks))
    want = st.ctx.tracks_opts(xs, shift_offsets=offs)
    got = st.ctx.tracks_rates(xs, [44100] * 3, shift_offsets=offs)
    assert all(same(a, b) for a, b in zip(got, want))
    wfiles, _ = st.ctx.tracks_flac(xs, spec, shift_offsets=offs)
    files, _ = st.ctx.tracks_rates(xs, [44100] * 3, spec, flac=True, shift_offsets=offs)
    assert files == wfiles


def test_refusals_name_the_track_and_write_nothing(st):
    dmx = st.dmx
    with pytest.raises(dmx.DmxError) as e:
        st.ctx.tracks_rates([st.x[0], np.zeros((2, 2), np.float32)], [48000, 768000], shift_offsets=[[1], [2]])
    assert "track 1: 2 frames at 768000 Hz leave 1 at 44100 Hz" in str(e.value)
    with pytest.raises(dmx.DmxError) as e:
        st.ctx.tracks_rates([st.x[0], st.x[1]], [48000, 768001], shift_offsets=[[1], [2]])
    assert "track 1: sample rate 768001" in str(e.value)


# ---- tracks given as .flac files at their own rates
@functools.lru_cache(maxsize=None)
def _files():
    """16-bit MONO at 48 kHz, 24-bit stereo at 96 kHz and 16-bit stereo at 44.1 kHz: 0.4, 2.2 and 1 segments after conversion"""
    rng = np.random.default_rng(92)
    ms = (int(0.4 * SEG * 48000 / 44100), int(2.2 * SEG * 96000 / 44100), SEG)
    xs = [fis._signal(rng, ms[0], 1, 16), fis._signal(rng, ms[1], 2, 24), fis._signal(rng, ms[2], 2, 16)]
    files, lays = [], []
    for x, bits, ch, rate in zip(xs, (16, 24, 16), (1, 2, 2), (48000, 96000, 44100)):
        sizes = fis._fixed_sizes(x.shape[0], 1152)
        f, lay = fis.write([fis.frame(b, subs=[fis.sub("FIXED", order=2, method=int(bits == 24))] * ch) for b in fis._blocks(x, sizes)], ch, bits,
                           rate=rate)
        files.append(f), lays.append(lay)
    return files, xs, (16, 24, 16), (48000, 96000, 44100), lays


def _floats(xs, bits):
    return [np.ascontiguousarray(fis.as_f32(np.repeat(x, 2, axis=1) if x.shape[1] == 1 else x, b).T) for x, b in zip(xs, bits)]


def test_flac_files_at_their_rates_equal_the_float_call_on_the_decoded_floats(st):
    dmx = st.dmx
    files, xs, bits, rates, _ = _files()
    audios = _floats(xs, bits)
    offs = [[4033], [12436], [7]]
    for enc, clip, flac_out in ((dmx.PCM_S16, dmx.CLIP_RESCALE, False), (dmx.PCM_S24, dmx.CLIP_CLAMP, True), (dmx.PCM_F32, dmx.CLIP_NONE, False)):
        spec = dmx.RemixSpec(rs.two_stems(4, 0, rs.OTHER_MINUS), enc, clip)
        got, gpeaks, status = st.ctx.tracks_from_flac(files, spec, shift_offsets=offs, flac_out=flac_out, any_rate=True)
        assert status.tolist() == [[fis.OK, x.shape[0]] for x in xs]
        want, wpeaks = st.ctx.tracks_rates(audios, rates, spec, flac=flac_out, shift_offsets=offs)
        if flac_out:
            assert got == want
            assert fs.decode(got[1][0])[1:] == (24, 96000) and fs.decode(got[0][1])[1:] == (24, 48000)
        else:
            assert all(same(a, b) for g, w in zip(got, want) for a, b in zip(g, w))
        assert all(same(a, b) for a, b in zip(gpeaks, wpeaks))


def test_a_damaged_48k_file_reports_native_frames_and_runs_on_silence(st):
    dmx = st.dmx
    files, xs, bits, rates, lays = _files()
    bad = bytearray(files[0])
    a, b = lays[0]["frames"][2]
    bad[(a + b) // 2] ^= 0x10  # inside the third frame
    bad = bytes(bad)
    ref = fis.decode(bad)
    assert (ref["status"], ref["good"]) == (fis.BROKEN, 2 * 1152)
    offs = [[4033], [12436]]
    spec = dmx.RemixSpec(rs.fractional(4)[:2], dmx.PCM_S16, dmx.CLIP_RESCALE)
    status = np.full(4, -5, np.int64)
    with pytest.raises(dmx.DmxError) as e:
        st.ctx.tracks_from_flac([bad, files[1]], spec, shift_offsets=offs, track_status=status, any_rate=True)
    assert "track 0" in str(e.value) and "sample 2304" in str(e.value), str(e.value)
    assert status.reshape(2, 2).tolist() == [[fis.BROKEN, 2 * 1152], [fis.OK, xs[1].shape[0]]]
    outs, peaks = e.value.partial
    dec, _, good, _ = dmx.flac_decode(bad)
    assert good == 2304 and not dec[good:].any()
    want, wpeaks = st.ctx.tracks_rates([np.ascontiguousarray(dec.T), _floats(xs, bits)[1]], rates[:2], spec, shift_offsets=offs)
    assert all(same(a, b) for g, w in zip(outs, want) for a, b in zip(g, w)) and all(same(a, b) for a, b in zip(peaks, wpeaks))


# ---- the batch CLI
def test_cli_writes_16_bit_two_stems_for_a_48k_wav(st, tmp_models, golden_dir, tmp_path):
    dmx = st.dmx
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    with wave.open(os.path.join(golden_dir, "gspi_stereo_short.wav")) as w:
        assert (w.getnchannels(), w.getsampwidth()) == (2, 2)
        raw = w.readframes(w.getnframes())
    pcm = np.frombuffer(raw, "<i2").reshape(-1, 2)
    src = str(tmp_path / "song48k.wav")
    with wave.open(src, "wb") as w:  # the same samples, declared as 48 kHz
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(48000)
        w.writeframes(raw)
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033", DMX_BATCH="2")
    env.pop("DMX_RESAMPLE", None)
    args = [batch, "--two-stems", "vocals", "--int16", tmp_models[4], str(tmp_path / "out"), src]
    r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "demucs.cpp only supports the following sample rate (Hz): 44100" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    r = subprocess.run(args, env=dict(env, DMX_RESAMPLE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    x = np.ascontiguousarray((pcm.astype(np.float32) / np.float32(32768.0)).T)  # cli/wav.hpp: (float)v / 32768.0f
    ctx = dmx.Context(st.model, 0, 2)
    try:
        spec = dmx.RemixSpec(dmx.remix_two_stems(4, 3, dmx.OTHER_ADD), dmx.PCM_S16, dmx.CLIP_RESCALE)
        want, _ = ctx.tracks_rates([x], [48000], spec, shift_offsets=[[4033]])
    finally:
        ctx.close()
    d = tmp_path / "out" / "song48k"
    assert sorted(os.listdir(d)) == ["target_0_vocals.wav", "target_1_no_vocals.wav"]
    for o, name in enumerate(sorted(os.listdir(d))):
        with wave.open(str(d / name)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, 48000, pcm.shape[0])
            assert w.readframes(w.getnframes()) == np.asarray(want[0][o]).tobytes(), name
    # the same track as a 48 kHz .flac file goes to the GPU as it is, and the files are the same
    os.makedirs(tmp_path / "in")
    flac = str(tmp_path / "in" / "song48k.flac")
    with open(flac, "wb") as f:
        f.write(dmx.flac_encode(np.ascontiguousarray(pcm), 16, sample_rate=48000))
    r = subprocess.run(args[:-2] + [str(tmp_path / "out_flac"), flac], env=dict(env, DMX_RESAMPLE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in sorted(os.listdir(d)):
        assert (tmp_path / "out_flac" / "song48k" / name).read_bytes() == (d / name).read_bytes(), name
