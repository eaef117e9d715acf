"""The look-ahead peak limiter on the GPU (csrc/limiter.hip) against tests/limiter_spec.py: the required
reduction M, the gain plane and the result EQUAL - as integers and as bits - at 44.1, 48 and 96 kHz, with and without the
true-peak level. Nothing in the limiter depends on an order of sums, so there is no tolerance in this file.

The lengths sit where the launches can go wrong (tests/limiter_cases.py): one and two frames, the edge of the tile of T = 2048
frames and just past it, three tiles, and 65 tiles and 5 frames, where a lane of the carry launch sweeps two tiles."""
import functools

import numpy as np
import pytest

import limiter_cases as lcs
import limiter_spec as lim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dmx():
    from demucs_cpp_amd import binding
    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


def _bits(v) -> int:
    return int(np.float32(v).view(np.uint32))


def _compare(dmx, kind, n, rate, tp, where):
    want = lcs.reference(kind, n, rate, tp)
    g, c, att, rel = lcs.params(kind)
    il = kind == "interleaved"
    x = want["x"]
    M, G, res = dmx.limit(np.ascontiguousarray(x.T) if il else x, rate, c, gain=g, true_peak=tp, attack_ms=att, release_ms=rel, interleaved=il)
    assert np.array_equal(M, want["M"]), where
    assert G.tobytes() == want["gain"].tobytes(), where
    assert _bits(res.peak_out) == _bits(want["peak_out"]), (where, res.peak_out, want["peak_out"])
    assert _bits(res.true_peak_out) == _bits(want["true_peak_out"]), (where, res.true_peak_out, want["true_peak_out"])
    assert (res.max_reduction, res.limited_frames) == (want["max_reduction"], want["limited_frames"]), where
    return res


@pytest.mark.parametrize("tp", (False, True), ids=("sample", "true_peak"))
@pytest.mark.parametrize("kind", lcs.KINDS)
@pytest.mark.parametrize("rate", lcs.RATES)
def test_limit_equals_the_spec(dmx, rate, kind, tp):
    c = lcs.params(kind)[1]
    for name, n in lcs.LENGTHS.items():
        res = _compare(dmx, kind, n, rate, tp, (kind, name, rate, tp))
        if kind not in ("nan", "cap"):
            assert res.peak_out <= c, name  # exactly, not to a tolerance
        if not tp:
            assert res.true_peak_out == 0.0
        if kind == "silence":
            assert (res.peak_out, res.max_reduction, res.limited_frames) == (0.0, 0, 0)


def test_limit_above_96_khz(dmx):
    """F = 2 from 96 kHz on; from 192 kHz on the level is the sample's and the true peak the sample peak"""
    for rate in (100000, 192000):
        for kind in ("noise", "peak_edge"):
            res = _compare(dmx, kind, 2 * lcs.T + 3, rate, True, (kind, rate))
    assert _bits(res.true_peak_out) == _bits(res.peak_out)


def test_a_signal_under_the_ceiling_is_left_alone(dmx):
    x = lcs.signal(3 * lcs.T + 1, "noise")
    for tp in (False, True):
        M, G, res = dmx.limit(x, 44100, 4.0, gain=0.3, true_peak=tp)
        assert not M.any() and (G == 1.0).all() and G.dtype == np.float32
        assert (res.max_reduction, res.limited_frames) == (0, 0)
        assert _bits(res.peak_out) == _bits(np.abs((np.float32(0.3) * x).astype(np.float32)).max())


def test_a_tone_six_db_over_is_reduced_by_six_db(dmx):
    fs = 48000
    t = np.arange(fs // 2)
    c = lcs.CEILING
    x = (float(c) * 10.0 ** (6.0 / 20.0) * np.sin(2 * np.pi * 1000.0 * t / fs + 0.1)).astype(np.float32)
    M, G, res = dmx.limit(np.stack([x, x]), fs, c)
    assert abs(lim.reduction_db(res.max_reduction) - 6.0) < 0.01
    assert res.peak_out <= c and res.limited_frames == t.size


# ------------------------------------------------------------------------------------------------ behind the loudness stage
import loudness_spec as ls  # noqa: E402
import meters_cases as mc  # noqa: E402
import meters_spec as ms  # noqa: E402


def _same(got, want):
    return len(got) == len(want) and all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(got, want))


@pytest.fixture(scope="module")
def stage():
    """four stems and their mixture under four rows of gains at 8 kHz: 13 tiles of the limiter"""
    v, mix = mc.stage_inputs()
    g = mc.stage_rows()
    mc.check_stage_fixture(v, mix, g, mc.STAGE_FS)
    return v, mix, g


TARGET, STAGE_CEILING = -10.0, 0.3


@functools.lru_cache(maxsize=None)
def _stage_want(encoding, clip, mode, true_peak):
    v, mix = mc.stage_inputs()
    return lim.apply(v, mix, mc.stage_rows(), encoding, clip, mode | lim.LIMIT | (ms.TRUE_PEAK if true_peak else 0), TARGET, STAGE_CEILING, mc.STAGE_FS)


def _limit_rows(rep):
    return [(_bits(r["peak_out"]), _bits(r["true_peak_out"]), int(r["max_reduction"]), int(r["limited_frames"])) for r in rep]


@pytest.mark.parametrize("clip", (0, 1, 2), ids=("none", "rescale", "clamp"))
@pytest.mark.parametrize("encoding", (0, 1, 2), ids=("f32", "s16", "s24"))
@pytest.mark.parametrize("mode", (ls.MIXTURE, ls.EACH, lim.UNITY), ids=("mixture", "each", "unity"))
def test_stage_with_the_limiter_equals_the_spec(dmx, stage, mode, encoding, clip):
    v, mix, g = stage
    fs = mc.STAGE_FS
    tp = clip == 1  # the true-peak level rides on one clip mode of every pair
    want, wpeaks, wlufs, wgain, wres = _stage_want(encoding, clip, mode, tp)
    spec = dmx.RemixSpec(g, encoding, clip)
    loud = dmx.LoudnessSpec(mode, TARGET, STAGE_CEILING, true_peak=tp, limit=True)
    assert loud.mode == mode | 0x200 | (0x100 if tp else 0)
    outs, peaks, report, meters, limit = dmx.loud_encode(v, mix, spec, loud, fs, meters=True, limit_report=True)
    assert list(report["lufs_c"]) == list(wlufs)
    assert report["gain"][:-1].tobytes() == wgain.tobytes() and report["gain"][-1] == 0.0
    assert _limit_rows(limit) == [(_bits(r["peak_out"]), _bits(r["true_peak_out"]), r["max_reduction"], r["limited_frames"]) for r in wres]
    assert peaks.tobytes() == wpeaks.tobytes() and peaks.tobytes() == limit["peak_out"].tobytes()
    assert _same(outs, want)
    assert (peaks <= np.float32(STAGE_CEILING)).all()  # exactly
    assert limit["limited_frames"].max() > 0, "bad fixture: nothing is limited"
    # the meters are of the signals as measured, and the reports do not depend on who asks for them
    wmeters = [ms.measure(s, fs) for s in mc.stage_signals(v, mix, g)]
    assert [(_bits(m["true_peak"]), int(m["lra_c"]), int(m["max_momentary_c"]), int(m["max_short_c"])) for m in meters] == \
        [(_bits(m[0]),) + tuple(m[1:]) for m in wmeters]
    outs1, peaks1, report1 = dmx.loud_encode(v, mix, spec, loud, fs)
    assert _same(outs, outs1) and peaks.tobytes() == peaks1.tobytes() and report.tobytes() == report1.tobytes()
    if mode == ls.MIXTURE:  # one envelope: the outputs keep their balance at every instant
        assert len({(int(r["max_reduction"]), int(r["limited_frames"])) for r in limit}) == 1
        assert all(r["gain"].tobytes() == wres[0]["gain"].tobytes() for r in wres)
    if mode == lim.UNITY:
        assert (report["gain"][:-1] == 1.0).all()
    else:  # the gain is the table's: the ceiling no longer lowers it
        plain = dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(mode, TARGET, STAGE_CEILING, true_peak=tp), fs)
        assert (report["gain"][:-1] >= plain[2]["gain"][:-1]).all() and report["gain"][0] > plain[2]["gain"][0]


def test_other_times_reach_the_stage(dmx, stage):
    v, mix, g = stage
    want = lim.apply(v, mix, g, 1, 0, ls.EACH | lim.LIMIT, TARGET, STAGE_CEILING, mc.STAGE_FS, attack_ms=0.5, release_ms=2000.0)
    loud = dmx.LoudnessSpec(ls.EACH, TARGET, STAGE_CEILING, limit=True, attack_ms=0.5, release_ms=2000.0)
    outs, peaks, report, limit = dmx.loud_encode(v, mix, dmx.RemixSpec(g, 1, 0), loud, mc.STAGE_FS, limit_report=True)
    assert _same(outs, want[0]) and peaks.tobytes() == want[1].tobytes()
    assert [int(r["limited_frames"]) for r in limit] == [r["limited_frames"] for r in want[4]]
    assert [int(r["limited_frames"]) for r in limit] != [r["limited_frames"] for r in _stage_want(1, 0, ls.EACH, False)[4]]


@pytest.mark.parametrize("mode", (ls.MEASURE, ls.MIXTURE, ls.EACH, ls.MIXTURE | 0x100))
def test_without_the_flag_the_new_entry_point_gives_the_bytes_of_the_old_ones(dmx, stage, mode):
    v, mix, g = stage
    spec = dmx.RemixSpec(g, 1, 1)
    loud = dmx.LoudnessSpec(mode, TARGET, STAGE_CEILING)
    old = dmx.loud_encode(v, mix, spec, loud, mc.STAGE_FS, meters=True)
    new = dmx.loud_encode(v, mix, spec, loud, mc.STAGE_FS, meters=True, limit_report=True)
    assert _same(old[0], new[0]) and all(a.tobytes() == b.tobytes() for a, b in zip(old[1:], new[1:4]))
    assert not new[4].tobytes().strip(b"\0")
    old = dmx.loud_encode(v, mix, spec, loud, mc.STAGE_FS)
    new = dmx.loud_encode(v, mix, spec, loud, mc.STAGE_FS, limit_report=True)
    assert _same(old[0], new[0]) and all(a.tobytes() == b.tobytes() for a, b in zip(old[1:], new[1:3]))
    want = ms.apply(v, mix, g, 1, 1, mode, TARGET, STAGE_CEILING, mc.STAGE_FS)
    assert _same(new[0], want[0]) and new[1].tobytes() == want[1].tobytes()


def _documented_work_bytes(dmx, n_out, n, meters, limited):
    """d_work of dmx_loud_encode(_meters | _limit)_device as include/demucs_hip.h states it"""
    per = dmx.loudness_workspace_bytes(n) + (dmx.meters_workspace_bytes(n) if meters else 0)
    plain = (n_out + 1) * per + 64
    return (plain + 63) // 64 * 64 + n_out * (dmx.limiter_workspace_bytes(n) + 64) if limited else plain


@pytest.mark.parametrize("meters", (False, True), ids=("plain", "meters"))
@pytest.mark.parametrize("mode", (ls.EACH, ls.MIXTURE | lim.LIMIT, ls.EACH | lim.LIMIT | ms.TRUE_PEAK, ls.EACH | ms.TRUE_PEAK),
                         ids=("each", "mixture-limit", "each-limit-tp", "each-tp"))
@pytest.mark.parametrize("n_out", (1, 8))
@pytest.mark.parametrize("n", (1, 2049))
def test_the_stage_stays_inside_its_documented_workspace(dmx, n, n_out, mode, meters):
    """the device entry point on a workspace of exactly the documented bytes between two guards of 4096 bytes: the guards are
    untouched, and everything it returns is, byte for byte, what the host call (which allocates its own workspace) returns.
    n_out = 8 fills the 64 bytes that the gains and the true peaks share; n = 2049 is one frame past the limiter's tile"""
    import ctypes
    import torch
    S, rate, guard = 2, 44100, 4096
    v = np.stack([lcs.signal(n, "noise")] * S)
    mix = v.sum(axis=0).astype(np.float32)
    g = np.array([[1.0 + 0.25 * o, 0.5 - 0.125 * o, 0.125 * (o % 3)] for o in range(n_out)], np.float32)
    spec = dmx.RemixSpec(g, 1, 0)
    loud = dmx.LoudnessSpec(mode & 0xff, TARGET, STAGE_CEILING, true_peak=bool(mode & ms.TRUE_PEAK), limit=bool(mode & lim.LIMIT))
    assert loud.mode == mode
    want = dmx.loud_encode(v, mix, spec, loud, rate, meters=meters, limit_report=True)
    dev = torch.device("cuda:0")
    stride = (n * 4 + 15) // 16 * 16
    bytes_ = _documented_work_bytes(dmx, n_out, n, meters, bool(mode & lim.LIMIT))
    d_in = torch.from_numpy(v).to(dev)
    d_mix = torch.from_numpy(np.ascontiguousarray(mix.T)).to(dev)
    d_out = torch.zeros(n_out * stride, dtype=torch.uint8, device=dev)
    d_peaks = torch.zeros(n_out, dtype=torch.float32, device=dev)
    d_report = torch.zeros((n_out + 1) * dmx.LOUDNESS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_meters = torch.zeros((n_out + 1) * dmx.METERS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_limit = torch.full((n_out * dmx.LIMIT_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device=dev)
    d_work = torch.full((guard + bytes_ + guard,), 0xA5, dtype=torch.uint8, device=dev)
    assert (d_work.data_ptr() + guard) % 16 == 0
    lspec = loud.limiter()
    dmx._chk(dmx.lib().dmx_loud_encode_limit_device(0, d_in.data_ptr(), S, n, n, d_mix.data_ptr(), ctypes.byref(spec.c), ctypes.byref(loud), rate,
                                                    d_out.data_ptr(), d_peaks.data_ptr(), d_report.data_ptr(), d_work.data_ptr() + guard, None,
                                                    d_meters.data_ptr() if meters else None, ctypes.byref(lspec), d_limit.data_ptr()))
    torch.cuda.synchronize()
    w = d_work.cpu().numpy()
    assert (w[:guard] == 0xA5).all(), "the guard in front of d_work was written"
    assert (w[guard + bytes_:] == 0xA5).all(), f"written past the documented {bytes_} bytes of d_work"
    out = d_out.cpu().numpy()
    assert [out[o * stride:o * stride + n * 4].tobytes() for o in range(n_out)] == [np.ascontiguousarray(a).tobytes() for a in want[0]]
    assert d_peaks.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_report.cpu().numpy().tobytes() == want[2].tobytes()
    if meters:
        assert d_meters.cpu().numpy().tobytes() == want[3].tobytes()
    assert d_limit.cpu().numpy().tobytes() == want[-1].tobytes()


# ------------------------------------------------------------------------------------------------ the track path
@pytest.fixture(scope="module")
def run(dmx, tmp_models):
    """a track at 44.1 kHz, one at 48 kHz and one of 0.3 s in one call, and the call's own fp32 stems"""
    import test_gpu_loudness_tracks as lt
    m = dmx.Model(tmp_models[4])
    ctx = dmx.Context(m, lt.SEG, 3)
    audios, pcm = lt._audios()
    stems = ctx.tracks_rates(audios, lt.RATES, None, shift_offsets=lt.OFFS)
    yield dmx, m, ctx, audios, pcm, stems, lt
    ctx.close()
    m.close()


def _track_equals_stage(dmx, got, t, stems, audio, spec, loud, rate):
    """(outs, peaks, report, meters, limit) of a track call against the stage alone on the call's own stems"""
    want = dmx.loud_encode(stems, audio, spec, loud, rate, meters=True, limit_report=True)
    assert _same(got[0][t], want[0]), t
    for k in (1, 2, 3, 4):
        assert got[k][t].tobytes() == want[k].tobytes(), (t, k, got[k][t], want[k])


@pytest.mark.parametrize("mode,tp,enc,clip", ((ls.MIXTURE, True, 1, 1), (ls.EACH, False, 2, 0), (lim.UNITY, False, 0, 2)),
                         ids=("mixture-tp-s16-rescale", "each-s24-none", "unity-f32-clamp"))
def test_tracks_with_the_limiter_equal_the_stage_alone_on_the_fp32_stems(run, mode, tp, enc, clip):
    dmx, m, ctx, audios, pcm, stems, lt = run
    spec = dmx.RemixSpec(lt._gains(), enc, clip)
    peak = max(float(np.abs(s).max()) for s in stems)
    loud = dmx.LoudnessSpec(mode, -12.0, np.float32(0.25 * peak), true_peak=tp, limit=True, attack_ms=2.0, release_ms=50.0)
    got = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud, meters=True, limit_report=True)
    assert len(got) == 5 and got[4].shape == (3, spec.n_out) and got[3].shape == (3, spec.n_out + 1)
    for t in range(3):  # the second track is at 48 kHz: the limiter runs at the track's own rate
        _track_equals_stage(dmx, got, t, stems[t], audios[t], spec, loud, lt.RATES[t])
    assert (got[4]["limited_frames"].max(axis=1) > 0).all(), "bad fixture: a track is never limited"
    assert (got[1] <= np.float32(0.25 * peak)).all()
    # through tracks_remix: a track at 44.1 kHz
    one = ctx.tracks_remix(audios[:1], spec, shift_offsets=lt.OFFS[:1], loudness=loud, meters=True, limit_report=True)
    assert _same(one[0][0], got[0][0]) and all(one[k][0].tobytes() == got[k][0].tobytes() for k in (1, 2, 3, 4))
    # without asking for the reports: the same bytes and peaks
    bare = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud)
    assert len(bare) == 3 and all(_same(a, b) for a, b in zip(bare[0], got[0])) and bare[2].tobytes() == got[2].tobytes()
    if mode == ls.MIXTURE:
        # the tracks as FLAC files, each at its own rate
        imgs = [dmx.flac_encode(p, 16, r) for p, r in zip(pcm, lt.RATES)]
        fo, fp, status, fr, fm, fl = ctx.tracks_from_flac(imgs, spec, shift_offsets=lt.OFFS, any_rate=True, loudness=loud, meters=True,
                                                           limit_report=True)
        assert (status[:, 0] == 0).all() and fr.tobytes() == got[2].tobytes() and fm.tobytes() == got[3].tobytes() and fl.tobytes() == got[4].tobytes()
        assert all(_same(a, b) for a, b in zip(fo, got[0])) and all(a.tobytes() == b.tobytes() for a, b in zip(fp, got[1]))
        # FLAC out: the files hold the limited PCM
        files, pk, rep, lrep = ctx.tracks_flac(audios[:1], spec, shift_offsets=lt.OFFS[:1], loudness=loud, limit_report=True)
        assert lrep.tobytes() == got[4][:1].tobytes() and pk[0].tobytes() == got[1][0].tobytes()
        for o in range(spec.n_out):
            assert dmx.flac_decode(files[0][o], dmx.PCM_S16)[0].tobytes() == np.ascontiguousarray(got[0][0][o]).tobytes(), o


@pytest.mark.parametrize("stem", (-1, 3), ids=("all-stems", "two-stems"))
def test_tracks_pcm_with_the_limiter_equals_the_stage_alone(run, stem):
    """tracks_pcm turns its OutputSpec into 0/1 gains of its own: all stems, and a stem against the sum of the others"""
    dmx, m, ctx, audios, pcm, stems, lt = run
    out = dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE, stem)
    g = np.eye(4, 5, dtype=np.float32) if stem < 0 else dmx.remix_two_stems(4, stem, dmx.OTHER_ADD)
    spec = dmx.RemixSpec(g, dmx.PCM_S16, dmx.CLIP_RESCALE)
    loud = dmx.LoudnessSpec(ls.EACH, -12.0, np.float32(0.25 * float(np.abs(stems[0]).max())), limit=True)
    got = ctx.tracks_pcm(audios[:1], out, shift_offsets=lt.OFFS[:1], loudness=loud, meters=True, limit_report=True)
    assert len(got) == 5 and got[4].shape == (1, spec.n_out)
    _track_equals_stage(dmx, got, 0, stems[0], audios[0], spec, loud, 44100)
    assert got[4]["limited_frames"].max() > 0, "bad fixture: nothing is limited"
    bare = ctx.tracks_pcm(audios[:1], out, shift_offsets=lt.OFFS[:1], loudness=loud)
    assert len(bare) == 3 and _same(bare[0][0], got[0][0]) and bare[1][0].tobytes() == got[1][0].tobytes()


def test_a_bag_with_the_limiter_equals_the_stage_alone(run, tmp_models):
    dmx, m, ctx, audios, pcm, stems, lt = run
    spec = dmx.RemixSpec(lt._gains(), 1, 1)
    models = [m, m]
    w = np.full((2, 4), 0.5, np.float32)
    offs = [[[o[0]], [o[0]]] for o in lt.OFFS[:1]]
    bag_stems = ctx.tracks_rates(audios[:1], lt.RATES[:1], None, models=models, weights=w, shift_offsets=offs)
    loud = dmx.LoudnessSpec(ls.EACH, -12.0, np.float32(0.25 * float(np.abs(bag_stems[0]).max())), limit=True)
    got = ctx.tracks_rates(audios[:1], lt.RATES[:1], spec, models=models, weights=w, shift_offsets=offs, loudness=loud, meters=True,
                           limit_report=True)
    _track_equals_stage(dmx, got, 0, bag_stems[0], audios[0], spec, loud, lt.RATES[0])
    assert got[4]["limited_frames"].max() > 0


@pytest.mark.parametrize("mode", (ls.MEASURE, ls.MIXTURE | 0x100, ls.EACH))
def test_without_the_flag_the_limit_track_calls_give_the_bytes_of_the_meters_calls(run, mode):
    """the old launch sequence for calls without the flag, through the new entry points"""
    dmx, m, ctx, audios, pcm, stems, lt = run
    spec = dmx.RemixSpec(lt._gains(), 1, 1)
    loud = dmx.LoudnessSpec(mode, -18.0, 0.25)
    a = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud, meters=True)
    b = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud, meters=True, limit_report=True)
    assert all(_same(x, y) for x, y in zip(a[0], b[0]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert not b[4].tobytes().strip(b"\0")
    c = ctx.tracks_rates(audios, lt.RATES, spec, shift_offsets=lt.OFFS, loudness=loud, limit_report=True)
    assert all(_same(x, y) for x, y in zip(a[0], c[0])) and a[2].tobytes() == c[2].tobytes()


def test_cli_limit_writes_the_bytes_of_the_call_and_prints_the_line(run, tmp_models, golden_dir, tmp_path):
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
    for name, flags, loud in (
            ("norm", ["--loudnorm", "-20", "--max-peak", "-30", "--limit", "--limit-attack", "2", "--limit-release", "40"],
             dmx.LoudnessSpec(ls.MIXTURE, -20.0, np.float32(10.0 ** (-30.0 / 20.0)), limit=True, attack_ms=2.0, release_ms=40.0)),
            ("alone", ["--clip-mode", "limit", "--max-peak", "-40"],
             dmx.LoudnessSpec(lim.UNITY, -14.0, np.float32(10.0 ** (-40.0 / 20.0)), limit=True))):
        out = tmp_path / name
        r = subprocess.run([batch, "--two-stems", "vocals"] + flags + [tmp_models[4], str(out), wav], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        spec = dmx.RemixSpec(dmx.remix_two_stems(4, 3, dmx.OTHER_ADD), 1, 1 if name == "norm" else 0)  # --clip-mode limit: nothing to clip
        want, _, report, lrep = full.tracks_remix([audio], spec, shift_offsets=[[4033]], loudness=loud, limit_report=True)
        for o, f in enumerate(("target_0_vocals.wav", "target_1_no_vocals.wav")):
            assert _read(out / "gspi_stereo_short" / f)[4] == want[0][o].tobytes(), (name, f)
        for o, who in enumerate(("vocals", "no_vocals")):
            line = re.search(rf"^{who}: .*, limited (\d+) frames, max (-?\d+\.\d\d) dB, peak (-?\d+\.\d\d|-inf) dBFS", r.stdout, re.M)
            assert line, r.stdout[-1500:]
            li = lrep[0][o]
            assert int(line.group(1)) == int(li["limited_frames"])
            assert line.group(2) == f"{-lim.reduction_db(int(li['max_reduction'])):.2f}", line.group(0)
            assert line.group(3) == (f"{20 * np.log10(float(li['peak_out'])):.2f}" if li["peak_out"] > 0 else "-inf"), line.group(0)
        assert lrep["limited_frames"].max() > 0, "bad fixture: nothing is limited"
    full.close()
