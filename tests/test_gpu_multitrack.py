"""Several tracks in one call (include/demucs_hip.h dmx_tracks_infer, binding Context.tracks, the C++ shim's
demucs_inference_batch through cli/demucs_batch.cpp.main): the segments of different tracks share batches, and every
track still gets exactly the bits of dmx_track_infer on that track alone (run with -m gpu on an MI355X)."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
import parity_utils as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
SEG = {4: 8000, 6: 8000, 3: 16384}  # reduced segments (test_track_vs_oracle_reduced, test_v3_track_vs_oracle)
SHIFTS5 = [0, 22049, 4033, 12436, 7]


def _tracks(seg, mults, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, m in enumerate(mults):
        n = max(2, int(seg * m)) if m else 2
        out.append((0.1 * rng.standard_normal((2, n)) + 0.01 * (i + 1)).astype(np.float32))
    return out


def _write_wav(path, audio, rate=44100):
    """(channels, n) float32 -> IEEE-float WAV of that many channels"""
    import struct
    audio = np.asarray(audio, np.float32)
    ch = audio.shape[0]
    data = np.ascontiguousarray(audio.T).tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 3, ch, rate, rate * 4 * ch, 4 * ch, 32))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def _five(seg, seed=11):
    return _tracks(seg, [0, 0.4, 1.0, 3.3, 7.9], seed)


@pytest.mark.parametrize("key", [4, 6, 3])
def test_tracks_equal_single_tracks_bitwise(key, dmx, tmp_models):
    """Five tracks (2 samples .. 7.9 segments, shift extremes) with max_batch 3: batches mix tracks and one track spans
    several batches; planar and Eigen layouts."""
    seg = SEG[key]
    audios = _five(seg)
    m = dmx.Model(tmp_models[key]); ctx = dmx.Context(m, seg, 3)
    singles = [ctx.track(a, s) for a, s in zip(audios, SHIFTS5)]
    for layout in (dmx.LAYOUT_PLANAR, dmx.LAYOUT_EIGEN):
        got = ctx.tracks(audios, SHIFTS5, layout=layout)
        for t, (g, r) in enumerate(zip(got, singles)):
            assert g.shape == r.shape and np.isfinite(g).all()
            assert np.array_equal(g, r), f"track {t}, layout {layout}"
    ctx.close(); m.close()


def test_tracks_order_and_batch_size_do_not_change_a_bit(dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 12)
    m = dmx.Model(tmp_models[4])
    ref = None
    for b in (1, 3, 8):
        ctx = dmx.Context(m, seg, b)
        got = ctx.tracks(audios, SHIFTS5)
        rev = ctx.tracks(audios[::-1], SHIFTS5[::-1])[::-1]
        if ref is None:
            ref = got
        for t in range(len(audios)):
            assert np.array_equal(got[t], ref[t]), f"max_batch {b}, track {t}"
            assert np.array_equal(rev[t], ref[t]), f"max_batch {b}, reversed, track {t}"
        ctx.close()
    m.close()


def test_tracks_vs_oracle_reduced(dmx, tmp_models):
    """One mixed call of three tracks against the CPU oracle's demucs_inference, track by track."""
    orc.lib().orc_set_num_threads(min(32, os.cpu_count() or 1))
    seg = SEG[4]
    audios = _tracks(seg, [0.4, 2.6, 1.3], 5)
    shifts = [22049, 4033, 0]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 2); om = orc.OracleModel(tmp_models[4])
    got = ctx.tracks(audios, shifts)
    for a, s, g in zip(audios, shifts, got):
        ref = om.track(a, s, seg)
        assert pu.relerr(g, ref) < TOL
        pu.assert_local_parity(g, ref, what="tracks")
    ctx.close(); m.close(); om.close()


def test_tracks_random_shifts_follow_successive_track_calls(dmx, tmp_models):
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    seg = SEG[4]
    audios = _five(seg, 13)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    libc.srand(7)
    got = ctx.tracks(audios, [-1] * len(audios))
    libc.srand(7)
    ref = [ctx.track(a, -1) for a in audios]
    for t, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), f"track {t}"
    libc.srand(7)
    got2 = ctx.tracks(audios, None)  # NULL shift_offsets: the same draws
    for t, (g, r) in enumerate(zip(got2, ref)):
        assert np.array_equal(g, r), f"track {t} (NULL shift_offsets)"
    ctx.close(); m.close()


def test_tracks_full_size_equal_single_tracks(dmx, tmp_models):
    """Production segment, max_batch 42: four 4s tracks of 10, 20, 31 and 45 s (2, 4, 6 and 8 segments: one batch)."""
    rng = np.random.default_rng(3)
    audios = [(0.1 * rng.standard_normal((2, int(sec * 44100)))).astype(np.float32) for sec in (10, 20, 31, 45)]
    shifts = [4033, 12436, 5427, 6865]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, 0, 42)
    got = ctx.tracks(audios, shifts)
    for t, (a, s) in enumerate(zip(audios, shifts)):
        assert np.array_equal(got[t], ctx.track(a, s)), f"track {t}"
    ctx.close(); m.close()


def test_tracks_context_reuse_has_no_stale_slots(dmx, tmp_models):
    """12 tracks, then 3 on the same context (one longer than any before: the slots grow): the second call equals a
    fresh context's."""
    seg = SEG[4]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    first = _tracks(seg, [0.3, 1.1, 0.2, 2.5, 0.7, 0.05, 1.6, 0.9, 3.1, 0.4, 0.15, 1.2], 21)
    ctx.tracks(first, [(97 * i) % 22050 for i in range(12)])
    second = _tracks(seg, [5.2, 0.6, 1.4], 22)
    shifts = [311, 20000, 0]
    got = ctx.tracks(second, shifts)
    fresh = dmx.Context(m, seg, 3)
    ref = fresh.tracks(second, shifts)
    for t in range(3):
        assert np.array_equal(got[t], ref[t]), f"track {t}"
        assert np.array_equal(got[t], fresh.track(second[t], shifts[t])), f"track {t} vs single"
    fresh.close(); ctx.close(); m.close()


def test_tracks_argument_errors_name_the_track(dmx, tmp_models):
    seg = SEG[4]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 2)
    L = dmx.lib()
    audios = _tracks(seg, [0.5, 0.8, 1.2], 4)
    outs = [np.zeros((4, 2, a.shape[1]), np.float32) for a in audios]

    def call(T, ap, ns, so):
        apa = (ctypes.c_void_p * len(ap))(*ap)
        opa = (ctypes.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        na = (ctypes.c_int64 * len(ns))(*ns)
        soa = (ctypes.c_int * len(so))(*so)
        return L.dmx_tracks_infer(ctx.h, T, apa, na, soa, opa, dmx.LAYOUT_PLANAR, None, None)

    ptrs = [a.ctypes.data for a in audios]
    ns = [a.shape[1] for a in audios]
    cases = [
        (0, ptrs, ns, [0, 0, 0], "n_tracks"),
        (3, [ptrs[0], None, ptrs[2]], ns, [0, 0, 0], "track 1"),
        (3, ptrs, [ns[0], ns[1], 1], [0, 0, 0], "track 2"),
        (3, ptrs, ns, [0, 22050, 0], "track 1"),
        (3, ptrs, ns, [-2, 0, 0], "track 0"),
    ]
    for T, ap, nn, so, what in cases:
        rc = call(T, ap, nn, so)
        assert rc == 5, (what, rc)  # DMX_ERR_ARG
        msg = L.dmx_last_error().decode()
        assert what in msg, msg
        with pytest.raises(dmx.DmxError):
            dmx._chk(rc)
    assert all(not o.any() for o in outs)  # nothing ran
    with pytest.raises(dmx.DmxError, match="track 1"):  # through the binding
        ctx.tracks(audios, [0, 22050, 0])
    with pytest.raises(dmx.DmxError, match="n_tracks"):
        ctx.tracks([], [])
    got = ctx.tracks(audios, [1, 2, 3])
    for a, s, g in zip(audios, [1, 2, 3], got):
        assert np.array_equal(g, ctx.track(a, s))
    ctx.close(); m.close()


def test_tracks_progress_is_monotone_and_ends_at_one(dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 14)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    msgs = []
    ctx.tracks(audios, SHIFTS5, progress=lambda p, s: msgs.append((p, s)))
    ps = [p for p, _ in msgs]
    total = sum(ctx.track_geometry(a.shape[1], s)[1] for a, s in zip(audios, SHIFTS5))
    assert len(ps) == 1 + (total + 2) // 3  # the start, then one report per batch
    assert all(b >= a for a, b in zip(ps, ps[1:])), ps
    assert ps[0] == 0.0 and abs(ps[-1] - 1.0) < 1e-6
    ctx.close(); m.close()


def test_cli_batch_equals_single_file_runs(dmx, tmp_models, tmp_path):
    """cli/demucs_batch.cpp.main on three WAVs (mono 3 s, stereo 9 s, stereo 20 s): every stem file is byte-identical to
    cli/demucs.cpp.main on that file alone."""
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    single = os.path.join(ROOT, "cli", "demucs.cpp.main")
    assert os.path.exists(batch) and os.path.exists(single), "CLIs not built (make cli)"
    rng = np.random.default_rng(9)
    wavs = []
    for name, ch, sec in (("mono3", 1, 3), ("stereo9", 2, 9), ("stereo20", 2, 20)):
        p = str(tmp_path / f"{name}.wav")
        _write_wav(p, (0.1 * rng.standard_normal((ch, int(sec * 44100)))).astype(np.float32))
        wavs.append(p)
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033")
    r = subprocess.run([batch, tmp_models[4], str(tmp_path / "batch")] + wavs, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = ["drums", "bass", "other", "vocals"]
    for p in wavs:
        stem = os.path.splitext(os.path.basename(p))[0]
        d = tmp_path / ("single_" + stem)
        r = subprocess.run([single, tmp_models[4], p, str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for i, nm in enumerate(names):
            f = f"target_{i}_{nm}.wav"
            a = (tmp_path / "batch" / stem / f).read_bytes()
            b = (d / f).read_bytes()
            assert a == b, f"{stem}/{f}"
