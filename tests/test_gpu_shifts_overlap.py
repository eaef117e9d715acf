"""demucs's shifts ensemble and segment overlap (include/demucs_hip.h dmx_tracks_infer_opts, binding Context.tracks_opts, the
C++ shim's inference_options through cli/demucs_batch.cpp.main): N shifted copies of every track are averaged in the
normalised domain, then de-normalised (run with -m gpu on an MI355X)."""
import ctypes
import ctypes.util
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
import parity_utils as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
MS = 22050
SEG = {4: 8000, 6: 8000, 3: 16384}  # reduced segments, as tests/test_gpu_multitrack.py
SHIFTS5 = [0, 22049, 4033, 12436, 7]


def _tracks(seg, mults, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, m in enumerate(mults):
        n = max(2, int(seg * m)) if m else 2
        out.append((0.1 * rng.standard_normal((2, n)) + 0.01 * (i + 1)).astype(np.float32))
    return out


def _five(seg, seed=11):
    return _tracks(seg, [0, 0.4, 1.0, 3.3, 7.9], seed)


def _stride(seg, ov):
    return int(np.float32(np.float32(1) - np.float32(ov)) * np.float32(seg))


def _write_wav(path, audio, rate=44100):
    import struct
    audio = np.asarray(audio, np.float32)
    ch = audio.shape[0]
    data = np.ascontiguousarray(audio.T).tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 3, ch, rate, rate * 4 * ch, 4 * ch, 32))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


# ---- the CPU oracle, computed once per module (the f32 and bf16x3 runs share it)
_ORC = {}
_SEGS = {}
_TRACKS = {}


def _oracle(path):
    if path not in _ORC:
        orc.lib().orc_set_num_threads(min(16, os.cpu_count() or 1))
        _ORC[path] = orc.OracleModel(path)
    return _ORC[path]


def _oracle_segment(path, chunk):
    key = (path, hashlib.sha1(chunk.tobytes()).hexdigest())
    if key not in _SEGS:
        _SEGS[key] = _oracle(path).segment(chunk)
    return _SEGS[key]


def _oracle_track(path, audio, shift, seg):
    key = (path, hashlib.sha1(audio.tobytes()).hexdigest(), shift, seg)
    if key not in _TRACKS:
        _TRACKS[key] = _oracle(path).track(audio, shift, seg)
    return _TRACKS[key]


def _ensemble(audio, shifts, seg, stride, segment, stats=None):
    """NumPy restatement of dmx_tracks_infer_opts on one track: normalise, shift, chunk, centre, segment(chunk),
    triangle-weighted overlap-add (float64), divide by the weight sum, average the copies, de-normalise.
    segment: (2, seg) float32 chunk -> (S, 2, seg); stats: (mean, std) as float32, else from NumPy."""
    n = audio.shape[1]
    if stats is None:
        ref = audio.astype(np.float64).mean(0)
        stats = (np.float32(ref.mean()), np.float32(ref.std(ddof=1)))
    mean, std = np.float32(stats[0]), np.float32(stats[1])
    norm = (audio.astype(np.float32) - mean) / std
    e = None
    half = seg // 2
    for s in shifts:
        off0 = MS - s
        ln = n + off0
        shifted = np.zeros((2, ln), np.float32)
        shifted[:, off0:] = norm
        acc, sw = None, np.zeros(ln)
        for g in range(-(-ln // stride)):
            off = g * stride
            chunk = min(seg, ln - off)
            left = (seg - chunk) // 2
            mix = np.zeros((2, seg), np.float32)
            mix[:, left:left + chunk] = shifted[:, off:off + chunk]
            o = segment(mix).astype(np.float64)[..., left:left + chunk]
            k = np.arange(chunk)
            w = np.where(k < half, k + 1, seg - k) / half
            if acc is None:
                acc = np.zeros(o.shape[:2] + (ln,))
            acc[..., off:off + chunk] += w * o
            sw[off:off + chunk] += w
        v = (acc / sw)[..., off0:off0 + n]
        e = v if e is None else e + v
    return e / len(shifts) * np.float64(std) + np.float64(mean)


# ---- 1. identity
@pytest.mark.parametrize("key", [4, 6, 3])
def test_one_shift_at_quarter_overlap_is_tracks_bitwise(key, dmx, tmp_models):
    seg = SEG[key]
    audios = _five(seg)
    m = dmx.Model(tmp_models[key]); ctx = dmx.Context(m, seg, 3)
    ref = ctx.tracks(audios, SHIFTS5)
    for layout in (dmx.LAYOUT_PLANAR, dmx.LAYOUT_EIGEN):
        got = ctx.tracks_opts(audios, 1, 0.25, [[s] for s in SHIFTS5], layout=layout)
        for t, (g, r) in enumerate(zip(got, ref)):
            assert g.shape == r.shape and np.isfinite(g).all()
            assert np.array_equal(g, r), f"track {t}, layout {layout}"
    ctx.close(); m.close()


# ---- 2. duplicated offsets: (v + v) / 2 = v exactly, so the ensemble kernel must give the single-shift bits
@pytest.mark.parametrize("key", [4, 3])
def test_duplicated_offsets_give_the_single_shift_bits(key, dmx, tmp_models):
    seg = SEG[key]
    audios = _five(seg, 15)
    m = dmx.Model(tmp_models[key]); ctx = dmx.Context(m, seg, 4)
    ref = ctx.tracks(audios, SHIFTS5)
    for layout in (dmx.LAYOUT_PLANAR, dmx.LAYOUT_EIGEN):
        got = ctx.tracks_opts(audios, 2, 0.25, [[s, s] for s in SHIFTS5], layout=layout)
        for t, (g, r) in enumerate(zip(got, ref)):
            assert np.array_equal(g, r), f"track {t}, layout {layout}"
    ctx.close(); m.close()


# ---- 3. against the oracle: the ensemble is the mean of the single-shift oracle tracks (de-normalisation is affine)
@pytest.mark.parametrize("key", [4, 3])
def test_three_shifts_vs_oracle_mean(key, dmx, tmp_models):
    seg = SEG[key]
    audio = _tracks(seg, [0.5], 31)[0]
    shifts = [0, 4033, 22049]
    m = dmx.Model(tmp_models[key]); ctx = dmx.Context(m, seg, 4)
    got = ctx.tracks_opts([audio], 3, 0.25, [shifts])[0]
    ref = np.mean([_oracle_track(tmp_models[key], audio, s, seg).astype(np.float64) for s in shifts], axis=0)
    assert np.isfinite(got).all()
    assert pu.relerr(got, ref) < TOL
    pu.assert_local_parity(got, ref, what="shifts ensemble")
    ctx.close(); m.close()


# ---- 4. overlap != 0.25 against the NumPy restatement over oracle segments
def _restatement_is_faithful(p):
    """Precondition of the comparisons below: at overlap 0.25 the restatement gives OracleModel.track within 1e-6."""
    audio = _tracks(8000, [1.25], 32)[0]
    ref = _oracle_track(p, audio, 22049, 8000)
    mine = _ensemble(audio, [22049], 8000, 6000, lambda c: _oracle_segment(p, c))
    err = pu.relerr(mine, ref)
    assert err < 1e-6, f"the NumPy restatement does not reproduce OracleModel.track: {err}"


OVERLAP_CASES = [(0.0, 1.5), (0.5, 1.25), (0.75, 0.5), (0.9, 0.19)]  # (overlap, track length in segments): a small CPU oracle


@pytest.mark.parametrize("ov,mult", OVERLAP_CASES)
def test_overlap_vs_restatement(ov, mult, dmx, tmp_models):
    p, seg = tmp_models[4], SEG[4]
    _restatement_is_faithful(p)  # cached oracle work after the first case
    audios = _tracks(seg, [mult, 0], 33)  # the second track: 2 samples
    shifts = [[22049, 15000], [22000, 21000]]
    stride = _stride(seg, ov)
    m = dmx.Model(p); ctx = dmx.Context(m, seg, 5)
    for N in (1, 2):
        got = ctx.tracks_opts(audios, N, ov, [s[:N] for s in shifts])
        for t, (a, s) in enumerate(zip(audios, shifts)):
            ref = _ensemble(a, s[:N], seg, stride, lambda c: _oracle_segment(p, c))
            assert np.isfinite(got[t]).all()
            err = pu.relerr(got[t], ref)
            assert err < TOL, (ov, N, t, err)
    ctx.close(); m.close()


# ---- 5. batching invariance at the ring's tightest
def test_batching_order_and_solo_runs_do_not_change_a_bit(dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 16)
    offs = np.array([[(3001 * t + 977 * k) % MS for k in range(5)] for t in range(5)])
    m = dmx.Model(tmp_models[4])
    ref = None
    for b in (1, 3, 8):
        ctx = dmx.Context(m, seg, b)
        got = ctx.tracks_opts(audios, 5, 0.75, offs)
        if ref is None:
            ref = got
        for t in range(5):
            assert np.array_equal(got[t], ref[t]), f"max_batch {b}, track {t}"
        if b == 3:
            rev = ctx.tracks_opts(audios[::-1], 5, 0.75, offs[::-1])[::-1]
            for t in range(5):
                assert np.array_equal(rev[t], ref[t]), f"reversed, track {t}"
            for t in range(5):
                solo = ctx.tracks_opts([audios[t]], 5, 0.75, offs[t:t + 1])[0]
                assert np.array_equal(solo, ref[t]), f"track {t} alone"
        ctx.close()
    m.close()


# ---- 6. copies of one track with different segment counts
def test_uneven_copies(dmx, tmp_models):
    p, seg = tmp_models[4], SEG[4]
    stride = _stride(seg, 0.25)
    n = 5000
    shifts = [21060, 21040, 4033]  # shifted lengths 5990, 6010, 23017: 1, 2 and 4 segments
    nsegs = [dmx.track_geometry(seg, n, s, 0.25)[1] for s in shifts]
    assert nsegs == [1, 2, 4]
    audios = _tracks(seg, [n / seg, 1.3, 0.4], 34)
    offs = [shifts, [5, 22000, 11111], [21060, 0, 21040]]
    m = dmx.Model(p); ctx = dmx.Context(m, seg, 3)
    got = ctx.tracks_opts(audios, 3, 0.25, offs)
    for t in range(3):
        solo = ctx.tracks_opts([audios[t]], 3, 0.25, [offs[t]])[0]
        assert np.array_equal(got[t], solo), f"track {t}"
    ref = _ensemble(audios[0], shifts, seg, stride, lambda c: _oracle_segment(p, c))
    assert pu.relerr(got[0], ref) < TOL
    ctx.close(); m.close()


# ---- 7. random draws in (track, copy) order
def test_random_offsets_are_drawn_in_track_copy_order(dmx, tmp_models):
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    seg = SEG[4]
    audios = _tracks(seg, [0.3, 1.4, 0.8], 17)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 4)
    libc.srand(7)
    draws = np.array([[libc.rand() % MS for _ in range(3)] for _ in range(3)])
    ref = ctx.tracks_opts(audios, 3, 0.5, draws)
    libc.srand(7)
    got_null = ctx.tracks_opts(audios, 3, 0.5, None)
    libc.srand(7)
    got_m1 = ctx.tracks_opts(audios, 3, 0.5, np.full((3, 3), -1))
    for t in range(3):
        assert np.array_equal(got_null[t], ref[t]), f"NULL offsets, track {t}"
        assert np.array_equal(got_m1[t], ref[t]), f"-1 offsets, track {t}"
    # explicit and -1 entries mixed: only the -1 entries draw, in (track, copy) order
    partial = draws.copy()
    partial[0, 1] = partial[2, 0] = partial[2, 2] = -1
    libc.srand(7)
    filled = partial.copy()
    for t, k in ((0, 1), (2, 0), (2, 2)):
        filled[t, k] = libc.rand() % MS
    want = ctx.tracks_opts(audios, 3, 0.5, filled)
    libc.srand(7)
    got_mixed = ctx.tracks_opts(audios, 3, 0.5, partial)
    for t in range(3):
        assert np.array_equal(got_mixed[t], want[t]), f"mixed offsets, track {t}"
    ctx.close(); m.close()


# ---- 8. argument errors name the track and the copy; nothing is written
def test_argument_errors_name_track_and_shift(dmx, tmp_models):
    seg = SEG[4]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 2)
    L = dmx.lib()
    audios = _tracks(seg, [0.5, 0.8, 1.2], 4)
    outs = [np.zeros((4, 2, a.shape[1]), np.float32) for a in audios]
    ap = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in audios])
    op = (ctypes.c_void_p * 3)(*[o.ctypes.data for o in outs])
    na = (ctypes.c_int64 * 3)(*[a.shape[1] for a in audios])

    def call(N, ov, offs):
        so = (ctypes.c_int * len(offs))(*offs) if offs is not None else None
        return L.dmx_tracks_infer_opts(ctx.h, 3, ap, na, N, ov, so, op, dmx.LAYOUT_PLANAR, None, None)

    ok2 = [0, 1, 2, 3, 4, 5]
    cases = [(0, 0.25, None, "n_shifts"), (33, 0.25, None, "n_shifts"), (2, -0.1, ok2, "overlap"), (2, 0.95, ok2, "overlap"),
             (2, float("nan"), ok2, "overlap"), (2, 0.25, [0, 1, 2, 22050, 4, 5], "track 1, shift 1"),
             (2, 0.25, [0, 1, 2, 3, -2, 5], "track 2, shift 0"), (3, 0.5, [0, 1, 2, 3, 4, 5, 6, 7, 99999], "track 2, shift 2")]
    for N, ov, offs, what in cases:
        rc = call(N, ov, offs)
        assert rc == 5, (what, rc)  # DMX_ERR_ARG
        msg = L.dmx_last_error().decode()
        assert what in msg and "dmx_tracks_infer_opts" in msg, msg
    assert all(not o.any() for o in outs)  # nothing ran
    with pytest.raises(dmx.DmxError, match="track 0, shift 1"):  # through the binding
        ctx.tracks_opts(audios, 2, 0.25, [[0, 22050], [0, 0], [0, 0]])
    ctx.close(); m.close()


# ---- 9. progress
def test_progress_is_monotone_one_report_per_batch_and_ends_at_one(dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 14)
    offs = np.array([[(701 * t + 5003 * k) % MS for k in range(4)] for t in range(5)])
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    msgs = []
    ctx.tracks_opts(audios, 4, 0.5, offs, progress=lambda p, s: msgs.append((p, s)))
    ps = [p for p, _ in msgs]
    items = sum(dmx.track_geometry(seg, a.shape[1], int(s), 0.5)[1] for a, row in zip(audios, offs) for s in row)
    assert len(ps) == 1 + (items + 2) // 3  # the start, then one report per batch
    assert all(b >= a for a, b in zip(ps, ps[1:])), ps
    assert ps[0] == 0.0 and abs(ps[-1] - 1.0) < 1e-6
    ctx.close(); m.close()


# ---- 10. full size against the NumPy ensemble over the GPU's own segment outputs
def test_full_size_vs_numpy_ensemble_of_gpu_segments(dmx, tmp_models):
    import torch

    seg, B, ov, N = 343980, 42, 0.5, 4
    stride = _stride(seg, ov)
    rng = np.random.default_rng(41)
    audio = (0.1 * rng.standard_normal((2, 60 * 44100))).astype(np.float32)
    shifts = [4033, 12436, 0, 22049]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, 0, B)
    got = ctx.tracks_opts([audio], N, ov, [shifts])[0]
    assert np.isfinite(got).all()
    # the GPU's statistics, then every chunk through segment_device
    d_audio = torch.from_numpy(np.ascontiguousarray(audio.T)).cuda()
    d_stats = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    ctx.track_stats_device(d_audio.data_ptr(), audio.shape[1], d_stats.data_ptr())
    ctx.synchronize()
    stats = d_stats.cpu().numpy()[:2]
    d_mix = torch.zeros((1, seg, 2), device="cuda")
    d_out = torch.zeros((1, 4, 2, seg), device="cuda")

    def gpu_segment(chunk):
        d_mix.copy_(torch.from_numpy(np.ascontiguousarray(chunk.T))[None])
        torch.cuda.synchronize()
        ctx.segment_device(d_mix.data_ptr(), d_out.data_ptr(), 1)
        ctx.synchronize()
        return d_out[0].cpu().numpy()

    ref = _ensemble(audio, shifts, seg, stride, gpu_segment, stats)
    err = pu.relerr(got, ref)
    assert err <= 2e-6, err
    ctx.close()
    ctx16 = dmx.Context(m, 0, 16)
    assert np.array_equal(ctx16.tracks_opts([audio], N, ov, [shifts])[0], got)
    ctx16.close(); m.close()


# ---- 11. context reuse
def test_context_reuse_after_an_ensemble_call(dmx, tmp_models):
    seg = SEG[4]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    first = _tracks(seg, [0.3, 2.2, 0.9, 1.7], 21)
    ctx.tracks_opts(first, 8, 0.75, None)
    second = _tracks(seg, [5.2, 0.6, 1.4], 22)
    shifts = [311, 20000, 0]
    got = ctx.tracks(second, shifts)
    fresh = dmx.Context(m, seg, 3)
    ref = fresh.tracks(second, shifts)
    for t in range(3):
        assert np.array_equal(got[t], ref[t]), f"track {t}"
    fresh.close(); ctx.close(); m.close()


# ---- 12. the batch CLI
def test_cli_batch_shifts_and_overlap_equal_tracks_opts(dmx, tmp_models, tmp_path):
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    rng = np.random.default_rng(19)
    wavs, audios = [], []
    for name, sec in (("a", 3), ("b", 9), ("c", 12)):
        a = (0.1 * rng.standard_normal((2, int(sec * 44100)))).astype(np.float32)
        p = str(tmp_path / f"{name}.wav")
        _write_wav(p, a)
        wavs.append(p), audios.append(a)
    offs = [5, 4033, 20000]
    env = dict(os.environ)
    env.pop("DMX_SHIFT_OFFSET", None)
    r = subprocess.run([batch, "--shifts", "3", "--overlap", "0.5", "--shift-offsets", ",".join(map(str, offs)), tmp_models[4],
                        str(tmp_path / "out")] + wavs, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, 0, 12)  # the shim's default max_batch; results do not depend on it
    ref = ctx.tracks_opts(audios, 3, 0.5, [offs] * 3)
    ctx.close(); m.close()
    names = ["drums", "bass", "other", "vocals"]
    for p, want in zip(wavs, ref):
        stem = os.path.splitext(os.path.basename(p))[0]
        for i, nm in enumerate(names):
            raw = (tmp_path / "out" / stem / f"target_{i}_{nm}.wav").read_bytes()
            data = np.frombuffer(raw[raw.index(b"data") + 8:], np.float32).reshape(-1, 2).T
            assert np.array_equal(data, want[i]), f"{stem}/{nm}"
    bad = [["--shifts", "0"], ["--shifts", "33"], ["--overlap", "0.95"], ["--overlap", "x"], ["--shift-offsets", "1,2"],
           ["--shift-offsets", "22050"], ["--bogus", "1"], ["--shifts"], ["--shifts", "2", "--shift-offsets", "5,4033,"],
           ["--shifts", "2", "--shift-offsets", ",5,4033"], ["--shifts", "2", "--shift-offsets", "5,,4033"]]
    for extra in bad:
        r = subprocess.run([batch] + extra + [tmp_models[4], str(tmp_path / "bad")] + wavs[:1], env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1, (extra, r.stdout[-500:], r.stderr[-500:])
        assert "Usage" in r.stderr, (extra, r.stderr[-500:])
    env2 = dict(env, DMX_SHIFT_OFFSET="4033")
    r = subprocess.run([batch, "--shifts", "2", tmp_models[4], str(tmp_path / "amb")] + wavs[:1], env=env2, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "DMX_SHIFT_OFFSET" in r.stderr, r.stderr[-500:]
