"""Bags of models on the multi-track path (include/demucs_hip.h dmx_tracks_infer_bag, csrc/tracks.hip track_ola_bag_kernel,
binding Context.tracks_bag, the C++ shim's demucs_bag through cli/demucs_batch.cpp.main): the fine-tuned bag (stem i from
model i) and weighted ensembles, with shifts, overlap and PCM output (run with -m gpu on an MI355X). The specification is
restated in tests/bag_spec.py."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

import bag_spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = 22050
FT = ["drums", "bass", "other", "vocals"]
SEG = {4: 8000, 3: 16384}  # reduced segments, as tests/test_gpu_shifts_overlap.py
SHIFTS5 = [0, 22049, 4033, 12436, 7]


def _tracks(seg, mults, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, m in enumerate(mults):
        n = max(2, int(seg * m)) if m else 2
        out.append((0.1 * rng.standard_normal((2, n)) + 0.01 * (i + 1)).astype(np.float32))
    return out


def _five(seg, seed=11):
    return _tracks(seg, [0, 0.4, 1.0, 3.3, 7.9], seed)  # 2 samples, 0.4, 1.0, 3.3 and 7.9 segments


def _write_wav(path, audio, rate=44100):
    import struct
    audio = np.asarray(audio, np.float32)
    ch = audio.shape[0]
    data = np.ascontiguousarray(audio.T).tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 3, ch, rate, rate * 4 * ch, 4 * ch, 32))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


@pytest.fixture(scope="module")
def bag_models(tmp_path_factory):
    """four synthetic 4-source models (seeds 50..53) in a directory that demucs_ft.cpp.main can scan, and two v3 models"""
    from demucs_cpp_amd.weights import write_synthetic_model

    d = tmp_path_factory.mktemp("bag")
    ft = d / "ft"
    ft.mkdir()
    paths = []
    for i, name in enumerate(FT):
        p = str(ft / f"ggml-model-htdemucs_ft_{name}-4s-f16.bin")
        write_synthetic_model(p, 4, 50 + i)
        paths.append(p)
    v3 = []
    for i in range(2):
        p = str(d / f"ggml-model-hdemucs_mmi-v3-{i}-f16.bin")
        write_synthetic_model(p, 4, 50 + i, "default", "v3")
        v3.append(p)
    return {"dir": str(ft), 4: paths, 3: v3}


def _offsets(T, Q, N, salt=0):
    """per (track, model, copy) offsets from SHIFTS5: the copies of a track have different segment counts"""
    return np.array([[[SHIFTS5[(t + 2 * q + 3 * k + salt) % 5] for k in range(N)] for q in range(Q)] for t in range(T)])


def _per_model(dmx, paths, seg, audios, N, ov, offs, max_batch=3):
    """each model's own tracks_opts results: refs[q][t] (S, 2, n_t)"""
    refs = []
    for q, p in enumerate(paths):
        m = dmx.Model(p); ctx = dmx.Context(m, seg, max_batch)
        refs.append(ctx.tracks_opts(audios, N, ov, offs[:, q, :]))
        ctx.close(); m.close()
    return refs


def _open(dmx, paths, seg, max_batch, entry=0):
    models = [dmx.Model(p) for p in paths]
    return models, dmx.Context(models[entry], seg, max_batch)


def _close(models, ctx):
    ctx.close()
    for m in models:
        m.close()


def _mean(audio):
    return float(audio.astype(np.float64).mean())


# ---- 1. the diagonal bag at N = 1, overlap 0.25: stem s is model s's tracks() result
def test_diagonal_bag_equals_each_models_tracks_bitwise(dmx, bag_models):
    seg = SEG[4]
    audios = _five(seg)
    offs = _offsets(5, 4, 1)
    refs = []
    for q, p in enumerate(bag_models[4]):
        m = dmx.Model(p); ctx = dmx.Context(m, seg, 3)
        refs.append(ctx.tracks(audios, [int(v) for v in offs[:, q, 0]]))
        ctx.close(); m.close()
    models, ctx = _open(dmx, bag_models[4], seg, 3)
    for layout in (dmx.LAYOUT_PLANAR, dmx.LAYOUT_EIGEN):
        got = ctx.tracks_bag(models, audios, shift_offsets=offs, layout=layout)
        for t in range(5):
            assert got[t].shape == (4, 2, audios[t].shape[1]) and np.isfinite(got[t]).all()
            for s in range(4):
                assert np.array_equal(got[t][s], refs[s][t][s]), f"track {t}, stem {s}, layout {layout}"
    _close(models, ctx)


# ---- 2. against the engine's fine-tuned bag at the production segment
def test_diagonal_bag_equals_the_engine_bitwise(dmx, bag_models):
    stride = 257985
    n = 2 * stride + 5000  # 3 segments per model = 12 items
    audio = (0.1 * np.random.default_rng(43).standard_normal((2, n))).astype(np.float32)
    shifts = [4033, 12436, 5427, 6865]
    eng = dmx.Engine(bag_models[4], [0], max_batch=3)
    want = eng.track(audio, shifts)
    eng.close()
    models, ctx = _open(dmx, bag_models[4], 0, 3)
    got = ctx.tracks_bag(models, [audio], shift_offsets=np.array(shifts).reshape(1, 4, 1))[0]
    assert np.array_equal(got, want)
    _close(models, ctx)


# ---- 3. shifts and overlap: N = 3, overlap 0.5, uneven copies
def test_diagonal_bag_with_shifts_and_overlap_equals_each_models_tracks_opts_bitwise(dmx, bag_models):
    seg = SEG[4]
    audios = _five(seg, 12)
    offs = _offsets(5, 4, 3, 1)
    nsegs = {dmx.track_geometry(seg, audios[3].shape[1], int(s), 0.5)[1] for s in offs[3, 0]}
    assert len(nsegs) > 1, "the copies of a track must differ in segment count"
    refs = _per_model(dmx, bag_models[4], seg, audios, 3, 0.5, offs, 4)
    models, ctx = _open(dmx, bag_models[4], seg, 4, entry=2)
    got = ctx.tracks_bag(models, audios, n_shifts=3, overlap=0.5, shift_offsets=offs)
    for t in range(5):
        for s in range(4):
            assert np.array_equal(got[t][s], refs[s][t][s]), f"track {t}, stem {s}"
    _close(models, ctx)


# ---- 4. one model, and one model listed twice
def test_one_model_and_duplicated_models_give_tracks_opts_bits(dmx, bag_models):
    seg = SEG[4]
    audios = _five(seg, 13)
    offs = _offsets(5, 1, 2, 2)
    p = bag_models[4][1]
    ref = _per_model(dmx, [p], seg, audios, 2, 0.25, offs)[0]
    models, ctx = _open(dmx, [p, p], seg, 3)
    got = ctx.tracks_bag(models[:1], audios, np.ones((1, 4)), 2, 0.25, offs)
    for t in range(5):
        assert np.array_equal(got[t], ref[t]), f"one model, track {t}"
    dup = np.repeat(offs, 2, axis=1)
    for wv, layout in ((1.0, dmx.LAYOUT_PLANAR), (2.0, dmx.LAYOUT_EIGEN)):
        got = ctx.tracks_bag(models, audios, np.full((2, 4), wv), 2, 0.25, dup, layout=layout)
        for t in range(5):
            assert np.array_equal(got[t], ref[t]), f"[A, A] at weights {wv}, track {t}"
    _close(models, ctx)


# ---- 5. general weights against the float64 recombination of the models' own results
W3 = np.array([[0.3, 0.0, 1.7, 0.45], [0.6, 2.2, 0.0, 0.45], [0.0, 0.9, 0.1, 0.45]], np.float32)


def test_general_weights_vs_float64_recombination(dmx, bag_models):
    seg = SEG[4]
    audios = _five(seg, 14)
    offs = _offsets(5, 3, 2, 3)
    paths = bag_models[4][:3]
    refs = _per_model(dmx, paths, seg, audios, 2, 0.25, offs)
    models, ctx = _open(dmx, paths, seg, 3)
    got = ctx.tracks_bag(models, audios, W3, 2, 0.25, offs)
    eff, _ = bag_spec.effective_weights(3, 4, W3)
    for t in range(5):
        outs = [refs[q][t] for q in range(3)]
        ref = bag_spec.recombine64(outs, eff)
        tol = bag_spec.tolerance(outs, _mean(audios[t]))
        err = float(np.abs(got[t] - ref).max())
        print(f"general weights, track {t}: max abs error {err:.3e}, tolerance {tol:.3e}")
        assert np.isfinite(got[t]).all()
        assert err <= tol, (t, err, tol)
    _close(models, ctx)


# ---- 6. PCM output of a bag
@pytest.mark.parametrize("enc,clip,stem", [("PCM_S16", "CLIP_RESCALE", 3), ("PCM_S24", "CLIP_CLAMP", -1)])
def test_bag_pcm_equals_pcm_encode_of_the_fp32_bag(enc, clip, stem, dmx, bag_models):
    seg = SEG[4]
    audios = [a * np.float32(8) for a in _five(seg, 15)]  # loud enough for the clip modes to act
    offs = _offsets(5, 4, 2, 4)
    models, ctx = _open(dmx, bag_models[4], seg, 4)
    fp32 = ctx.tracks_bag(models, audios, n_shifts=2, overlap=0.25, shift_offsets=offs)
    spec = dmx.OutputSpec(getattr(dmx, enc), getattr(dmx, clip), stem)
    outs, peaks = ctx.tracks_bag(models, audios, n_shifts=2, overlap=0.25, shift_offsets=offs, spec=spec)
    for t in range(5):
        want, wpk = dmx.pcm_encode(fp32[t], spec)
        assert len(outs[t]) == len(want) == (4 if stem < 0 else 2)
        assert np.array_equal(peaks[t], wpk), f"track {t}: peaks"
        for o, (g, w) in enumerate(zip(outs[t], want)):
            assert np.array_equal(g, w), f"track {t}, output {o}"
    _close(models, ctx)


# ---- 7. independence of batching, track order and earlier calls; the context keeps its entry model
def test_batching_order_and_reuse_do_not_change_a_bit(dmx, bag_models):
    seg = SEG[4]
    audios = _five(seg, 16)
    offs = _offsets(5, 3, 2, 1)
    paths = bag_models[4][:3]
    ref = None
    for b in (1, 3, 7):
        models, ctx = _open(dmx, paths, seg, b, entry=1)
        if b == 3:
            before = ctx.tracks(audios[1:4], [5, 4033, 20000])
            ctx.tracks_bag(models, _tracks(seg, [2.2, 0.3, 1.1, 0.6], 23), W3, 2, 0.25, None)  # other tracks first: no stale slots
        got = ctx.tracks_bag(models, audios, W3, 2, 0.25, offs)
        if ref is None:
            ref = got
        for t in range(5):
            assert np.array_equal(got[t], ref[t]), f"max_batch {b}, track {t}"
        if b == 3:
            rev = ctx.tracks_bag(models, audios[::-1], W3, 2, 0.25, offs[::-1])[::-1]
            for t in range(5):
                assert np.array_equal(rev[t], ref[t]), f"reversed, track {t}"
            solo = ctx.tracks_bag(models, [audios[3]], W3, 2, 0.25, offs[3:4])[0]
            assert np.array_equal(solo, ref[3]), "track 3 alone"
            after = ctx.tracks(audios[1:4], [5, 4033, 20000])  # the entry model (model 1) is bound again
            for t in range(3):
                assert np.array_equal(after[t], before[t]), f"entry model, track {t}"
        _close(models, ctx)


# ---- 8. random shifts are drawn in (track, model, copy) order
def test_random_offsets_are_drawn_in_track_model_copy_order(dmx, bag_models):
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    seg = SEG[4]
    audios = _tracks(seg, [0.3, 1.4, 0.8], 17)
    paths = bag_models[4][:2]
    models, ctx = _open(dmx, paths, seg, 4)
    w = np.ones((2, 4))
    libc.srand(7)
    draws = np.array([[[libc.rand() % MS for _ in range(2)] for _ in range(2)] for _ in range(3)])
    ref = ctx.tracks_bag(models, audios, w, 2, 0.5, draws)
    libc.srand(7)
    got_null = ctx.tracks_bag(models, audios, w, 2, 0.5, None)
    libc.srand(7)
    got_m1 = ctx.tracks_bag(models, audios, w, 2, 0.5, np.full((3, 2, 2), -1))
    partial = draws.copy()
    partial[0, 1, 0] = partial[2, 0, 1] = -1
    libc.srand(7)
    filled = partial.copy()
    for idx in ((0, 1, 0), (2, 0, 1)):
        filled[idx] = libc.rand() % MS
    want = ctx.tracks_bag(models, audios, w, 2, 0.5, filled)
    libc.srand(7)
    got_mixed = ctx.tracks_bag(models, audios, w, 2, 0.5, partial)
    for t in range(3):
        assert np.array_equal(got_null[t], ref[t]), f"NULL offsets, track {t}"
        assert np.array_equal(got_m1[t], ref[t]), f"-1 offsets, track {t}"
        assert np.array_equal(got_mixed[t], want[t]), f"mixed offsets, track {t}"
    _close(models, ctx)


# ---- 9. argument errors: every message, nothing written
def test_argument_errors_name_what_is_wrong(dmx, bag_models, tmp_models):
    seg = SEG[4]
    models, ctx = _open(dmx, bag_models[4], seg, 2)
    six = dmx.Model(tmp_models[6])
    L = dmx.lib()
    audios = _tracks(seg, [0.5, 0.8, 1.2], 4)
    outs = [np.zeros((4, 2, a.shape[1]), np.float32) for a in audios]
    ap = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in audios])
    op = (ctypes.c_void_p * 3)(*[o.ctypes.data for o in outs])
    na = (ctypes.c_int64 * 3)(*[a.shape[1] for a in audios])
    h = [m.h.value for m in models]

    def call(ms, w, N=1, ov=0.25, offs=None, spec=None):
        mp = (ctypes.c_void_p * max(len(ms), 1))(*ms) if ms is not None else None
        wa = np.ascontiguousarray(w, np.float32) if w is not None else None
        so = (ctypes.c_int * len(offs))(*offs) if offs is not None else None
        return L.dmx_tracks_infer_bag(ctx.h, mp, len(ms) if ms is not None else 4, wa.ctypes.data if wa is not None else None, 3, ap, na,
                                      N, ov, so, ctypes.byref(spec) if spec is not None else None, op, None, dmx.LAYOUT_PLANAR,
                                      None, None)

    ones = np.ones((4, 4))
    no_stem1 = ones.copy(); no_stem1[:, 1] = 0
    no_model3 = ones.copy(); no_model3[3] = 0
    neg = ones.copy(); neg[2, 0] = -1
    nan = ones.copy(); nan[1, 3] = np.nan
    offs24 = [0] * 24
    bad_off = list(offs24); bad_off[(2 * 4 + 1) * 2 + 0] = 22050
    cases = [
        ([], None, {}, "n_models must be in [1, 8]"),
        (h * 3, np.ones((12, 4)), {}, "n_models must be in [1, 8]"),
        (None, None, {}, "null models array"),
        (h[:2] + [None] + h[3:], None, {}, "model 2: null"),
        (h[:2] + [six.h.value] + h[3:], None, {}, "model 2: differs in architecture or device from the context's"),
        (h[:3], None, {}, "needs n_models == n_sources"),
        (h, no_stem1, {}, "weights: stem 1 has no model"),
        (h, no_model3, {}, "weights: model 3 has no non-zero weight"),
        (h, neg, {}, "model 2, stem 0"),
        (h, nan, {}, "model 1, stem 3"),
        (h * 2, np.ones((8, 4)), {"N": 33}, "n_models * n_shifts"),
        (h, None, {"N": 0}, "n_shifts"),
        (h, None, {"ov": 0.95}, "overlap"),
        (h, None, {"N": 2, "offs": bad_off}, "track 2, model 1, shift 0"),
        (h, None, {"spec": dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE, 7)}, "stem 7 of a 4-source model"),
    ]
    for ms, w, kw, what in cases:
        rc = call(ms, w, **kw)
        assert rc == 5, (what, rc)  # DMX_ERR_ARG
        msg = L.dmx_last_error().decode()
        assert what in msg and "dmx_tracks_infer_bag" in msg, (what, msg)
    assert all(not o.any() for o in outs)  # nothing ran
    with pytest.raises(dmx.DmxError, match="weights: stem 1 has no model"):  # through the binding
        ctx.tracks_bag(models, audios, no_stem1)
    ref = ctx.tracks(audios, [1, 2, 3])  # and the context still serves its own model
    assert all(np.isfinite(r).all() for r in ref)
    six.close()
    _close(models, ctx)


# ---- 10. progress
def test_progress_is_monotone_and_ends_at_one(dmx, bag_models):
    seg = SEG[4]
    audios = _five(seg, 14)
    offs = _offsets(5, 4, 2)
    models, ctx = _open(dmx, bag_models[4], seg, 3)
    msgs = []
    ctx.tracks_bag(models, audios, None, 2, 0.5, offs, progress=lambda p, s: msgs.append((p, s)))
    ps = [p for p, _ in msgs]
    per_model = [sum(dmx.track_geometry(seg, a.shape[1], int(s), 0.5)[1] for a, row in zip(audios, offs[:, q, :]) for s in row)
                 for q in range(4)]
    assert len(ps) == 1 + sum((m + 2) // 3 for m in per_model)  # the start, then one report per batch of one model
    assert all(b >= a for a, b in zip(ps, ps[1:])), ps
    assert ps[0] == 0.0 and abs(ps[-1] - 1.0) < 1e-6
    _close(models, ctx)


# ---- 11. Demucs v3
def test_v3_bag_of_two_models(dmx, bag_models):
    seg = SEG[3]
    audios = _tracks(seg, [0, 0.4, 1.3], 18)
    offs = _offsets(3, 2, 2, 2)
    w = np.ones((2, 4))
    refs = _per_model(dmx, bag_models[3], seg, audios, 2, 0.25, offs)
    models, ctx = _open(dmx, bag_models[3], seg, 3)
    got = ctx.tracks_bag(models, audios, w, 2, 0.25, offs)
    for t in range(3):
        outs = [refs[0][t], refs[1][t]]
        ref = bag_spec.recombine64(outs, w)
        tol = bag_spec.tolerance(outs, _mean(audios[t]))
        err = float(np.abs(got[t] - ref).max())
        print(f"v3, two models, track {t}: max abs error {err:.3e}, tolerance {tol:.3e}")
        assert np.isfinite(got[t]).all() and err <= tol, (t, err, tol)
    same = np.repeat(offs[:, :1, :], 2, axis=1)
    dup = ctx.tracks_bag([models[0], models[0]], audios, w, 2, 0.25, same)
    for t in range(3):
        assert np.array_equal(dup[t], refs[0][t]), f"duplicates, track {t}"
    _close(models, ctx)


# ---- 12. the batch CLI
def test_cli_batch_takes_bags(dmx, bag_models, tmp_path):
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    ft = os.path.join(ROOT, "cli", "demucs_ft.cpp.main")
    assert os.path.exists(batch) and os.path.exists(ft), "CLI not built (make cli)"
    rng = np.random.default_rng(19)
    wavs = []
    for name, sec in (("a", 3), ("b", 9)):
        a = (0.1 * rng.standard_normal((2, int(sec * 44100)))).astype(np.float32)
        p = str(tmp_path / f"{name}.wav")
        _write_wav(p, a)
        wavs.append(p)
    env = dict(os.environ, DMX_SHIFT_OFFSET="1337")
    r = subprocess.run([batch, bag_models["dir"], str(tmp_path / "out")] + wavs, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for p in wavs:
        stem = os.path.splitext(os.path.basename(p))[0]
        r = subprocess.run([ft, bag_models["dir"], p, str(tmp_path / "ft" / stem)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for i, nm in enumerate(FT):
            got = (tmp_path / "out" / stem / f"target_{i}_{nm}.wav").read_bytes()
            want = (tmp_path / "ft" / stem / f"target_{i}_{nm}.wav").read_bytes()
            assert got == want, f"{stem}/{nm}"
    two = ",".join(bag_models[4][:2])
    wts = ",".join(["0.3"] * 4 + ["0.7", "0", "1", "2.5"])
    r = subprocess.run([batch, "--bag-weights", wts, "--shifts", "2", "--shift-offsets", "5,4033", "--two-stems", "vocals", two,
                        str(tmp_path / "ens")] + wavs[:1], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "ens" / "a" / "target_0_vocals.wav").exists() and (tmp_path / "ens" / "a" / "target_1_no_vocals.wav").exists()
    r = subprocess.run([batch, two, str(tmp_path / "avg")] + wavs[:1], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    bad = [[two + ","], ["," + two], [two.replace(",", ",,")], ["--bag-weights", "1,1,1", two], ["--bag-weights", wts + ",", two],
           ["--bag-weights", "1,x,1,1,1,1,1,1", two], ["--bag-weights", "1,-1,1,1,1,1,1,1", two],
           ["--bag-weights", "0,1,1,1,0,1,1,1", two], ["--bag-weights", "1,1,1,1", bag_models["dir"]]]
    for extra in bad:
        r = subprocess.run([batch] + extra + [str(tmp_path / "bad")] + wavs[:1], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1, (extra, r.stdout[-500:], r.stderr[-500:])
        assert "Usage" in r.stderr, (extra, r.stderr[-500:])
