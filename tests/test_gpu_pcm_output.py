"""Stems as WAV-ready PCM, encoded on the GPU (include/demucs_hip.h dmx_tracks_infer_pcm / dmx_pcm_encode, csrc/pcm.hip,
binding Context.tracks_pcm / pcm_encode, demucscpp::demucs_inference_batch_pcm through cli/demucs_batch.cpp.main): two-stems,
clip mode and 16 / 24-bit / float32 encoding of the finished track. Every comparison is exact (bytes, or float bit patterns)
against the NumPy specification tests/pcm_spec.py (run with -m gpu on an MI355X)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import pcm_spec as ps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SEG = {4: 8000, 6: 8000, 3: 16384}  # reduced segments, as tests/test_gpu_shifts_overlap.py
ENCODINGS = [ps.PCM_F32, ps.PCM_S16, ps.PCM_S24]
CLIPS = [ps.CLIP_NONE, ps.CLIP_RESCALE, ps.CLIP_CLAMP]
LENGTHS = [1, 2, 3, 4, 5, 7, 255, 256, 1023, 100003]
NAMES = ["drums", "bass", "other", "vocals", "guitar", "piano"]


def _rescale_edge():
    """(the largest fp32 peak with 1.01f * peak <= 1, the smallest with 1.01f * peak > 1)"""
    p = F(1) / F(1.01)
    while F(1.01) * p > 1:
        p = np.nextafter(p, F(0))
    while F(1.01) * np.nextafter(p, F(2)) <= 1:
        p = np.nextafter(p, F(2))
    return p, np.nextafter(p, F(2))


def _specials():
    e16, e24 = 2.0 ** -15, 2.0 ** -23
    v = [(k + 0.5) * e16 for k in (-3, -2, -1, 0, 1, 2, 16382, 32766)]  # exact ties of the 16-bit grid
    v += [(k + 0.5) * e24 for k in (-2, -1, 0, 1, 4194302)]  # and of the 24-bit grid (k + 0.5 needs < 24 bits)
    v += [1.0, -1.0, 1.0 - 2.0 ** -16, -(1.0 - 2.0 ** -16), np.nextafter(F(1), F(2)), -np.nextafter(F(1), F(2)), 1.25, -3.0]
    v += [0.99, -0.99, np.nextafter(F(0.99), F(2)), -np.nextafter(F(0.99), F(2)), np.nextafter(F(0.99), F(0))]
    v += [1e-40, -1e-40, 0.0, -0.0, np.nan, np.inf, -np.inf, 32767.4 * e16, -32768.6 * e16]
    return np.array(v, F)


def _crafted(S, n, seed):
    """(S, 2, n): stem 0 carries the special values (at the head and the tail of long tracks, rotated through short ones),
    stem 1 is all zero (peak 0 -> d = 1), the peaks of stems 2 and 3 put 1.01 * peak just below and just above 1"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.3, 0.3, (S, 2, n)).astype(F)
    sp = np.roll(_specials(), -3 * n)
    flat = v[0].reshape(-1)  # channel-major: both channels get specials
    k = min(len(sp), flat.size)
    flat[:k] = sp[:k]
    if flat.size >= 2 * len(sp):
        flat[-len(sp):] = sp[::-1]
        mid = flat.size // 2  # the end of channel 0 and the start of channel 1
        flat[mid - 8:mid + 8] = sp[:16]
    v[1] = 0
    below, above = _rescale_edge()
    for s, pk in ((2, below), (3, above)):
        v[s] = (rng.uniform(-1, 1, (2, n)) * pk * 0.999).astype(F)
        v[s, (n // 2) % 2, n // 2] = pk if s == 2 else -pk
    return v


# ---- 1. the stage alone
@pytest.mark.parametrize("S", [4, 6])
def test_stage_alone_equals_the_specification(S, dmx):
    below, above = _rescale_edge()
    assert F(1.01) * below <= 1 < F(1.01) * above
    on = off = 0
    for n in LENGTHS:
        v = _crafted(S, n, 100 * S + n)
        for stem in (-1, 0, S - 1):
            for enc in ENCODINGS:
                for clip in CLIPS:
                    got, peaks = dmx.pcm_encode(v, dmx.OutputSpec(enc, clip, stem))
                    want, wpeaks = ps.encode(v, enc, clip, stem)
                    what = f"S {S} n {n} stem {stem} encoding {enc} clip {clip}"
                    assert len(got) == len(want) == (S if stem < 0 else 2), what
                    assert np.array_equal(peaks.view(np.uint32), wpeaks.view(np.uint32)), (what, peaks, wpeaks)
                    for o, (g, w) in enumerate(zip(got, want)):
                        assert ps.same(g, w), f"{what} output {o}: {int((np.asarray(g) != np.asarray(w)).sum())} elements differ"
            if stem < 0:
                assert wpeaks[1] == 0 and wpeaks[2] == below and wpeaks[3] == above, wpeaks
                on += int((F(1.01) * wpeaks[np.isfinite(wpeaks)] > 1).sum())
                off += int((F(1.01) * wpeaks <= 1).sum())
    assert on and off


def test_stage_alone_on_device_memory_with_a_plane_stride(dmx):
    """dmx_pcm_encode_device: planes at a stride larger than n and misaligned against each other, outputs at the 16-byte
    rounded stride, enqueued on a caller's stream"""
    import torch

    S, n, stride = 4, 1021, 1027
    v = _crafted(S, n, 5)
    d_in = torch.zeros(S * 2 * stride + 3, device="cuda")
    d_in[1:1 + S * 2 * stride].view(S * 2, stride)[:, :n] = torch.from_numpy(v.reshape(S * 2, n)).cuda()  # base 4 bytes off 16
    for enc, per in ((ps.PCM_S16, 4), (ps.PCM_S24, 6), (ps.PCM_F32, 8)):
        spec = dmx.OutputSpec(enc, ps.CLIP_RESCALE, 3)
        ostride = (n * per + 15) // 16 * 16
        d_out = torch.full((2 * ostride,), 0x5A, dtype=torch.uint8, device="cuda")
        d_pk = torch.full((2,), -1.0, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        dmx._chk(dmx.lib().dmx_pcm_encode_device(0, d_in.data_ptr() + 4, S, n, stride, ctypes.byref(spec), d_out.data_ptr(),
                                                 d_pk.data_ptr(), s.cuda_stream))
        s.synchronize()
        want, wpeaks = ps.encode(v, enc, ps.CLIP_RESCALE, 3)
        raw = d_out.cpu().numpy()
        assert np.array_equal(d_pk.cpu().numpy().view(np.uint32), wpeaks.view(np.uint32))
        for o in range(2):
            got = dmx.pcm_views(raw[o * ostride:o * ostride + n * per], spec, n, 1)[0]
            assert ps.same(got, want[o]), (enc, o)
    bad = dmx.lib().dmx_pcm_encode_device(0, d_in.data_ptr(), S, n, stride, ctypes.byref(spec), d_out.data_ptr() + 4, d_pk.data_ptr(), None)
    assert bad == 5 and "16-byte aligned" in dmx.lib().dmx_last_error().decode()


# ---- 2. end to end = the specification applied to the fp32 call
AMPS = [0.002, 0.05, 0.5, 5.0, 50.0]  # the result scales with the input: peaks far below and far above 1 / 1.01


def _five(seg, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, (m, amp) in enumerate(zip([0, 0.4, 1.0, 3.3, 7.9], AMPS)):
        n = max(2, int(seg * m)) if m else 2
        out.append((amp * (rng.standard_normal((2, n)) + 0.1 * (i + 1))).astype(F))
    return out


def _offsets(T, N):
    base = [0, 22049, 4033, 12436, 7, 311, 20000]
    return [[base[(t + 2 * k) % len(base)] for k in range(N)] for t in range(T)]


def _check_tracks(got, peaks, ref, enc, clip, stem, what):
    on = off = 0
    for t, (g, pk, r) in enumerate(zip(got, peaks, ref)):
        want, wpeaks = ps.encode(r, enc, clip, stem)
        assert np.array_equal(pk.view(np.uint32), wpeaks.view(np.uint32)), (what, t, pk, wpeaks)
        assert len(g) == len(want)
        for o, (a, b) in enumerate(zip(g, want)):
            assert ps.same(a, b), f"{what} track {t} output {o}: {int((np.asarray(a) != np.asarray(b)).sum())} elements differ"
        on += int((F(1.01) * wpeaks > 1).sum())
        off += int((F(1.01) * wpeaks <= 1).sum())
    return on, off


@pytest.mark.parametrize("N,ov", [(1, 0.25), (3, 0.5)])
@pytest.mark.parametrize("key", [4, 6, 3])
def test_tracks_pcm_equals_the_specification_on_tracks_opts(key, N, ov, dmx, tmp_models):
    seg = SEG[key]
    audios = _five(seg, 31 + key)
    offs = _offsets(5, N)
    m = dmx.Model(tmp_models[key])
    S = m.n_sources
    assert dmx.lib().dmx_output_count(m.h, ctypes.byref(dmx.OutputSpec())) == S
    assert dmx.lib().dmx_output_count(m.h, ctypes.byref(dmx.OutputSpec(stem=S - 1))) == 2
    assert dmx.lib().dmx_output_count(m.h, ctypes.byref(dmx.OutputSpec(stem=S))) == -1
    specs = [(ps.PCM_S16, ps.CLIP_RESCALE, -1), (ps.PCM_S24, ps.CLIP_CLAMP, 0), (ps.PCM_F32, ps.CLIP_RESCALE, S - 1),
             (ps.PCM_S16, ps.CLIP_NONE, 1), (ps.PCM_S24, ps.CLIP_RESCALE, -1)]
    ref = None
    on = off = 0
    for mb in (3, 16):  # 3: every track but the shortest is finished in several pieces
        ctx = dmx.Context(m, seg, mb)
        if ref is None:
            ref = ctx.tracks_opts(audios, N, ov, offs)
        for enc, clip, stem in specs:
            got, peaks = ctx.tracks_pcm(audios, dmx.OutputSpec(enc, clip, stem), N, ov, offs)
            a, b = _check_tracks(got, peaks, ref, enc, clip, stem, f"model {key} N {N} overlap {ov} max_batch {mb} spec {(enc, clip, stem)}")
            if clip == ps.CLIP_RESCALE:
                on, off = on + a, off + b
        if mb == 16 and N == 1:  # the long track alone: all of its segments in one batch, finished in one piece
            assert ctx.track_geometry(audios[4].shape[1], offs[4][0])[1] <= 16
            for enc, clip, stem in specs[:3]:
                got, peaks = ctx.tracks_pcm(audios[4:], dmx.OutputSpec(enc, clip, stem), N, ov, offs[4:])
                _check_tracks(got, peaks, ref[4:], enc, clip, stem, f"model {key} long track alone, spec {(enc, clip, stem)}")
        again = ctx.tracks_opts(audios, N, ov, offs)  # the fp32 call behind PCM calls on the same context: the same bits
        for r, g in zip(ref, again):
            assert np.array_equal(r, g)
        ctx.close()
    print(f"rescale taken for {on} outputs, not taken for {off}")
    assert on > 0 and off > 0, (on, off)  # the test must not pass with the rescale branch never (or always) taken
    m.close()


# ---- 3. / 4. float32 / none / all stems is the fp32 result; batching and company do not change a byte
def test_f32_none_is_the_planar_result_transposed_and_batching_does_not_change_a_byte(dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 77)
    offs = _offsets(5, 1)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    ref = ctx.tracks_opts(audios, 1, 0.25, offs)
    plain = ctx.tracks(audios, [o[0] for o in offs])
    got, peaks = ctx.tracks_pcm(audios, dmx.OutputSpec(ps.PCM_F32, ps.CLIP_NONE, -1), shift_offsets=offs)
    for t in range(5):
        assert np.array_equal(ref[t], plain[t])
        for s in range(4):
            assert np.array_equal(got[t][s].view(np.uint32), np.ascontiguousarray(ref[t][s].T).view(np.uint32)), (t, s)
            assert peaks[t][s] == np.abs(ref[t][s]).max()
    eig, _ = ctx.tracks_pcm(audios, dmx.OutputSpec(ps.PCM_F32, ps.CLIP_NONE, -1), shift_offsets=offs, layout=dmx.LAYOUT_EIGEN)
    for t in range(5):
        for s in range(4):
            assert np.array_equal(eig[t][s].view(np.uint32), got[t][s].view(np.uint32))  # the input layout is plumbing
    spec = dmx.OutputSpec(ps.PCM_S16, ps.CLIP_RESCALE, 3)
    base, bpk = ctx.tracks_pcm(audios, spec, shift_offsets=offs)
    ctx.close()
    for mb in (1, 2, 5, 16):
        c2 = dmx.Context(m, seg, mb)
        g, pk = c2.tracks_pcm(audios, spec, shift_offsets=offs)
        for t in range(5):
            assert np.array_equal(pk[t], bpk[t])
            for o in range(2):
                assert np.array_equal(g[t][o], base[t][o]), (mb, t, o)
        if mb == 2:  # each track alone, and in another order
            for t in (4, 0, 2):
                g1, pk1 = c2.tracks_pcm([audios[t]], spec, shift_offsets=[offs[t]])
                assert np.array_equal(pk1[0], bpk[t]) and all(np.array_equal(g1[0][o], base[t][o]) for o in range(2)), t
            order = [3, 1, 4, 0, 2]
            g2, _ = c2.tracks_pcm([audios[t] for t in order], spec, shift_offsets=[offs[t] for t in order])
            for i, t in enumerate(order):
                assert all(np.array_equal(g2[i][o], base[t][o]) for o in range(2)), t
        c2.close()
    m.close()


# ---- 5. errors on a live context
def test_errors_on_a_live_context_name_the_field_and_write_nothing(dmx, tmp_models):
    seg = SEG[4]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    L = dmx.lib()
    audios = _five(seg, 5)[:3]
    ns = [a.shape[1] for a in audios]
    outs = [np.full(4 * n * 8, 0xA5, np.uint8) for n in ns]
    pk = np.full(12, -7.0, F)
    ptrs = [a.ctypes.data for a in audios]

    def call(T, ap, nn, so, spec, N=1, ov=0.25, op=None):
        apa = (ctypes.c_void_p * 3)(*ap)
        opa = (ctypes.c_void_p * 3)(*(op if op is not None else [o.ctypes.data for o in outs]))
        na = (ctypes.c_int64 * 3)(*nn)
        soa = (ctypes.c_int * len(so))(*so)
        return L.dmx_tracks_infer_pcm(ctx.h, T, apa, na, N, ov, soa, ctypes.byref(dmx.OutputSpec(*spec)), opa, pk.ctypes.data,
                                      dmx.LAYOUT_PLANAR, None, None)

    good = (ps.PCM_S16, ps.CLIP_RESCALE, -1)
    cases = [
        (3, ptrs, ns, [0, 0, 0], (ps.PCM_S16, ps.CLIP_RESCALE, 4), {}, "output spec: stem 4 of a 4-source model"),
        (3, ptrs, ns, [0, 0, 0], (ps.PCM_S16, ps.CLIP_RESCALE, 7), {}, "output spec: stem 7 of a 4-source model"),
        (3, ptrs, ns, [0, 0, 0], (ps.PCM_S16, ps.CLIP_RESCALE, -2), {}, "output spec: stem -2"),
        (3, ptrs, ns, [0, 0, 0], (3, ps.CLIP_RESCALE, -1), {}, "output spec: encoding 3"),
        (3, ptrs, ns, [0, 0, 0], (ps.PCM_S16, -1, -1), {}, "output spec: clip -1"),
        (0, ptrs, ns, [0, 0, 0], good, {}, "n_tracks"),
        (3, [ptrs[0], None, ptrs[2]], ns, [0, 0, 0], good, {}, "track 1"),
        (3, ptrs, [ns[0], ns[1], 1], [0, 0, 0], good, {}, "track 2"),
        (3, ptrs, ns, [0, 22050, 0], good, {}, "track 1"),
        (3, ptrs, ns, [0, 0, 0], good, {"op": [outs[0].ctypes.data, outs[1].ctypes.data, None]}, "track 2: null out pointer"),
        (3, ptrs, ns, [0] * 3, good, {"N": 0}, "n_shifts"),
        (3, ptrs, ns, [0] * 3, good, {"ov": 0.95}, "overlap"),
    ]
    for T, ap, nn, so, spec, kw, what in cases:
        rc = call(T, ap, nn, so, spec, **kw)
        assert rc == 5, (what, rc)  # DMX_ERR_ARG
        msg = L.dmx_last_error().decode()
        assert "dmx_tracks_infer_pcm" in msg and what in msg, msg
        assert all((o == 0xA5).all() for o in outs) and (pk == -7.0).all(), what
    with pytest.raises(dmx.DmxError, match="stem 5 of a 4-source model"):  # through the binding
        ctx.tracks_pcm(audios, dmx.OutputSpec(stem=5))
    # the context still works, and the same call with good arguments fills every byte
    assert call(3, ptrs, ns, [1, 2, 3], (ps.PCM_F32, ps.CLIP_NONE, -1)) == 0
    ref = ctx.tracks(audios, [1, 2, 3])
    for t in range(3):
        g = dmx.pcm_views(outs[t], dmx.OutputSpec(ps.PCM_F32, ps.CLIP_NONE, -1), ns[t], 4)
        for s in range(4):
            assert np.array_equal(g[s].view(np.uint32), np.ascontiguousarray(ref[t][s].T).view(np.uint32))
    assert (pk >= 0).all()
    ctx.close(); m.close()


# ---- 6. progress
@pytest.mark.parametrize("clip", [ps.CLIP_RESCALE, ps.CLIP_CLAMP])
def test_progress_is_monotone_and_ends_at_one(clip, dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 14)
    offs = _offsets(5, 2)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    msgs = []
    ctx.tracks_pcm(audios, dmx.OutputSpec(ps.PCM_S16, clip, 3), 2, 0.25, offs, progress=lambda p, s: msgs.append((p, s)))
    ps_ = [p for p, _ in msgs]
    total = sum(ctx.track_geometry(a.shape[1], s)[1] for a, o in zip(audios, offs) for s in o)
    assert len(ps_) == 1 + (total + 2) // 3  # the start, then one report per batch
    assert all(b >= a for a, b in zip(ps_, ps_[1:])), ps_
    assert ps_[0] == 0.0 and abs(ps_[-1] - 1.0) < 1e-6
    ctx.close(); m.close()


# ---- 7. the batch CLI
def _write_wav(path, audio, rate=44100):
    audio = np.asarray(audio, F)
    ch = audio.shape[0]
    data = np.ascontiguousarray(audio.T).tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 3, ch, rate, rate * 4 * ch, 4 * ch, 32))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def _read(path):
    """(format tag, channels, rate, bits, data bytes) of a canonical 44-byte-header WAV file"""
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    assert struct.unpack_from("<I", b, 4)[0] == len(b) - 8 and struct.unpack_from("<I", b, 40)[0] == len(b) - 44
    _, tag, nch, rate, brate, align, bits = struct.unpack_from("<IHHIIHH", b, 16)
    assert align == nch * bits // 8 and brate == rate * align
    return tag, nch, rate, bits, b[44:]


def test_cli_output_options(dmx, tmp_models, tmp_path):
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    single = os.path.join(ROOT, "cli", "demucs.cpp.main")
    assert os.path.exists(batch) and os.path.exists(single), "CLIs not built (make cli)"
    rng = np.random.default_rng(23)
    wavs = []
    for name, sec, amp in (("quiet", 3, 0.01), ("loud", 9, 3.0)):
        p = str(tmp_path / f"{name}.wav")
        _write_wav(p, (amp * rng.standard_normal((2, int(sec * 44100)))).astype(F))
        wavs.append(p)
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033")

    def run(exe, extra, out, files):
        args = [exe] + extra + ([tmp_models[4], str(tmp_path / out)] + files if exe == batch else [tmp_models[4], files[0], str(tmp_path / out)])
        return subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)

    r = run(batch, [], "plain", wavs)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # without the new options: the files of the untouched single-file CLI, byte for byte
    r = run(single, [], "single", wavs[1:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for i in range(4):
        f = f"target_{i}_{NAMES[i]}.wav"
        assert (tmp_path / "plain" / "loud" / f).read_bytes() == (tmp_path / "single" / f).read_bytes(), f
    stems = {}
    for w in ("quiet", "loud"):
        planes = []
        for i in range(4):
            tag, nch, rate, bits, data = _read(tmp_path / "plain" / w / f"target_{i}_{NAMES[i]}.wav")
            assert (tag, nch, rate, bits) == (3, 2, 44100, 32)
            planes.append(np.frombuffer(data, F).reshape(-1, 2).T)
        stems[w] = np.stack(planes)

    r = run(batch, ["--two-stems", "vocals", "--int24", "--clip-mode", "clamp"], "karaoke", wavs)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for w in ("quiet", "loud"):
        want, _ = ps.encode(stems[w], ps.PCM_S24, ps.CLIP_CLAMP, 3)
        assert sorted(os.listdir(tmp_path / "karaoke" / w)) == ["target_0_vocals.wav", "target_1_no_vocals.wav"]
        for o, f in enumerate(("target_0_vocals.wav", "target_1_no_vocals.wav")):
            tag, nch, rate, bits, data = _read(tmp_path / "karaoke" / w / f)
            assert (tag, nch, rate, bits) == (1, 2, 44100, 24), f
            assert data == want[o].tobytes(), (w, f)

    r = run(batch, ["--int16"], "int16", wavs)  # the defaults with any output option: demucs's rescale, all stems
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    on = off = 0
    for w in ("quiet", "loud"):
        want, peaks = ps.encode(stems[w], ps.PCM_S16, ps.CLIP_RESCALE, -1)
        on, off = on + int((F(1.01) * peaks > 1).sum()), off + int((F(1.01) * peaks <= 1).sum())
        for i in range(4):
            tag, nch, rate, bits, data = _read(tmp_path / "int16" / w / f"target_{i}_{NAMES[i]}.wav")
            assert (tag, nch, rate, bits) == (1, 2, 44100, 16)
            assert data == want[i].tobytes(), (w, i)
    print(f"CLI --int16: rescale taken for {on} stems, not taken for {off}")

    r = run(batch, ["--two-stems", "guitar"], "guitar", wavs[:1])  # a stem name, but not of this model: known after loading
    assert r.returncode == 1 and "Usage" not in r.stderr and "guitar" in r.stderr and "no such stem" in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "guitar").exists()


# ---- 8. full size
def test_full_size_two_stems_int16_rescale(dmx, tmp_models):
    seg = 343980
    rng = np.random.default_rng(3)
    audio = (0.6 * rng.standard_normal((2, int(2.3 * seg) + 1))).astype(F)  # an odd length: misaligned planes, an edge group
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, 0, 2)
    ref = ctx.tracks_opts([audio], 1, 0.25, [[4033]])
    for enc, clip, stem in ((ps.PCM_S16, ps.CLIP_RESCALE, 3), (ps.PCM_S24, ps.CLIP_RESCALE, -1)):
        got, peaks = ctx.tracks_pcm([audio], dmx.OutputSpec(enc, clip, stem), shift_offsets=[[4033]])
        _check_tracks(got, peaks, ref, enc, clip, stem, f"full size {(enc, clip, stem)}")
        print("full size peaks", peaks[0])
    ctx.close(); m.close()
