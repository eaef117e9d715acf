"""Stems as FLAC, coded on the GPU (include/demucs_hip.h dmx_flac_encode / dmx_tracks_infer_flac, csrc/flac.hip, binding
flac_encode / Context.tracks_flac, demucscpp::remix_options.flac through cli/demucs_batch.cpp.main --flac). Every file is
compared byte for byte with the NumPy specification tests/flac_spec.py and decoded by its independent decoder; the PCM
behind a file is the bytes Context.tracks_remix returns for the same arguments (run with -m gpu on an MI355X)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import flac_spec as fs
import pcm_spec as ps
import remix_spec as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SEG = {4: 8000, 3: 16384}  # reduced segments, as tests/test_gpu_pcm_output.py
BITS = {ps.PCM_S16: 16, ps.PCM_S24: 24}


@pytest.fixture(scope="module")
def stage():
    """the binding without a GEMM mode: the stage alone is integer code behind no model"""
    from demucs_cpp_amd import binding

    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


@functools.lru_cache(maxsize=None)
def _reference(name, n, bits):
    x = fs.crafted(name, n, bits)
    return x, fs.encode(x, bits)[0]


def _as_pcm(x, bits):
    """int (n, 2) -> what the PCM stage returns: np.int16 (n, 2) or np.uint8 (n, 2, 3)"""
    b = fs.pcm_bytes(x, bits)
    return b.view("<i2").reshape(-1, 2) if bits == 16 else b.reshape(-1, 2, 3)


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))
    return f"lengths {len(a)} / {len(b)}, first differing byte {int(d[0]) if d.size else m}"


# ---- 1. the stage alone, byte for byte
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("name", fs.SIGNALS)
def test_stage_alone_equals_the_specification(name, bits, stage):
    for n in fs.LENGTHS:
        x, want = _reference(name, n, bits)
        got = stage.flac_encode(_as_pcm(x, bits), bits)
        assert got == want, (name, n, bits, _first_difference(got, want))
        y, b, rate = fs.decode(got)
        assert (b, rate) == (bits, 44100) and np.array_equal(x, y), (name, n, bits)
        assert len(got) <= stage.flac_bound(bits, n)


def test_stage_alone_on_device_memory_at_48_khz(stage):
    import torch

    L = stage.lib()
    n, bits = 3 * 4096 + 123, 24
    x = fs.crafted("sine_noise", n, bits)
    want, _ = fs.encode(x, bits, 48000)
    bound, work = stage.flac_bound(bits, n), L.dmx_flac_workspace_bytes(bits, n)
    d_pcm = torch.from_numpy(fs.pcm_bytes(x, bits).copy()).cuda()
    d_out = torch.full((bound + 3,), 0x5A, dtype=torch.uint8, device="cuda")
    d_size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_work = torch.zeros(work, dtype=torch.uint8, device="cuda")
    # an output at an odd address: frames and the header are placed with byte and dword stores
    stage._chk(L.dmx_flac_encode_device(0, d_pcm.data_ptr(), bits, n, 48000, d_out.data_ptr() + 3, d_size.data_ptr(), d_work.data_ptr(), None))
    torch.cuda.synchronize()
    size = int(d_size.item())
    raw = d_out.cpu().numpy()
    got = raw[3:3 + size].tobytes()
    assert got == want, _first_difference(got, want)
    assert (raw[:3] == 0x5A).all() and (raw[3 + size:] == 0x5A).all()  # nothing outside the file is written
    y, b, rate = fs.decode(got)
    assert (b, rate) == (bits, 48000) and np.array_equal(x, y)
    d_out.fill_(0x5A)
    assert L.dmx_flac_encode_device(0, d_pcm.data_ptr() + 4, bits, n - 1, 48000, d_out.data_ptr(), d_size.data_ptr(), d_work.data_ptr(), None) == 5
    assert "16-byte aligned" in L.dmx_last_error().decode()
    assert L.dmx_flac_encode_device(0, d_pcm.data_ptr(), bits, n, 48000, d_out.data_ptr(), None, d_work.data_ptr(), None) == 5
    assert "d_size" in L.dmx_last_error().decode()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()


# ---- 2. frame numbers up to the 3-byte form
def test_frame_numbers_reach_the_three_byte_form(stage):
    n = 2049 * 4096 + 7
    x = np.zeros((n, 2), np.int16)
    got = stage.flac_encode(x, 16)
    want, decisions = fs.encode(x, 16)
    assert len(decisions) == 2050 and all(s["type"] == "CONSTANT" for d in decisions for s in d["sub"])
    assert got == want, _first_difference(got, want)
    # 128 one-byte, 1920 two-byte and 2 three-byte frame numbers; the last frame carries its block size
    full = lambda nb: 4 + nb + 1 + 2 * 3 + 2  # header, CRC-8, two CONSTANT subframes of 8 + 16 bits, CRC-16
    assert len(got) == 42 + 128 * full(1) + 1920 * full(2) + 1 * full(3) + (full(3) + 2)
    info = int.from_bytes(got[8:26], "big")
    assert (info >> 88) & 0xFFFFFF == full(1) and (info >> 64) & 0xFFFFFF == full(3) + 2  # min / max frame size
    assert info & ((1 << 36) - 1) == n and info >> 128 == 4096 and (info >> 112) & 0xFFFF == 4096
    y, bits, rate = fs.decode(got)
    assert bits == 16 and y.shape == (n, 2) and not y.any()


# ---- 3. the track path: the files hold the bytes of tracks_remix
def _tracks(seg, seed, mults=(0, 0.4, 1.0, 3.3, 7.9), amps=(0.002, 0.05, 0.5, 5.0, 50.0)):
    rng = np.random.default_rng(seed)
    out = []
    for i, (m, amp) in enumerate(zip(mults, amps)):
        n = max(2, int(seg * m)) if m else 2
        out.append((amp * (rng.standard_normal((2, n)) + 0.1 * (i + 1))).astype(F))
    return out


def _offsets(T, N):
    base = [0, 22049, 4033, 12436, 7, 311, 20000]
    return [[base[(t + 2 * k) % len(base)] for k in range(N)] for t in range(T)]


def _check_files(files, fpeaks, pcm, peaks, bits, what):
    assert len(files) == len(pcm)
    for t, (ft, pt) in enumerate(zip(files, pcm)):
        assert np.array_equal(np.asarray(fpeaks[t]).view(np.uint32), np.asarray(peaks[t]).view(np.uint32)), (what, t)
        assert len(ft) == len(pt)
        for o, (f, p) in enumerate(zip(ft, pt)):
            x = fs.pcm_ints(np.ascontiguousarray(p).view(np.uint8), bits)
            y, b, rate = fs.decode(f)
            assert (b, rate) == (bits, 44100) and np.array_equal(x, y), f"{what} track {t} output {o}: the file does not decode to the PCM"
            want = fs.encode(x, bits)[0]
            assert f == want, f"{what} track {t} output {o}: {_first_difference(f, want)}"
            assert len(f) <= fs.bound(bits, x.shape[0])


@pytest.mark.parametrize("N,ov", [(1, 0.25), (3, 0.5)])
@pytest.mark.parametrize("enc", [ps.PCM_S16, ps.PCM_S24])
@pytest.mark.parametrize("clip", [ps.CLIP_CLAMP, ps.CLIP_RESCALE])
def test_tracks_flac_holds_the_bytes_of_tracks_remix(clip, enc, N, ov, dmx, tmp_models):
    seg = SEG[4]
    audios = _tracks(seg, 61)
    offs = _offsets(5, N)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)  # every track but the shortest is finished in several pieces
    spec = dmx.RemixSpec(rs.fractional(4)[:2], enc, clip)
    pcm, peaks = ctx.tracks_remix(audios, spec, n_shifts=N, overlap=ov, shift_offsets=offs)
    sizes = np.full(10, -1, np.int64)
    files, fpeaks = ctx.tracks_flac(audios, spec, n_shifts=N, overlap=ov, shift_offsets=offs, sizes=sizes)
    assert [len(f) for ft in files for f in ft] == list(sizes)
    _check_files(files, fpeaks, pcm, peaks, BITS[enc], f"clip {clip} enc {enc} N {N} overlap {ov}")
    again, _ = ctx.tracks_remix(audios, spec, n_shifts=N, overlap=ov, shift_offsets=offs)  # the PCM call behind a FLAC call: the same bytes
    assert all(np.array_equal(a, b) for ta, tb in zip(pcm, again) for a, b in zip(ta, tb))
    ctx.close(); m.close()


def test_tracks_flac_on_the_v3_model(dmx, tmp_models):
    seg = SEG[3]
    audios = _tracks(seg, 62, (0, 1.0, 2.6), (0.01, 0.5, 20.0))
    offs = _offsets(3, 1)
    m = dmx.Model(tmp_models[3]); ctx = dmx.Context(m, seg, 3)
    spec = dmx.RemixSpec(rs.fractional(4)[:2], ps.PCM_S16, ps.CLIP_RESCALE)
    pcm, peaks = ctx.tracks_remix(audios, spec, shift_offsets=offs)
    files, fpeaks = ctx.tracks_flac(audios, spec, shift_offsets=offs)
    _check_files(files, fpeaks, pcm, peaks, 16, "v3")
    ctx.close(); m.close()


def test_tracks_flac_with_a_two_model_bag(dmx, tmp_path):
    from demucs_cpp_amd.weights import write_synthetic_model

    paths = [str(tmp_path / f"ggml-model-htdemucs_bag_{i}-4s-f16.bin") for i in range(2)]
    for i, p in enumerate(paths):
        write_synthetic_model(p, 4, 70 + i)
    seg = SEG[4]
    audios = _tracks(seg, 63, (0.4, 1.0, 3.3), (0.05, 0.5, 30.0))
    offs = np.array([[[(4033 * (t + 1) + 977 * q) % 22050] for q in range(2)] for t in range(3)])
    models = [dmx.Model(p) for p in paths]
    ctx = dmx.Context(models[0], seg, 3)
    w = np.array([[1, 0.5, 0, 2], [1, 0.5, 3, 0]], F)
    spec = dmx.RemixSpec(rs.fractional(4)[:2], ps.PCM_S24, ps.CLIP_RESCALE)
    pcm, peaks = ctx.tracks_remix(audios, spec, models=models, weights=w, shift_offsets=offs)
    files, fpeaks = ctx.tracks_flac(audios, spec, models=models, weights=w, shift_offsets=offs)
    _check_files(files, fpeaks, pcm, peaks, 24, "bag")
    ctx.close()
    for m in models:
        m.close()


def test_two_stems_minus_the_eigen_layout_and_batching_do_not_change_a_byte(dmx, tmp_models):
    seg = SEG[4]
    audios = _tracks(seg, 64, (0, 0.4, 1.0, 3.3), (0.002, 0.05, 0.5, 40.0))
    offs = _offsets(4, 1)
    m = dmx.Model(tmp_models[4])
    spec = dmx.RemixSpec(dmx.remix_two_stems(4, 3, dmx.OTHER_MINUS), ps.PCM_S16, ps.CLIP_RESCALE)
    base = None
    for mb in (1, 4):
        ctx = dmx.Context(m, seg, mb)
        files, fpeaks = ctx.tracks_flac(audios, spec, shift_offsets=offs)
        eig, epeaks = ctx.tracks_flac(audios, spec, shift_offsets=offs, layout=dmx.LAYOUT_EIGEN)
        assert eig == files and all(np.array_equal(a, b) for a, b in zip(epeaks, fpeaks))  # the input layout is plumbing
        if base is None:
            base = files
            pcm, peaks = ctx.tracks_remix(audios, spec, shift_offsets=offs)
            _check_files(files, fpeaks, pcm, peaks, 16, "two-stems minus")
        assert files == base, mb
        ctx.close()
    m.close()


# ---- 4. errors on a live context
def test_errors_on_a_live_context_name_the_field_and_write_nothing(dmx, tmp_models):
    seg = SEG[4]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    L = dmx.lib()
    audios = _tracks(seg, 5)[:3]
    ns = [a.shape[1] for a in audios]
    outs = [np.full(2 * dmx.flac_bound(16, n), 0xA5, np.uint8) for n in ns]
    pk = np.full(6, -7.0, F)
    sizes = np.full(6, -9, np.int64)
    g = rs.fractional(4)[:2]

    def call(enc=ps.PCM_S16, rate=44100, sz=sizes.ctypes.data, T=3, so=(1, 2, 3)):
        spec = dmx.RemixSpec(g, enc, ps.CLIP_RESCALE)
        apa = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in audios])
        opa = (ctypes.c_void_p * 3)(*[o.ctypes.data for o in outs])
        na = (ctypes.c_int64 * 3)(*ns)
        soa = (ctypes.c_int * 3)(*so)
        return L.dmx_tracks_infer_flac(ctx.h, None, 0, None, T, apa, na, 1, 0.25, soa, ctypes.byref(spec.c), rate, opa, sz, pk.ctypes.data,
                                       dmx.LAYOUT_PLANAR, None, None)

    for kw, what in (({"enc": ps.PCM_F32}, "encoding DMX_PCM_F32"), ({"enc": 3}, "encoding 3"), ({"sz": None}, "sizes"),
                     ({"rate": 0}, "sample_rate 0"), ({"rate": 655351}, "sample_rate 655351"), ({"T": 0}, "n_tracks"),
                     ({"so": (1, 22050, 3)}, "track 1")):
        rc = call(**kw)
        assert rc == 5, (what, rc)  # DMX_ERR_ARG
        msg = L.dmx_last_error().decode()
        assert "dmx_tracks_infer_flac" in msg and what in msg, msg
        assert all((o == 0xA5).all() for o in outs) and (pk == -7.0).all() and (sizes == -9).all(), what
    with pytest.raises(dmx.DmxError, match="encoding DMX_PCM_F32"):  # through the binding
        ctx.tracks_flac(audios, dmx.RemixSpec(g, ps.PCM_F32, ps.CLIP_NONE))
    # the context still works: the same call with good arguments writes the files and nothing behind them
    assert call() == 0
    pcm, peaks = ctx.tracks_remix(audios, dmx.RemixSpec(g, ps.PCM_S16, ps.CLIP_RESCALE), shift_offsets=[[1], [2], [3]])
    for t in range(3):
        bd = dmx.flac_bound(16, ns[t])
        for o in range(2):
            sz = int(sizes[2 * t + o])
            want = fs.encode(pcm[t][o], 16)[0]
            assert outs[t][o * bd:o * bd + sz].tobytes() == want, (t, o)
            assert (outs[t][o * bd + sz:(o + 1) * bd] == 0xA5).all(), (t, o)  # one copy of exactly the file's length
    assert np.array_equal(pk.view(np.uint32), np.concatenate(peaks).view(np.uint32))
    ctx.close(); m.close()


# ---- 5. progress
@pytest.mark.parametrize("clip", [ps.CLIP_RESCALE, ps.CLIP_CLAMP])
def test_progress_is_monotone_and_ends_at_one(clip, dmx, tmp_models):
    seg = SEG[4]
    audios = _tracks(seg, 14)
    offs = _offsets(5, 2)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    msgs = []
    ctx.tracks_flac(audios, dmx.RemixSpec(rs.fractional(4)[:2], ps.PCM_S16, clip), n_shifts=2, overlap=0.25, shift_offsets=offs,
                    progress=lambda p, s: msgs.append((p, s)))
    ps_ = [p for p, _ in msgs]
    total = sum(ctx.track_geometry(a.shape[1], s)[1] for a, o in zip(audios, offs) for s in o)
    assert len(ps_) == 1 + (total + 2) // 3  # the start, then one report per batch
    assert all(b >= a for a, b in zip(ps_, ps_[1:])), ps_
    assert ps_[0] == 0.0 and abs(ps_[-1] - 1.0) < 1e-6
    ctx.close(); m.close()


# ---- 6. the batch CLI
def _wav_data(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    return int.from_bytes(b[34:36], "little"), b[44:]


def test_cli_flac(dmx, tmp_models, golden_dir, tmp_path):
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    wav = os.path.join(golden_dir, "gspi_stereo_short.wav")
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033", DMX_BATCH="2")

    def run(extra, out):
        return subprocess.run([batch] + extra + [tmp_models[4], str(tmp_path / out), wav], env=env, capture_output=True, text=True, timeout=600)

    for name, extra, files, bits in (("two", ["--two-stems", "vocals"], ["target_0_vocals", "target_1_no_vocals"], 16),
                                     ("int24", ["--int24"], ["target_0_drums", "target_1_bass", "target_2_other", "target_3_vocals"], 24)):
        r = run(extra, name + "_wav")
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        r = run(extra + ["--flac"], name + "_flac")
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        d = tmp_path / (name + "_flac") / "gspi_stereo_short"
        assert sorted(os.listdir(d)) == [f + ".flac" for f in files]
        for f in files:
            wbits, data = _wav_data(tmp_path / (name + "_wav") / "gspi_stereo_short" / (f + ".wav"))
            assert wbits == bits
            y, b, rate = fs.decode((d / (f + ".flac")).read_bytes())
            assert (b, rate) == (bits, 44100)
            assert fs.pcm_bytes(y, bits).tobytes() == data, f
    r = run(["--float32", "--flac"], "bad")
    assert r.returncode == 1 and "--float32" in r.stderr and "--flac" in r.stderr and "exclude each other" in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "bad").exists()
