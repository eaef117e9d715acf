"""The FLAC input stage on the GPU (csrc/flac_in.hip) against tests/flac_in_spec.py: the ground truth of a
written stream is the integers handed to the writer, the reference decoder defines status and `good` of a damaged one.
Every comparison is by equality. The written files are made once per module."""
import functools
import os
import wave

import numpy as np
import pytest

import flac_in_spec as fis
import flac_spec as fs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stage():
    """the binding without a GEMM mode: the stage alone is integer code behind no model"""
    from demucs_cpp_amd import binding

    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


@functools.lru_cache(maxsize=None)
def _matrix():
    return fis.matrix()


@functools.lru_cache(maxsize=None)
def _damaged():
    return {k: (v, fis.decode(v)) for k, v in fis.damaged().items()}


def _stereo(x):
    return np.repeat(x, 2, axis=1) if x.shape[1] == 1 else x


def test_matrix_decodes_to_the_samples_the_writer_was_given(stage):
    m = _matrix()
    assert len(m) >= 55
    for name, (data, x, bits, channels, lay) in m.items():
        got, status, good, info = stage.flac_decode(data)
        assert (status, good) == (fis.OK, x.shape[0]), name
        assert (info.channels, info.bits, info.first_frame) == (channels, bits, lay["first"]), name
        assert got.dtype == np.float32 and np.array_equal(got, fis.as_f32(_stereo(x), bits)), name
        if channels == 2 and bits in (16, 24):
            enc = stage.PCM_S16 if bits == 16 else stage.PCM_S24
            raw, status, good, _ = stage.flac_decode(data, enc)
            assert (status, good) == (fis.OK, x.shape[0]), name
            assert np.array_equal(fs.pcm_ints(raw.view(np.uint8), bits), x), name


@pytest.mark.parametrize("bits", [16, 24])
def test_round_trip_through_the_encoder_stage(bits, stage):
    enc = stage.PCM_S16 if bits == 16 else stage.PCM_S24
    for sig in fs.SIGNALS:
        for n in (1, 4095, 4096, 4097, 12293):
            x = fs.crafted(sig, n, bits)
            b = fs.pcm_bytes(x, bits)
            pcm = b.view("<i2").reshape(-1, 2) if bits == 16 else b.reshape(-1, 2, 3)
            data = stage.flac_encode(pcm, bits)
            raw, status, good, _ = stage.flac_decode(data, enc)
            assert (status, good) == (fis.OK, n), (sig, n)
            assert raw.dtype == pcm.dtype and np.array_equal(raw, pcm), (sig, n)
            f, status, good, _ = stage.flac_decode(data)
            assert (status, good) == (fis.OK, n) and np.array_equal(f, fis.as_f32(x, bits)), (sig, n)


def test_a_wav_written_as_flac_decodes_to_the_floats_of_the_wav(stage, golden_dir):
    with wave.open(os.path.join(golden_dir, "gspi_stereo.wav")) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, 44100)
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2)
    want = pcm.astype(np.float32) / np.float32(32768.0)  # cli/wav.hpp: (float)v / 32768.0f
    data = stage.flac_encode(np.ascontiguousarray(pcm), 16)
    assert len(data) < 0.8 * pcm.nbytes
    got, status, good, info = stage.flac_decode(data)
    assert (status, good, info.sample_rate) == (fis.OK, pcm.shape[0], 44100)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_damaged_files_give_the_reference_status_good_and_zeros(stage):
    d = _damaged()
    assert len(d) == 40
    for name, (data, ref) in d.items():
        got, status, good, info = stage.flac_decode(data)
        assert (status, good) == (ref["status"], ref["good"]) and status == fis.BROKEN, (name, status, good, ref["good"])
        assert np.array_equal(got, fis.as_f32(ref["samples"], 16)), name
        assert not got[good:].any(), name
        raw, status, good, _ = stage.flac_decode(data, stage.PCM_S16)
        assert (status, good) == (ref["status"], ref["good"]) and np.array_equal(raw, ref["samples"].astype(np.int16)), name


def test_too_many_header_look_alikes_are_a_status_not_a_fault(stage):
    got, status, good, info = stage.flac_decode(fis.too_many_candidates())
    assert (status, good, info.total_samples) == (fis.TOO_MANY_CANDIDATES, 0, 4096) and not got.any()


def test_on_device_memory_with_a_dirty_workspace_and_output(stage):
    """dmx_flac_decode_device: asynchronous on a stream, the workspace and the output need no initialisation"""
    import ctypes

    import torch

    data, ref = _damaged()["residual_bit"]
    info = stage.flac_probe(data)
    n = int(info.total_samples)
    L = stage.lib()
    wb = L.dmx_flac_decode_workspace_bytes(ctypes.byref(info), len(data))
    assert wb > 0 and wb % 16 == 0
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_work = torch.full((wb,), 0xA5, dtype=torch.uint8, device="cuda")
    d_out = torch.full(((n * 8 + 15) // 16 * 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_status = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = L.dmx_flac_decode_device(0, d_file.data_ptr(), len(data), ctypes.byref(info), stage.PCM_F32, d_out.data_ptr(), d_status.data_ptr(),
                                  d_work.data_ptr(), s.cuda_stream)
    assert rc == 0, L.dmx_last_error()
    s.synchronize()
    assert d_status.cpu().tolist() == [ref["status"], ref["good"]]
    got = d_out.cpu().numpy()[:n * 8].view(np.float32).reshape(n, 2)
    assert np.array_equal(got, fis.as_f32(ref["samples"], 16))


# ---- the track path: tracks given as .flac files
import pcm_spec as ps  # noqa: E402
import remix_spec as rs  # noqa: E402

SEG = 8000  # the reduced segment of tests/test_gpu_flac.py


@functools.lru_cache(maxsize=None)
def _track_files():
    """three tracks of 0.4, 1 and 3.3 segments as .flac files: 16-bit stereo, 16-bit MONO, 24-bit stereo - and their integers"""
    rng = np.random.default_rng(91)
    ns = (int(0.4 * SEG), SEG, int(3.3 * SEG))
    xs = [fis._signal(rng, ns[0], 2, 16), fis._signal(rng, ns[1], 1, 16), fis._signal(rng, ns[2], 2, 24)]
    files = []
    for x, bits, ch in zip(xs, (16, 16, 24), (2, 1, 2)):
        sizes = fis._fixed_sizes(x.shape[0], 1152)
        files.append(fis.write([fis.frame(b, assignment=10 if ch == 2 else None, subs=[fis.sub("FIXED", order=2, method=int(bits == 24))] * ch)
                                for b in fis._blocks(x, sizes)], ch, bits)[0])
    return files, xs, (16, 16, 24)


def _planar(files, xs, bits):
    return [np.ascontiguousarray(fis.as_f32(_stereo(x), b).T) for x, b in zip(xs, bits)]


def _same(a, b):
    return all(np.array_equal(np.asarray(p).view(np.uint8), np.asarray(q).view(np.uint8)) for ta, tb in zip(a, b) for p, q in zip(ta, tb))


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("clip", [ps.CLIP_CLAMP, ps.CLIP_RESCALE])
def test_tracks_from_flac_equals_tracks_remix_on_the_decoded_floats(clip, N, dmx, tmp_models):
    files, xs, bits = _track_files()
    audios = _planar(files, xs, bits)
    offs = [[(4033 * (t + 1) + 311 * k) % 22050 for k in range(N)] for t in range(3)]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, SEG, 3)
    for enc, flac_out in ((ps.PCM_F32, False), (ps.PCM_S16, False), (ps.PCM_S24, True)):
        spec = dmx.RemixSpec(rs.fractional(4)[:2], enc, clip)
        got, gpeaks, status = ctx.tracks_from_flac(files, spec, n_shifts=N, shift_offsets=offs, flac_out=flac_out)
        assert status.tolist() == [[fis.OK, x.shape[0]] for x in xs]
        if flac_out:
            want, wpeaks = ctx.tracks_flac(audios, spec, n_shifts=N, shift_offsets=offs)
            assert got == want
            assert fs.decode(got[2][0])[1:] == (24, 44100)
        else:
            want, wpeaks = ctx.tracks_remix(audios, spec, n_shifts=N, shift_offsets=offs)
            assert _same(got, want)
        assert all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(gpeaks, wpeaks))
    ctx.close(); m.close()


def test_tracks_from_flac_with_a_two_model_bag(dmx, tmp_path):
    from demucs_cpp_amd.weights import write_synthetic_model

    paths = [str(tmp_path / f"ggml-model-htdemucs_bag_{i}-4s-f16.bin") for i in range(2)]
    for i, p in enumerate(paths):
        write_synthetic_model(p, 4, 80 + i)
    files, xs, bits = _track_files()
    audios = _planar(files, xs, bits)
    offs = np.array([[[(4033 * (t + 1) + 977 * q) % 22050] for q in range(2)] for t in range(3)])
    models = [dmx.Model(p) for p in paths]
    ctx = dmx.Context(models[0], SEG, 3)
    w = np.array([[1, 0.5, 0, 2], [1, 0.5, 3, 0]], np.float32)
    spec = dmx.RemixSpec(rs.fractional(4)[:2], ps.PCM_S16, ps.CLIP_RESCALE)
    want, wpeaks = ctx.tracks_remix(audios, spec, models=models, weights=w, shift_offsets=offs)
    got, gpeaks, status = ctx.tracks_from_flac(files, spec, models=models, weights=w, shift_offsets=offs)
    assert _same(got, want) and status[:, 0].tolist() == [0, 0, 0]
    assert all(np.array_equal(a, b) for a, b in zip(gpeaks, wpeaks))
    ctx.close()
    for m in models:
        m.close()


def test_a_damaged_middle_track_fails_the_call_and_leaves_the_others_whole(dmx, tmp_models):
    files, xs, bits = _track_files()
    lay = fis.write([fis.frame(b, subs=[fis.sub("FIXED", order=2)]) for b in fis._blocks(xs[1], fis._fixed_sizes(SEG, 1152))], 1, 16)[1]
    bad = bytearray(files[1])
    a, b = lay["frames"][3]
    bad[(a + b) // 2] ^= 0x10  # inside the fourth frame
    bad = bytes(bad)
    ref = fis.decode(bad)
    assert (ref["status"], ref["good"]) == (fis.BROKEN, 3 * 1152)
    offs = [[4033], [12436], [7]]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, SEG, 3)
    spec = dmx.RemixSpec(rs.fractional(4)[:2], ps.PCM_S16, ps.CLIP_RESCALE)
    alone, apeaks, _ = ctx.tracks_from_flac([files[0], files[2]], spec, shift_offsets=[offs[0], offs[2]])
    status = np.full(6, -5, np.int64)
    with pytest.raises(dmx.DmxError) as e:
        ctx.tracks_from_flac([files[0], bad, files[2]], spec, shift_offsets=offs, track_status=status)
    assert "track 1" in str(e.value) and "sample 3456" in str(e.value), str(e.value)
    assert status.reshape(3, 2).tolist() == [[fis.OK, xs[0].shape[0]], [fis.BROKEN, 3 * 1152], [fis.OK, xs[2].shape[0]]]
    outs, peaks = e.value.partial
    assert _same([outs[0], outs[2]], alone) and np.array_equal(peaks[0], apeaks[0]) and np.array_equal(peaks[2], apeaks[1])
    # the damaged track ran on its good samples and silence: what the decoded floats give
    dec, st, good, _ = dmx.flac_decode(bad)
    want, _ = ctx.tracks_remix([np.ascontiguousarray(dec.T)], spec, shift_offsets=[offs[1]])
    assert _same([outs[1]], want)
    # a file the probe refuses, or at another rate: the call fails before any GPU work and names the track
    for badfile, text in ((files[2][:30], "track 2"), (fis.write([fis.frame(xs[0][:64])], 2, 16, rate=48000)[0], "track 2: sample rate 48000")):
        with pytest.raises(dmx.DmxError) as e:
            ctx.tracks_from_flac([files[0], files[1], badfile], spec, shift_offsets=offs)
        assert text in str(e.value), str(e.value)
    ctx.close(); m.close()


# ---- the batch CLI
def test_cli_writes_for_a_flac_input_what_it_writes_for_the_wav(stage, tmp_models, golden_dir, tmp_path):
    import shutil
    import subprocess

    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    wav = os.path.join(golden_dir, "gspi_stereo_short.wav")
    with wave.open(wav) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, 44100)
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2)
    os.makedirs(tmp_path / "in")
    flac = str(tmp_path / "in" / "gspi_stereo_short.flac")
    with open(flac, "wb") as f:
        f.write(fis.id3v2(33) + stage.flac_encode(np.ascontiguousarray(pcm), 16))
    other = str(tmp_path / "in" / "second.wav")
    shutil.copy(wav, other)
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033", DMX_BATCH="2")

    def run(extra, out, inputs):
        r = subprocess.run([batch] + extra + [tmp_models[4], str(tmp_path / out)] + inputs, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        d = tmp_path / out / "gspi_stereo_short"
        return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}

    want, got = run([], "plain_wav", [wav]), run([], "plain_flac", [flac])  # the file goes to the GPU as it is
    assert len(want) == 4 and got.keys() == want.keys() and all(got[k] == want[k] for k in want)
    # with output options; and beside a WAV input, where the .flac file is decoded first (dmx_flac_decode) and takes the WAV path
    two = ["--two-stems", "vocals", "--flac"]
    want = run(two, "two_wav", [wav])
    for out, inputs in (("two_flac", [flac]), ("two_mixed", [flac, other])):
        got = run(two, out, inputs)
        assert len(want) == 2 and got.keys() == want.keys() and all(got[k] == want[k] for k in want), out
