"""The FLAC output stage's compression levels on the GPU (include/demucs_hip.h dmx_flac_encode_level /
dmx_ctx_set_flac_level, csrc/flac.hip, binding flac_encode(level=) / Context.flac_level, demucscpp::remix_options.flac_level
through cli/demucs_batch.cpp.main --flac-level). Every file is compared byte for byte with the NumPy specification
tests/flac_lpc_spec.py - which is what proves that the kernel's binary64 Levinson-Durbin rounds as Python's floats do - and
the project's own GPU reader (csrc/flac_in.hip) takes the LPC streams back (run with -m gpu on an MI355X)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import flac_in_spec as fis
import flac_lpc_spec as ls
import flac_spec as fs
import pcm_spec as ps
import remix_spec as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SEG = {4: 8000, 3: 16384}  # reduced segments, as tests/test_gpu_flac.py
BITS = {ps.PCM_S16: 16, ps.PCM_S24: 24}


@pytest.fixture(scope="module")
def stage():
    """the binding without a GEMM mode: the stage alone is integer and binary64 code behind no model"""
    from demucs_cpp_amd import binding

    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


@functools.lru_cache(maxsize=None)
def _reference(name, n, bits, level, rate=44100):
    x = ls.crafted(name, n, bits)
    data, decisions = ls.encode(x, bits, rate, level)
    return x, data, decisions


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
@pytest.mark.parametrize("name", ls.SIGNALS)
def test_stage_alone_equals_the_specification(name, bits, stage):
    for n in ls.LENGTHS:
        for level in (1, 2):
            x, want, _ = _reference(name, n, bits, level)
            got = stage.flac_encode(_as_pcm(x, bits), bits, level=level)
            assert got == want, (name, n, bits, level, _first_difference(got, want))
            assert len(got) <= stage.flac_bound(bits, n)


@pytest.mark.parametrize("bits", [16, 24])
def test_level_0_through_the_new_entry_point_is_the_old_entry_point(bits, stage):
    L = stage.lib()
    for name in ("sine_noise", "ar2_resonance", "white_noise"):
        for n in (15, 4097, 3 * 4096 + 123):
            x = ls.crafted(name, n, bits)
            pcm = np.ascontiguousarray(_as_pcm(x, bits))
            old = stage.flac_encode(pcm, bits)
            out = np.zeros(stage.flac_bound(bits, n), np.uint8)
            size = np.zeros(1, np.int64)
            stage._chk(L.dmx_flac_encode_level(0, pcm.ctypes.data, bits, n, 44100, 0, out.ctypes.data, size.ctypes.data))
            new = out[:int(size[0])].tobytes()
            assert new == old, (name, n, bits, _first_difference(new, old))
            assert old == fs.encode(x, bits)[0]


def test_stage_alone_on_device_memory_at_48_khz(stage):
    import torch

    L = stage.lib()
    n, bits, level = 3 * 4096 + 123, 24, 2
    x, want, decisions = _reference("sine_noise", n, bits, level, 48000)
    assert any(s["type"] == "LPC" for d in decisions for s in d["sub"])
    bound, work = stage.flac_bound(bits, n), L.dmx_flac_workspace_bytes(bits, n)
    d_pcm = torch.from_numpy(fs.pcm_bytes(x, bits).copy()).cuda()
    d_out = torch.full((bound + 3,), 0x5A, dtype=torch.uint8, device="cuda")
    d_size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_work = torch.full((work,), 0xC3, dtype=torch.uint8, device="cuda")  # a dirty workspace
    # an output at an odd address: frames and the header are placed with byte and dword stores
    stage._chk(L.dmx_flac_encode_device_level(0, d_pcm.data_ptr(), bits, n, 48000, level, d_out.data_ptr() + 3, d_size.data_ptr(),
                                              d_work.data_ptr(), None))
    torch.cuda.synchronize()
    size = int(d_size.item())
    raw = d_out.cpu().numpy()
    got = raw[3:3 + size].tobytes()
    assert got == want, _first_difference(got, want)
    assert (raw[:3] == 0x5A).all() and (raw[3 + size:] == 0x5A).all()  # nothing outside the file is written
    ref = fis.decode(got)
    assert ref["status"] == fis.OK and ref["info"]["rate"] == 48000 and np.array_equal(ref["samples"], x)
    d_out.fill_(0x5A)
    for bad in (-1, 3):
        assert L.dmx_flac_encode_device_level(0, d_pcm.data_ptr(), bits, n, 48000, bad, d_out.data_ptr(), d_size.data_ptr(),
                                              d_work.data_ptr(), None) == 5
        assert f"level {bad}" in L.dmx_last_error().decode()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()


# ---- 2. the writer meets the project's reader on LPC streams
@pytest.mark.parametrize("name,bits,order", [("sine_noise", 24, 12), ("ar2_resonance", 16, 8)])
def test_the_gpu_reader_takes_back_what_the_gpu_writer_wrote(name, bits, order, stage):
    n = 3 * 4096 + 123
    x, want, decisions = _reference(name, n, bits, 2)
    assert any(s["type"] == "LPC" and s["order"] == order for d in decisions for s in d["sub"])
    data = stage.flac_encode(_as_pcm(x, bits), bits, level=2)
    assert data == want
    samples, status, good, info = stage.flac_decode(data, ps.PCM_S16 if bits == 16 else ps.PCM_S24)
    assert (status, good) == (stage.FLAC_OK, n) and (info.bits, info.sample_rate, info.total_samples) == (bits, 44100, n)
    assert np.array_equal(fs.pcm_ints(np.ascontiguousarray(samples).view(np.uint8), bits), x)


# ---- 3. the track path: the files hold the bytes of tracks_remix, coded at the context's level
def _tracks(seg, seed, mults=(0, 0.4, 1.0, 3.3), amps=(0.002, 0.05, 0.5, 5.0)):
    rng = np.random.default_rng(seed)
    out = []
    for i, (m, amp) in enumerate(zip(mults, amps)):
        n = max(2, int(seg * m)) if m else 2
        out.append((amp * (rng.standard_normal((2, n)) + 0.1 * (i + 1))).astype(F))
    return out


def _check_files(files, pcm, bits, level, what):
    assert len(files) == len(pcm)
    for t, (ft, pt) in enumerate(zip(files, pcm)):
        assert len(ft) == len(pt)
        for o, (f, p) in enumerate(zip(ft, pt)):
            x = fs.pcm_ints(np.ascontiguousarray(p).view(np.uint8), bits)
            want = ls.encode(x, bits, 44100, level)[0]
            assert f == want, f"{what} track {t} output {o}: {_first_difference(f, want)}"
            assert len(f) <= fs.bound(bits, x.shape[0])


@pytest.mark.parametrize("clip,enc", [(ps.CLIP_CLAMP, ps.PCM_S16), (ps.CLIP_RESCALE, ps.PCM_S24)])
def test_tracks_flac_codes_the_bytes_of_tracks_remix_at_the_contexts_level(clip, enc, dmx, tmp_models):
    seg = SEG[4]
    audios = _tracks(seg, 61)
    offs = [[4033], [7], [311], [12436]]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    spec = dmx.RemixSpec(rs.fractional(4)[:2], enc, clip)
    assert ctx.flac_level == 0
    pcm, peaks = ctx.tracks_remix(audios, spec, shift_offsets=offs)
    before, _ = ctx.tracks_flac(audios, spec, shift_offsets=offs)
    ctx.flac_level = 2
    assert ctx.flac_level == 2
    files, fpeaks = ctx.tracks_flac(audios, spec, shift_offsets=offs)
    _check_files(files, pcm, BITS[enc], 2, f"clip {clip} enc {enc} level 2")
    assert all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(fpeaks, peaks))
    assert all(len(f) <= len(b) for ft, bt in zip(files, before) for f, b in zip(ft, bt))
    with pytest.raises(dmx.DmxError, match="dmx_ctx_set_flac_level: level 3"):
        ctx.flac_level = 3
    with pytest.raises(dmx.DmxError, match="dmx_ctx_set_flac_level: level -1"):
        ctx.flac_level = -1
    assert ctx.flac_level == 2  # a refused value changes nothing
    ctx.flac_level = 0
    after, _ = ctx.tracks_flac(audios, spec, shift_offsets=offs)
    assert after == before
    _check_files(after, pcm, BITS[enc], 0, "back at level 0")
    ctx.close(); m.close()


def test_tracks_from_flac_with_flac_out_at_level_1(dmx, tmp_models):
    seg = SEG[4]
    xs = [ls.crafted("ar2_resonance", int(0.4 * seg), 16), ls.crafted("sine_noise", int(2.3 * seg), 24)]
    inputs = [dmx.flac_encode(_as_pcm(x, b), b, level=2) for x, b in zip(xs, (16, 24))]  # LPC streams in, too
    offs = [[4033], [311]]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    spec = dmx.RemixSpec(rs.fractional(4)[:2], ps.PCM_S16, ps.CLIP_RESCALE)
    pcm, peaks, status = ctx.tracks_from_flac(inputs, spec, shift_offsets=offs)
    assert status.tolist() == [[fis.OK, x.shape[0]] for x in xs]
    ctx.flac_level = 1
    files, fpeaks, status = ctx.tracks_from_flac(inputs, spec, shift_offsets=offs, flac_out=True)
    assert status.tolist() == [[fis.OK, x.shape[0]] for x in xs]
    _check_files(files, pcm, 16, 1, "from flac, level 1")
    ctx.close(); m.close()


# ---- 4. the batch CLI
def _wav_data(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    return int.from_bytes(b[34:36], "little"), b[44:]


def test_cli_flac_level(dmx, tmp_models, golden_dir, tmp_path):
    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    wav = os.path.join(golden_dir, "gspi_stereo_short.wav")
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033", DMX_BATCH="2")

    def run(extra, out):
        return subprocess.run([batch] + extra + [tmp_models[4], str(tmp_path / out), wav], env=env, capture_output=True, text=True, timeout=600)

    names = ["target_0_drums", "target_1_bass", "target_2_other", "target_3_vocals"]
    r = run(["--int16"], "wav")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = run(["--flac", "--flac-level", "2"], "flac2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = tmp_path / "flac2" / "gspi_stereo_short"
    assert sorted(os.listdir(d)) == [f + ".flac" for f in names]
    for f in names:
        wbits, data = _wav_data(tmp_path / "wav" / "gspi_stereo_short" / (f + ".wav"))
        assert wbits == 16
        blob = (d / (f + ".flac")).read_bytes()
        ref = fis.decode(blob)
        assert ref["status"] == fis.OK and (ref["info"]["bits"], ref["info"]["rate"]) == (16, 44100)
        assert fs.pcm_bytes(ref["samples"], 16).tobytes() == data, f
        assert blob == ls.encode(fs.pcm_ints(np.frombuffer(data, np.uint8), 16), 16, 44100, 2)[0], f
    for bad in ("3", "-1", "two"):
        r = run(["--flac", "--flac-level", bad], "bad")
        assert r.returncode == 1 and "Usage:" in r.stderr and "--flac-level" in r.stderr, r.stderr[-500:]
        assert not (tmp_path / "bad").exists()
