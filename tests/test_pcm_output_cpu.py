"""The PCM output stage without a GPU (include/demucs_hip.h dmx_output_count / dmx_output_bytes / dmx_tracks_infer_pcm,
cli/wav.hpp write_pcm_file, the batch CLI's option parsing) and the self-checks of its NumPy specification
(tests/pcm_spec.py). The kernels themselves are pinned against that specification in tests/test_gpu_pcm_output.py."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import pcm_spec as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMX_ERR_ARG = 5
HARNESS = os.path.join(ROOT, "tests", "_build", "pcm_wav_harness")
BATCH = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
F = np.float32


@pytest.fixture(scope="module")
def dmx():
    so = os.path.join(ROOT, "demucs_cpp_amd", "lib", "libdemucs_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", ROOT, "demucs_cpp_amd/lib/libdemucs_hip.so"], stdout=subprocess.DEVNULL)
    from demucs_cpp_amd import binding
    return binding


# ---- the ABI
def test_header_constants_and_exports(dmx):
    hdr = open(os.path.join(ROOT, "include", "demucs_hip.h")).read()
    for line in ("#define DMX_PCM_F32 0", "#define DMX_PCM_S16 1", "#define DMX_PCM_S24 2", "#define DMX_CLIP_NONE 0",
                 "#define DMX_CLIP_RESCALE 1", "#define DMX_CLIP_CLAMP 2"):
        assert line in hdr, line
    for sym in ("dmx_output_count", "dmx_output_bytes", "dmx_tracks_infer_pcm", "dmx_pcm_encode_device", "dmx_pcm_encode"):
        assert sym in dmx.EXPORTS and hasattr(dmx.lib(), sym), sym
    assert (dmx.PCM_F32, dmx.PCM_S16, dmx.PCM_S24) == (ps.PCM_F32, ps.PCM_S16, ps.PCM_S24) == (0, 1, 2)
    assert (dmx.CLIP_NONE, dmx.CLIP_RESCALE, dmx.CLIP_CLAMP) == (ps.CLIP_NONE, ps.CLIP_RESCALE, ps.CLIP_CLAMP) == (0, 1, 2)
    assert "packed" in hdr.lower() and "dmx_engine_track_infer returns fp32" in hdr  # 24 bit is 3 bytes; the engine is out of scope
    d = dmx.OutputSpec()  # demucs's defaults
    assert (d.encoding, d.clip, d.stem) == (dmx.PCM_S16, dmx.CLIP_RESCALE, -1)


def test_output_bytes_table(dmx):
    L = dmx.lib()
    for enc, per in ((dmx.PCM_F32, 8), (dmx.PCM_S16, 4), (dmx.PCM_S24, 6)):
        for clip in (0, 1, 2):
            for stem in (-1, 0, 5):
                for n in (0, 1, 2, 3, 343980, 10_584_000, 1 << 33):
                    assert dmx.output_bytes(dmx.OutputSpec(enc, clip, stem), n) == n * per
    assert L.dmx_output_bytes(None, 10) == -1
    assert L.dmx_output_bytes(ctypes.byref(dmx.OutputSpec(3, 0, -1)), 10) == -1
    assert L.dmx_output_bytes(ctypes.byref(dmx.OutputSpec(-1, 0, -1)), 10) == -1
    assert L.dmx_output_bytes(ctypes.byref(dmx.OutputSpec(1, 3, -1)), 10) == -1
    assert L.dmx_output_bytes(ctypes.byref(dmx.OutputSpec(1, 1, -2)), 10) == -1
    assert L.dmx_output_bytes(ctypes.byref(dmx.OutputSpec()), -1) == -1
    with pytest.raises(dmx.DmxError, match="output spec: encoding 7"):
        dmx.output_bytes(dmx.OutputSpec(7, 0, -1), 4)


def test_output_count_needs_a_model_and_a_valid_spec(dmx):
    """(the counts themselves - S, or 2 in two-stems mode - need a loaded model: tests/test_gpu_pcm_output.py)"""
    L = dmx.lib()
    assert L.dmx_output_count(None, ctypes.byref(dmx.OutputSpec())) == -1
    assert L.dmx_output_count(None, None) == -1


def _call(dmx, spec, ctx=None):
    L = dmx.lib()
    a = np.zeros((2, 100), np.float32)
    o = np.full(4 * 100 * 8, 0xA5, np.uint8)
    pk = np.full(4, -7.0, np.float32)
    ap = (ctypes.c_void_p * 1)(a.ctypes.data)
    op = (ctypes.c_void_p * 1)(o.ctypes.data)
    na = (ctypes.c_int64 * 1)(100)
    rc = L.dmx_tracks_infer_pcm(ctx, 1, ap, na, 1, 0.25, None, ctypes.byref(spec) if spec is not None else None, op, pk.ctypes.data,
                                dmx.LAYOUT_PLANAR, None, None)
    assert (o == 0xA5).all() and (pk == -7.0).all()  # nothing written
    return rc, L.dmx_last_error().decode()


@pytest.mark.parametrize("spec,what", [(None, "output spec: null"), ((3, 0, -1), "output spec: encoding 3"),
                                       ((-1, 0, -1), "output spec: encoding -1"), ((1, -1, -1), "output spec: clip -1"),
                                       ((1, 3, -1), "output spec: clip 3"), ((1, 1, -2), "output spec: stem -2")])
def test_tracks_infer_pcm_rejects_a_bad_spec_before_anything(dmx, spec, what):
    """the spec's own fields are checked first: no context, no device (stem >= S needs the model: GPU test)"""
    rc, msg = _call(dmx, dmx.OutputSpec(*spec) if spec is not None else None)
    assert rc == DMX_ERR_ARG
    assert "dmx_tracks_infer_pcm" in msg and what in msg, msg


def test_tracks_infer_pcm_rejects_a_null_context(dmx):
    rc, msg = _call(dmx, dmx.OutputSpec())
    assert rc == DMX_ERR_ARG and "null context" in msg, msg


def test_pcm_encode_rejects_bad_arguments_before_the_device(dmx):
    L = dmx.lib()
    x = np.zeros((4, 2, 8), np.float32)
    out = np.full(4 * 8 * 8, 0xA5, np.uint8)
    for spec, ns, n, what in (((3, 0, -1), 4, 8, "encoding 3"), ((1, 1, 4), 4, 8, "stem 4 of a 4-source model"), ((1, 1, -1), 0, 8, "n_sources"),
                              ((1, 1, -1), 4, 0, "n < 1")):
        rc = L.dmx_pcm_encode(0, x.ctypes.data, ns, n, ctypes.byref(dmx.OutputSpec(*spec)), out.ctypes.data, None)
        assert rc == DMX_ERR_ARG and what in L.dmx_last_error().decode(), (spec, L.dmx_last_error())
    assert (out == 0xA5).all()


# ---- the specification's self-checks
def test_spec_ties_go_to_even():
    k = np.arange(-6, 7)
    y = ((k + 0.5) / 32768).astype(F)  # exact in fp32
    x = np.stack([y, y])[None]
    (q,), _ = ps.encode(x, ps.PCM_S16, ps.CLIP_NONE)
    want = np.where(k % 2 == 0, k, k + 1)  # k + 0.5 -> the even neighbour
    assert np.array_equal(q[:, 0], want) and np.array_equal(q[:, 1], want)
    y24 = ((k + 0.5) / 8388608).astype(F)
    (b,), _ = ps.encode(np.stack([y24, y24])[None], ps.PCM_S24, ps.CLIP_NONE)
    assert np.array_equal(ps.s24_to_int(b)[:, 0], want)


def test_spec_saturation_and_special_values():
    v = np.array([1.0, -1.0, 1.0 - 2.0 ** -16, -(1.0 - 2.0 ** -16), 1.5, -1.5, np.inf, -np.inf, np.nan, 1e-40, 0.0], F)
    x = np.stack([v, v])[None]
    (q,), pk = ps.encode(x, ps.PCM_S16, ps.CLIP_NONE)
    assert q[:, 0].tolist() == [32767, -32768, 32767, -32768, 32767, -32768, 32767, -32768, 0, 0, 0]  # (1 - 2^-16) 2^15 = 32767.5 -> 32768 -> sat
    assert np.isinf(pk[0])  # NaN ignored, inf is the peak
    (b,), _ = ps.encode(x, ps.PCM_S24, ps.CLIP_NONE)
    assert ps.s24_to_int(b)[:, 1].tolist() == [8388607, -8388608, 8388480, -8388480, 8388607, -8388608, 8388607, -8388608, 0, 0, 0]
    assert b[0, 0].tolist() == [0xFF, 0xFF, 0x7F] and b[1, 0].tolist() == [0x00, 0x00, 0x80]  # little-endian, 3 bytes
    (f,), _ = ps.encode(x, ps.PCM_F32, ps.CLIP_NONE)
    assert ps.same(f, np.ascontiguousarray(x[0].T))
    (c,), _ = ps.encode(x, ps.PCM_F32, ps.CLIP_CLAMP)
    assert c[:8, 0].tolist() == [F(0.99), F(-0.99)] * 4 and np.isnan(c[8, 0]) and c[9, 0] == F(1e-40)
    assert ps.peak(np.full((2, 3), np.nan, F)) == 0 and ps.peak(np.zeros((2, 0), F)) == 0


def test_spec_rescale_branch_on_and_off():
    below = np.nextafter(F(1) / F(1.01), F(0))  # 1.01 * peak < 1
    while F(1.01) * below >= 1:
        below = np.nextafter(below, F(0))
    above = np.nextafter(below, F(2))
    while F(1.01) * above <= 1:
        above = np.nextafter(above, F(2))
    for pk, on in ((below, False), (above, True), (F(0), False), (F(3), True)):
        x = np.array([[pk, -pk / 2, pk / 8], [pk / 16, pk / 4, -pk]], F)[None]
        (y,), peaks = ps.encode(x, ps.PCM_F32, ps.CLIP_RESCALE)
        assert peaks[0] == pk
        d = F(1.01) * pk
        assert (d > 1) == on
        want = (x[0] / d).astype(F) if on else x[0]
        assert ps.same(y, np.ascontiguousarray(want.T))
        if on:
            assert np.abs(y).max() < 1  # what rescale is for: 1 / 1.01 at the peak
    x = np.array([[2.0, -1.0], [0.5, 0.25]], F)[None]
    (q,), _ = ps.encode(x, ps.PCM_S16, ps.CLIP_RESCALE)
    assert q.tolist() == [[int(np.rint(F(2) / F(2.02) * F(32768))), int(np.rint(F(0.5) / F(2.02) * F(32768)))],
                          [int(np.rint(F(-1) / F(2.02) * F(32768))), int(np.rint(F(0.25) / F(2.02) * F(32768)))]]


def test_spec_two_stems_adds_the_other_stems_in_increasing_order_from_the_first():
    # fp32 addition is not associative: (1 + 2^-24) + 2^-24 = 1 (both ties to even), 1 + (2^-24 + 2^-24) = 1 + 2^-23
    e = F(2.0 ** -24)
    v = np.zeros((4, 2, 1), F)
    v[0], v[1], v[2], v[3] = 1.0, e, e, 7.0
    o = ps.outputs(v, 3)
    assert o.shape == (2, 2, 1) and o[0, 0, 0] == 7 and o[1, 0, 0] == F(1)
    o = ps.outputs(v[[1, 2, 0, 3]], 3)  # e + e + 1
    assert o[1, 0, 0] == F(1) + F(2.0 ** -23)
    # "starting from the first of them": -0 alone stays -0 (0 + -0 would be +0)
    v = np.zeros((4, 2, 1), F)
    v[1:] = -0.0
    assert np.signbit(ps.outputs(v, 0)[1]).all()
    assert ps.outputs(v, -1).shape == (4, 2, 1)
    outs, peaks = ps.encode(np.ones((6, 2, 5), F), ps.PCM_S16, ps.CLIP_RESCALE, 2)
    assert len(outs) == 2 and peaks.tolist() == [1.0, 5.0] and outs[0].shape == (5, 2) and outs[0].dtype == np.int16


# ---- cli/wav.hpp write_pcm_file
@pytest.mark.parametrize("enc,tag,bits", [(ps.PCM_F32, 3, 32), (ps.PCM_S16, 1, 16), (ps.PCM_S24, 1, 24)])
@pytest.mark.parametrize("n", [1, 2, 5, 1000])
def test_write_pcm_file_header_and_round_trip(enc, tag, bits, n, tmp_path):
    if not os.path.exists(HARNESS):
        subprocess.check_call(["make", "-C", ROOT, "tests/_build/pcm_wav_harness"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(n)
    x = (1.2 * rng.uniform(-1, 1, (1, 2, n))).astype(F)
    (enc_out,), _ = ps.encode(x, enc, ps.CLIP_NONE)
    raw, wav, dump = tmp_path / "in.raw", tmp_path / "out.wav", tmp_path / "dump.f32"
    raw.write_bytes(enc_out.tobytes())
    r = subprocess.run([HARNESS, str(enc), "44100", str(raw), str(wav), str(dump)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    b = wav.read_bytes()
    align = 2 * bits // 8
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and struct.unpack_from("<I", b, 4)[0] == len(b) - 8
    assert struct.unpack_from("<IHHIIHH", b, 16) == (16, tag, 2, 44100, 44100 * align, align, bits)
    assert b[36:40] == b"data" and struct.unpack_from("<I", b, 40)[0] == n * align and len(b) == 44 + n * align
    assert b[44:] == enc_out.tobytes()  # the bytes as they are
    got = np.fromfile(dump, F).reshape(n, 2)
    if enc == ps.PCM_F32:
        want = enc_out
    elif enc == ps.PCM_S16:
        want = enc_out.astype(F) / F(32768)
    else:
        want = ps.s24_to_int(enc_out).astype(F) / F(8388608)
    assert np.array_equal(got, want)
    # another rate goes into the header (the reader refuses it, as the reference does)
    r = subprocess.run([HARNESS, str(enc), "48000", str(raw), str(wav), str(dump)], capture_output=True, text=True)
    assert r.returncode == 0 and struct.unpack_from("<II", wav.read_bytes(), 24) == (48000, 48000 * align)


# ---- the batch CLI's options: usage errors come before the model is loaded
@pytest.mark.parametrize("extra", [["--two-stems", "flute"], ["--two-stems", ""], ["--two-stems"], ["--clip-mode", "soft"],
                                   ["--clip-mode", ""], ["--clip-mode"], ["--int16", "--two-stems"], ["--int32"],
                                   ["--float32", "--clip-mode", "Rescale"], ["--two-stems", "Vocals"]])
def test_cli_usage_errors(extra, tmp_path):
    if not os.path.exists(BATCH):
        subprocess.check_call(["make", "-C", ROOT, "cli/demucs_batch.cpp.main"], stdout=subprocess.DEVNULL)
    args = [BATCH] + extra
    if len(extra) > 1 or extra[0] == "--int32":  # a lone option that needs a value stays the last argument
        args += [str(tmp_path / "no-such-model.bin"), str(tmp_path / "out"), str(tmp_path / "no-such.wav")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (extra, r.stdout, r.stderr)
    assert "Usage" in r.stderr and "--two-stems NAME" in r.stderr and "--int16|--int24|--float32" in r.stderr, r.stderr
    assert "Error loading model" not in r.stderr and not (tmp_path / "out").exists()


@pytest.mark.parametrize("extra", [["--two-stems", "guitar"], ["--int24"], ["--int16", "--float32", "--clip-mode", "none"],
                                   ["--shifts", "2", "--int16", "--overlap", "0.5"]])
def test_cli_valid_options_get_as_far_as_the_model(extra, tmp_path):
    """all six stem names parse (whether the loaded model has the stem is known only after loading); value-less options
    do not swallow the next argument"""
    args = [BATCH] + extra + [str(tmp_path / "no-such-model.bin"), str(tmp_path / "out"), str(tmp_path / "no-such.wav")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage" not in r.stderr and "Error loading model" in r.stderr, (r.stdout, r.stderr)
