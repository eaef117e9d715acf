"""The FLAC stage's specification and its independent decoder (tests/flac_spec.py), and the pure-host entry points
(include/demucs_hip.h dmx_flac_bound / dmx_flac_workspace_bytes). No GPU. There is no FLAC decoder on the machines that
run this suite, so conformance rests on the decoder in tests/flac_spec.py, written from RFC 9639, and on the CRC check
values below."""
import functools
import os
import re

import numpy as np
import pytest

import flac_spec as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _encoded(name, n, bits):
    x = fs.crafted(name, n, bits)
    data, decisions = fs.encode(x, bits)
    return x, data, decisions


def test_crc_check_values():
    msg = b"123456789"
    assert fs.enc_crc8(msg) == 0xF4 and fs.enc_crc16(msg) == 0xFEE8
    assert fs.dec_crc8(msg) == 0xF4 and fs.dec_crc16(msg) == 0xFEE8 and fs._dec_crc16_fast(msg) == 0xFEE8


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("name", fs.SIGNALS)
def test_round_trip_on_the_crafted_inputs(name, bits):
    for n in fs.LENGTHS:
        x, data, decisions = _encoded(name, n, bits)
        assert x.shape == (n, 2) and x.min() >= -(1 << (bits - 1)) and x.max() < 1 << (bits - 1)
        assert len(decisions) == (n + 4095) // 4096
        y, b, rate = fs.decode(data)
        assert (b, rate) == (bits, 44100)
        assert np.array_equal(x, y), (name, n, bits)
        assert len(data) <= fs.bound(bits, n), (name, n, bits, len(data))
        assert np.array_equal(fs.pcm_ints(fs.pcm_bytes(x, bits), bits), x)


def test_the_decoder_rejects_a_flipped_bit_and_other_rates_survive():
    x, data, _ = _encoded("sine_noise", 4097, 16)
    for pos in (len(data) - 1, len(data) // 2, 46):
        bad = bytearray(data)
        bad[pos] ^= 0x10
        with pytest.raises(fs.FlacError):
            fs.decode(bytes(bad))
    for rate in (48000, 96000, 1, 655350):  # 96000 is carried by STREAMINFO alone (sample rate nibble 0000)
        d, _ = fs.encode(x, 16, rate)
        y, b, r = fs.decode(d)
        assert r == rate and np.array_equal(x, y)
        assert d[42 + 2] & 0xF == {48000: 0b1010}.get(rate, 0)


def test_the_crafted_inputs_cover_every_decision():
    types, orders, channels, parts, big_k = set(), set(), set(), set(), False
    for bits in (16, 24):
        for name in fs.SIGNALS:
            for n in fs.LENGTHS:
                for d in _encoded(name, n, bits)[2]:
                    channels.add(d["channels"])
                    for s in d["sub"]:
                        types.add(s["type"])
                        if s["type"] == "FIXED":
                            orders.add(s["order"])
                            parts.add(s["p"])
                            assert len(s["k"]) == 1 << s["p"] and max(s["k"]) <= (14 if bits == 16 else 30)
                            big_k = big_k or (bits == 24 and max(s["k"]) > 14)
    assert types == {"CONSTANT", "VERBATIM", "FIXED"}
    assert orders == {0, 1, 2, 3, 4}
    assert channels == {0b0001, 0b1000, 0b1001, 0b1010}
    assert 0 in parts and max(parts) >= 1
    assert big_k


def test_the_bound_holds_on_full_scale_noise_and_equals_the_library():
    from demucs_cpp_amd import binding as dmx

    L = dmx.lib()
    for bits in (16, 24):
        for n in fs.LENGTHS + (8192, 1 << 20, (1 << 36) - 1):
            want = (42 + 18 * ((n + 4095) // 4096) + n * 2 * bits // 8 + 15) // 16 * 16
            assert fs.bound(bits, n) == want == L.dmx_flac_bound(bits, n) == dmx.flac_bound(bits, n)
            assert L.dmx_flac_workspace_bytes(bits, n) >= want - 42 and L.dmx_flac_workspace_bytes(bits, n) % 16 == 0
        for n in fs.LENGTHS:  # the worst case: every subframe VERBATIM
            x, data, decisions = _encoded("white_noise", n, bits)
            assert len(data) <= fs.bound(bits, n)
            full = decisions[:n // 4096]  # (a short last frame may be CONSTANT or find a cheaper FIXED)
            assert all(s["type"] == "VERBATIM" for d in full for s in d["sub"])
            if full:
                assert len(data) > n * 2 * bits // 8


def test_pure_host_entry_points_reject_bad_arguments_and_are_declared():
    from demucs_cpp_amd import binding as dmx

    L = dmx.lib()
    for fn in (L.dmx_flac_bound, L.dmx_flac_workspace_bytes):
        assert fn(8, 100) == -1 and fn(16, 0) == -1 and fn(24, 1 << 36) == -1 and fn(32, 5) == -1 and fn(16, -3) == -1
        assert fn(16, 1) > 0 and fn(24, (1 << 36) - 1) > 0
    with pytest.raises(dmx.DmxError):
        dmx.flac_bound(8, 100)
    hdr = open(os.path.join(ROOT, "include", "demucs_hip.h")).read()
    for sym in ("dmx_flac_bound", "dmx_flac_workspace_bytes", "dmx_flac_encode_device", "dmx_flac_encode", "dmx_tracks_infer_flac"):
        assert sym in dmx.EXPORTS and hasattr(L, sym) and re.search(r"\b%s\(" % sym, hdr), sym
    # the argument checks of the stage come before any GPU work
    size = np.zeros(1, np.int64)
    buf = np.zeros(64, np.uint8)
    for args, what in (((0, buf.ctypes.data, 8, 4, 44100, buf.ctypes.data, size.ctypes.data), "bits 8"),
                       ((0, buf.ctypes.data, 16, 0, 44100, buf.ctypes.data, size.ctypes.data), "n = 0"),
                       ((0, buf.ctypes.data, 16, 1 << 36, 44100, buf.ctypes.data, size.ctypes.data), "n = 68719476736"),
                       ((0, buf.ctypes.data, 16, 4, 0, buf.ctypes.data, size.ctypes.data), "sample_rate 0"),
                       ((0, buf.ctypes.data, 16, 4, 655351, buf.ctypes.data, size.ctypes.data), "sample_rate 655351"),
                       ((0, None, 16, 4, 44100, buf.ctypes.data, size.ctypes.data), "null pcm")):
        assert L.dmx_flac_encode(*args) == 5, what
        assert "dmx_flac_encode" in L.dmx_last_error().decode() and what in L.dmx_last_error().decode(), L.dmx_last_error()


def test_a_real_recording_shrinks():
    from wavio import read_wav

    _, audio = read_wav(os.path.join(ROOT, "tests", "golden", "gspi_stereo.wav"))
    x = np.clip(np.rint(np.asarray(audio, np.float64).T * 32768.0), -32768, 32767).astype(np.int32)
    data, decisions = fs.encode(x, 16)
    y, bits, rate = fs.decode(data)
    assert bits == 16 and np.array_equal(x, y)
    print(f"gspi_stereo.wav, {x.shape[0]} frames at 16 bit: {len(data)} FLAC bytes for {x.shape[0] * 4} PCM bytes "
          f"(ratio {len(data) / (x.shape[0] * 4):.3f})")
    assert len(data) < x.shape[0] * 4
