"""The FLAC output stage's compression levels without a GPU: the specification tests/flac_lpc_spec.py (level 0 is
tests/flac_spec.py; levels 1 and 2 add LPC candidates of order 8 / 8 and 12) against the independent LPC-capable reference
decoder of tests/flac_in_spec.py, the kernel text of csrc/flac.hip compiled as host code (make flac_host flac_host_asan:
plain and under AddressSanitizer + UBSan) against the specification's bytes, and the pure-host argument checks of the new
entry points (include/demucs_hip.h dmx_flac_encode_level, dmx_ctx_set_flac_level)."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import flac_in_spec as fis
import flac_lpc_spec as ls
import flac_spec as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _encoded(name, n, bits, level, rate=44100):
    x = ls.crafted(name, n, bits)
    data, decisions = ls.encode(x, bits, rate, level)
    return x, data, decisions


# ---- level 0 is the encoder of flac_spec
@pytest.mark.parametrize("bits", [16, 24])
def test_level_0_is_flac_spec(bits):
    for name in ls.SIGNALS:
        for n in ls.LENGTHS:
            x = ls.crafted(name, n, bits)
            if name in fs.SIGNALS:
                assert np.array_equal(x, fs.crafted(name, n, bits))
            assert x.shape == (n, 2) and x.min() >= -(1 << (bits - 1)) and x.max() < 1 << (bits - 1)
            assert _encoded(name, n, bits, 0)[1] == fs.encode(x, bits)[0], (name, n, bits)


# ---- round trip through the independent decoder that knows LPC
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("name", ls.SIGNALS)
def test_round_trip_through_the_reference_decoder(name, bits):
    for n in ls.LENGTHS:
        sizes = {}
        for level in LEVELS:
            x, data, decisions = _encoded(name, n, bits, level)
            sizes[level] = ls.frame_sizes(data)
            assert len(sizes[level]) == len(decisions) == (n + 4095) // 4096 and sum(sizes[level]) + 42 == len(data)
            assert len(data) <= fs.bound(bits, n), (name, n, bits, level)
            if level == 0:
                continue
            ref = fis.decode(data)
            assert ref["status"] == fis.OK and ref["good"] == n, (name, n, bits, level)
            assert np.array_equal(ref["samples"], x), (name, n, bits, level)
            info = fis.probe(data)
            assert (info["bits"], info["rate"], info["total"], info["min_block"], info["max_block"]) == (bits, 44100, n, 4096, 4096)
        # frame by frame, a level never costs a byte
        assert all(c <= b <= a for a, b, c in zip(sizes[0], sizes[1], sizes[2])), (name, n, bits)


def test_the_crafted_inputs_cover_every_decision():
    lpc_orders, lpc_channels, shifts = set(), set(), set()
    fixed_over_both = short_block = big_k = False
    chosen = {}
    for bits in (16, 24):
        for name in ls.SIGNALS:
            for n in ls.LENGTHS:
                for level in (1, 2):
                    for f, d in enumerate(_encoded(name, n, bits, level)[2]):
                        bs = min(4096, n - 4096 * f)
                        for s, valid in zip(d["sub"], d["lpc_valid"]):
                            if bs <= 32:
                                short_block = True
                                assert s["type"] != "LPC" and valid == ()
                            if s["type"] == "LPC":
                                assert s["order"] in ls.ORDERS[level] and s["order"] in valid
                                assert len(s["q"]) == s["order"] and 0 <= s["shift"] <= 15
                                lim = 1 << ((12 if bits == 16 else 15) - 1)
                                assert all(-lim <= q < lim for q in s["q"])
                                assert len(s["k"]) == 1 << s["p"] and max(s["k"]) <= (14 if bits == 16 else 30)
                                assert (bs >> s["p"]) > s["order"]
                                lpc_orders.add(s["order"])
                                lpc_channels.add(d["channels"])
                                shifts.add(s["shift"])
                                big_k = big_k or (bits == 24 and max(s["k"]) > 14)
                                if n == 3 * 4096 + 123:
                                    chosen.setdefault(name, set()).add(s["order"])
                            elif s["type"] == "FIXED" and level == 2 and valid == (8, 12):
                                fixed_over_both = True
    assert lpc_orders == {8, 12}
    assert fixed_over_both and short_block and big_k
    assert lpc_channels == {0b0001, 0b1000, 0b1001, 0b1010}
    assert len(shifts) >= 2, shifts
    # what the signals were made for
    assert chosen["sine_noise"] == {8, 12} and 8 in chosen["alternating"] and 8 in chosen["ar2_resonance"] and 12 in chosen["quiet_tone"]
    assert not {"ramp", "loud_quiet", "jump_40db"} & set(chosen)


def test_the_residual_range_guard():
    # no crafted signal reaches the discard (the specification's docstring says what was tried): the largest residual of a
    # candidate of the likeliest one, full-scale alternation at the block edges at 24 bits, stays far inside the range ...
    worst = 0
    for n in (4096, 3 * 4096 + 123):
        x = ls.crafted("edge_burst", n, 24).astype(np.int64)
        for f in range((n + 4095) // 4096):
            blk = x[f * 4096:(f + 1) * 4096]
            for sig in (blk[:, 0], blk[:, 1], (blk[:, 0] + blk[:, 1]) >> 1, blk[:, 0] - blk[:, 1]):
                if sig.size <= 32:
                    continue
                R = ls.autocorrelation(sig)
                for m, a in ls.levinson(R, (8, 12)).items() if R[0] else ():
                    qs = ls.quantise(a, 24)
                    if qs is not None:
                        worst = max(worst, int(np.abs(ls.lpc_residual(sig, *qs)).max()))
    print(f"largest |residual| of an LPC candidate on edge_burst at 24 bits: {worst} = 2^{np.log2(max(worst, 1)):.2f} (the guard: 2^29)")
    assert 0 < worst < ls.RES_LIM
    # ... so the candidate function is called with hand-made coefficients that overflow it
    full = 1 << 23
    sig = np.where(np.arange(256) % 2 == 0, -full, full - 1).astype(np.int64) * 2 - np.where(np.arange(256) % 2 == 0, 0, 1)  # side: +-2^24
    sig = np.clip(sig, -(1 << 24), (1 << 24) - 1)
    q_bad = [16383, -16384] * 4  # the predictor doubles an alternating signal 8 times over at shift 0
    r = ls.lpc_residual(sig, q_bad, 0)
    assert r.max() >= ls.RES_LIM or r.min() < -ls.RES_LIM
    assert ls.lpc_candidate(sig, 25, 24, q_bad, 0) is None
    # the edges of the range: -2^29 is inside, 2^29 is not
    for value, inside in ((-(1 << 29), True), ((1 << 29) - 1, True), (1 << 29, False), (-(1 << 29) - 1, False)):
        sig = np.zeros(64, np.int64)
        sig[8] = -(1 << 15) if value < 0 else 1 << 15  # the prediction of sample 9 is -16384 * sig[8] = +-2^29
        sig[9] = value + (1 << 29) if value < 0 else value - (1 << 29)
        q = [-16384, 0, 0, 0, 0, 0, 0, 0]
        r = ls.lpc_residual(sig, q, 0)
        assert r[1] == value and np.abs(np.delete(r, 1)).max() <= 1 << 15, (value, r[:3])
        assert (ls.lpc_candidate(sig, 25, 24, q, 0) is not None) == inside, value
    good = ls.lpc_candidate(np.arange(64, dtype=np.int64) * 3, 24, 24, [2, -1, 0, 0, 0, 0, 0, 0], 0)
    assert good is not None and good[1]["order"] == 8 and good[0] == 8 + 8 * 24 + 4 + 5 + 8 * 15 + 6 + 5 + 56 * 1


# ---- the recording
def _recording(bits):
    from wavio import read_wav

    _, audio = read_wav(os.path.join(ROOT, "tests", "golden", "gspi_stereo.wav"))
    full = float(1 << (bits - 1))
    return np.clip(np.rint(np.asarray(audio, np.float64).T * full), -full, full - 1).astype(np.int32)


@pytest.mark.parametrize("bits,cap1,cap2", [(16, 0.85, 0.80), (24, 0.92, 0.90)])
def test_a_real_recording_shrinks_with_the_level(bits, cap1, cap2):
    x = _recording(bits)
    size = {}
    for level in LEVELS:
        data, _ = ls.encode(x, bits, 44100, level)
        ref = fis.decode(data)
        assert ref["status"] == fis.OK and np.array_equal(ref["samples"], x)
        size[level] = len(data)
    pcm = x.shape[0] * 2 * bits // 8
    print(f"gspi_stereo.wav, {x.shape[0]} frames at {bits} bit, {pcm} PCM bytes: "
          + ", ".join(f"level {lv} {size[lv]} bytes ({size[lv] / pcm:.4f} of the PCM, {size[lv] / size[0]:.4f} of level 0)" for lv in LEVELS))
    assert size[1] <= cap1 * size[0] and size[2] <= cap2 * size[0]
    assert size[2] <= size[1] <= size[0]


# ---- the kernel text as host code
def _host_jobs():
    """(key, bits, level, rate, x, want)"""
    jobs = []
    for bits in (16, 24):
        for name in ls.SIGNALS:
            for n in ls.LENGTHS:
                for level in LEVELS:
                    x, data, _ = _encoded(name, n, bits, level)
                    jobs.append((f"{name}_{n}_{bits}", bits, level, 44100, x, data))
    x = ls.crafted("sine_noise", 3 * 4096 + 123, 24)  # the 48 kHz case of tests/test_gpu_flac.py
    jobs += [("sine48k", 24, level, 48000, x, ls.encode(x, 24, 48000, level)[0]) for level in LEVELS]
    zeros = np.zeros((2049 * 4096 + 7, 2), np.int32)  # its 2050 frames: frame numbers up to the three-byte form
    want = fs.encode(zeros, 16)[0]
    assert ls.encode(zeros[:3 * 4096 + 7], 16, 44100, 2)[0] == fs.encode(zeros[:3 * 4096 + 7], 16)[0]  # CONSTANT at every level
    jobs += [("frames2050", 16, level, 44100, zeros, want) for level in LEVELS]
    return jobs


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))
    return f"lengths {len(a)} / {len(b)}, first differing byte {int(d[0]) if d.size else m}"


def _run_host(program, tmp_path):
    jobs = _host_jobs()
    lines, written = [], set()
    for i, (key, bits, level, rate, x, want) in enumerate(jobs):
        if key not in written:
            fs.pcm_bytes(x, bits).tofile(str(tmp_path / f"{key}.pcm"))
            written.add(key)
        lines.append(f"{bits} {level} {rate} {tmp_path / f'{key}.pcm'} {tmp_path / f'{i}.flac'}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([program, str(tmp_path / "list.txt")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"{len(jobs)} jobs"
    for i, (key, bits, level, rate, x, want) in enumerate(jobs):
        got = (tmp_path / f"{i}.flac").read_bytes()
        assert got == want, (key, level, rate, _first_difference(got, want))


def test_kernel_text_as_host_code_equals_the_specification(tmp_path):
    subprocess.check_call(["make", "-C", ROOT, "flac_host"], stdout=subprocess.DEVNULL)
    _run_host(os.path.join(ROOT, "tests", "_build", "flac_host_main"), tmp_path)


def test_kernel_text_as_host_code_under_address_and_undefined_sanitizers(tmp_path):
    subprocess.check_call(["make", "-C", ROOT, "flac_host_asan"], stdout=subprocess.DEVNULL)
    _run_host(os.path.join(ROOT, "tests", "_build", "flac_host_main_asan"), tmp_path)


# ---- the host entry points
def test_host_entry_points_reject_bad_levels_and_are_declared():
    from demucs_cpp_amd import binding as dmx

    L = dmx.lib()
    hdr = open(os.path.join(ROOT, "include", "demucs_hip.h")).read()
    for sym in ("dmx_flac_encode_device_level", "dmx_flac_encode_level", "dmx_flac_encode_device_timed", "dmx_ctx_set_flac_level",
                "dmx_ctx_flac_level"):
        assert sym in dmx.EXPORTS and hasattr(L, sym) and re.search(r"\b%s\(" % sym, hdr), sym
    size = np.full(1, -5, np.int64)
    buf = np.full(64, 0xA5, np.uint8)
    for level in (-1, 3):  # before any GPU work: these run on a machine without one
        assert L.dmx_flac_encode_level(0, buf.ctypes.data, 16, 4, 44100, level, buf.ctypes.data, size.ctypes.data) == 5
        msg = L.dmx_last_error().decode()
        assert "dmx_flac_encode_level" in msg and f"level {level}" in msg, msg
        assert L.dmx_flac_encode_device_level(0, buf.ctypes.data, 16, 4, 44100, level, buf.ctypes.data, size.ctypes.data, buf.ctypes.data,
                                              None) == 5
        msg = L.dmx_last_error().decode()
        assert "dmx_flac_encode_device_level" in msg and f"level {level}" in msg, msg
        with pytest.raises(dmx.DmxError, match=f"level {level}"):
            dmx.flac_encode(np.zeros((4, 2), np.int16), 16, level=level)
    assert size[0] == -5 and (buf == 0xA5).all()
    # the older checks hold in front of the level's
    assert L.dmx_flac_encode_level(0, buf.ctypes.data, 8, 4, 44100, 1, buf.ctypes.data, size.ctypes.data) == 5
    assert "dmx_flac_encode_level" in L.dmx_last_error().decode() and "bits 8" in L.dmx_last_error().decode()
    # the setter: its own message, whatever the handle is (a null context has its own)
    assert L.dmx_ctx_set_flac_level(None, 1) == 5 and "dmx_ctx_set_flac_level" in L.dmx_last_error().decode()
    assert L.dmx_ctx_flac_level(None) == -1
    dummy = ctypes.create_string_buffer(1 << 16)  # never dereferenced: the level is checked first
    for level in (-1, 3):
        assert L.dmx_ctx_set_flac_level(ctypes.addressof(dummy), level) == 5
        msg = L.dmx_last_error().decode()
        assert "dmx_ctx_set_flac_level" in msg and f"level {level}" in msg, msg
