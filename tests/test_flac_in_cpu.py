"""The FLAC input stage without a GPU: the writer and the reference decoder of tests/flac_in_spec.py
against each other and against tests/flac_spec.py, the probe (a pure host function of the library), and the kernel text of
csrc/flac_in.hip run as host code by a stand-alone program (tests/flac_in_host_main.cpp), plain and under
-fsanitize=address,undefined, over the whole corpus: the matrix, every single-byte truncation of two small files, 500 seeded
single-bit flips and the 40 damaged files of the GPU tests."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import flac_in_spec as fis
import flac_spec as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _matrix():
    return fis.matrix()


def _stereo(x):
    return np.repeat(x, 2, axis=1) if x.shape[1] == 1 else x


def test_the_reference_decoder_returns_what_the_writer_was_given():
    m = _matrix()
    assert len(m) >= 55
    for name, (data, x, bits, channels, _) in m.items():
        r = fis.decode(data)
        assert (r["status"], r["good"]) == (fis.OK, x.shape[0]), name
        assert r["info"]["bits"] == bits and r["info"]["channels"] == channels, name
        assert np.array_equal(r["samples"], _stereo(x)), name


def test_the_two_specifications_read_each_other():
    m = _matrix()
    for name in ("fixed0", "fixed4", "bs192", "bs4096", "constant", "verbatim", "porder4", "depth16_ch2", "depth24_ch2"):
        data, x, bits, _, _ = m[name]
        pcm, b, rate = fs.decode(data)
        assert b == bits and rate == 44100 and np.array_equal(pcm, x), name
    for sig in ("sine_noise", "white_noise", "l_eq_minus_r", "jump_40db"):
        for bits in (16, 24):
            for n in (1, 4097):
                x = fs.crafted(sig, n, bits)
                r = fis.decode(fs.encode(x, bits)[0])
                assert (r["status"], r["good"]) == (fis.OK, n) and np.array_equal(r["samples"], x), (sig, bits, n)


def test_damaged_files_break_where_they_were_damaged():
    d = fis.damaged()
    assert len(d) == 40
    r = {k: fis.decode(v) for k, v in d.items()}
    for k in ("header_bit", "frame_removed"):
        assert (r[k]["status"], r[k]["good"]) == (fis.BROKEN, 2 * 192), k
    for k in ("crc8_byte", "illegal_partition_order", "partition_smaller_than_order", "reserved_type", "reserved_type_fixed5",
              "reserved_method", "frame_number_skips", "reserved_header_bit", "frame_says_24_bits", "frame_says_48_khz",
              "unary_to_end_of_frame", "frame_repeated"):
        assert (r[k]["status"], r[k]["good"]) == (fis.BROKEN, 3 * 192), k
    assert r["crc16_byte"]["good"] == 192 and r["residual_bit"]["good"] == 4 * 192 and r["first_frame"]["good"] == 0
    assert r["truncated_mid_frame"]["good"] == 5 * 192 == r["truncated_at_frame"]["good"]
    assert r["short_of_total"]["good"] == 6 * 192 + 50 and r["short_of_total"]["status"] == fis.BROKEN
    assert r["overshoots_total"]["good"] == 6 * 192 and r["unary_to_end_of_file"]["good"] == 6 * 192
    assert r["order_above_block_size"]["good"] == 6 * 192 == r["order_equal_block_size"]["good"]
    assert r["garbage_between_frames"]["good"] == 4 * 192
    # frame 3's first subframe is LPC: the LPC-only fields are what broke it
    assert r["negative_shift"]["good"] == 3 * 192 == r["reserved_precision"]["good"]
    assert all(v["status"] == fis.BROKEN for v in r.values())


PROBE_FAILURES = [
    ("short", lambda d, L: d[:3], "shorter than any FLAC file"),
    ("ogg", lambda d, L: b"OggS" + d, "Ogg FLAC is not supported"),
    ("marker", lambda d, L: b"fLaX" + d[4:], "no fLaC marker"),
    ("id3_size", lambda d, L: b"ID3\x04\x00\x00\x00\x00\x80\x00" + d, "ID3v2 tag with a malformed size"),
    ("id3_past", lambda d, L: b"ID3\x04\x00\x00\x00\x00\x7f\x7f" + d, "ID3v2 tag runs past the end"),
    ("meta_past", lambda d, L: d[:30], "runs past the end of the file"),
    ("not_streaminfo", lambda d, L: d[:4] + b"\x81" + d[5:], "first metadata block is not a STREAMINFO"),
    ("type127", lambda d, L: d[:4] + b"\x00" + d[5:42] + b"\xff\x00\x00\x00" + d[42:], "type 127 is invalid"),
    ("second_streaminfo", lambda d, L: d[:4] + b"\x00" + d[5:42] + b"\x80\x00\x00\x00" + d[42:], "second STREAMINFO"),
    ("channels", lambda d, L: _si(d, channels=3), "3 channels (1 or 2 are supported)"),
    ("bits32", lambda d, L: _si(d, bits=32), "32-bit samples are not supported"),
    ("bits17", lambda d, L: _si(d, bits=17), "17 bits per sample"),
    ("rate0", lambda d, L: _si(d, rate=0), "sample rate 0"),
    ("unknown_length", lambda d, L: _si(d, total=0), "unknown length"),
    ("too_long", lambda d, L: _si(d, total=1 << 31), "2^31 samples and more"),
    ("block_range", lambda d, L: _si(d, min_block=15), "block size range"),
    ("no_frame", lambda d, L: d[:L["first"]], "no audio frame after the metadata"),
    ("no_sync", lambda d, L: d[:L["first"]] + b"\x00" + d[L["first"] + 1:], "no frame sync code"),
]


def _si(d, **kw):
    si = int.from_bytes(d[8:26], "big")
    f = dict(min_block=si >> 128, max_block=(si >> 112) & 0xFFFF, frames=(si >> 64) & ((1 << 48) - 1), rate=(si >> 44) & 0xFFFFF,
             channels=((si >> 41) & 7) + 1, bits=((si >> 36) & 31) + 1, total=si & ((1 << 36) - 1))
    f.update(kw)
    si = (f["min_block"] << 128) | (f["max_block"] << 112) | (f["frames"] << 64) | (f["rate"] << 44) | ((f["channels"] - 1) << 41) | \
        ((f["bits"] - 1) << 36) | f["total"]
    return d[:8] + si.to_bytes(18, "big") + d[26:]


def test_probe_fields_and_one_message_per_failure():
    from demucs_cpp_amd import binding as dmx

    m = _matrix()
    for name, (data, x, bits, channels, lay) in m.items():
        i, want = dmx.flac_probe(data), fis.probe(data)
        assert (i.sample_rate, i.channels, i.bits, i.total_samples, i.min_block, i.max_block, i.variable_blocking, i.first_frame) == \
            (want["rate"], channels, bits, x.shape[0], want["min_block"], want["max_block"], want["variable"], lay["first"]), name
        sizes = [b - a for a, b in lay["frames"]]
        assert (i.min_frame, i.max_frame) == (min(sizes), max(sizes)), name
        assert dmx.lib().dmx_flac_decode_workspace_bytes(dmx.ctypes.byref(i), len(data)) >= 8 * x.shape[0], name
    data, _, _, _, lay = m["fixed2"]
    seen = set()
    for name, mutate, text in PROBE_FAILURES:
        bad = mutate(data, lay)
        with pytest.raises(fis.ProbeError):
            fis.probe(bad)
        with pytest.raises(dmx.DmxError) as e:
            dmx.flac_probe(bad)
        assert text in str(e.value) and "dmx_flac_probe" in str(e.value), (name, str(e.value))
        seen.add(str(e.value))
    assert len(seen) == len(PROBE_FAILURES)
    hdr = open(os.path.join(ROOT, "include", "demucs_hip.h")).read()
    for sym in ("dmx_flac_probe", "dmx_flac_decode_workspace_bytes", "dmx_flac_decode_device", "dmx_flac_decode"):
        assert sym in dmx.EXPORTS and hasattr(dmx.lib(), sym) and re.search(r"\b%s\(" % sym, hdr), sym


def test_decode_checks_its_arguments_before_any_gpu_work():
    from demucs_cpp_amd import binding as dmx

    m = _matrix()
    for name, enc, text in (("depth16_ch1", dmx.PCM_S16, "needs a stereo stream"), ("depth24_ch2", dmx.PCM_S16, "exactly that depth"),
                            ("depth16_ch2", dmx.PCM_S24, "exactly that depth"), ("depth16_ch2", 7, "encoding 7")):
        with pytest.raises(dmx.DmxError) as e:
            dmx.flac_decode(m[name][0], enc)
        assert text in str(e.value), str(e.value)


def _corpus():
    """(name, file bytes, encoding) of every job of the stand-alone program"""
    jobs = [(k, v[0], 0) for k, v in _matrix().items()]
    jobs += [("s16_" + k, _matrix()[k][0], 1) for k in ("bs17", "variable", "fixed3", "n1")]
    jobs += [("s24_" + k, _matrix()[k][0], 2) for k in ("depth24_ch2", "assign_full_range", "escape_25")]
    a, b = fis.small_files()
    jobs += [(f"trunc_a_{n}", a[:n], 0) for n in range(len(a))] + [(f"trunc_b_{n}", b[:n], 0) for n in range(len(b))]
    jobs += [(f"flip_{i}", d, 0) for i, d in enumerate(fis.bit_flips())]
    jobs += [("damaged_" + k, v, 0) for k, v in fis.damaged().items()]
    return jobs


def _run_corpus(program, tmp_path):
    jobs = _corpus()
    assert len(jobs) > 500 + 40 + 55
    lines = []
    for i, (name, data, enc) in enumerate(jobs):
        (tmp_path / f"{i}.flac").write_bytes(data)
        lines.append(f"{enc} {tmp_path / f'{i}.flac'} {tmp_path / f'{i}.out'}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([program, str(tmp_path / "list.txt")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"{len(jobs)} jobs"
    refused = broken = 0
    for i, (name, data, enc) in enumerate(jobs):
        raw = (tmp_path / f"{i}.out").read_bytes()
        head = np.frombuffer(raw[:32], np.int64)
        try:
            ref = fis.decode(data)
        except fis.ProbeError:
            assert head[0] == 1, name
            refused += 1
            continue
        n = ref["info"]["total"]
        assert tuple(head) == (0, ref["status"], ref["good"], n), (name, tuple(head), ref["status"], ref["good"])
        broken += ref["status"] != fis.OK
        assert np.all(ref["samples"][ref["good"]:] == 0)
        if enc == 0:
            got = np.frombuffer(raw[32:], np.float32).reshape(n, 2)
            assert np.array_equal(got, fis.as_f32(ref["samples"], ref["info"]["bits"])), name
        else:
            got = fs.pcm_ints(np.frombuffer(raw[32:], np.uint8), 16 if enc == 1 else 24)
            assert np.array_equal(got, ref["samples"]), name
    assert refused > 50 and broken > 500  # the corpus does hold both kinds


def test_too_many_header_look_alikes_are_a_status_not_a_fault(tmp_path):
    data = fis.too_many_candidates()
    ref = fis.decode(data)
    assert (ref["status"], ref["good"]) == (fis.OK, 4096)  # the stream itself is valid
    (tmp_path / "a.flac").write_bytes(data)
    (tmp_path / "list.txt").write_text(f"0 {tmp_path / 'a.flac'} {tmp_path / 'a.out'}\n")
    subprocess.check_call(["make", "-C", ROOT, "flac_in_host_asan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "tests", "_build", "flac_in_host_main_asan"), str(tmp_path / "list.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = (tmp_path / "a.out").read_bytes()
    assert tuple(np.frombuffer(raw[:32], np.int64)) == (0, fis.TOO_MANY_CANDIDATES, 0, 4096)
    assert not np.frombuffer(raw[32:], np.float32).any()


def test_kernel_text_as_host_code_equals_the_reference(tmp_path):
    _run_corpus(os.path.join(ROOT, "tests", "_build", "flac_in_host_main"), tmp_path)


def test_kernel_text_as_host_code_under_address_and_undefined_sanitizers(tmp_path):
    out = os.path.join(ROOT, "tests", "_build", "flac_in_host_main_asan")
    subprocess.check_call(["make", "-C", ROOT, "flac_in_host_asan"], stdout=subprocess.DEVNULL)
    _run_corpus(out, tmp_path)
