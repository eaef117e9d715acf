"""Tracks at other sample rates on the multi-track path (dmx_tracks_infer_rates), the host arithmetic,
without a GPU: dmx_resample_ready against its closed form and against the oracle's resampler, the plan's native-rate ranges
through the stand-alone tests/track_rates_harness.cpp (built from csrc/tracks_plan.cpp alone), and the argument errors the two
entry points report before they need a device.

TRACK_RATES_HARNESS names another build of the harness (e.g. one compiled with -fsanitize=address,undefined)."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import resample_oracle as ro  # noqa: E402

import flac_in_spec as fis  # noqa: E402

RATES_OUT = [48000, 22050, 96000, 8000, 32000]
LENGTHS = [2, 37, 1000, 4801]
SEG = 8000
POOL = [0, 22049, 4033, 12436, 7, 6865, 5427, 21999, 1, 11025]


@pytest.fixture(scope="module")
def dmx():
    from demucs_cpp_amd import binding
    return binding


def ready(hi, n, rate_in, rate_out, m):
    """the closed form of the issue, in Python integers"""
    if hi == n:
        return m
    L, M = ro.ratio(rate_in, rate_out)
    c = 16 * max(L, M)
    return min(m, max(0, -(-(hi * L - c) // M)))


@pytest.mark.parametrize("rate", RATES_OUT)
def test_resample_ready_is_the_closed_form_and_safe_against_the_oracle(rate, dmx):
    rng = np.random.default_rng(rate)
    L, M = ro.ratio(44100, rate)
    c = 16 * max(L, M)
    for n in LENGTHS:
        m = ro.out_length(n, 44100, rate)
        x = rng.standard_normal((2, n))
        y = ro.resample(x, 44100, rate)
        for hi in sorted({0, 1, n // 3, n - 1, n}):
            K = dmx.resample_ready(hi, n, 44100, rate, m)
            assert K == ready(hi, n, 44100, rate, m), (n, hi)
            assert 0 <= K <= m
            x2 = x.copy()
            x2[:, hi:] = 1e6 * rng.standard_normal((2, n - hi))  # what is not final yet may still become anything
            y2 = ro.resample(x2, 44100, rate)
            assert np.array_equal(y[:, :K], y2[:, :K]), (n, hi)
            if K < m:  # K is the first output that reads input hi or later
                assert (c + K * M) // L >= hi, (n, hi)
                assert K == 0 or (c + (K - 1) * M) // L < hi, (n, hi)
    assert dmx.resample_ready(5, 4, 44100, rate, 9) == -1 and dmx.resample_ready(-1, 4, 44100, rate, 9) == -1
    assert dmx.resample_ready(1, 4, 0, rate, 9) == -1 and dmx.resample_ready(1, 4, 44100, rate, -1) == -1


def test_the_round_trip_is_never_shorter_than_the_track():
    """ceil(ceil(m 44100 / r) r / 44100) >= m: the cut to the first m frames always has them"""
    for rate in RATES_OUT + [11025, 44056, 192000, 768000, 1]:
        for m in list(range(1, 400)) + [4801, 10584000, 10584001]:
            assert ro.out_length(ro.out_length(m, rate, 44100), 44100, rate) >= m, (rate, m)


# ---- the plan
def _harness():
    exe = os.environ.get("TRACK_RATES_HARNESS")
    if exe:
        return exe
    exe = os.path.join(ROOT, "tests", "_build", "track_rates_harness")
    subprocess.check_call(["make", "-C", ROOT, "rates_harness"], stdout=subprocess.DEVNULL)
    return exe


def _plans(cases):
    text = "\n".join(" ".join(str(v) for v in c) for c in cases) + "\n"
    r = subprocess.run([_harness()], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def _cases():
    """the tracks of tests/test_gpu_track_rates.py (0.4, 1 and 3.3 segments after conversion, one at 44100) and a few more,
    over max_batch, bags, shifts, overlaps and both output kinds"""
    tracks = [(int(0.4 * SEG * 48000 / 44100), 48000), (SEG, 44100), (SEG // 2, 22050), (int(3.3 * SEG * 96000 / 44100), 96000),
              (3, 96000), (int(1.3 * SEG * 8000 / 44100), 8000), (int(2.1 * SEG * 32000 / 44100), 32000)]
    out = []
    for B in (1, 2, 5):
        for Q, N in ((1, 1), (1, 2), (2, 1), (4, 3)):
            for stride in (SEG, int(0.75 * SEG), SEG // 10):
                for pcm in (0, 1):
                    for sel in (tracks, tracks[::-1], tracks[:1], tracks[3:4]):
                        shifts = [POOL[(3 * t + 5 * q + k) % len(POOL)] for t in range(len(sel)) for q in range(Q) for k in range(N)]
                        out.append([SEG, stride, B, Q, N, pcm, len(sel)] + [m for m, _ in sel] + [r for _, r in sel] + shifts)
    return out


def test_native_ranges_tile_each_track_and_never_run_ahead_of_their_pieces(dmx):
    cases = _cases()
    for case, p in zip(cases, _plans(cases)):
        assert "error" not in p, (case, p)
        T = case[6]
        ms, rates = case[7:7 + T], case[7 + T:7 + 2 * T]
        assert p["mmax"] == max([m for m, r in zip(ms, rates) if r != 44100], default=0)
        done44, done = [0] * T, [0] * T
        for k, (pieces, native) in enumerate(zip(p["pieces"], p["native"])):
            for t, lo, hi in pieces:
                assert lo == done44[t] and hi >= lo
                done44[t] = hi
            for t, lo, hi in native:
                j = p["jobs"][t]
                assert rates[t] != 44100 and j["kFirst"] <= k <= j["kLast"]
                assert lo == done[t] and hi > lo, (case, k, t)  # in order, no overlap, no empty range
                done[t] = hi
                # every input the range reads is final after this batch: the newest tap of its last output
                L, M = ro.ratio(44100, rates[t])
                assert (16 * max(L, M) + (hi - 1) * M) // L < done44[t] or done44[t] == j["n"], (case, k, t)
                # and it is all that is: the closed form on what is final
                assert hi == ready(done44[t], j["n"], 44100, rates[t], ms[t]) == dmx.resample_ready(done44[t], j["n"], 44100, rates[t], ms[t])
        for t in range(T):
            assert p["jobs"][t]["n"] == (ms[t] if rates[t] == 44100 else ro.out_length(ms[t], rates[t], 44100)) == done44[t]
            assert done[t] == (ms[t] if rates[t] != 44100 else 0), (case, t)
        if case[5]:  # the PCM ranges: output frames, whole groups of 4 inside a track, within what is final
            donep, fin = [0] * T, [0] * T
            for k, pcm in enumerate(p["pcm"]):
                for t, lo, hi in p["pieces"][k]:
                    fin[t] = hi if rates[t] == 44100 else ready(hi, p["jobs"][t]["n"], 44100, rates[t], ms[t])
                for t, lo, hi in pcm:
                    assert lo == donep[t] and hi > lo and lo % 4 == 0 and (hi % 4 == 0 or hi == ms[t]) and hi <= fin[t]
                    donep[t] = hi
            assert donep == ms
        else:
            assert p["pcm"] == []


def test_a_call_at_44100_plans_what_it_planned_before():
    """rates of 44100 alone: no native ranges, and the pieces and PCM ranges of the plan without rates (the other harness)"""
    ns = [int(0.4 * SEG), SEG, int(3.3 * SEG)]
    shifts = [4033, 12436, 7]
    got = _plans([[SEG, 6000, 2, 1, 1, 1, 3] + ns + [44100] * 3 + shifts])[0]
    subprocess.check_call(["make", "-C", ROOT, "plan_harness"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "tests", "_build", "tracks_plan_harness")] + [str(v) for v in [SEG, 6000, 2, 1, 1, 1] + ns + shifts],
                       capture_output=True, text=True, timeout=60)
    want = json.loads(r.stdout)
    assert got["mmax"] == 0 and got["native"] == []
    assert got["pcm"] == want["pcm"]
    assert got["pieces"] == [[[pc["t"], pc["lo"], pc["hi"]] for pc in b] for b in want["pieces"]]


# ---- the entry points: what they refuse before they need a device
def _call_rates(dmx, n, rates, spec=None, flac_out=0, ctx=None):
    T = len(n)
    x = [np.zeros((2, max(v, 1)), np.float32) for v in n]
    ap = (ctypes.c_void_p * T)(*[a.ctypes.data for a in x])
    na = (ctypes.c_int64 * T)(*n)
    ra = (ctypes.c_int * T)(*rates) if rates is not None else None
    out = [np.full(64, 0x5A, np.uint8) for _ in n]
    op = (ctypes.c_void_p * T)(*[o.ctypes.data for o in out])
    sizes = np.full(T * 8, -3, np.int64)
    peaks = np.full(T * 8, -3, np.float32)
    rc = dmx.lib().dmx_tracks_infer_rates(ctx, None, 0, None, T, ap, na, ra, 1, 0.25, None, ctypes.byref(spec.c) if spec else None, flac_out, op,
                                          sizes.ctypes.data, peaks.ctypes.data, dmx.LAYOUT_PLANAR, None, None)
    assert all((o == 0x5A).all() for o in out) and (sizes == -3).all() and (peaks == -3).all()  # nothing is written on error
    return rc, dmx.lib().dmx_last_error().decode()


def test_rates_entry_point_names_the_track_it_refuses(dmx):
    spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_CLAMP)
    rc, msg = _call_rates(dmx, [100, 2], [44100, 768000])
    assert rc != 0 and "dmx_tracks_infer_rates: track 1: 2 frames at 768000 Hz leave 1 at 44100 Hz" in msg, msg
    rc, msg = _call_rates(dmx, [100, 100, 100], [48000, 44100, 768001])
    assert rc != 0 and "track 2: sample rate 768001" in msg and "768000" in msg, msg
    rc, msg = _call_rates(dmx, [100, 100], [0, 48000])
    assert rc != 0 and "track 0: sample rate 0" in msg, msg
    rc, msg = _call_rates(dmx, [100000, 100000], [48000, 11], spec)  # a decimation whose input window does not fit the kernel
    assert rc != 0 and "track 1: sample rate 11" in msg, msg
    rc, msg = _call_rates(dmx, [100, 100000], [48000, 700000], spec, flac_out=1)
    assert rc != 0 and "track 1: sample rate 700000" in msg and "655350" in msg, msg
    rc, msg = _call_rates(dmx, [100], None)
    assert rc != 0 and "null rates array" in msg, msg
    rc, msg = _call_rates(dmx, [100], [48000], None, flac_out=1)
    assert rc != 0 and "need a remix spec" in msg, msg
    # rates that pass: the next thing the call needs is its context
    rc, msg = _call_rates(dmx, [100, 100], [48000, 96000], spec)
    assert rc != 0 and "null context" in msg, msg
    rc, msg = _call_rates(dmx, [100, 100000], [48000, 700000], spec)  # PCM has no such limit
    assert rc != 0 and "null context" in msg, msg


def test_from_flac_rates_entry_point_reads_the_rates_from_the_files(dmx):
    rng = np.random.default_rng(5)
    x = fis._signal(rng, 64, 2, 16)

    def call(files, flac_out, any_rate=True):
        T = len(files)
        imgs = [np.frombuffer(f, np.uint8) for f in files]
        fp = (ctypes.c_void_p * T)(*[f.ctypes.data for f in imgs])
        fn = (ctypes.c_int64 * T)(*[f.size for f in imgs])
        spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_CLAMP)
        out = [np.full(64, 0x5A, np.uint8) for _ in files]
        op = (ctypes.c_void_p * T)(*[o.ctypes.data for o in out])
        status, sizes = np.full(2 * T, -9, np.int64), np.full(4 * T, -9, np.int64)
        f = dmx.lib().dmx_tracks_infer_from_flac_rates if any_rate else dmx.lib().dmx_tracks_infer_from_flac
        rc = f(None, None, 0, None, T, fp, fn, 1, 0.25, None, ctypes.byref(spec.c), flac_out, op, sizes.ctypes.data, None, status.ctypes.data,
               None, None)
        assert all((o == 0x5A).all() for o in out) and (status == -9).all() and (sizes == -9).all()  # nothing is written on error
        return rc, dmx.lib().dmx_last_error().decode()

    f44 = fis.write([fis.frame(x)], 2, 16)[0]
    f48 = fis.write([fis.frame(x)], 2, 16, rate=48000)[0]
    fhi = fis.write([fis.frame(x)], 2, 16, rate=655350)[0]
    rc, msg = call([f44, f48], 0, any_rate=False)
    assert rc != 0 and "track 1: sample rate 48000" in msg, msg  # the old entry point keeps refusing
    rc, msg = call([f44, f48], 0)
    assert rc != 0 and "dmx_tracks_infer_from_flac_rates: null context" in msg, msg  # the rates pass
    rc, msg = call([f44, f48, fhi], 1)
    assert rc != 0 and "null context" in msg, msg  # 655350 Hz still has a FLAC form
    rc, msg = call([f44, f48[:30]], 0)
    assert rc != 0 and "track 1" in msg, msg
    short = fis.write([fis.frame(x[:20])], 2, 16, rate=655350)[0]  # 20 frames at 655350 Hz: 2 at 44100 would need 15 or more
    rc, msg = call([f44, short], 0)
    assert (rc != 0 and "null context" in msg) if ro.out_length(20, 655350, 44100) >= 2 else "leave" in msg, msg
    tiny = fis.write([fis.frame(x[:8])], 2, 16, rate=655350)[0]
    rc, msg = call([f44, tiny], 0)
    assert rc != 0 and "track 1: 8 frames at 655350 Hz leave 1 at 44100 Hz" in msg, msg
