"""Tracks at their own sample rates (dmx_tracks_infer_rates through Context.tracks_rates): a 4-minute
48 kHz track, host buffers in, 16-bit PCM stems out, in ONE process. Prints one JSON line.

  (a) rates      Context.tracks_rates: both conversions inside the track slot on the device
  (b) composed   what (a) replaces, through the public calls: resample 48000 -> 44100, Context.tracks_opts, resample of the
                 stems 44100 -> 48000 cut to the track's frames, pcm_encode. Two more uploads and downloads of fp32 stems.
Both compute the same bytes (asserted on the first call). One warm-up call of each, then --reps repetitions in which the two
alternate (in forward and backward order by turns); median and spread (max - min) of each side.
  converter_ms   the converter's arithmetic alone on device memory between HIP events, in its whole-signal form
                 (dmx_resample_device, the same workgroup body as the piece-table kernel): the stems 44100 -> 48000 (8 planes)
                 and the track 48000 -> 44100 (interleaved stereo); median of --reps after a warm-up.
The track is tests/golden/gspi_stereo.wav tiled, declared as 48 kHz; synthetic weights, seed 0; shift offset 4033.

    python tools/rates_bench.py [--reps 5] [--batch 42] [--seconds 240] [--gemm bf16x3]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE = 48000
SHIFT = 4033


def recording(n):
    with wave.open(os.path.join(ROOT, "tests", "golden", "gspi_stereo.wav")) as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2)
    pcm = np.tile(pcm, ((n + pcm.shape[0] - 1) // pcm.shape[0], 1))[:n]
    return np.ascontiguousarray((pcm.astype(np.float32) / np.float32(32768.0)).T)


def converter_ms(dmx, n44, m, reps):
    import torch

    L = dmx.lib()
    stems = torch.rand((8, n44), dtype=torch.float32, device="cuda")
    up = torch.empty((8, dmx.resample_length(n44, 44100, RATE)), dtype=torch.float32, device="cuda")
    track = torch.rand((m, 2), dtype=torch.float32, device="cuda")
    down = torch.empty((dmx.resample_length(m, RATE, 44100), 2), dtype=torch.float32, device="cuda")
    i64, vp, ci = __import__("ctypes").c_int64, __import__("ctypes").c_void_p, __import__("ctypes").c_int
    L.dmx_resample_device.argtypes = [ci, vp, i64, ci, i64, i64, ci, ci, vp, i64, i64, vp]
    out = {}
    for name, call in (("stems_44100_to_48000", lambda: L.dmx_resample_device(0, stems.data_ptr(), n44, 8, n44, 1, 44100, RATE, up.data_ptr(),
                                                                               up.shape[1], 1, None)),
                       ("track_48000_to_44100", lambda: L.dmx_resample_device(0, track.data_ptr(), m, 2, 1, 2, RATE, 44100, down.data_ptr(), 1, 2,
                                                                               None))):
        ms = []
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(torch.cuda.default_stream())
            dmx._chk(call())
            e1.record(torch.cuda.default_stream())
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[name] = round(float(np.median(ms[1:])), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=int, default=240)
    a = ap.parse_args()
    from demucs_cpp_amd import binding as dmx
    from demucs_cpp_amd.weights import write_synthetic_model

    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    m = a.seconds * RATE
    x = recording(m)
    res = {"tool": "rates_bench", "model": "4s", "gemm": a.gemm, "max_batch": a.batch, "reps": a.reps, "rate": RATE, "track_frames": m}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ggml-model-htdemucs-4s-f16.bin")
        write_synthetic_model(path, 4, 0)
        model = dmx.Model(path, 0)
        ctx = dmx.Context(model, 0, a.batch, gemm)
        spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_RESCALE)
        ospec = dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE)

        def rates():
            return ctx.tracks_rates([x], [RATE], spec, shift_offsets=[[SHIFT]])[0][0]

        def composed():
            x44 = dmx.resample(x, RATE, 44100)
            v44 = ctx.tracks_opts([x44], shift_offsets=[[SHIFT]])[0]
            v = dmx.resample(v44.reshape(8, -1), 44100, RATE)[:, :m]
            return dmx.pcm_encode(np.ascontiguousarray(v).reshape(4, 2, m), ospec)[0]

        got, want = rates(), composed()  # the warm-up calls: slots, staging buffers, plans, filters
        res["same_bytes"] = bool(all(np.array_equal(p, q) for p, q in zip(got, want)))
        assert res["same_bytes"]
        del got, want
        walls = {"rates": [], "composed": []}
        legs = [("rates", rates), ("composed", composed)]
        for rep in range(a.reps):
            for name, call in (legs if rep % 2 == 0 else legs[::-1]):
                t0 = time.perf_counter()
                call()
                walls[name].append(time.perf_counter() - t0)
        for k, w in walls.items():
            res[k + "_wall_s"] = [round(v, 4) for v in w]
            res[k + "_median_s"] = round(float(np.median(w)), 4)
            res[k + "_spread_s"] = round(max(w) - min(w), 4)
        res["converter_ms"] = converter_ms(dmx, dmx.resample_length(m, RATE, 44100), m, a.reps)
        ctx.close()
        model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
