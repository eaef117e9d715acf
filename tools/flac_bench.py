"""The FLAC output stage (dmx_tracks_infer_flac through Context.tracks_flac; csrc/flac.hip): what it costs, and saves, to let
a track leave the GPU as lossless .flac files instead of 16-bit WAV data or fp32 planes. Prints one JSON line.

Workload of tools/pcm_bench.py: one 4-minute track (10 584 000 samples, shift offset 4033), synthetic weights (seed 0),
0.1 N(0,1) audio, host (numpy) buffers in and out. Measured, each after one warm-up call, --reps times, ALTERNATING the
variants inside every repetition so that drift of the shared host hits all of them alike:
  track      Context.track                                      (fp32 planes out: the yardstick)
  pcm_all    Context.tracks_remix, S16 / rescale / identity     (16-bit PCM stems out)
  flac_all   Context.tracks_flac,  S16 / rescale / identity     (16-bit FLAC stems out)
The record holds every wall time, the medians, the yardstick's own spread (max - min over its repetitions: a difference
inside that spread is not a difference) and the bytes that left the device. The stems of synthetic weights on noise are
noise: they barely compress, so this is the stage's WORST case for bytes saved.
--stage times the stage alone on device memory with HIP events (dmx_flac_encode_device) on tests/golden/gspi_stereo.wav
repeated to FRAMES frames, at 16 and 24 bits, beside a pinned device-to-host copy of the PCM bytes it replaces and of the
FLAC bytes it leaves, and records the compression ratio of the recording itself:

    python tools/flac_bench.py [--model 4s] [--gemm bf16x3] [--batch 42] [--reps 5]
    python tools/flac_bench.py --stage 10584000
    rocprofv3 --kernel-trace --stats -d DIR -o flac -- python tools/flac_bench.py --only flac_all
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from demucs_cpp_amd import binding as dmx  # noqa: E402
from demucs_cpp_amd.weights import write_synthetic_model  # noqa: E402

SR = 44100
N_TRACK = 240 * SR
SHIFT = 4033


def _recording(bits):
    """tests/golden/gspi_stereo.wav quantised to `bits`: int32 (n, 2)"""
    from wavio import read_wav

    _, audio = read_wav(os.path.join(ROOT, "tests", "golden", "gspi_stereo.wav"))
    full = float(1 << (bits - 1))
    return np.clip(np.rint(np.asarray(audio, np.float64).T * full), -full, full - 1).astype(np.int32)


def _pcm_bytes(x, bits):
    if bits == 16:
        return x.astype("<i2").view(np.uint8).ravel()
    q = x.astype(np.int64) & 0xFFFFFF
    return np.stack([(q >> (8 * b)).astype(np.uint8) for b in range(3)], axis=-1).ravel()


def stage_alone(n, reps):
    import torch

    L = dmx.lib()
    out = {}
    for bits in (16, 24):
        x = _recording(bits)
        own = dmx.flac_encode(_pcm_bytes(x, bits).view("<i2").reshape(-1, 2) if bits == 16 else _pcm_bytes(x, bits).reshape(-1, 2, 3), bits)
        tiled = np.tile(x, ((n + x.shape[0] - 1) // x.shape[0], 1))[:n]
        raw = _pcm_bytes(tiled, bits)
        d_pcm = torch.from_numpy(raw.copy()).cuda()
        d_out = torch.zeros(dmx.flac_bound(bits, n), dtype=torch.uint8, device="cuda")
        d_size = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_work = torch.zeros(L.dmx_flac_workspace_bytes(bits, n), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream

        def call():
            dmx._chk(L.dmx_flac_encode_device(0, d_pcm.data_ptr(), bits, n, SR, d_out.data_ptr(), d_size.data_ptr(), d_work.data_ptr(), s))

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            return [round(v, 4) for v in ms]

        ms = timed(call)
        size = int(d_size.item())
        h_pcm = torch.empty(raw.size, dtype=torch.uint8).pin_memory()
        h_flac = torch.empty(size, dtype=torch.uint8).pin_memory()
        ms_pcm = timed(lambda: h_pcm.copy_(d_pcm, non_blocking=True))
        ms_flac = timed(lambda: h_flac.copy_(d_out[:size], non_blocking=True))
        out[f"s{bits}"] = {"frames": n, "pcm_bytes": int(raw.size), "flac_bytes": size, "ratio": round(size / raw.size, 4),
                           "encode_ms": ms, "encode_median_ms": round(float(np.median(ms)), 4),
                           "d2h_pcm_ms": ms_pcm, "d2h_pcm_median_ms": round(float(np.median(ms_pcm)), 4),
                           "d2h_flac_ms": ms_flac, "d2h_flac_median_ms": round(float(np.median(ms_flac)), 4),
                           "recording_frames": int(x.shape[0]), "recording_flac_bytes": len(own),
                           "recording_ratio": round(len(own) / (x.shape[0] * 2 * bits // 8), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="4s", choices=["4s", "6s"])
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["track", "pcm_all", "flac_all"])
    ap.add_argument("--stage", type=int, default=0, metavar="FRAMES")
    a = ap.parse_args()
    S = 4 if a.model == "4s" else 6
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    res = {"tool": "flac_bench", "model": a.model, "gemm": a.gemm, "max_batch": a.batch, "reps": a.reps, "track_samples": N_TRACK}
    if a.stage:
        res["stage"] = stage_alone(a.stage, max(a.reps, 5))
        print(json.dumps(res))
        return
    rng = np.random.default_rng(1)
    audio = (0.1 * rng.standard_normal((2, N_TRACK))).astype(np.float32)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"ggml-model-htdemucs-{a.model}-f16.bin")
        write_synthetic_model(path, S, 0)
        model = dmx.Model(path, 0)
        ctx = dmx.Context(model, 0, a.batch, gemm)
        out = np.zeros((S, 2, N_TRACK), np.float32)
        spec = dmx.RemixSpec(np.eye(S, S + 1, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_RESCALE)
        buf_pcm = [np.zeros(S * N_TRACK * 4, np.uint8)]  # reused, like `out`
        buf_flac = [np.zeros(S * dmx.flac_bound(16, N_TRACK), np.uint8)]
        sizes = np.zeros(S, np.int64)
        variants = {
            "track": lambda: ctx.track(audio, SHIFT, out=out),
            "pcm_all": lambda: ctx.tracks_remix([audio], spec, shift_offsets=[[SHIFT]], out=buf_pcm),
            "flac_all": lambda: ctx.tracks_flac([audio], spec, shift_offsets=[[SHIFT]], out=buf_flac, sizes=sizes),
        }
        if a.only:
            variants[a.only]()
            t0 = time.perf_counter()
            variants[a.only]()
            res.update({"only": a.only, "wall_s": round(time.perf_counter() - t0, 4)})
        else:
            for fn in variants.values():
                fn()  # warm-up: slots, staging buffers, plans
            walls = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():
                    t0 = time.perf_counter()
                    fn()
                    walls[k].append(time.perf_counter() - t0)
            for k, w in walls.items():
                res[k + "_wall_s"] = [round(x, 4) for x in w]
                res[k + "_median_s"] = round(float(np.median(w)), 4)
            res["track_spread_s"] = round(max(walls["track"]) - min(walls["track"]), 4)
            res["bytes_out_MB"] = {"track": round(out.nbytes / 1e6, 1), "pcm_all": round(S * N_TRACK * 4 / 1e6, 1),
                                   "flac_all": round(float(sizes.sum()) / 1e6, 1)}
        ctx.close()
        model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
