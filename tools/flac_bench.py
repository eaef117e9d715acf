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
FLAC bytes it leaves, and records the compression ratio of the recording itself.
--level N or --level 0,1,2 chooses the compression level(s) (dmx_ctx_set_flac_level; dmx_flac_encode_device_timed): several
levels run as further legs of the same alternation (flac_all_l0, flac_all_l1, ...), and --stage records, per level, the three
kernels (frames, scan, compact) between HIP events:

    python tools/flac_bench.py [--model 4s] [--gemm bf16x3] [--batch 42] [--reps 5] [--level 0,1,2]
    python tools/flac_bench.py --stage 10584000 --level 0,1,2
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
    return np.ascontiguousarray(np.clip(np.rint(np.asarray(audio, np.float64).T * full), -full, full - 1).astype(np.int32))


def _pcm_bytes(x, bits):
    if bits == 16:
        return x.astype("<i2").view(np.uint8).ravel()
    q = x.astype(np.int64) & 0xFFFFFF
    return np.stack([(q >> (8 * b)).astype(np.uint8) for b in range(3)], axis=-1).ravel()


def stage_alone(n, reps, levels):
    import ctypes

    import torch

    L = dmx.lib()
    out = {}
    for bits in (16, 24):
        x = _recording(bits)
        as_pcm = _pcm_bytes(x, bits).view("<i2").reshape(-1, 2) if bits == 16 else _pcm_bytes(x, bits).reshape(-1, 2, 3)
        own = {lv: len(dmx.flac_encode(as_pcm, bits, level=lv)) for lv in levels}
        tiled = np.tile(x, ((n + x.shape[0] - 1) // x.shape[0], 1))[:n]
        raw = _pcm_bytes(tiled, bits)
        d_pcm = torch.from_numpy(raw.copy()).cuda()
        d_out = torch.zeros(dmx.flac_bound(bits, n), dtype=torch.uint8, device="cuda")
        d_size = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_work = torch.zeros(L.dmx_flac_workspace_bytes(bits, n), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ms3 = (ctypes.c_float * 3)()

        def call(lv):
            dmx._chk(L.dmx_flac_encode_device_timed(0, d_pcm.data_ptr(), bits, n, SR, lv, d_out.data_ptr(), d_size.data_ptr(),
                                                    d_work.data_ptr(), s, ms3))
            return [float(v) for v in ms3]

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

        for lv in levels:
            call(lv)  # warm-up: the code objects
        kern = {lv: [] for lv in levels}
        for _ in range(reps):  # the levels alternate inside every repetition
            for lv in levels:
                kern[lv].append(call(lv))
        rec = {"frames": n, "pcm_bytes": int(raw.size), "recording_frames": int(x.shape[0])}
        size0 = None
        for lv in levels:
            call(lv)
            size = int(d_size.item())
            size0 = size if size0 is None else size0
            k = np.array(kern[lv])
            rec[f"level{lv}"] = {"flac_bytes": size, "ratio": round(size / raw.size, 4),
                                 "frames_kernel_ms": [round(v, 4) for v in k[:, 0]], "frames_kernel_median_ms": round(float(np.median(k[:, 0])), 4),
                                 "scan_kernel_median_ms": round(float(np.median(k[:, 1])), 4),
                                 "compact_kernel_median_ms": round(float(np.median(k[:, 2])), 4),
                                 "encode_median_ms": round(float(np.median(k.sum(axis=1))), 4),
                                 "recording_flac_bytes": own[lv], "recording_ratio": round(own[lv] / (x.shape[0] * 2 * bits // 8), 4)}
        h_pcm = torch.empty(raw.size, dtype=torch.uint8).pin_memory()
        h_flac = torch.empty(size0, dtype=torch.uint8).pin_memory()
        ms_pcm = timed(lambda: h_pcm.copy_(d_pcm, non_blocking=True))
        ms_flac = timed(lambda: h_flac.copy_(d_out[:size0], non_blocking=True))
        rec.update({"d2h_pcm_ms": ms_pcm, "d2h_pcm_median_ms": round(float(np.median(ms_pcm)), 4),
                    "d2h_flac_ms": ms_flac, "d2h_flac_median_ms": round(float(np.median(ms_flac)), 4)})
        out[f"s{bits}"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="4s", choices=["4s", "6s"])
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["track", "pcm_all", "flac_all"])  # (flac_all: with ONE --level)
    ap.add_argument("--stage", type=int, default=0, metavar="FRAMES")
    ap.add_argument("--level", default="0", metavar="N[,N...]", help="FLAC compression level(s): 0, 1, 2 or a comma-separated list")
    a = ap.parse_args()
    levels = [int(v) for v in a.level.split(",")]
    if not levels or any(lv not in (0, 1, 2) for lv in levels):
        ap.error("--level: 0, 1, 2 or a comma-separated list of them")
    S = 4 if a.model == "4s" else 6
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    res = {"tool": "flac_bench", "model": a.model, "gemm": a.gemm, "max_batch": a.batch, "reps": a.reps, "track_samples": N_TRACK,
           "levels": levels}
    if a.stage:
        res["stage"] = stage_alone(a.stage, max(a.reps, 5), levels)
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
        sizes = {lv: np.zeros(S, np.int64) for lv in levels}

        def flac_leg(lv):
            ctx.flac_level = lv
            return ctx.tracks_flac([audio], spec, shift_offsets=[[SHIFT]], out=buf_flac, sizes=sizes[lv])

        variants = {
            "track": lambda: ctx.track(audio, SHIFT, out=out),
            "pcm_all": lambda: ctx.tracks_remix([audio], spec, shift_offsets=[[SHIFT]], out=buf_pcm),
        }
        for lv in levels:  # one level: the leg keeps its name
            variants["flac_all" if len(levels) == 1 else f"flac_all_l{lv}"] = (lambda lv=lv: flac_leg(lv))
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
            res["bytes_out_MB"] = {"track": round(out.nbytes / 1e6, 1), "pcm_all": round(S * N_TRACK * 4 / 1e6, 1)}
            for lv in levels:
                res["bytes_out_MB"]["flac_all" if len(levels) == 1 else f"flac_all_l{lv}"] = round(float(sizes[lv].sum()) / 1e6, 1)
        ctx.close()
        model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
