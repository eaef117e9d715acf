"""Many short tracks: a Python loop of Context.track (one dmx_track_infer per track) against ONE Context.tracks call
(dmx_tracks_infer: the tracks' segments share batches). Prints one JSON line.

Workload (fixed): 64 tracks of 20 s + 8 tracks of 3 s, stereo, synthetic weights (seed 0), host (numpy) buffers in and
out, fixed shift offsets. Each leg runs once as warmup, then --reps times; the median wall time is reported as
track-seconds per second. The two legs' results are also compared bit for bit.

    python tools/multitrack_bench.py [--model 4s] [--gemm bf16x3] [--batch 42] [--reps 3]
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

from demucs_cpp_amd import binding as dmx  # noqa: E402
from demucs_cpp_amd.weights import write_synthetic_model  # noqa: E402

SR = 44100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="4s", choices=["4s", "6s"])
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    S = 4 if a.model == "4s" else 6
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    rng = np.random.default_rng(0)
    secs = [20.0] * 64 + [3.0] * 8
    audios = [(0.1 * rng.standard_normal((2, int(s * SR)))).astype(np.float32) for s in secs]
    shifts = [int(x) for x in rng.integers(0, dmx.MAX_SHIFT, len(audios))]
    total_s = sum(secs)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"ggml-model-htdemucs-{a.model}-f16.bin")
        write_synthetic_model(path, S, 0)
        model = dmx.Model(path, 0)
        ctx = dmx.Context(model, 0, a.batch, gemm)
        out_loop = [np.zeros((S, 2, x.shape[1]), np.float32) for x in audios]
        out_batch = [np.zeros((S, 2, x.shape[1]), np.float32) for x in audios]

        def loop():
            for x, s, o in zip(audios, shifts, out_loop):
                ctx.track(x, s, out=o)

        def batch():
            ctx.tracks(audios, shifts, out=out_batch)

        times = {}
        for name, fn in (("loop", loop), ("tracks", batch)):
            fn()  # warmup (slot / ring growth, plan and graph builds)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            times[name] = float(np.median(ts))
        identical = all(np.array_equal(x, y) for x, y in zip(out_loop, out_batch))
        n_segments = sum(ctx.track_geometry(x.shape[1], s)[1] for x, s in zip(audios, shifts))
        ctx.close()
        model.close()
    loop_tps, batch_tps = total_s / times["loop"], total_s / times["tracks"]
    print(json.dumps({
        "tool": "multitrack_bench", "model": a.model, "gemm": a.gemm, "max_batch": a.batch,
        "workload": "64 x 20 s + 8 x 3 s", "tracks": len(audios), "track_seconds": total_s, "segments": n_segments,
        "reps": a.reps, "loop_wall_s": round(times["loop"], 4), "tracks_wall_s": round(times["tracks"], 4),
        "loop_track_s_per_s": round(loop_tps, 2), "tracks_track_s_per_s": round(batch_tps, 2),
        "speedup": round(batch_tps / loop_tps, 3), "bit_identical": identical,
    }))


if __name__ == "__main__":
    main()
