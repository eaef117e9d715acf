"""The shifts ensemble (dmx_tracks_infer_opts through Context.tracks_opts): what N shifted copies of a track cost. Prints one
JSON line.

Legs (synthetic weights, seed 0; host (numpy) buffers in and out; fixed shift offsets; overlap 0.25):
  a  one 4-minute track at N = 1, 2, 5, 10 shifts: wall time of each, and N=10 / (10 x N=1)
  b  64 tracks of 20 s at N = 5: ONE tracks_opts call against five Context.tracks calls with the same offsets followed by
     the host-side average of the five results (what a caller without the option does); throughput of each in
     track-seconds per second, and the largest relative difference of the two results
Each measurement runs once as warmup, then --reps times; the median wall time is reported.
--only-n N runs a single tracks_opts call of leg a at N shifts (after one warmup), for a kernel trace:

    python tools/shifts_bench.py [--model 4s] [--gemm bf16x3] [--batch 42] [--reps 3] [--legs ab]
    rocprofv3 --kernel-trace --stats -d DIR -o shifts -- python tools/shifts_bench.py --only-n 10
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


def timed(fn, reps):
    fn()  # warmup (slot / ring growth, plan and graph builds)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="4s", choices=["4s", "6s"])
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--only-n", type=int, default=0)
    a = ap.parse_args()
    S = 4 if a.model == "4s" else 6
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    rng = np.random.default_rng(0)
    offs10 = [int(x) for x in rng.integers(0, dmx.MAX_SHIFT, 10)]
    res = {"tool": "shifts_bench", "model": a.model, "gemm": a.gemm, "max_batch": a.batch, "overlap": 0.25, "reps": a.reps}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"ggml-model-htdemucs-{a.model}-f16.bin")
        write_synthetic_model(path, S, 0)
        model = dmx.Model(path, 0)
        ctx = dmx.Context(model, 0, a.batch, gemm)
        long = (0.1 * rng.standard_normal((2, 240 * SR))).astype(np.float32)
        out_long = [np.zeros((S, 2, long.shape[1]), np.float32)]
        if a.only_n:
            N = a.only_n
            ctx.tracks_opts([long], N, 0.25, [offs10[:N]], out=out_long)
            t0 = time.perf_counter()
            ctx.tracks_opts([long], N, 0.25, [offs10[:N]], out=out_long)
            res.update({"leg": "a", "shifts": N, "wall_s": round(time.perf_counter() - t0, 4)})
            a.legs = ""
        if "a" in a.legs:
            walls = {}
            for N in (1, 2, 5, 10):
                walls[N] = timed(lambda: ctx.tracks_opts([long], N, 0.25, [offs10[:N]], out=out_long), a.reps)
            res["a_workload"] = "one 240 s track"
            res["a_wall_s"] = {str(N): round(w, 4) for N, w in walls.items()}
            res["a_track_s_per_s"] = {str(N): round(240.0 / w, 2) for N, w in walls.items()}
            res["a_n10_over_10x_n1"] = round(walls[10] / (10 * walls[1]), 4)
        if "b" in a.legs:
            N = 5
            audios = [(0.1 * rng.standard_normal((2, 20 * SR))).astype(np.float32) for _ in range(64)]
            offs = rng.integers(0, dmx.MAX_SHIFT, (64, N))
            one = [np.zeros((S, 2, x.shape[1]), np.float32) for x in audios]
            sep = [[np.zeros((S, 2, x.shape[1]), np.float32) for x in audios] for _ in range(N)]
            avg = [np.zeros((S, 2, x.shape[1]), np.float32) for x in audios]

            def one_call():
                ctx.tracks_opts(audios, N, 0.25, offs, out=one)

            def five_calls():
                for k in range(N):
                    ctx.tracks(audios, [int(s) for s in offs[:, k]], out=sep[k])
                for t in range(len(audios)):
                    np.mean([sep[k][t] for k in range(N)], axis=0, out=avg[t])

            w1, w5 = timed(one_call, a.reps), timed(five_calls, a.reps)
            total = 64 * 20.0
            diff = max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(one, avg))
            items = sum(dmx.track_geometry(dmx.SEGMENT_SAMPLES, x.shape[1], int(s))[1] for x, row in zip(audios, offs) for s in row)
            res.update({"b_workload": "64 x 20 s, 5 shifts", "b_items": items,
                        "b_tracks_opts_wall_s": round(w1, 4), "b_five_tracks_calls_wall_s": round(w5, 4),
                        "b_tracks_opts_track_s_per_s": round(total / w1, 2), "b_five_tracks_calls_track_s_per_s": round(total / w5, 2),
                        "b_speedup": round(w5 / w1, 3), "b_max_rel_diff": diff})
        ctx.close()
        model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
