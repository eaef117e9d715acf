"""Bags of models on the track path (dmx_tracks_infer_bag through Context.tracks_bag) against the engine's fine-tuned bag
(Engine.track). Prints one JSON line.

Legs (four synthetic 4-source models, seeds 50..53; host (numpy) buffers in and out; fixed shift offsets; overlap 0.25):
  a  one 4-minute track through the diagonal bag: Context.tracks_bag and Engine(paths, [0]).track ALTERNATE within the run;
     median, min and max of each, and bag / engine. The kernels are the same, so the bag must not be slower than the engine
     by more than the engine's own spread.
  b  16 tracks of 20 s: ONE tracks_bag call against a loop of Engine.track; track-seconds per second of each and the ratio;
     the results compared bit for bit.
  c  the 4-minute track at 2 shifts through the bag.
Every measurement is warmed once, then repeated --reps times.
--only bag|tracks runs a single call (after one warmup) of the 4-minute track through the bag, or through Context.tracks on
one model, for a kernel trace:

    python tools/bag_bench.py [--gemm bf16x3] [--batch 42] [--reps 3] [--legs abc]
    rocprofv3 --kernel-trace --stats -d DIR -o bag -- python tools/bag_bench.py --only bag
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
SHIFTS = (4033, 12436, 5427, 6865)
FT = ("drums", "bass", "other", "vocals")


def stats(ts):
    return {"median_s": round(float(np.median(ts)), 4), "min_s": round(float(min(ts)), 4), "max_s": round(float(max(ts)), 4)}


def alternate(fns, reps):
    """each function warmed once, then reps rounds in which they alternate: {name: [seconds]}"""
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--only", default="", choices=["", "bag", "tracks"])
    a = ap.parse_args()
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    dmx.set_default_gemm(gemm)  # the engine's contexts take the process default
    rng = np.random.default_rng(0)
    res = {"tool": "bag_bench", "model": "4s x 4 (diagonal bag)", "gemm": a.gemm, "max_batch": a.batch, "overlap": 0.25, "reps": a.reps}
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, name in enumerate(FT):
            paths.append(os.path.join(d, f"ggml-model-htdemucs_ft_{name}-4s-f16.bin"))
            write_synthetic_model(paths[-1], 4, 50 + i)
        models = [dmx.Model(p, 0) for p in paths]
        ctx = dmx.Context(models[0], 0, a.batch, gemm)
        long = (0.1 * rng.standard_normal((2, 240 * SR))).astype(np.float32)
        out_bag = [np.zeros((4, 2, long.shape[1]), np.float32)]
        offs1 = np.array(SHIFTS).reshape(1, 4, 1)

        def bag_long():
            ctx.tracks_bag(models, [long], shift_offsets=offs1, out=out_bag)

        if a.only:
            fn = bag_long if a.only == "bag" else (lambda: ctx.tracks([long], [SHIFTS[0]], out=out_bag))
            fn()
            t0 = time.perf_counter()
            fn()
            res.update({"only": a.only, "wall_s": round(time.perf_counter() - t0, 4)})
            a.legs = ""
        eng = dmx.Engine(paths, [0], max_batch=a.batch) if a.legs else None
        if "a" in a.legs:
            out_eng = np.zeros((4, 2, long.shape[1]), np.float32)
            ts = alternate({"bag": bag_long, "engine": lambda: eng.track(long, list(SHIFTS), out=out_eng)}, a.reps)
            res["a_workload"] = "one 240 s track, diagonal bag"
            res["a_tracks_bag"] = stats(ts["bag"])
            res["a_engine_track"] = stats(ts["engine"])
            res["a_bag_over_engine"] = round(float(np.median(ts["bag"]) / np.median(ts["engine"])), 4)
            res["a_engine_spread"] = round(float((max(ts["engine"]) - min(ts["engine"])) / np.median(ts["engine"])), 4)
            res["a_x_realtime"] = round(240.0 / float(np.median(ts["bag"])), 1)
            res["a_bitwise_equal"] = bool(np.array_equal(out_bag[0], out_eng))
        if "b" in a.legs:
            audios = [(0.1 * rng.standard_normal((2, 20 * SR))).astype(np.float32) for _ in range(16)]
            offs = np.tile(np.array(SHIFTS).reshape(1, 4, 1), (16, 1, 1))
            one = [np.zeros((4, 2, x.shape[1]), np.float32) for x in audios]
            sep = [np.zeros((4, 2, x.shape[1]), np.float32) for x in audios]

            def engine_loop():
                for x, o in zip(audios, sep):
                    eng.track(x, list(SHIFTS), out=o)

            ts = alternate({"bag": lambda: ctx.tracks_bag(models, audios, shift_offsets=offs, out=one), "engine": engine_loop}, a.reps)
            total = 16 * 20.0
            res.update({"b_workload": "16 x 20 s, diagonal bag", "b_tracks_bag": stats(ts["bag"]), "b_engine_loop": stats(ts["engine"]),
                        "b_tracks_bag_track_s_per_s": round(total / float(np.median(ts["bag"])), 2),
                        "b_engine_loop_track_s_per_s": round(total / float(np.median(ts["engine"])), 2),
                        "b_speedup": round(float(np.median(ts["engine"]) / np.median(ts["bag"])), 3),
                        "b_bitwise_equal": bool(all(np.array_equal(x, y) for x, y in zip(one, sep)))})
        if "c" in a.legs:
            offs2 = np.array([[[s, (s + 11025) % dmx.MAX_SHIFT] for s in SHIFTS]])
            ts = alternate({"bag2": lambda: ctx.tracks_bag(models, [long], None, 2, 0.25, offs2, out=out_bag)}, a.reps)
            res["c_workload"] = "one 240 s track, diagonal bag, 2 shifts"
            res["c_tracks_bag"] = stats(ts["bag2"])
            res["c_x_realtime"] = round(240.0 / float(np.median(ts["bag2"])), 1)
        if eng:
            eng.close()
        ctx.close()
        for m in models:
            m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
