"""The PCM output stage (dmx_tracks_infer_pcm through Context.tracks_pcm): what it costs to let a track leave the GPU as
16-bit WAV data instead of fp32 planes. Prints one JSON line.

Workload of tools/track_bench.py: one 4-minute track (10 584 000 samples, shift offset 4033), synthetic weights (seed 0),
0.1 N(0,1) audio, host (numpy) buffers in and out. Measured, each after one warm-up call, --reps times, ALTERNATING the
variants inside every repetition so that drift of the shared host hits all of them alike:
  track        Context.track                                  (fp32 planes out: the yardstick)
  pcm_all      Context.tracks_pcm, S16 / rescale / all stems  (half the bytes out)
  pcm_vocals   Context.tracks_pcm, S16 / rescale / two-stems  (a quarter, 4 sources)
  pcm_clamp    Context.tracks_pcm, S16 / clamp / all stems    (encoded and copied piece by piece)
The record holds every wall time, the medians, and the yardstick's own spread (max - min over its repetitions): a
difference inside that spread is not a difference. --lib PATH measures `track` alone through the C ABI in child processes,
alternating this build and another build of the library (the parent commit's), in the same session: `track_alone_*`.
--only NAME runs one variant twice (warm-up + one call), for a kernel trace; --stage N times the stage alone on device
memory (dmx_pcm_encode_device on N frames) with HIP events:

    python tools/pcm_bench.py [--model 4s] [--gemm bf16x3] [--batch 42] [--reps 5] [--lib OTHER.so]
    rocprofv3 --kernel-trace --stats -d DIR -o pcm -- python tools/pcm_bench.py --only pcm_all
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from demucs_cpp_amd import binding as dmx  # noqa: E402
from demucs_cpp_amd.weights import write_synthetic_model  # noqa: E402

SR = 44100
N_TRACK = 240 * SR
SHIFT = 4033


def stage_alone(S, n, reps):
    """GB/s of the peak + encode kernels on device memory (algorithmic bytes: the planes each kernel reads, the PCM written)"""
    import ctypes

    import torch

    rng = np.random.default_rng(2)
    d_in = torch.from_numpy((0.4 * rng.standard_normal((S * 2, n))).astype(np.float32)).cuda()
    out = {}
    for name, enc, per, stem in (("s16_all", dmx.PCM_S16, 4, -1), ("s16_two_stems", dmx.PCM_S16, 4, 3), ("s24_all", dmx.PCM_S24, 6, -1),
                                 ("f32_all", dmx.PCM_F32, 8, -1)):
        spec = dmx.OutputSpec(enc, dmx.CLIP_RESCALE, stem)
        n_out = S if stem < 0 else 2
        ostride = (n * per + 15) // 16 * 16
        d_out = torch.zeros(n_out * ostride, dtype=torch.uint8, device="cuda")
        d_pk = torch.zeros(n_out, device="cuda")
        s = torch.cuda.current_stream().cuda_stream

        def call():
            dmx._chk(dmx.lib().dmx_pcm_encode_device(0, d_in.data_ptr(), S, n, n, ctypes.byref(spec), d_out.data_ptr(), d_pk.data_ptr(), s))

        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        read = S * 2 * n * 4  # every plane once per kernel (two-stems reads them all as well)
        total = 2 * read + n_out * n * per
        out[name] = {"ms": round(float(np.median(ms)), 4), "bytes": total, "GBps": round(total / (float(np.median(ms)) * 1e-3) / 1e9, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="4s", choices=["4s", "6s"])
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another libdemucs_hip.so whose Context.track is measured in a child process")
    ap.add_argument("--only", default=None, choices=["track", "pcm_all", "pcm_vocals", "pcm_clamp"])
    ap.add_argument("--stage", type=int, default=0, metavar="FRAMES")
    a = ap.parse_args()
    S = 4 if a.model == "4s" else 6
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    res = {"tool": "pcm_bench", "model": a.model, "gemm": a.gemm, "max_batch": a.batch, "reps": a.reps, "track_samples": N_TRACK}
    if a.stage:
        res["stage_frames"] = a.stage
        res["stage"] = stage_alone(S, a.stage, max(a.reps, 5))
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
        buf_all, buf_two = [np.zeros(S * N_TRACK * 4, np.uint8)], [np.zeros(2 * N_TRACK * 4, np.uint8)]  # reused, like `out`
        variants = {
            "track": lambda: ctx.track(audio, SHIFT, out=out),
            "pcm_all": lambda: ctx.tracks_pcm([audio], dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE, -1), shift_offsets=[[SHIFT]], out=buf_all),
            "pcm_vocals": lambda: ctx.tracks_pcm([audio], dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE, 3), shift_offsets=[[SHIFT]], out=buf_two),
            "pcm_clamp": lambda: ctx.tracks_pcm([audio], dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_CLAMP, -1), shift_offsets=[[SHIFT]], out=buf_all),
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
                                   "pcm_vocals": round(2 * N_TRACK * 4 / 1e6, 1)}
        ctx.close()
        model.close()
    if a.lib and not a.only:
        # the yardstick alone on this build and on another one, each run in its own process (one library per process), alternating
        runs = {"this": [], "other": []}
        for which in ("this", "other", "this", "other"):
            env = dict(os.environ, DMX_LIB=os.path.abspath(a.lib if which == "other" else dmx.LIB_PATH))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", a.model, "--gemm", a.gemm, "--batch", str(a.batch),
                                "--reps", str(a.reps), "--track-only"], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError("--lib run failed: " + r.stderr[-2000:])
            runs[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
        res["track_alone_other_lib"] = os.path.basename(a.lib)
        for which in runs:
            res[f"track_alone_{which}_wall_s"] = [x["track_wall_s"] for x in runs[which]]
            res[f"track_alone_{which}_median_s"] = [x["track_median_s"] for x in runs[which]]
    print(json.dumps(res))


def track_only():
    """child mode of --lib: only Context.track (the other build has no tracks_pcm)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="4s")
    ap.add_argument("--gemm", default="bf16x3")
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--track-only", action="store_true")
    a = ap.parse_args()
    S = 4 if a.model == "4s" else 6
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    rng = np.random.default_rng(1)
    audio = (0.1 * rng.standard_normal((2, N_TRACK))).astype(np.float32)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"ggml-model-htdemucs-{a.model}-f16.bin")
        write_synthetic_model(path, S, 0)
        import ctypes

        # the other build lacks symbols that the binding declares: load it directly and use the C ABI that both have
        L = ctypes.CDLL(dmx.LIB_PATH)
        vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.dmx_last_error.restype = ctypes.c_char_p
        L.dmx_model_load.argtypes = [ctypes.c_char_p, ci, ctypes.POINTER(vp)]
        L.dmx_ctx_create_gemm.argtypes = [vp, i64, ci, ci, ctypes.POINTER(vp)]
        L.dmx_track_infer.argtypes = [vp, vp, i64, ci, vp, ci, vp, vp]
        L.dmx_ctx_free.argtypes = [vp]
        L.dmx_model_free.argtypes = [vp]

        def chk(rc):
            if rc != 0:
                raise RuntimeError(L.dmx_last_error().decode(errors="replace"))

        h, c = vp(), vp()
        chk(L.dmx_model_load(path.encode(), 0, ctypes.byref(h)))
        chk(L.dmx_ctx_create_gemm(h, 0, a.batch, gemm, ctypes.byref(c)))
        out = np.zeros((S, 2, N_TRACK), np.float32)

        def call():
            chk(L.dmx_track_infer(c, audio.ctypes.data, N_TRACK, SHIFT, out.ctypes.data, dmx.LAYOUT_PLANAR, None, None))

        call()
        w = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            w.append(time.perf_counter() - t0)
        L.dmx_ctx_free(c)
        L.dmx_model_free(h)
    print(json.dumps({"track_wall_s": [round(x, 4) for x in w], "track_median_s": round(float(np.median(w)), 4)}))


if __name__ == "__main__":
    if "--track-only" in sys.argv:
        track_only()
    else:
        main()
