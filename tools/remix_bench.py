"""Remixed outputs (dmx_tracks_infer_remix through Context.tracks_remix): what a gain matrix over the stems and the mixture
costs beside the hard-wired two-stems output of Context.tracks_pcm. Prints one JSON line.

Workload of tools/pcm_bench.py: one 4-minute track (10 584 000 samples, shift offset 4033), synthetic weights (seed 0),
0.1 N(0,1) audio, host (numpy) buffers in and out, reused. All legs write 16 bit / rescale. Measured, each after one warm-up
call, --reps times, ALTERNATING the legs inside every repetition so that drift of the shared host hits all of them alike:
  two_stems_old    Context.tracks_pcm, stem = vocals                (the OLD entry point: the leg compared with the parent
                                                                     commit's `pcm_vocals` of tools/pcm_bench.py)
  two_stems_remix  Context.tracks_remix, the same matrix (add)      (the same bytes through the gain-table kernels)
  minus            Context.tracks_remix, [vocals; mixture - vocals]  (adds one read of the 2 x n mixture)
  eight            Context.tracks_remix, 8 outputs, fractional gains on every stem and the mixture (the worst case: S + 1
                                                                     plane pairs read per output, twice under rescale)
The record holds every wall time, the medians and the first leg's own spread (max - min over its repetitions): a difference
inside that spread is not a difference. Beside each leg, `stage_ms`: the peak + encode kernels alone (and the memset of
the peaks) on device memory for the same matrix and frame count, between HIP events (dmx_pcm_encode_device for the old
entry point, dmx_remix_encode_device for the others), median of --reps runs, and the bytes they move at least.
--only NAME runs one leg twice (warm-up + one call), for a kernel trace that separates the two kernels:

    python tools/remix_bench.py [--model 4s] [--gemm bf16x3] [--batch 42] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -o remix -- python tools/remix_bench.py --only eight
"""
import argparse
import ctypes
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
N_TRACK = 240 * SR
SHIFT = 4033
LEGS = ["two_stems_old", "two_stems_remix", "minus", "eight"]


def matrices(S):
    rng = np.random.default_rng(8)
    eight = rng.uniform(0.1, 1.2, (8, S + 1)).astype(np.float32) * np.where(rng.uniform(size=(8, S + 1)) < 0.5, -1, 1).astype(np.float32)
    return {"two_stems_remix": dmx.remix_two_stems(S, 3, dmx.OTHER_ADD), "minus": dmx.remix_two_stems(S, 3, dmx.OTHER_MINUS), "eight": eight}


def stage_alone(S, n, reps, mats):
    """ms of memset + peak + encode on device memory per leg; bytes: the planes each kernel must read, the PCM written"""
    import torch

    rng = np.random.default_rng(2)
    d_in = torch.from_numpy((0.4 * rng.standard_normal((S * 2, n))).astype(np.float32)).cuda()
    d_mix = torch.from_numpy((0.4 * rng.standard_normal((n, 2))).astype(np.float32)).cuda()
    ostride = (n * 4 + 15) // 16 * 16
    d_out = torch.zeros(8 * ostride, dtype=torch.uint8, device="cuda")
    d_pk = torch.zeros(8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    old = dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE, 3)
    out = {}
    for leg in LEGS:
        if leg == "two_stems_old":
            n_out, planes = 2, 2 * S

            def call():
                dmx._chk(dmx.lib().dmx_pcm_encode_device(0, d_in.data_ptr(), S, n, n, ctypes.byref(old), d_out.data_ptr(), d_pk.data_ptr(), s))
        else:
            g = mats[leg]
            spec = dmx.RemixSpec(g, dmx.PCM_S16, dmx.CLIP_RESCALE)
            n_out, planes = g.shape[0], 2 * int((g != 0).sum())  # a plane pair per non-zero gain (the mixture counts as one pair)

            def call(spec=spec):
                dmx._chk(dmx.lib().dmx_remix_encode_device(0, d_in.data_ptr(), S, n, n, d_mix.data_ptr(), ctypes.byref(spec.c),
                                                           d_out.data_ptr(), d_pk.data_ptr(), s))
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
        total = 2 * planes * n * 4 + n_out * n * 4
        med = float(np.median(ms))
        out[leg] = {"stage_ms": round(med, 4), "stage_bytes": total, "stage_GBps": round(total / (med * 1e-3) / 1e9, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="4s", choices=["4s", "6s"])
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=LEGS)
    a = ap.parse_args()
    S = 4 if a.model == "4s" else 6
    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    res = {"tool": "remix_bench", "model": a.model, "gemm": a.gemm, "max_batch": a.batch, "reps": a.reps, "track_samples": N_TRACK}
    mats = matrices(S)
    rng = np.random.default_rng(1)
    audio = (0.1 * rng.standard_normal((2, N_TRACK))).astype(np.float32)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"ggml-model-htdemucs-{a.model}-f16.bin")
        write_synthetic_model(path, S, 0)
        model = dmx.Model(path, 0)
        ctx = dmx.Context(model, 0, a.batch, gemm)
        bufs = {2: [np.zeros(2 * N_TRACK * 4, np.uint8)], 8: [np.zeros(8 * N_TRACK * 4, np.uint8)]}  # reused, as in pcm_bench.py
        specs = {k: dmx.RemixSpec(g, dmx.PCM_S16, dmx.CLIP_RESCALE) for k, g in mats.items()}
        variants = {"two_stems_old": lambda: ctx.tracks_pcm([audio], dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE, 3), shift_offsets=[[SHIFT]],
                                                            out=bufs[2])}
        for k in LEGS[1:]:
            variants[k] = lambda k=k: ctx.tracks_remix([audio], specs[k], shift_offsets=[[SHIFT]], out=bufs[specs[k].n_out])
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
            res["two_stems_old_spread_s"] = round(max(walls["two_stems_old"]) - min(walls["two_stems_old"]), 4)
            res["bytes_out_MB"] = {k: round((2 if k != "eight" else 8) * N_TRACK * 4 / 1e6, 1) for k in LEGS}
        ctx.close()
        model.close()
    if not a.only:
        res["stage"] = stage_alone(S, N_TRACK, max(a.reps, 5), mats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
