"""The FLAC input stage (dmx_tracks_infer_from_flac through Context.tracks_from_flac; csrc/flac_in.hip): what it costs to take
a track as the bytes of a .flac file instead of fp32 planes the host has decoded. Prints one JSON line.

The track is tests/golden/gspi_stereo.wav tiled to 4 minutes (10 584 000 samples), as 16-bit integers: its .flac file (written
by the FLAC output stage) for the FLAC legs, its floats v / 32768 for the fp32 legs, so every leg computes the same outputs
(16-bit PCM stems, rescale, identity gains; synthetic weights, seed 0; shift offset 4033; host buffers in and out).

Legs, each in a worker process of its own that stays alive (one warm-up call, then one timed call per repetition), the workers
ALTERNATING inside every repetition (in forward and backward order by turns) so that drift of the shared host hits all of them alike:
  parent_fp32   Context.tracks_remix from fp32 on the PARENT commit's tree (--parent-root: a checkout of the parent commit
                with its library built): the yardstick, with its own spread (max - min over its repetitions) beside it
  fp32          the same call on this tree: the old path must be inside that spread
  flac          Context.tracks_from_flac on this tree
  many_fp32 / many_flac   64 tracks of 20 s in one call on this tree, from fp32 and from .flac files
--stage: the five launches alone between HIP events (dmx_flac_decode_profile) on the 4-minute file in device memory, and the
file bytes per second of each.

    python tools/flac_in_bench.py --parent-root DIR [--reps 5] [--batch 42] [--gemm bf16x3] >> profiles/flac_in_4s_bf16x3_b42.jsonl
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 44100
N_TRACK = 240 * SR
SHIFT = 4033


def recording(n):
    with wave.open(os.path.join(ROOT, "tests", "golden", "gspi_stereo.wav")) as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2)
    return np.ascontiguousarray(np.tile(pcm, ((n + pcm.shape[0] - 1) // pcm.shape[0], 1))[:n])


def worker(a):
    """one leg: reads 'go' lines, answers each with the wall time of one call"""
    sys.path.insert(0, a.root)
    from demucs_cpp_amd import binding as dmx
    from demucs_cpp_amd.weights import write_synthetic_model

    gemm = {"f32": dmx.GEMM_F32, "bf16x3": dmx.GEMM_BF16X3, "fp16x3": dmx.GEMM_FP16X3}[a.gemm]
    many = a.worker.startswith("many")
    pcm = [recording(20 * SR + 1000 * t) for t in range(64)] if many else [recording(N_TRACK)]
    T = len(pcm)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ggml-model-htdemucs-4s-f16.bin")
        write_synthetic_model(path, 4, 0)
        model = dmx.Model(path, 0)
        ctx = dmx.Context(model, 0, a.batch, gemm)
        spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_RESCALE)
        offs = [[SHIFT]] * T
        if a.worker.endswith("flac"):
            files = [dmx.flac_encode(x, 16) for x in pcm]
            bufs = [np.zeros(4 * x.shape[0] * 4, np.uint8) for x in pcm]
            call = lambda: ctx.tracks_from_flac(files, spec, shift_offsets=offs, out=bufs)  # noqa: E731
            in_bytes = sum(len(f) for f in files)
        else:
            audios = [np.ascontiguousarray((x.astype(np.float32) / np.float32(32768.0)).T) for x in pcm]
            bufs = [np.zeros(4 * x.shape[0] * 4, np.uint8) for x in pcm]
            call = lambda: ctx.tracks_remix(audios, spec, shift_offsets=offs, out=bufs)  # noqa: E731
            in_bytes = sum(x.nbytes for x in audios)
        call()  # warm-up: slots, staging buffers, plans
        print(json.dumps({"ready": a.worker, "bytes_in": in_bytes}), flush=True)
        for line in sys.stdin:
            if line.strip() != "go":
                break
            t0 = time.perf_counter()
            call()
            print(json.dumps({"wall_s": time.perf_counter() - t0}), flush=True)
        ctx.close()
        model.close()


def stage(a):
    sys.path.insert(0, ROOT)
    import torch

    from demucs_cpp_amd import binding as dmx

    data = dmx.flac_encode(recording(N_TRACK), 16)
    info = dmx.flac_probe(data)
    L = dmx.lib()
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_work = torch.empty(L.dmx_flac_decode_workspace_bytes(ctypes.byref(info), len(data)), dtype=torch.uint8, device="cuda")
    d_out = torch.empty(N_TRACK * 8, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(2, dtype=torch.int64, device="cuda")
    ms = (ctypes.c_float * 5)()
    rows = []
    for _ in range(a.reps + 1):
        dmx._chk(L.dmx_flac_decode_profile(0, d_file.data_ptr(), len(data), ctypes.byref(info), dmx.PCM_F32, d_out.data_ptr(),
                                           d_status.data_ptr(), d_work.data_ptr(), None, ms))
        rows.append([float(v) for v in ms])
    assert d_status.cpu().tolist() == [0, N_TRACK]
    med = np.median(np.array(rows[1:]), axis=0)  # the first call is the warm-up
    names = ("candidates", "scan", "chain", "decode", "finish")
    return {"file_bytes": len(data), "fp32_bytes": N_TRACK * 8, "ratio_to_s16": round(len(data) / (N_TRACK * 4), 4),
            "ms": {k: round(float(v), 4) for k, v in zip(names, med)}, "total_ms": round(float(med.sum()), 4),
            "file_GB_per_s": {k: round(len(data) / (float(v) * 1e-3) / 1e9, 3) for k, v in zip(names, med)}, "all_ms": rows[1:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--gemm", default="bf16x3", choices=["f32", "bf16x3", "fp16x3"])
    ap.add_argument("--batch", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage", action="store_true")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = {"tool": "flac_in_bench", "model": "4s", "gemm": a.gemm, "max_batch": a.batch, "reps": a.reps, "track_samples": N_TRACK}
    if a.stage:
        res["stage"] = stage(a)
        print(json.dumps(res))
        return
    legs = {"fp32": ROOT, "flac": ROOT, "many_fp32": ROOT, "many_flac": ROOT}
    if a.parent_root:
        legs = dict([("parent_fp32", os.path.abspath(a.parent_root))] + list(legs.items()))
    procs = {}
    for name, root in legs.items():
        kind = "fp32" if name == "parent_fp32" else name
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root, "--gemm", a.gemm, "--batch",
                                        str(a.batch)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
    walls = {k: [] for k in legs}
    try:
        for name, p in procs.items():
            res[name + "_bytes_in_MB"] = round(json.loads(p.stdout.readline())["bytes_in"] / 1e6, 1)
        for rep in range(a.reps):
            for name, p in (list(procs.items()) if rep % 2 == 0 else reversed(list(procs.items()))):  # no leg always behind the same one
                p.stdin.write("go\n")
                p.stdin.flush()
                walls[name].append(json.loads(p.stdout.readline())["wall_s"])
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=120)
    for k, w in walls.items():
        res[k + "_wall_s"] = [round(x, 4) for x in w]
        res[k + "_median_s"] = round(float(np.median(w)), 4)
    y = "parent_fp32" if a.parent_root else "fp32"
    res["yardstick"] = y
    res["yardstick_spread_s"] = round(max(walls[y]) - min(walls[y]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
