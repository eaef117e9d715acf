"""The log-mel stage on the GPU (csrc/logmel.hip): what its launches cost. Prints one JSON line per case.

Cases: a 4-minute mono plane at 16 kHz with the presets whisper and whisper128, and the eight planes of a 4-stem stereo track at
22.05 kHz with librosa.
  stages     dmx_logmel_device_timed on device memory, --reps times after one warm-up: the tables, the power-mel launch and the
             finish launch between HIP events; the median and the spread (max - min) of each.
  needed     the binary64 operations the power-mel launch needs: 2 n_fft (n_fft + 2) per frame for the first product and
             2 x 256 per frame tile of 16 for each non-zero 16 x 16 block of W for the second, over the median time, as a fraction
             of --peak-tflops (78.6, the figure of BASELINE.md and DESIGN.md section 2.18).
  issued     the same with what the MFMAs issue: bin tiles padded to 16 (2 x 32 n_fft per frame per bin tile), frames padded to
             the tile of the workgroup.
  whole      binding.logmel_from_stems host to host on a stereo stem set at 44.1 kHz of the same duration (fold, resampler, the
             stage, allocation and copies), --reps times.
  cpu        with --cpu: torch.stft + matmul + log in float64 on this machine's CPU, the same case, once.

    python tools/logmel_bench.py [--reps 10] [--seconds 240] [--cpu]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from demucs_cpp_amd import binding as dmx  # noqa: E402


def operations(spec, P, n):
    chunks, frames = dmx.logmel_frames(spec, n)
    ft = dmx.logmel_geometry(spec)[0]
    W = dmx.logmel_filters(spec)
    nft, nmt = -(-W.shape[1] // 16), -(-spec.n_mels // 16)
    Wp = np.zeros((nmt * 16, nft * 16))
    Wp[:W.shape[0], :W.shape[1]] = W
    blocks = int((np.abs(Wp).reshape(nmt, 16, nft, 16).max(axis=(1, 3)) > 0).sum())
    T = P * chunks * frames
    Tp = P * chunks * -(-frames // ft) * ft
    needed = 2 * spec.n_fft * (spec.n_fft + 2) * T + 2 * 256 * blocks * T
    issued = 2 * 32 * spec.n_fft * nft * Tp + 2 * 256 * blocks * Tp
    return needed, issued


def cpu_route(x, spec):
    import torch
    t0 = time.perf_counter()
    W = torch.from_numpy(dmx.logmel_filters(spec))
    X = torch.stft(torch.from_numpy(x).double(), spec.n_fft, spec.hop, window=torch.hann_window(spec.n_fft, dtype=torch.float64), return_complex=True)
    M = W @ (X.real ** 2 + X.imag ** 2)
    torch.log10(torch.clamp(M, min=1e-10))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=240)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("logmel_bench: no GPU (there is no CPU fallback; nothing is measured)")
    for preset, P in (("whisper", 1), ("whisper128", 1), ("librosa", 8)):
        spec = dmx.logmel_preset(preset)
        n = spec.sr * a.seconds
        x = (0.1 * np.random.default_rng(P).standard_normal((P, n))).astype(np.float32)
        chunks, frames = dmx.logmel_frames(spec, n)
        wbytes = dmx.logmel_workspace_bytes(spec, P, n)
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.empty((P, chunks, spec.n_mels, frames), dtype=torch.float32, device="cuda")
        work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        ms, rows = np.zeros(3, np.float32), []
        for r in range(a.reps + 1):
            dmx._chk(dmx.lib().dmx_logmel_device_timed(0, d_x.data_ptr(), P, n, n, ctypes.byref(spec), d_out.data_ptr(), work.data_ptr(), wbytes,
                                                       None, ms.ctypes.data))
            if r:
                rows.append(ms.copy())
        rows = np.array(rows, np.float64)
        med, spread = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0)
        needed, issued = operations(spec, P, n)
        S = max(P // 2, 1)
        stems = (0.1 * np.random.default_rng(S).standard_normal((S, 2, 44100 * a.seconds))).astype(np.float32)
        whole = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            dmx.logmel_from_stems(stems, 44100, spec)
            if r:
                whole.append(time.perf_counter() - t0)
        res = {"preset": preset, "planes": P, "samples": n, "chunks": chunks, "frames": frames, "tile": dmx.logmel_geometry(spec),
               "workspace_mb": wbytes / 1e6, "equals_host_call": bool(np.array_equal(d_out.cpu().numpy(), dmx.logmel(x, spec))),
               **{k + "_ms": float(med[i]) for i, k in enumerate(("tables", "power_mel", "finish"))},
               **{k + "_spread_ms": float(spread[i]) for i, k in enumerate(("tables", "power_mel", "finish"))},
               "needed_gflop": needed / 1e9, "issued_gflop": issued / 1e9,
               "needed_of_peak": needed / (med[1] * 1e-3) / 1e12 / a.peak_tflops, "issued_of_peak": issued / (med[1] * 1e-3) / 1e12 / a.peak_tflops,
               "from_stems_sources": S, "from_stems_host_to_host_s": float(np.median(whole)), "from_stems_spread_s": float(max(whole) - min(whole)),
               "peak_tflops": a.peak_tflops}
        if a.cpu:
            res["cpu_torch_stft_matmul_s"] = cpu_route(x, spec)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
