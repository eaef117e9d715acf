"""WPE de-reverberation on the GPU (csrc/dereverb.hip): what its stages cost on a track.
Prints one JSON line.

A track of --seconds (240) of noise stems at 44.1 kHz, --sources (4) stereo stems:
  stages     dmx_dereverb_device_timed on device memory, --reps times after one warm-up: the forward STFT (with the floor and
             the first lam), each iteration (correlation, solve, filter) and the inverse between HIP events; the median and
             the spread (max - min) of each and of their sum.
  flops      the correlation of one iteration over J x 2049 bins x T frames: needed = 4 M (M + 1) + 8 M C per frame (the lower
             triangle of the Hermitian R and P, 8 flops per complex multiply-add), issued = 512 per 16 x 16 tile and frame over
             the tiles on and below the diagonal of the 2 M + 2 C real rows. An iteration's time holds the solve and the filter
             as well, so the shares of --peak-tflops (78.6, binary64 matrix) over it are lower bounds for the kernel; its own
             time comes from a kernel trace of this tool.
  whole      binding.dereverb host to host (allocation, copies and the kernels), --reps times.

    python tools/dereverb_bench.py [--reps 10] [--seconds 240] [--sources 4] [--taps 10] [--delay 3] [--iterations 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=240)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--taps", type=int, default=10)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    a = ap.parse_args()
    import torch

    J, C, n, it = a.sources, 2, 44100 * a.seconds, a.iterations
    rng = np.random.default_rng(J)
    x = (0.1 * rng.standard_normal((J, C, n))).astype(np.float32)
    spec = dmx.DereverbSpec(a.taps, a.delay, it)
    wbytes = dmx.dereverb_workspace_bytes(spec, J, C, n)
    d_x = torch.from_numpy(x).cuda()
    d_out, work = torch.empty_like(d_x), torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    stages = ["stft"] + [f"iter{k}" for k in range(it)] + ["istft"]
    ms, rows = np.zeros(len(stages), np.float32), []
    for r in range(a.reps + 1):
        dmx._chk(dmx.lib().dmx_dereverb_device_timed(0, d_x.data_ptr(), J, C, n, n, ctypes.byref(spec), d_out.data_ptr(), work.data_ptr(),
                                                     wbytes, None, ms.ctypes.data))
        if r:
            rows.append(ms.copy())
    rows = np.array(rows, np.float64)
    med, spread, total = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0), rows.sum(axis=1)
    T, M = 1 + n // 1024, C * a.taps
    nt = (2 * M + 2 * C + 15) // 16
    cells = J * 2049 * T
    needed, issued = cells * (4 * M * (M + 1) + 8 * M * C), cells * 512 * nt * (nt + 1) // 2
    it_ms = float(np.median(rows[:, 1:1 + it]))
    whole = []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        out = dmx.dereverb(x, spec)
        if r:
            whole.append(time.perf_counter() - t0)
    same = bool(np.array_equal(out, d_out.cpu().numpy()))
    print(json.dumps({"sources": J, "channels": C, "frames": n, "taps": a.taps, "delay": a.delay, "iterations": it,
                      "workspace_gb": wbytes / 1e9, "device_equals_host_call": same,
                      **{k + "_ms": float(med[i]) for i, k in enumerate(stages)},
                      **{k + "_spread_ms": float(spread[i]) for i, k in enumerate(stages)},
                      "corr_needed_gflop": needed / 1e9, "corr_issued_gflop": issued / 1e9,
                      "iteration_needed_of_peak": needed / (it_ms * 1e-3) / 1e12 / a.peak_tflops,
                      "iteration_issued_of_peak": issued / (it_ms * 1e-3) / 1e12 / a.peak_tflops,
                      "total_ms": float(np.median(total)), "total_spread_ms": float(total.max() - total.min()),
                      "host_to_host_s": float(np.median(whole)), "host_to_host_spread_s": float(max(whole) - min(whole)),
                      "peak_tflops": a.peak_tflops}))


if __name__ == "__main__":
    main()
