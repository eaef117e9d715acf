"""The multichannel Wiener post-filter on the GPU (csrc/wiener.hip): what its stages cost on a track.
Prints one JSON line.

A track of --seconds (240) of noise stems at 44.1 kHz, --sources (4) stereo sources, estimates = sources + 30 % noise:
  stages     dmx_wiener_device_timed on device memory, --reps times after one warm-up: the forward STFT, each EM launch and the
             inverse between HIP events; the median and the spread (max - min) of each and of their sum.
  bytes      what each stage must move through HBM with P = C T 2064 x 8 bytes per plane set: the STFT reads the (1 + J) C
             sample planes and writes (1 + J) P; the first EM launch reads X and E twice and writes y: (3 S + 2) P with
             S = J + residual; a later launch reads y twice, x once and writes y: (3 S + 1) P; the inverse reads J P and writes
             the J C sample planes. Reported as GB/s over the median time and as a fraction of --peak-gbs (8000).
  whole      binding.wiener host to host (allocation, copies and the kernels), --reps times.

    python tools/wiener_bench.py [--reps 10] [--seconds 240] [--sources 4] [--iterations 2] [--residual]
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
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--residual", action="store_true")
    ap.add_argument("--win-len", type=int, default=300)
    ap.add_argument("--peak-gbs", type=float, default=8000.0)
    a = ap.parse_args()
    import torch

    J, C, n, it, res = a.sources, 2, 44100 * a.seconds, a.iterations, int(a.residual)
    rng = np.random.default_rng(J)
    src = 0.1 * rng.standard_normal((J, C, n))
    ests = (src + 0.03 * rng.standard_normal((J, C, n))).astype(np.float32)
    mix = src.sum(axis=0).astype(np.float32)
    spec = dmx.WienerSpec(it, res, a.win_len)
    wbytes = dmx.wiener_workspace_bytes(spec, J, C, n)
    d_mix, d_ests = torch.from_numpy(mix).cuda(), torch.from_numpy(ests).cuda()
    d_out, work = torch.empty_like(d_ests), torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    stages = ["stft"] + [f"em{k}" for k in range(it)] + ["istft"]
    ms, rows = np.zeros(len(stages), np.float32), []
    for r in range(a.reps + 1):
        dmx._chk(dmx.lib().dmx_wiener_device_timed(0, d_mix.data_ptr(), d_ests.data_ptr(), J, C, n, n, ctypes.byref(spec), d_out.data_ptr(),
                                                   work.data_ptr(), wbytes, None, ms.ctypes.data))
        if r:
            rows.append(ms.copy())
    rows = np.array(rows, np.float64)
    med, spread, total = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0), rows.sum(axis=1)
    T, S = 1 + n // 1024, J + res
    P, planes = C * T * 2064 * 8, C * n * 4
    moved = [(1 + J) * (planes + P)] + [(3 * S + (2 if k == 0 else 1)) * P for k in range(it)] + [J * (P + planes)]
    whole = []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        out = dmx.wiener(mix, ests, it, bool(res), a.win_len)
        if r:
            whole.append(time.perf_counter() - t0)
    same = bool(np.array_equal(out, d_out.cpu().numpy()))
    print(json.dumps({"sources": J, "channels": C, "frames": n, "iterations": it, "residual": res, "win_len": a.win_len,
                      "workspace_gb": wbytes / 1e9, "device_equals_host_call": same,
                      **{k + "_ms": float(med[i]) for i, k in enumerate(stages)},
                      **{k + "_spread_ms": float(spread[i]) for i, k in enumerate(stages)},
                      **{k + "_gb": moved[i] / 1e9 for i, k in enumerate(stages)},
                      **{k + "_gbs": moved[i] / (med[i] * 1e-3) / 1e9 for i, k in enumerate(stages)},
                      **{k + "_of_peak": moved[i] / (med[i] * 1e-3) / 1e9 / a.peak_gbs for i, k in enumerate(stages)},
                      "total_ms": float(np.median(total)), "total_spread_ms": float(total.max() - total.min()),
                      "host_to_host_s": float(np.median(whole)), "host_to_host_spread_s": float(max(whole) - min(whole)),
                      "peak_gbs": a.peak_gbs}))


if __name__ == "__main__":
    main()
