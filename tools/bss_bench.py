"""BSS Eval v4 on the GPU (csrc/bss.hip): what its six stages cost on a track. Prints one JSON line.

A track of --seconds (240) of noise stems at 44.1 kHz, --sources (4) stereo sources, estimates = references + a little of the
other sources + noise, museval's defaults (1 s windows, 512 taps):
  stages     dmx_bss_eval_device_timed on device memory, --reps times after one warm-up: gram, fill, cholesky, solve, project and
             windows between HIP events; the median and the spread (max - min) of each and of their sum.
  rates      the binary64 operations the algorithm needs (not the padded MFMA tiles' work): gram 2 (J C) (2 J C) L n, project
             2 (J C) (J C L + C L) n, over the median time, and as a fraction of --peak-tflops (78.6: half the fp32 MFMA peak of
             BASELINE.md, AMD's published binary64 matrix figure). The Gram kernel pads the J C reference planes to the 16 rows of a tile and the projection
             computes the own-source filters as a block-diagonal matrix of the full order, so at J C = 8 the tiles do 2 x and
             3.2 x these operations.

    python tools/bss_bench.py [--reps 20] [--seconds 240] [--sources 4]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from demucs_cpp_amd import binding as dmx  # noqa: E402

STAGES = ("gram", "fill", "cholesky", "solve", "project", "windows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=240)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--filters-len", type=int, default=512)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    a = ap.parse_args()
    import torch

    J, C, L, n = a.sources, 2, a.filters_len, 44100 * a.seconds
    rng = np.random.default_rng(J)
    refs = (0.1 * rng.standard_normal((J, C, n))).astype(np.float32)
    ests = (refs + 0.05 * refs[::-1] + 0.03 * rng.standard_normal((J, C, n))).astype(np.float32)
    spec = dmx.BssSpec(44100, 44100, L)
    nwin, wbytes = dmx.bss_windows(n, 44100, 44100), dmx.bss_eval_workspace_bytes(J, C, n, L)
    d_refs, d_ests = torch.from_numpy(refs).cuda(), torch.from_numpy(ests).cuda()
    work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    metrics = torch.zeros((4, J, nwin), dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ms, rows = np.zeros(6, np.float32), []
    for r in range(a.reps + 1):
        rc = dmx.lib().dmx_bss_eval_device_timed(0, d_refs.data_ptr(), d_ests.data_ptr(), J, C, n, n, ctypes.byref(spec), metrics.data_ptr(),
                                                 status.data_ptr(), None, work.data_ptr(), None, ms.ctypes.data)
        if rc != 0:
            raise RuntimeError(dmx.lib().dmx_last_error().decode())
        if r:
            rows.append(ms.copy())
    rows = np.array(rows, np.float64)
    med, spread, total = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0), rows.sum(axis=1)
    flop = {"gram": 2.0 * (J * C) * (2 * J * C) * L * n, "project": 2.0 * (J * C) * (J * C * L + C * L) * n}
    m = metrics.cpu().numpy()
    print(json.dumps({"sources": J, "channels": C, "frames": n, "filters_len": L, "order": J * C * L, "windows": nwin,
                      "workspace_gb": wbytes / 1e9, "status": int(status.item()),
                      "median_db": {k: [float(v) for v in np.nanmedian(m[i], axis=1)] for i, k in enumerate(("sdr", "isr", "sir", "sar"))},
                      **{k + "_ms": float(med[i]) for i, k in enumerate(STAGES)}, **{k + "_spread_ms": float(spread[i]) for i, k in enumerate(STAGES)},
                      "total_ms": float(np.median(total)), "total_spread_ms": float(total.max() - total.min()),
                      **{k + "_tflops": flop[k] / (med[STAGES.index(k)] * 1e-3) / 1e12 for k in flop},
                      **{k + "_of_peak": flop[k] / (med[STAGES.index(k)] * 1e-3) / 1e12 / a.peak_tflops for k in flop},
                      "peak_tflops": a.peak_tflops}))


if __name__ == "__main__":
    main()
