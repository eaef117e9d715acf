"""Time stretch and pitch shift on the GPU (csrc/stretch.hip): what its stages cost on a track.
Prints one JSON line per case.

A track of --seconds (240) of noise stems at 44.1 kHz, --sources (4) stereo stems, at the rates 4/5 and 5/4 and one semitone
up at the tempo 1 (dmx_stretch_ratio(2^(1/12), 512)):
  stages     dmx_stretch_device_timed on device memory, --reps times after one warm-up: the forward STFT (with the flags of the
             all-zero frames), the phasor products with the carry, the vocoder fused into the inverse and the converter between
             HIP events; the median and the spread (max - min) of each and of their sum.
  bytes      what the launches must move: the products read the rows of D that some output frame uses once (all at a rate of
             1 or below) and write a complex128 row per plane and range; the fused inverse reads those rows of D once, a carry
             row per plane and chunk, and writes the samples. The shares of --peak-tbs (8.0, HBM) are these bytes over the
             stage's time; the products' stage holds the carry launch as well, so its share is a lower bound for the kernel.
  whole      binding.stretch host to host (allocation, copies and the kernels), --reps times.
  cents      the largest error of dmx_stretch_ratio(2^(s / 12), 512) over s = +-1 .. 12, in cents (no GPU).

    python tools/stretch_bench.py [--reps 10] [--seconds 240] [--sources 4]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from demucs_cpp_amd import binding as dmx  # noqa: E402


def ratio_cents():
    worst = 0.0
    for s in list(range(-12, 0)) + list(range(1, 13)):
        p, q = dmx.stretch_ratio(2.0 ** (s / 12.0), 512)
        worst = max(worst, abs(1200.0 * math.log2(p / q) - 100.0 * s))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=240)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    a = ap.parse_args()
    import torch

    J, C, n = a.sources, 2, 44100 * a.seconds
    rng = np.random.default_rng(J)
    x = (0.1 * rng.standard_normal((J, C, n))).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    p, q = dmx.stretch_ratio(2.0 ** (1.0 / 12.0), 512)
    cents = ratio_cents()
    stages = ["stft", "products_carry", "vocoder_istft", "converter"]
    for name, spec in (("4/5", dmx.StretchSpec(4, 5)), ("5/4", dmx.StretchSpec(5, 4)), ("semitone_up", dmx.StretchSpec(q, p, p, q))):
        wbytes, m = dmx.stretch_workspace_bytes(spec, J, C, n), dmx.stretch_length(spec, n)
        d_out, work = torch.empty((J, C, m), device="cuda"), torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        ms, rows = np.zeros(4, np.float32), []
        for r in range(a.reps + 1):
            dmx._chk(dmx.lib().dmx_stretch_device_timed(0, d_x.data_ptr(), J, C, n, n, ctypes.byref(spec), d_out.data_ptr(), m, work.data_ptr(),
                                                        wbytes, None, ms.ctypes.data))
            if r:
                rows.append(ms.copy())
        rows = np.array(rows, np.float64)
        med, spread, total = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0), rows.sum(axis=1)
        T, n2 = 1 + n // 1024, -(-n * spec.den // spec.num)
        T2 = 1 + n2 // 1024
        chunks = -(-T2 // 12)
        used = len({t * spec.num // spec.den + d for t in range(T2) for d in (0, 1)} & set(range(T)))  # rows some frame reads
        d_bytes, carry_bytes = J * C * used * 2049 * 8, J * C * chunks * 2049 * 16
        need1, need3 = d_bytes + carry_bytes, d_bytes + carry_bytes + J * C * n2 * 4
        whole = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            out = dmx.stretch(x, spec)
            if r:
                whole.append(time.perf_counter() - t0)
        same = bool(np.array_equal(out, d_out.cpu().numpy()))
        print(json.dumps({"case": name, "sources": J, "channels": C, "frames_in": n, "frames_out": m, "num": spec.num, "den": spec.den,
                          "pitch_num": spec.pitch_num, "pitch_den": spec.pitch_den, "workspace_gb": wbytes / 1e9,
                          "device_equals_host_call": same,
                          **{k + "_ms": float(med[i]) for i, k in enumerate(stages)},
                          **{k + "_spread_ms": float(spread[i]) for i, k in enumerate(stages)},
                          "products_needed_gb": need1 / 1e9, "vocoder_istft_needed_gb": need3 / 1e9,
                          "products_carry_of_hbm": need1 / (med[1] * 1e-3) / 1e12 / a.peak_tbs,
                          "vocoder_istft_of_hbm": need3 / (med[2] * 1e-3) / 1e12 / a.peak_tbs,
                          "total_ms": float(np.median(total)), "total_spread_ms": float(total.max() - total.min()),
                          "host_to_host_s": float(np.median(whole)), "host_to_host_spread_s": float(max(whole) - min(whole)),
                          "ratio_worst_cents": cents, "peak_tbs": a.peak_tbs}), flush=True)
        del d_out, work


if __name__ == "__main__":
    main()
