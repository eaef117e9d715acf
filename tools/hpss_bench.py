"""Harmonic/percussive split on the GPU (csrc/hpss.hip): what its stages cost on a track.
Prints one JSON line per case.

A track of --seconds (240) of noise stems at 44.1 kHz, --sources (4) stereo stems, at the defaults (windows 31, 31, power 2,
margins 1, 1) and with the residual as a third output:
  stages     dmx_hpss_device_timed on device memory, --reps times after one warm-up: the forward STFT, the filter kernel (the
             one launch between its two events) and the inverses (one launch per kind of output) between HIP events; the
             median and the spread (max - min) of each and of their sum.
  floor      what the filter kernel must move: D read once and two fp32 mask planes written, over --peak-tbs (8.0, HBM); and
             what it must compute: per cell two medians of kMedianNet.ops = 274 v_min / v_max each (the selection network of
             hpss.hip) - the lane operations of the network alone, without the window's selects, the loads or the masks.
  whole      binding.hpss host to host (allocation, copies and the kernels), --reps times.

    python tools/hpss_bench.py [--reps 10] [--seconds 240] [--sources 4]
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

NETWORK_OPS = 274  # v_min_f32 / v_max_f32 of one median of 31 (csrc/hpss.hip: kMedianNet.ops)


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
    stages = ["stft", "filter", "inverses"]
    T = 1 + n // 1024
    cells = J * C * T * 2049
    for name, spec in (("defaults", dmx.HpssSpec()), ("residual", dmx.HpssSpec(residual=1))):
        K = 2 + spec.residual
        wbytes = dmx.hpss_workspace_bytes(spec, J, C, n)
        d_out, work = torch.empty((J, K, C, n), device="cuda"), torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        ms, rows = np.zeros(3, np.float32), []
        for r in range(a.reps + 1):
            dmx._chk(dmx.lib().dmx_hpss_device_timed(0, d_x.data_ptr(), J, C, n, n, ctypes.byref(spec), d_out.data_ptr(), n, work.data_ptr(),
                                                     wbytes, None, ms.ctypes.data))
            if r:
                rows.append(ms.copy())
        rows = np.array(rows, np.float64)
        med, spread, total = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0), rows.sum(axis=1)
        need = cells * (8 + 4 + 4)
        floor_ms = need / (a.peak_tbs * 1e12) * 1e3
        lane_ops = cells * 2 * NETWORK_OPS
        whole = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            out = dmx.hpss(x, spec)
            if r:
                whole.append(time.perf_counter() - t0)
        same = bool(np.array_equal(out, d_out.cpu().numpy()))
        print(json.dumps({"case": name, "sources": J, "channels": C, "samples": n, "frames": T, "kinds": K, "workspace_bytes": wbytes,
                          "device_equals_host_call": same,
                          **{k + "_ms": float(med[i]) for i, k in enumerate(stages)},
                          **{k + "_spread_ms": float(spread[i]) for i, k in enumerate(stages)},
                          "total_ms": float(np.median(total)), "total_spread_ms": float(total.max() - total.min()),
                          "filter_needed_gb": need / 1e9, "filter_hbm_floor_ms": floor_ms, "filter_of_hbm": floor_ms / float(med[1]),
                          "filter_cells": cells, "filter_network_lane_ops": lane_ops,
                          "filter_network_lane_ops_per_s": lane_ops / (float(med[1]) * 1e-3),
                          "host_to_host_s": float(np.median(whole)), "host_to_host_spread_s": float(max(whole) - min(whole)),
                          "peak_tbs": a.peak_tbs}), flush=True)
        del d_out, work


if __name__ == "__main__":
    main()
