"""The meters (csrc/meters.hip): what the true-peak kernel costs beside the peak kernel that reads the
same samples, what the meters launch costs, and what the true-peak ceiling and a meters report add to the 16-bit output
of a 4-minute track. Prints one JSON line.

For a 4-minute stereo track of 0.1 N(0,1) noise at 44.1 kHz (F = 4) and at 96 kHz (F = 2):
  launches   dmx_meters_device_timed on device memory, --reps times after one warm-up: the true-peak launch, the peak kernel
             on the same signal and the meters launch between HIP events; the median and the spread (max - min) of each,
             and the ratio of the true-peak launch to the peak kernel. Both read the planes once: the ratio's floor is 1.
  stems      host to host, 4 stems as 16-bit PCM (identity gains, clip rescale): dmx_loud_encode under MIXTURE (the call as
             it was) and dmx_loud_encode_meters under MIXTURE | TRUE_PEAK with a meters report, ALTERNATING inside every
             repetition; medians and the spread of each. The times include the upload of the stems and the download of
             the bytes, which dominate.

    python tools/meters_bench.py [--reps 5] [--seconds 240]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from demucs_cpp_amd import binding as dmx  # noqa: E402


def launches(rate, seconds, reps):
    import torch

    n = rate * seconds
    rng = np.random.default_rng(rate)
    x = torch.from_numpy((0.1 * rng.standard_normal((2, n))).astype(np.float32)).cuda()
    work = torch.zeros(dmx.loudness_workspace_bytes(n) + dmx.meters_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    ms = np.zeros(3, np.float32)
    rows = []
    for r in range(reps + 1):
        rc = dmx.lib().dmx_meters_device_timed(0, x.data_ptr(), n, n, rate, work.data_ptr(), None, ms.ctypes.data)
        if rc != 0:
            raise RuntimeError(dmx.lib().dmx_last_error().decode())
        if r:
            rows.append(ms.copy())
    rows = np.array(rows)
    med, spread = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0)
    return {"rate": rate, "frames": n, "factor": dmx.true_peak_filter(rate)[0],
            "true_peak_ms": float(med[0]), "true_peak_spread_ms": float(spread[0]), "peak_ms": float(med[1]), "peak_spread_ms": float(spread[1]),
            "meters_ms": float(med[2]), "meters_spread_ms": float(spread[2]), "ratio_to_peak": float(med[0] / med[1]),
            "plane_gb_per_s": float(8.0 * n / med[0] / 1e6)}


def stems(rate, seconds, reps):
    n = rate * seconds
    rng = np.random.default_rng(rate + 1)
    v = (0.05 * rng.standard_normal((4, 2, n))).astype(np.float32)
    mix = v.sum(axis=0).astype(np.float32)
    spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_RESCALE)
    legs = {"mixture": lambda: dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(dmx.LOUD_MIXTURE, -14.0), rate),
            "mixture_true_peak_meters": lambda: dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(dmx.LOUD_MIXTURE, -14.0, true_peak=True), rate,
                                                                meters=True)}
    for f in legs.values():
        f()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    return {"rate": rate, "frames": n,
            **{k + "_s": {"median": float(np.median(t)), "spread": float(max(t) - min(t))} for k, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=int, default=240)
    a = ap.parse_args()
    out = {"launches": [launches(r, a.seconds, a.reps) for r in (44100, 96000)],
           "stems": [stems(r, a.seconds, a.reps) for r in (44100, 96000)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
