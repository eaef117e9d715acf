"""The loudness stage (csrc/loudness.hip): what the measurement costs beside the peak kernel that
reads the same samples, and what the stage adds to the 16-bit output of a 4-minute track. Prints one JSON line.

For a 4-minute stereo track of 0.1 N(0,1) noise at 44.1 kHz and at 48 kHz:
  launches   dmx_loudness_device_timed on device memory, --reps times after one warm-up: the four launches (states, scan,
             energies, final) and the peak kernel on the same signal between HIP events; the median of each, and the ratio of
             the loudness launches' sum to the peak kernel. The design reads the planes twice where the peak kernel reads
             them once: the ratio's floor is about 2.
  stems      host to host, 4 stems as 16-bit PCM (identity gains, clip rescale): dmx_remix_encode (loudness off) and
             dmx_loud_encode under MEASURE, MIXTURE and EACH, ALTERNATING inside every repetition; medians and the spread
             (max - min) of each. The times include the upload of the stems and the download of the bytes, which dominate.

    python tools/loudness_bench.py [--reps 7] [--seconds 240]
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
    work = torch.zeros(dmx.loudness_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    res = torch.zeros(16, dtype=torch.uint8, device="cuda")
    ms = np.zeros(5, np.float32)
    rows = []
    for r in range(reps + 1):
        rc = dmx.lib().dmx_loudness_device_timed(0, x.data_ptr(), n, n, rate, res.data_ptr(), None, work.data_ptr(), None, ms.ctypes.data)
        if rc != 0:
            raise RuntimeError(dmx.lib().dmx_last_error().decode())
        if r:
            rows.append(ms.copy())
    med = np.median(np.array(rows), axis=0)
    lufs_c = int(res.cpu().numpy().view(dmx.LOUDNESS_DTYPE)[0]["lufs_c"])
    return {"rate": rate, "frames": n, "lufs_c": lufs_c, "states_ms": float(med[0]), "scan_ms": float(med[1]), "energies_ms": float(med[2]),
            "final_ms": float(med[3]), "loudness_ms": float(med[:4].sum()), "peak_ms": float(med[4]),
            "ratio_to_peak": float(med[:4].sum() / med[4]), "workspace_bytes": dmx.loudness_workspace_bytes(n)}


def stems(rate, seconds, reps):
    n = rate * seconds
    rng = np.random.default_rng(rate + 1)
    v = (0.05 * rng.standard_normal((4, 2, n))).astype(np.float32)
    mix = v.sum(axis=0).astype(np.float32)
    spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_RESCALE)
    legs = {"off": lambda: dmx.remix_encode(v, mix, spec)}
    for name, mode in (("measure", dmx.LOUD_MEASURE), ("mixture", dmx.LOUD_MIXTURE), ("each", dmx.LOUD_EACH)):
        legs[name] = (lambda m: lambda: dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(m, -14.0), rate))(mode)
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=int, default=240)
    a = ap.parse_args()
    out = {"launches": [launches(r, a.seconds, a.reps) for r in (44100, 48000)],
           "stems": [stems(r, a.seconds, a.reps) for r in (44100, 48000)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
