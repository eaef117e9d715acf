"""The look-ahead peak limiter (csrc/limiter.hip): what its launches cost beside the peak kernel that
reads the same samples. Prints one JSON line.

For a 4-minute stereo track of noise at 44.1 kHz and at 96 kHz, scaled so that about 1 % of the frames exceed the ceiling of
-1 dBFS, with the sample level and with the true-peak level (F = 4 resp. 2):
  launches   dmx_limit_device_timed on device memory, --reps times after one warm-up: detect, carry, envelope and (true peak)
             the limited signal's true-peak launch between HIP events, and the peak kernel on the same signal; the median and
             the spread (max - min) of each, and the ratio of the three limiter launches to the peak kernel. The floor: two
             reads of the planes (16 bytes per frame) and one write and one read of M and one write of the gain plane (12 bytes
             per frame) against the peak kernel's one read of the planes (8 bytes per frame): a ratio of 3.5.
  stems      host to host, 4 stems as 16-bit PCM (identity gains, clip rescale, target -1 LUFS under -1 dBFS, which the noise then exceeds): dmx_loud_encode
             under MIXTURE (the call as it was: the ceiling lowers the gain) and dmx_loud_encode_limit under MIXTURE | LIMIT,
             ALTERNATING inside every repetition; medians and the spread of each, the gains and what was limited. The times
             include the upload of the stems and the download of the bytes, which dominate.

    python tools/limiter_bench.py [--reps 5] [--seconds 240]
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

CEILING = 10.0 ** (-1.0 / 20.0)


def launches(rate, seconds, reps, true_peak):
    import torch

    n = rate * seconds
    rng = np.random.default_rng(rate)
    h = (0.32 * rng.standard_normal((2, n))).astype(np.float32)
    x = torch.from_numpy(h).cuda()
    work = torch.zeros(dmx.limiter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    res = torch.zeros(dmx.LIMIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ms = np.zeros(5, np.float32)
    rows = []
    for r in range(reps + 1):
        rc = dmx.lib().dmx_limit_device_timed(0, x.data_ptr(), n, n, rate, 1.0, CEILING, int(true_peak), None, res.data_ptr(), work.data_ptr(),
                                              None, ms.ctypes.data)
        if rc != 0:
            raise RuntimeError(dmx.lib().dmx_last_error().decode())
        if r:
            rows.append(ms.copy())
    rows = np.array(rows)
    med, spread = np.median(rows, axis=0), rows.max(axis=0) - rows.min(axis=0)
    out = np.frombuffer(res.cpu().numpy().tobytes(), dmx.LIMIT_DTYPE)[0]
    three = rows[:, :3].sum(axis=1)
    names = ("detect", "carry", "envelope", "true_peak_out", "peak")
    return {"rate": rate, "frames": n, "true_peak": bool(true_peak), "over_ceiling": float((np.abs(h).max(axis=0) > CEILING).mean()),
            "limited_frames": int(out["limited_frames"]), "max_reduction_db": float(out["max_reduction"]) / 65536 * 6.0206,
            **{k + "_ms": float(med[i]) for i, k in enumerate(names)}, **{k + "_spread_ms": float(spread[i]) for i, k in enumerate(names)},
            "limiter_ms": float(np.median(three)), "limiter_spread_ms": float(three.max() - three.min()),
            "ratio_to_peak": float(np.median(three) / med[4]), "floor_gb_per_s": float(28.0 * n / np.median(three) / 1e6)}


def stems(rate, seconds, reps):
    n = rate * seconds
    rng = np.random.default_rng(rate + 1)
    v = (0.05 * rng.standard_normal((4, 2, n))).astype(np.float32)
    mix = v.sum(axis=0).astype(np.float32)
    spec = dmx.RemixSpec(np.eye(4, 5, dtype=np.float32), dmx.PCM_S16, dmx.CLIP_RESCALE)
    legs = {"mixture": lambda: dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(dmx.LOUD_MIXTURE, -1.0), rate),
            "mixture_limit": lambda: dmx.loud_encode(v, mix, spec, dmx.LoudnessSpec(dmx.LOUD_MIXTURE, -1.0, limit=True), rate, limit_report=True)}
    last = {k: f() for k, f in legs.items()}
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    lrep = last["mixture_limit"][3]
    return {"rate": rate, "frames": n, "gain_capped": float(last["mixture"][2]["gain"][0]), "gain_limited": float(last["mixture_limit"][2]["gain"][0]),
            "limited_frames": int(lrep["limited_frames"][0]), "max_reduction_db": float(lrep["max_reduction"][0]) / 65536 * 6.0206,
            "peak_out": float(lrep["peak_out"].max()),
            **{k + "_s": {"median": float(np.median(t)), "spread": float(max(t) - min(t))} for k, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=int, default=240)
    a = ap.parse_args()
    assert ctypes.sizeof(dmx.LimitResult) == dmx.LIMIT_DTYPE.itemsize
    print(json.dumps({"launches": [launches(r, a.seconds, a.reps, tp) for r in (44100, 96000) for tp in (False, True)],
                      "stems": [stems(r, a.seconds, a.reps) for r in (44100, 96000)]}))


if __name__ == "__main__":
    main()
