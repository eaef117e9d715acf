"""The signals on which the limiter's kernels are compared with tests/limiter_spec.py: on the CPU through the kernel text
compiled as host code (test_limiter_cpu.py) and on the GPU (test_gpu_limiter.py). All small.

The launches cut a signal into tiles of T = 2048 frames, a lane takes 8 consecutive frames, and the carry launch sweeps
units of ceil(tiles / 64) tiles: the lengths sit at a frame, at the tile's edge and just past it, and at 65 tiles and 5
frames, where a unit holds two tiles. The specification is evaluated whole, the kernels cut: equality is the test."""
import functools

import numpy as np

import limiter_spec as lim

T = lim.TILE
F32 = np.float32
CEILING = F32(10.0 ** (-1.0 / 20.0))  # -1 dBFS
RATES = (44100, 48000, 96000)
LENGTHS = {"1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3, "65T+5": 65 * T + 5}
SLOW_MS = 1000.0  # 2 or 1 units per frame at the rates above: the tent of a peak 6 dB over spans 16 tiles and more
KINDS = ("noise", "peak_first", "peak_last", "peak_edge", "slow_release", "slow_attack", "hidden", "all_over", "silence", "nan", "cap",
         "gain", "interleaved")


def signal(n: int, kind: str) -> np.ndarray:
    """(2, n) float32"""
    rng = np.random.default_rng([n, KINDS.index(kind)])
    x = (0.32 * rng.standard_normal((2, n))).astype(F32)  # about 1 % of the frames exceed -1 dBFS
    quiet = (0.01 * rng.standard_normal((2, n))).astype(F32)
    if kind in ("noise", "interleaved", "gain"):
        return x
    if kind == "silence":
        return np.zeros((2, n), F32)
    if kind == "all_over":
        return (np.sign(x) * (np.abs(x) + F32(1.0))).astype(F32)
    x = quiet
    if kind == "peak_first":
        x[0, 0] = 1.5
    elif kind == "peak_last":
        x[1, n - 1] = -1.7
    elif kind == "peak_edge":
        x[0, min(T - 1, n - 1)] = 1.9  # the last frame of tile 0, and the first of tile 1 on the other channel
        x[1, min(T, n - 1)] = -1.3
        x[0, min(7, n - 1)] = 1.2      # the last frame of a lane, and the first of the next
        x[1, min(8, n - 1)] = 1.25
        x[0, min(511, n - 1)] = 1.4    # the last frame of a wave, and the first of the next
        x[1, min(512, n - 1)] = -1.45
    elif kind == "slow_release":
        x[0, min(5, n - 1)] = 1.8      # its release runs over every tile behind it
    elif kind == "slow_attack":
        x[1, n - 1 - min(5, n - 1)] = -1.8
    elif kind == "hidden":
        x[0, n // 2] = 3.5
        x[1, min(n // 2 + 40, n - 1)] = 1.0  # over the ceiling, under the large one's release
        x[1, max(n // 2 - 30, 0)] = -0.95    # and under its attack
    elif kind == "nan":
        x[0, n // 3] = 2.0
        x[1, n // 3] = np.nan                # the same frame, the other channel
        x[0, min(n // 3 + 1, n - 1)] = np.nan
    elif kind == "cap":
        x[0, n // 2] = F32(2.0 ** 25)        # past 2^24 c
        x[1, min(n // 2 + 9, n - 1)] = np.inf
    return x


def params(kind: str):
    """(gain, ceiling, attack_ms, release_ms)"""
    if kind == "slow_release":
        return F32(1.0), CEILING, lim.ATTACK_MS, SLOW_MS
    if kind == "slow_attack":
        return F32(1.0), CEILING, SLOW_MS, lim.RELEASE_MS
    if kind == "gain":
        return F32(10.0 ** (7.3 / 20.0)), F32(0.5), 0.1, 10000.0  # the fastest attack, the slowest release
    return F32(1.0), CEILING, lim.ATTACK_MS, lim.RELEASE_MS


def cases(kinds=KINDS, lengths=LENGTHS):
    for kind in kinds:
        for name, n in lengths.items():
            yield f"{kind}/{name}", kind, n


@functools.lru_cache(maxsize=None)
def reference(kind: str, n: int, rate: int, true_peak: bool):
    """the specification's answer, computed once and shared; the arrays are read-only"""
    g, c, att, rel = params(kind)
    qa, qr = lim.slopes(rate, att, rel)
    x = signal(n, kind)
    r = lim.limit(x, c, qa, qr, g, true_peak, rate)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    r["x"], r["qa"], r["qr"] = x, qa, qr
    x.setflags(write=False)
    return r
