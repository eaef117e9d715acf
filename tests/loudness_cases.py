"""The signals on which the loudness kernels are compared with tests/loudness_spec.py: on the CPU through the kernel text
compiled as host code (test_loudness_cpu.py) and on the GPU (test_gpu_loudness.py). Rates x lengths x signals, all small.

The kernels cut a signal into lane chunks of 64 frames, 64 of them to a wave and a workgroup tile (4096 frames), and the
second-level scan gives each of its 64 lanes a unit of ceil(tiles / 64) tiles: the lengths sit one frame under and over
multiples of each, and 3 s spans several tiles and units at every rate (at 96 kHz it is 71 tiles: units of 2 tiles)."""
import math

import numpy as np

import loudness_spec as ls

RATES = (8000, 11025, 44100, 48000, 96000)
SIGNALS = ("noise", "silence", "down15", "lf_dc", "impulse", "nan", "interleaved")
CHUNK, TILE = 64, 4096

# (rate, length name, signal) -> seed, where seed 0 leaves 100 L within 0.001 of a half-integer or a block within 1e-6 of a
# gate; found on the CPU by tests/loudness_cases.py's search(), fixed here
SEEDS = {}


def lengths(fs: int):
    h = ls.hop(fs)
    m = -(-(9 * h // 2) // CHUNK) * CHUNK
    M = -(-(9 * h // 2) // TILE) * TILE
    return {"4h-1": 4 * h - 1, "4h": 4 * h, "5h-1": 5 * h - 1, "3s": 3 * fs, "chunk-1": m - 1, "chunk+1": m + 1, "tile-1": M - 1,
            "tile+1": M + 1}


def signal(fs: int, name: str, n: int, kind: str) -> np.ndarray:
    """(2, n) float32"""
    rng = np.random.default_rng([fs, n, SIGNALS.index(kind), SEEDS.get((fs, name, kind), 0)])
    x = (0.1 * rng.standard_normal((2, n))).astype(np.float32)  # noise at -20 dBFS
    a, b = n // 3, 2 * n // 3
    if kind == "silence":
        x[:, a:b] = 0.0
    elif kind == "down15":
        x[:, a:b] *= np.float32(10.0 ** (-15.0 / 20.0))
    elif kind == "lf_dc":
        t = np.arange(n) / fs
        x[0] = (0.5 * np.sin(2 * np.pi * 20.0 * t) + 0.25).astype(np.float32)
        x[1] = (0.4 * np.cos(2 * np.pi * 20.0 * t) - 0.125).astype(np.float32) + x[1] * np.float32(1e-3)
    elif kind == "impulse":
        x[:] = 0.0
        x[0, min((n // 2) // CHUNK * CHUNK + CHUNK - 1, n - 1)] = 1.0  # the last frame of a lane's chunk
        x[1, CHUNK - 1] = -0.5
    elif kind == "nan":
        x[1, n // 3] = np.nan
    return x


def cases(fs: int, kind: str):
    for name, n in lengths(fs).items():
        yield name, n, signal(fs, name, n, kind)


def check_fixture(x: np.ndarray, fs: int):
    """the condition of a fixture: a failure is a bad fixture (choose another seed), never a reason to skip"""
    d, m = ls.fixture_margin(x, fs)
    assert d >= 0.001, f"bad fixture: 100 L lies {d:.6f} from a half-integer"
    assert m >= 1e-6, f"bad fixture: a block's energy lies within {m:.3e} of a gate"


def compare_with_spec(L, c, e, x, fs):
    Ls, cs, es = ls.measure(x, fs)
    assert c == cs, (c, cs, L, Ls)
    assert e.shape == es.shape
    if cs == ls.UNMEASURABLE:
        assert math.isnan(L)
    else:
        assert abs(L - Ls) <= 1e-6, (L, Ls)
    # a NaN stays in its channel's filter from its hop on: the same hops are NaN, and every finite one is held to the bound
    assert np.array_equal(np.isnan(e), np.isnan(es))
    fin = ~np.isnan(es)
    for c in range(2):
        if fin[c].any():
            bound = 1e-9 * es[c][fin[c]].max()
            err = np.abs(e[c][fin[c]] - es[c][fin[c]])
            assert (err <= bound).all(), (c, float(err.max() / max(bound, 1e-300)))


def search():
    """prints the SEEDS entries that the cases need"""
    for fs in RATES:
        for kind in SIGNALS:
            for name, n in lengths(fs).items():
                for seed in range(100):
                    SEEDS[(fs, name, kind)] = seed
                    d, m = ls.fixture_margin(signal(fs, name, n, kind), fs)
                    if d >= 0.002 and m >= 1e-5:
                        break
                if seed:
                    print(f"    ({fs}, {name!r}, {kind!r}): {seed},")
                else:
                    del SEEDS[(fs, name, kind)]


if __name__ == "__main__":
    search()
