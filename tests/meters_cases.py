"""The signals on which the meters' kernels are compared with tests/meters_spec.py: on the CPU through the kernel text
compiled as host code (test_meters_cpu.py) and on the GPU (test_gpu_meters.py). All small.

The true-peak kernel cuts a signal into tiles of T = 2048 frames at multiples of T, each staged with a halo of 6 frames:
the lengths sit at the halo, at the tile's edge and just past it. The hop meters have blocks of 4 and of 30 hops: the
lengths sit one frame under and at the first block of each."""
import numpy as np

import loudness_spec as ls
import meters_spec as ms

T = 2048  # kTpTile
TP_RATES = (8000, 44100, 48000, 96000)
TP_SIGNALS = ("lowpass", "impulse_edge", "impulse_ends", "tone45", "silence", "nan", "interleaved")
HOP_RATES = (8000, 44100, 48000, 96000)
HOP_SIGNALS = ("noise", "silence", "down15", "lf_dc", "impulse", "nan", "interleaved", "step15", "amp100", "amp1e-5")

# (rate, length name, signal) -> seed, where seed 0 fails meters_spec.fixture_ok; found on the CPU by search(), fixed here
SEEDS = {
    (8000, '6s', 'down15'): 1,
    (8000, '30h-1', 'interleaved'): 1,
    (44100, '30h-1', 'noise'): 2,
    (44100, '31h-1', 'step15'): 1,
    (44100, '30h-1', 'amp100'): 1,
    (44100, '6s', 'amp100'): 2,
    (48000, '30h', 'silence'): 1,
    (48000, '6s', 'amp100'): 1,
    (96000, '30h', 'down15'): 1,
    (96000, '30h-1', 'interleaved'): 1,
    (96000, '30h', 'amp1e-5'): 1,
}


def tp_lengths(fs: int):
    return {"1": 1, "5": 5, "6": 6, "7": 7, "12": 12, "13": 13, "T-6": T - 6, "T-1": T - 1, "T": T, "T+1": T + 1, "T+6": T + 6,
            "T+7": T + 7, "2T+3": 2 * T + 3, "3s": 3 * fs}


def tp_signal(fs: int, n: int, kind: str) -> np.ndarray:
    """(2, n) float32"""
    if kind in ("lowpass", "nan", "interleaved"):
        for seed in range(64):  # the first seed whose largest value lies between the samples (from 12 frames on one exists)
            w = np.random.default_rng([fs, n, TP_SIGNALS.index(kind), seed]).standard_normal((2, n + 7))
            x = (0.1 * sum(w[:, k:n + k] for k in range(8))).astype(np.float32)  # white noise through a moving average of 8
            if n < 12 or ms.true_peak(x, fs)[1] != 0:
                break
        if kind == "nan":
            x[1, n // 3] = np.nan
        return x
    x = np.zeros((2, n), np.float32)
    if kind == "impulse_edge":
        x[0, min(T - 1, n - 1)] = 1.0  # its response lies in the next tile's halo
        x[1, min(T, n - 1)] = -0.75
    elif kind == "impulse_ends":
        x[0, 0] = 0.5
        x[1, n - 1] = -1.0
    elif kind == "tone45":
        t = np.arange(n)
        x[:] = (0.5 * np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0)).astype(np.float32)
    return x


def tp_cases(fs: int, kind: str):
    for name, n in tp_lengths(fs).items():
        yield name, n, tp_signal(fs, n, kind)


def hop_lengths(fs: int):
    h = ls.hop(fs)
    return {"4h-1": 4 * h - 1, "4h": 4 * h, "30h-1": 30 * h - 1, "30h": 30 * h, "31h-1": 31 * h - 1, "6s": 6 * fs}


def hop_signal(fs: int, name: str, n: int, kind: str) -> np.ndarray:
    """(2, n) float32: the signals of loudness_cases (with a floor of -140 dBFS where those are digital silence, and more noise on
    the low-frequency one, so that a seed can meet the fixture's condition), a level step of -15 dB at a third of the signal,
    amplitude 100 (the top bin's clamp) and amplitude 1e-5 (everything under the absolute gate)"""
    rng = np.random.default_rng([fs, n, HOP_SIGNALS.index(kind), SEEDS.get((fs, name, kind), 0)])
    x = (0.1 * rng.standard_normal((2, n))).astype(np.float32)  # noise at -20 dBFS
    a, b = n // 3, 2 * n // 3
    if kind == "silence":
        x[:, a:b] *= np.float32(1e-6)  # not digital silence: the filter's tail would decay through the subnormal energies
    elif kind == "down15":
        x[:, a:b] *= np.float32(10.0 ** (-15.0 / 20.0))
    elif kind == "step15":
        x[:, a:] *= np.float32(10.0 ** (-15.0 / 20.0))
    elif kind == "amp100":
        x *= np.float32(1000.0)
        x[:, a:] *= np.float32(10.0 ** (-15.0 / 20.0))
    elif kind == "amp1e-5":
        x *= np.float32(1e-4)
    elif kind == "lf_dc":
        t = np.arange(n) / fs
        x[0] = (0.5 * np.sin(2 * np.pi * 20.0 * t) + 0.25).astype(np.float32)
        x[1] = (0.4 * np.cos(2 * np.pi * 20.0 * t) - 0.125).astype(np.float32) + x[1] * np.float32(0.05)
    elif kind == "impulse":
        x *= np.float32(1e-6)  # a floor, as under "silence"
        x[0, min((n // 2) // 64 * 64 + 63, n - 1)] = 1.0
        x[1, 63] = -0.5
    elif kind == "nan":
        x[1, n // 3] = np.nan
    return x


def hop_cases(fs: int, kind: str):
    for name, n in hop_lengths(fs).items():
        yield name, n, hop_signal(fs, name, n, kind)


# ---- the stage: S = 4 stems and their mixture under four rows of gains
STAGE_FS = 8000
STAGE_N = 31 * 800 + 3  # 31 hops and an odd tail: 28 momentary and 2 short-term blocks, 13 true-peak tiles
STAGE_SEED = 0  # found by stage_search(): every measured signal meets the fixtures' conditions


def stage_rows(S: int = 4) -> np.ndarray:
    """stem 0, stem 1, the other stems added (stem 0's plane is not read), mixture - stem 0"""
    g = np.zeros((4, S + 1), np.float32)
    g[0, 0] = 1
    g[1, 1] = 1
    g[2, 1:S] = 1
    g[3, 0], g[3, S] = -1, 1
    return g


def stage_inputs(seed: int = None, S: int = 4, n: int = STAGE_N):
    """(v (S, 2, n), mix (2, n)): low-passed noise at different levels, the first third 15 dB up"""
    rng = np.random.default_rng([S, n, STAGE_SEED if seed is None else seed])
    level = np.array([0.2, 0.05, 0.1, 0.02, 0.15, 0.08], np.float32)[:S]
    w = rng.standard_normal((S, 2, n + 3))
    v = (level[:, None, None] * 0.5 * (w[:, :, 0:n] + w[:, :, 1:n + 1] + w[:, :, 2:n + 2] + w[:, :, 3:n + 3])).astype(np.float32)
    v[:, :, n // 3:] *= np.float32(10.0 ** (-15.0 / 20.0))
    mix = (v.sum(axis=0) + 0.01 * rng.standard_normal((2, n))).astype(np.float32)
    return v, mix


def stage_signals(v, mix, g):
    import remix_spec as rs
    return list(rs.outputs(v, mix, g)) + [mix]


def check_stage_fixture(v, mix, g, fs):
    import loudness_cases as lc
    for x in stage_signals(v, mix, g):
        lc.check_fixture(x, fs)
        check_fixture(x, fs)


def stage_search():
    for seed in range(100):
        v, mix = stage_inputs(seed)
        try:
            check_stage_fixture(v, mix, stage_rows(), STAGE_FS)
        except AssertionError:
            continue
        print("STAGE_SEED =", seed)
        return


def check_fixture(x: np.ndarray, fs: int):
    """the condition of a fixture: a failure is a bad fixture (choose another seed), never a reason to skip"""
    why = ms.fixture_ok(x, fs)
    assert why is None, f"bad fixture: {why}"


def search():
    """prints the SEEDS entries that the cases need"""
    for fs in HOP_RATES:
        for kind in HOP_SIGNALS:
            for name, n in hop_lengths(fs).items():
                for seed in range(100):
                    SEEDS[(fs, name, kind)] = seed
                    if ms.fixture_ok(hop_signal(fs, name, n, kind), fs) is None:
                        break
                else:
                    print(f"    # no seed for ({fs}, {name!r}, {kind!r})")
                if seed:
                    print(f"    ({fs}, {name!r}, {kind!r}): {seed},")
                else:
                    del SEEDS[(fs, name, kind)]


if __name__ == "__main__":
    search()
    stage_search()
