"""The loudness stage's specification (csrc/loudness.hip), restated in NumPy binary64.

Integrated loudness after ITU-R BS.1770-4 of a stereo signal x[2][n] of fp32 samples at fs Hz: the K-weighting as two
biquads whose coefficients are computed for the rate (math.tan / math.pow: the host's libm, as the library does), 400 ms
blocks at 75 % overlap built from 100 ms hop energies, the absolute gate at -70 LUFS and the relative gate 10 LU under
the mean of the absolutely gated blocks. The result is quantised to hundredths of a LU (`lufs_c`); the gain, the ceiling
and the applied bytes are functions of that integer, so they are reproducible whatever the order of the device's sums.

A gate EXCLUDES a block whose loudness is <= its threshold: a block whose energy is NaN is therefore kept, makes L NaN
and the signal unmeasurable - one NaN anywhere in the signal does that, since it stays in the filter's state.
"""
import math

import numpy as np

UNMEASURABLE = -(2 ** 31)  # INT32_MIN
MEASURE, MIXTURE, EACH = 0, 1, 2
MIN_RATE = 4000


def coefficients(fs: int) -> np.ndarray:
    """[b0 b1 b2 a1 a2] of the shelf, then of the high-pass (whose b is 1 -2 1, not normalised): 10 doubles"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
          (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    s2 = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(s1 + s2, np.float64)


def _biquad(b, a, x):
    """sequential, from zero state, binary64 (transposed direct form II, as scipy.signal.lfilter evaluates it)"""
    try:
        from scipy.signal import lfilter
        return lfilter(b, a, x)
    except ImportError:
        y = np.empty_like(x)
        s1 = s2 = 0.0
        b0, b1, b2 = (float(v) for v in b)
        a1, a2 = float(a[1]), float(a[2])
        for i, v in enumerate(x.tolist()):
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            y[i] = o
        return y


def hop(fs: int) -> int:
    return (fs + 5) // 10


def hop_energies(x: np.ndarray, fs: int) -> np.ndarray:
    """x [2][n] -> e[2][H]"""
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[0] == 2
    k = coefficients(fs)
    h = hop(fs)
    H = x.shape[1] // h
    e = np.zeros((2, H), np.float64)
    for c in range(2):
        y = _biquad(k[0:3], np.array([1.0, k[3], k[4]]), x[c].astype(np.float64))
        y = _biquad(k[5:8], np.array([1.0, k[8], k[9]]), y)
        with np.errstate(over="ignore", invalid="ignore"):
            e[c] = (y[:H * h].reshape(H, h) ** 2).sum(axis=1)
    return e


def block_energies(e: np.ndarray, h: int) -> np.ndarray:
    H = e.shape[1]
    if H < 4:
        return np.zeros(0, np.float64)
    s = e[0] + e[1]
    return (s[0:H - 3] + s[1:H - 2] + s[2:H - 1] + s[3:H]) / (4.0 * h)


def integrated(e: np.ndarray, h: int):
    """(L, lufs_c, z, absolute threshold in z, relative threshold in z); L is NaN and lufs_c UNMEASURABLE when unmeasurable"""
    z = block_energies(e, h)
    nan = float("nan")
    if z.size == 0:
        return nan, UNMEASURABLE, z, nan, nan
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
        keep = ~(l <= -70.0)
        if not keep.any():
            return nan, UNMEASURABLE, z, nan, nan
        rel = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
        keep2 = keep & ~(l <= rel)
        if not keep2.any():
            return nan, UNMEASURABLE, z, nan, nan
        L = -0.691 + 10.0 * math.log10(z[keep2].mean()) if z[keep2].mean() > 0 else nan
        if np.isnan(z[keep2].mean()):
            L = nan
    if not math.isfinite(L):
        return nan, UNMEASURABLE, z, nan, nan
    return float(L), int(np.rint(100.0 * L)), z, 10.0 ** ((-70.0 + 0.691) / 10.0), 10.0 ** ((rel + 0.691) / 10.0)


def measure(x: np.ndarray, fs: int):
    """(L, lufs_c, e[2][H])"""
    e = hop_energies(x, fs)
    L, c, _, _, _ = integrated(e, hop(fs))
    return L, c, e


def fixture_margin(x: np.ndarray, fs: int):
    """(distance of 100 L from the nearest half-integer, smallest relative distance of a block's z from a gate): the condition
    under which a device that sums in another order must give the same lufs_c (inf where there is nothing to compare)"""
    e = hop_energies(x, fs)
    L, c, z, ta, tr = integrated(e, hop(fs))
    if c == UNMEASURABLE:
        return math.inf, math.inf
    v = 100.0 * L
    d = abs(v - math.floor(v) - 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = min(np.abs(z / ta - 1.0).min(), np.abs(z / tr - 1.0).min())
    return d, float(m)


def gain_table() -> np.ndarray:
    """T[i] = (float) 10^((i - 6000) / 2000): the gain of k hundredths of a LU is T[k + 6000]"""
    return np.array([math.pow(10.0, (i - 6000) / 2000.0) for i in range(12001)], np.float64).astype(np.float32)


_T = None


def gain(lufs_c: int, target_lufs: float, peak, max_peak) -> np.float32:
    """the fp32 gain of a signal of lufs_c whose sample peak is `peak`"""
    global _T
    if _T is None:
        _T = gain_table()
    if lufs_c == UNMEASURABLE:
        return np.float32(1.0)
    target_c = int(np.rint(np.float32(100.0) * np.float32(target_lufs)))
    k = max(-6000, min(6000, target_c - int(lufs_c)))
    g = _T[k + 6000]
    P, M = np.float32(peak), np.float32(max_peak)
    if P > 0 and np.float32(g * P) > M:
        g = np.float32(M / P)
    return np.float32(g)


def check_spec(mode: int, target_lufs: float, max_peak: float, rate: int):
    """None, or the name of the first field the library refuses"""
    if mode not in (MEASURE, MIXTURE, EACH):
        return "mode"
    if not math.isfinite(target_lufs) or target_lufs < -70.0 or target_lufs > 0.0:
        return "target_lufs"
    if not max_peak > 0.0:
        return "max_peak"
    if rate < MIN_RATE:
        return "rate"
    return None


def apply(v, mix, gains, encoding, clip_mode, mode, target_lufs, max_peak, fs):
    """the stage composed with remix_spec and pcm_spec: v (S, 2, n), mix (2, n) ->
    (encoded outputs, peaks (n_out,) float32, lufs_c (n_out + 1,) the mixture last, gains applied (n_out,) float32)"""
    import pcm_spec as ps
    import remix_spec as rs
    F = np.float32
    outs = rs.outputs(v, mix, gains)
    P = np.array([ps.peak(o) for o in outs], F)
    lufs = [measure(o, fs)[1] for o in outs] + [measure(np.asarray(mix, F), fs)[1]]
    if mode == MEASURE:
        g = np.ones(len(outs), F)
    elif mode == MIXTURE:
        g = np.full(len(outs), gain(lufs[-1], target_lufs, P.max(), max_peak), F)
    else:
        g = np.array([gain(lufs[o], target_lufs, P[o], max_peak) for o in range(len(outs))], F)
    with np.errstate(all="ignore"):
        gained = [(F(g[o]) * outs[o]).astype(F) if mode != MEASURE else outs[o] for o in range(len(outs))]
        peaks = np.array([F(g[o] * P[o]) if mode != MEASURE else P[o] for o in range(len(outs))], F)
    enc = [ps.encode_output(y, encoding, clip_mode, p) for y, p in zip(gained, peaks)]
    return enc, peaks, np.array(lufs, np.int64), g
