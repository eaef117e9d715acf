"""The meters' specification (csrc/meters.hip), restated in NumPy: true peak, loudness range, and
the maxima of momentary and short-term loudness of a stereo signal x[2][n] of fp32 samples at fs Hz.

True peak is the largest |y| of the signal oversampled F times by a Hann-windowed sinc of 12 taps per phase. The taps are made
in binary64 (math.sin / math.cos: the host's libm, as the library does) and rounded once to fp32; the arithmetic is fp32 with
every product and every sum rounded on its own, in a fixed order, which float32 NumPy restates bit for bit. A maximum does
not depend on its order, so TP is specified exactly.

The hop meters are functions of the K-weighted 100 ms hop energies e[c][j] of tests/loudness_spec.py, quantised to
hundredths of a LU; the loudness range is a pure function of those integers (EBU Tech 3342 over an integer histogram).
"""
import math

import numpy as np

import loudness_spec as ls

UNMEASURABLE = ls.UNMEASURABLE
TRUE_PEAK = 0x100  # DMX_LOUD_TRUE_PEAK, OR-ed into the mode
TAPS, HALO, SHORT = 12, 6, 30
F32 = np.float32


def factor(fs: int) -> int:
    return 4 if fs < 96000 else (2 if fs < 192000 else 1)


def taps(fs: int) -> np.ndarray:
    """h[k], k = 0 .. 12 F: float32"""
    F = factor(fs)
    h = np.zeros(TAPS * F + 1, np.float64)
    for k in range(TAPS * F + 1):
        t = (k - HALO * F) / F
        sinc = 1.0 if k == HALO * F else math.sin(math.pi * t) / (math.pi * t)
        w = 0.5 * (1.0 - math.cos(2.0 * math.pi * k / (12.0 * F)))
        h[k] = sinc * w
    return h.astype(F32)


def phases(x: np.ndarray, fs: int) -> np.ndarray:
    """x [2][n] float32 -> y [F][2][n] float32: y[0] is x, y[p][c][i] = sum_j h[p + F j] x[c][i + 6 - j], j ascending"""
    x = np.asarray(x, F32)
    assert x.ndim == 2 and x.shape[0] == 2
    n = x.shape[1]
    F, h = factor(fs), taps(fs)
    xp = np.zeros((2, n + TAPS), F32)  # xp[:, k] = x[:, k - 5]
    xp[:, HALO - 1:HALO - 1 + n] = x
    y = np.zeros((F, 2, n), F32)
    y[0] = x
    with np.errstate(all="ignore"):
        for p in range(1, F):
            acc = None
            for j in range(TAPS):
                q = (h[p + F * j] * xp[:, TAPS - 1 - j:TAPS - 1 - j + n]).astype(F32)  # x[i + 6 - j] = xp[i + 11 - j]
                acc = q if acc is None else (acc + q).astype(F32)
            y[p] = acc
    return y


def _max_ignoring_nan(a: np.ndarray) -> np.float32:
    a = np.abs(a[~np.isnan(a)])
    return F32(a.max()) if a.size else F32(0.0)


def true_peak(x: np.ndarray, fs: int):
    """(TP float32, the phase that wins: 0 the samples themselves)"""
    y = phases(x, fs)
    per = [_max_ignoring_nan(y[p]) for p in range(y.shape[0])]
    tp = max(per)
    return F32(tp), int(per.index(tp))


def sample_peak(x: np.ndarray) -> np.float32:
    return _max_ignoring_nan(np.asarray(x, F32))


def _quantum(z: np.ndarray):
    """hundredths of a LU of the blocks of mean square z (float64; -inf for a block of zero energy), and whether a block is
    not finite"""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = -0.691 + 10.0 * np.log10(z)
    zero = z == 0.0
    bad = bool((~np.isfinite(v) & ~zero).any())
    c = np.where(zero | ~np.isfinite(v), -np.inf, np.rint(100.0 * np.where(np.isfinite(v), v, 0.0)))
    return c, bad


def short_energies(e: np.ndarray, h: int) -> np.ndarray:
    """the mean squares of the 3 s blocks: hops b .. b + 29 summed in increasing order, channel 0 then channel 1 of a hop"""
    H = e.shape[1]
    nb = max(H - (SHORT - 1), 0)
    acc = np.zeros(nb, np.float64)
    with np.errstate(all="ignore"):
        for j in range(SHORT):
            acc = acc + e[0][j:j + nb]
            acc = acc + e[1][j:j + nb]
        return acc / (30.0 * h)


def block_values(e: np.ndarray, h: int):
    """(100 l[b], 100 S[b]) as float64, unrounded: what a fixture keeps away from the half-integers"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (100.0 * (-0.691 + 10.0 * np.log10(ls.block_energies(e, h))),
                100.0 * (-0.691 + 10.0 * np.log10(short_energies(e, h))))


def _maximum(c: np.ndarray, bad: bool) -> int:
    if bad or c.size == 0 or not np.isfinite(c).any():
        return UNMEASURABLE
    return int(c[np.isfinite(c)].max())


def lra_of(s_c, n_hops: int, bad: bool = False):
    """(lra_c, 100 * 10 * log10(mean) or None): the loudness range of the short-term quanta s_c (-inf: a silent block)"""
    if n_hops < SHORT or bad:
        return UNMEASURABLE, None
    cnt = np.zeros(9001, np.int64)
    for v in s_c:
        if not np.isfinite(v):
            continue
        v = min(int(v), 2000)
        if v > -7000:
            cnt[v + 7000] += 1
    tot = int(cnt.sum())
    if tot == 0:
        return UNMEASURABLE, None
    total = 0.0
    for k in range(1, 9001):
        if cnt[k]:
            total += float(cnt[k]) * math.pow(10.0, (k - 7000) / 1000.0)
    mean = total / float(tot)
    edge = 100.0 * (10.0 * math.log10(mean))
    r_c = math.floor(edge) - 2000
    kept = [(k - 7000, int(cnt[k])) for k in range(1, 9001) if k - 7000 > r_c and cnt[k]]
    m = sum(c for _, c in kept)
    if m == 0:
        return UNMEASURABLE, edge
    v = np.repeat([a for a, _ in kept], [c for _, c in kept])
    i10, i95 = ((m - 1) * 10 + 50) // 100, ((m - 1) * 95 + 50) // 100
    return int(v[i95] - v[i10]), edge


def hop_meters(e: np.ndarray, h: int):
    """e [2][H] -> (lra_c, max_momentary_c, max_short_c)"""
    H = e.shape[1]
    mc, mbad = _quantum(ls.block_energies(e, h))
    sc, sbad = _quantum(short_energies(e, h))
    return lra_of(sc, H, sbad)[0], _maximum(mc, mbad), _maximum(sc, sbad)


def measure(x: np.ndarray, fs: int):
    """(TP float32, lra_c, max_momentary_c, max_short_c)"""
    e = ls.hop_energies(x, fs)
    return (true_peak(x, fs)[0],) + hop_meters(e, ls.hop(fs))


def fixture_ok(x: np.ndarray, fs: int):
    """None, or what is wrong with a fixture: a device that sums in another order must give the same three integers"""
    e = ls.hop_energies(x, fs)
    h = ls.hop(fs)
    pos = e[np.isfinite(e) & (e != 0.0)]
    if pos.size and pos.min() < 1e-300:
        return "a non-zero hop energy lies below 1e-300"
    for name, v in zip(("100 l", "100 S"), block_values(e, h)):
        v = v[np.isfinite(v)]
        if v.size:
            d = np.abs(v - np.floor(v) - 0.5).min()
            if d < 0.001:
                return f"{name} lies {d:.6f} from a half-integer"
    sc, sbad = _quantum(short_energies(e, h))
    edge = lra_of(sc, e.shape[1], sbad)[1]
    if edge is not None and abs(edge - round(edge)) < 1e-6:
        # the relative gate r_c = floor(edge) - 2000 may come out one lower or higher on a device whose pow and log10 round
        # differently. Where all blocks share a bin the edge IS an integer (one block of 30 hops: always), so the condition is
        # asked only where it decides something: a block sits in the one bin, round(edge) - 2000, that the two gates disagree on
        at = int(round(edge)) - 2000
        if any(np.isfinite(v) and min(int(v), 2000) == at for v in sc):
            return f"100 * 10 log10(mean) lies {abs(edge - round(edge)):.3e} from an integer and a block sits on the gate"
    return None


def gain(lufs_c: int, target_lufs: float, tp, max_peak) -> np.float32:
    """the ceiling by true peak: the gain rule of loudness_spec.gain reads TP where it read P"""
    return ls.gain(lufs_c, target_lufs, tp, max_peak)


def check_spec(mode: int, target_lufs: float, max_peak: float, rate: int):
    """None, or the name of the first field the library refuses: the flag may be OR-ed into the three modes"""
    if mode & ~TRUE_PEAK not in (ls.MEASURE, ls.MIXTURE, ls.EACH) or mode < 0:
        return "mode"
    return ls.check_spec(mode & ~TRUE_PEAK, target_lufs, max_peak, rate)


def apply(v, mix, gains, encoding, clip_mode, mode, target_lufs, max_peak, fs):
    """loudness_spec.apply under a mode that may carry TRUE_PEAK ->
    (encoded outputs, peaks (n_out,) float32, lufs_c (n_out + 1,), gains applied (n_out,) float32, meters: n_out + 1 tuples
    (TP, lra_c, max_momentary_c, max_short_c), the mixture last)"""
    import pcm_spec as ps
    import remix_spec as rs
    outs = rs.outputs(v, mix, gains)
    sigs = list(outs) + [np.asarray(mix, F32)]
    meters = [measure(s, fs) for s in sigs]
    base = mode & ~TRUE_PEAK
    if not mode & TRUE_PEAK:
        enc, peaks, lufs, g = ls.apply(v, mix, gains, encoding, clip_mode, base, target_lufs, max_peak, fs)
        return enc, peaks, lufs, g, meters
    P = np.array([ps.peak(o) for o in outs], F32)
    TP = np.array([m[0] for m in meters[:-1]], F32)
    lufs = [ls.measure(s, fs)[1] for s in sigs]
    if base == ls.MEASURE:
        g = np.ones(len(outs), F32)
    elif base == ls.MIXTURE:
        g = np.full(len(outs), gain(lufs[-1], target_lufs, TP.max(), max_peak), F32)
    else:
        g = np.array([gain(lufs[o], target_lufs, TP[o], max_peak) for o in range(len(outs))], F32)
    with np.errstate(all="ignore"):
        gained = [(F32(g[o]) * outs[o]).astype(F32) if base != ls.MEASURE else outs[o] for o in range(len(outs))]
        peaks = np.array([F32(g[o] * P[o]) if base != ls.MEASURE else P[o] for o in range(len(outs))], F32)
    enc = [ps.encode_output(y, encoding, clip_mode, p) for y, p in zip(gained, peaks)]
    return enc, peaks, np.array(lufs, np.int64), g, meters
