"""The look-ahead peak limiter's specification (csrc/limiter.hip), restated in NumPy.

The limiter is exact: equal bits on the GPU and here, whatever the cut into tiles. Everything that depends on time runs in
integers in the log domain, one octave being U = 65536 units, and only maxima carry state; a maximum has no order.

  level      p[j] = max over the channels of |g x[c][j]| (the fp32 product), NaN ignored; under `true_peak` also of the
             F - 1 interpolated phases |g y_p[j]| of tests/meters_spec.py at frame j
  required   M[j] = min(U e + LUT[m >> 11], 24 U) where p[j] > c, with e the unbiased exponent and m the mantissa bits of
             the correctly rounded fp32 quotient p[j] / c; else 0
  envelope   D[i] = max(0, max_{j <= i} M[j] - qr (i - j), max_{j >= i} M[j] - qa (j - i))
  gain       G(D) = THI[D >> 12] * TLO[D & 4095], one fp32 product; G(0) == 1
  apply      y = (g x) G(D): two fp32 products in that order

The three tables are made in binary64 with the host's libm (math.log2, math.pow), as the library makes them.
"""
import math

import numpy as np

import meters_spec as ms

F32 = np.float32
U = 65536
CAP = 24 * U
LIMIT, UNITY = 0x200, 3  # DMX_LOUD_LIMIT, OR-ed into the mode; DMX_LOUD_UNITY
ATTACK_MS, RELEASE_MS = 5.0, 100.0
MS_MIN, MS_MAX = 0.1, 10000.0
TILE = 2048  # frames of a workgroup of the detect and envelope launches


def _toward_zero(d: float) -> np.float32:
    """a positive binary64 rounded to fp32 towards zero"""
    f = F32(d)
    return np.nextafter(f, F32(0.0)) if float(f) > d else f


_TABLES = None


def tables():
    """(LUT int32[4096], THI float32[385], TLO float32[4096])"""
    global _TABLES
    if _TABLES is None:
        lut = np.array([math.ceil(U * math.log2(1.0 + (k + 1) / 4096.0)) + 2 for k in range(4096)], np.int32)
        thi = np.array([_toward_zero(math.pow(2.0, -a / 16.0)) for a in range(16 * 24 + 1)], F32)
        tlo = np.array([_toward_zero(math.pow(2.0, -b / 65536.0)) for b in range(4096)], F32)
        _TABLES = (lut, thi, tlo)
    return _TABLES


def slopes(rate: int, attack_ms: float = ATTACK_MS, release_ms: float = RELEASE_MS):
    """(qa, qr) in units per frame: the reduction moves by 10 dB in attack_ms resp. release_ms"""
    def q(t):
        v = U * math.log2(math.pow(10.0, 0.5)) * 1000.0 / (t * rate)
        return int(min(max(np.rint(v), 1.0), float(2 ** 20)))
    return q(attack_ms), q(release_ms)


def check_times(attack_ms: float, release_ms: float):
    """None, or the name of the first field the library refuses"""
    for name, v in (("attack_ms", attack_ms), ("release_ms", release_ms)):
        if not math.isfinite(v) or v < MS_MIN or v > MS_MAX:
            return name
    return None


def gain_of(D) -> np.ndarray:
    """G(D) for reductions 0 <= D <= 24 U"""
    _, thi, tlo = tables()
    D = np.asarray(D, np.int64)
    return (thi[D >> 12] * tlo[D & 4095]).astype(F32)


def level(x: np.ndarray, g=1.0, true_peak: bool = False, fs: int = 44100) -> np.ndarray:
    """x [2][n] float32 -> p[n] float32"""
    x = np.asarray(x, F32)
    g = F32(g)
    with np.errstate(all="ignore"):
        y = ms.phases(x, fs) if true_peak else x[None]
        a = np.abs((g * y).astype(F32)).reshape(-1, x.shape[1])
    a = np.where(np.isnan(a), F32(0.0), a)
    return a.max(axis=0).astype(F32)


def required(p: np.ndarray, c) -> np.ndarray:
    """p[n] float32 (no NaN) -> M[n] int32"""
    lut = tables()[0]
    p, c = np.asarray(p, F32), F32(c)
    with np.errstate(all="ignore"):
        r = (p / c).astype(F32)
    bits = r.view(np.uint32).astype(np.int64)
    e = (bits >> 23) - 127
    m = bits & 0x7FFFFF
    M = np.minimum(U * e + lut[m >> 11].astype(np.int64), CAP)
    return np.where(p > c, M, 0).astype(np.int32)


def envelope(M: np.ndarray, qa: int, qr: int) -> np.ndarray:
    """D[n] int32: a prefix maximum of M[j] + qr j and a suffix maximum of M[j] - qa j"""
    M = np.asarray(M, np.int64)
    j = np.arange(M.size, dtype=np.int64)
    fwd = np.maximum.accumulate(M + qr * j) - qr * j
    bwd = np.maximum.accumulate((M - qa * j)[::-1])[::-1] + qa * j
    return np.maximum(0, np.maximum(fwd, bwd)).astype(np.int32)


def envelope_brute(M: np.ndarray, qa: int, qr: int) -> np.ndarray:
    """the definition, as a double loop (short signals only)"""
    M = [int(v) for v in M]
    n = len(M)
    D = np.zeros(n, np.int32)
    for i in range(n):
        d = 0
        for j in range(n):
            d = max(d, M[j] - (qr * (i - j) if j <= i else qa * (j - i)))
        D[i] = d
    return D


def limit(x, c, qa: int, qr: int, g=1.0, true_peak: bool = False, fs: int = 44100, link=None):
    """one envelope over the stereo signal x [2][n] (and, under MIXTURE, over the further signals in `link`, which share g):
    dict with M, D, gain (the plane G(D)), y (the limited signal), and the result fields"""
    x = np.asarray(x, F32)
    p = level(x, g, true_peak, fs)
    for other in link or ():
        p = np.maximum(p, level(other, g, true_peak, fs))
    M = required(p, c)
    D = envelope(M, qa, qr)
    G = gain_of(D)
    with np.errstate(all="ignore"):
        y = ((F32(g) * x).astype(F32) * G[None]).astype(F32)
    return {
        "p": p, "M": M, "D": D, "gain": G, "y": y,
        "peak_out": ms.sample_peak(y),
        "true_peak_out": ms.true_peak(y, fs)[0] if true_peak else F32(0.0),
        "max_reduction": int(D.max()) if D.size else 0,
        "limited_frames": int((D > 0).sum()),
    }


def reduction_db(D: int) -> float:
    """a reduction in units as dB (positive)"""
    return D / U * 20.0 * math.log10(2.0)


def check_spec(mode: int, target_lufs: float, max_peak: float, rate: int, attack_ms: float = ATTACK_MS, release_ms: float = RELEASE_MS):
    """None, or the name of the first field dmx_limiter_check refuses"""
    base, limited = mode & ~(ms.TRUE_PEAK | LIMIT), bool(mode & LIMIT)
    if mode < 0 or base not in (0, 1, 2, UNITY) or (limited and base == 0) or (not limited and base == UNITY):
        return "mode"
    why = ms.check_spec((0 if base == UNITY else base) | (mode & ms.TRUE_PEAK), target_lufs, max_peak, rate)
    if why:
        return why
    if limited and not math.isfinite(max_peak):
        return "max_peak"
    return check_times(attack_ms, release_ms)


def apply(v, mix, gains, encoding, clip_mode, mode, target_lufs, max_peak, fs, attack_ms: float = ATTACK_MS, release_ms: float = RELEASE_MS):
    """the loudness stage with LIMIT in the mode, composed with remix_spec and pcm_spec: v (S, 2, n), mix (2, n) ->
    (encoded outputs, peaks (n_out,) float32, lufs_c (n_out + 1,), gains applied (n_out,) float32, limit results: n_out dicts)"""
    import loudness_spec as ls
    import pcm_spec as ps
    import remix_spec as rs
    assert mode & LIMIT
    base, tp = mode & ~(ms.TRUE_PEAK | LIMIT), bool(mode & ms.TRUE_PEAK)
    outs = rs.outputs(v, mix, gains)
    lufs = [ls.measure(o, fs)[1] for o in outs] + [ls.measure(np.asarray(mix, F32), fs)[1]]
    if base == UNITY:
        g = np.ones(len(outs), F32)
    elif base == ls.MIXTURE:
        g = np.full(len(outs), ls.gain(lufs[-1], target_lufs, 0.0, max_peak), F32)  # a peak of 0: the ceiling rule stays out
    else:
        g = np.array([ls.gain(lufs[o], target_lufs, 0.0, max_peak) for o in range(len(outs))], F32)
    qa, qr = slopes(fs, attack_ms, release_ms)
    res = []
    for o, x in enumerate(outs):
        link = [outs[q] for q in range(len(outs)) if q != o] if base == ls.MIXTURE else None
        res.append(limit(x, max_peak, qa, qr, g[o], tp, fs, link))
    peaks = np.array([r["peak_out"] for r in res], F32)
    enc = [ps.encode_output(r["y"], encoding, clip_mode, p) for r, p in zip(res, peaks)]
    return enc, peaks, np.array(lufs, np.int64), g, res
