"""The multichannel Wiener post-filter with EM re-estimation, restated in NumPy: the specification
csrc/wiener.hip is held to. dtype=np.float64 is the reference; with np.float32 only the STFT and the inverse run in single
precision (scipy.fft keeps float32), which sizes the tolerance of tests/test_gpu_wiener.py. The EM arithmetic is binary64 and
its storage complex64 in both."""
import numpy as np
import scipy.fft

NFFT, HOP, PAD, EPS = 4096, 1024, 2048, 1e-10


def window(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(NFFT) / NFFT)).astype(dtype)


def stft(x, dtype=np.float64):
    """x (..., n) -> complex64 (..., T, 2049), T = 1 + n // 1024: centred, reflect padding, periodic Hann, no scaling"""
    n = x.shape[-1]
    xp = np.pad(x.astype(dtype), [(0, 0)] * (x.ndim - 1) + [(PAD, PAD)], mode="reflect")
    idx = HOP * np.arange(1 + n // HOP)[:, None] + np.arange(NFFT)
    return scipy.fft.rfft(xp[..., idx] * window(dtype), axis=-1).astype(np.complex64)


def istft(Y, n, dtype=np.float64):
    """complex64 (..., T, 2049) -> (..., n) float32: window, overlap-add in frame order, division by the window-square sum"""
    w = window(dtype)
    frames = scipy.fft.irfft(Y.astype(np.complex64 if dtype == np.float32 else np.complex128), n=NFFT, axis=-1) * w
    T = Y.shape[-2]
    out = np.zeros(Y.shape[:-2] + (HOP * (T - 1) + NFFT,), dtype)
    wss = np.zeros(out.shape[-1], dtype)
    for t in range(T):
        out[..., HOP * t:HOP * t + NFFT] += frames[..., t, :]
        wss[HOP * t:HOP * t + NFFT] += w * w
    return (out[..., PAD:PAD + n] / wss[PAD:PAD + n]).astype(np.float32)


def c64(z):
    """the storage format between the iterations"""
    return z.astype(np.complex64).astype(np.complex128)


def em_step(y, x):
    """one iteration on a block: y (S, C, T, F) and x (C, T, F) complex128 -> the new y, rounded to complex64"""
    S, C = y.shape[:2]
    p = y.real ** 2 + y.imag ** 2
    v = p.sum(axis=1) / C                                  # (S, T, F)
    den = EPS + v.sum(axis=1)                              # (S, F)
    reg = np.sqrt(EPS)
    if C == 1:
        Ra = p[:, 0].sum(axis=1) / den
        A = (v * Ra[:, None]).sum(axis=0) + reg
        return c64((v * Ra[:, None] * (x[0] / A))[:, None])
    Ra, Rd = p[:, 0].sum(axis=1) / den, p[:, 1].sum(axis=1) / den
    Rb = (y[:, 0] * y[:, 1].conj()).sum(axis=1) / den      # R = [[Ra, Rb], [conj Rb, Rd]]
    A, D = (v * Ra[:, None]).sum(axis=0) + reg, (v * Rd[:, None]).sum(axis=0) + reg
    B = (v * Rb[:, None]).sum(axis=0)
    det = A * D - (B.real ** 2 + B.imag ** 2)              # Cxx^-1 = [[D, -B], [-conj B, A]] / det
    g0, g1 = (D * x[0] - B * x[1]) / det, (A * x[1] - B.conj() * x[0]) / det
    u0 = Ra[:, None] * g0 + Rb[:, None] * g1
    u1 = Rb.conj()[:, None] * g0 + Rd[:, None] * g1
    return c64(np.stack([v * u0, v * u1], axis=1))


def wiener(mix, ests, iterations=1, residual=False, win_len=300, dtype=np.float64):
    """mix (C, n), ests (J, C, n) float32 -> (J, C, n) float32"""
    J, C, n = ests.shape
    X = stft(mix, dtype).astype(np.complex128)             # (C, T, F)
    E = stft(ests, dtype).astype(np.complex128)            # (J, C, T, F)
    a = np.sqrt(X.real ** 2 + X.imag ** 2)
    pos = a > 0
    safe = np.where(pos, a, 1.0)
    phr, phi = np.where(pos, X.real / safe, 1.0), np.where(pos, X.imag / safe, 0.0)
    m = np.sqrt(E.real ** 2 + E.imag ** 2)
    y = m * phr + 1j * (m * phi)                           # the estimate's magnitude with the mixture's phase
    if residual:
        r = X.copy()
        for j in range(J):
            r = r - y[j]
        y = np.concatenate([y, r[None]])
    Y = np.zeros(y.shape, np.complex64)
    for t0 in range(0, X.shape[1], win_len):
        blk = slice(t0, t0 + win_len)
        s = max(1.0, float(np.sqrt((X[:, blk].real ** 2 + X[:, blk].imag ** 2).max())) / 10.0)
        xb, yb = X[:, blk] / s, c64(y[:, :, blk] / s)
        for _ in range(iterations):
            yb = em_step(yb, xb)
        Y[:, :, blk] = (yb * s).astype(np.complex64)
    return istft(Y[:J], n, dtype)
