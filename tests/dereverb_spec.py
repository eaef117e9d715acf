"""Weighted Prediction Error de-reverberation of stems, restated in NumPy: the specification
csrc/dereverb.hip is held to. dtype=np.float64 is the reference; with np.float32 only the STFT and the inverse run in single
precision (scipy.fft keeps float32), which sizes the tolerance of tests/test_gpu_dereverb.py. The WPE core is binary64 in both."""
import numpy as np

from wiener_spec import istft, stft


def wpe(Y, taps, delay, iterations, eps, reg):
    """one stem: Y (C, T, F) complex128 -> Z (C, T, F) complex128"""
    C, T, F = Y.shape
    M = C * taps
    floor = eps * float((Y.real ** 2 + Y.imag ** 2).max())
    if floor == 0.0:
        return np.zeros_like(Y)
    Yt = np.zeros((F, M, T), np.complex128)                # row (k, c) is Y_c(t - delay - k), zero before the first frame
    for k in range(taps):
        s = delay + k
        if s < T:
            Yt[:, k * C:(k + 1) * C, s:] = Y[:, :T - s].transpose(2, 0, 1)
    Yf = Y.transpose(2, 0, 1)                              # (F, C, T)
    Z = Yf
    for _ in range(iterations):
        lam = np.maximum((Z.real ** 2 + Z.imag ** 2).sum(axis=1) / C, floor)  # (F, T)
        W = Yt / lam[:, None, :]
        R = W @ Yt.conj().transpose(0, 2, 1)               # (F, M, M)
        P = W @ Yf.conj().transpose(0, 2, 1)               # (F, M, C)
        tr = np.einsum("fmm->f", R).real
        R = R + (reg * tr / M)[:, None, None] * np.eye(M)
        G = np.linalg.solve(R, P)
        Z = Yf - G.conj().transpose(0, 2, 1) @ Yt
    return Z.transpose(1, 2, 0)


def dereverb(x, taps=10, delay=3, iterations=3, eps=1e-10, reg=1e-10, dtype=np.float64):
    """x (J, C, n) float32 -> (J, C, n) float32: every stem on its own, its C channels the array"""
    n = x.shape[-1]
    Y = stft(x, dtype).astype(np.complex128)               # (J, C, T, F), complex64 values
    Z = np.stack([wpe(Yj, taps, delay, iterations, eps, reg) for Yj in Y])
    return istft(Z.astype(np.complex64), n, dtype)
