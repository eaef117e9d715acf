"""Median-filter harmonic/percussive separation of stems, restated in NumPy: the specification
csrc/hpss.hip is held to; librosa.decompose.hpss with soft masks. dtype=np.float64 is the reference; with np.float32 only the
STFT and the inverse run in single precision (scipy.fft keeps float32), which sizes the tolerance of tests/test_gpu_hpss.py.
The magnitudes, the medians and the masks are the same in both."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from wiener_spec import istft, stft

FLT_MIN = float(np.finfo(np.float32).tiny)


def magnitudes(D):
    """complex64 values -> float32: the squares, the sum and the root in binary64"""
    re, im = D.real.astype(np.float64), D.imag.astype(np.float64)
    return np.sqrt(re * re + im * im).astype(np.float32)


def medians(S, kernel_h, kernel_p):
    """S (T, F) float32 -> H (median along time), P (along frequency); symmetric reflection, repeated as often as needed"""
    h, p = kernel_h // 2, kernel_p // 2
    H = np.median(sliding_window_view(np.pad(S, ((h, h), (0, 0)), mode="symmetric"), kernel_h, axis=0), axis=-1)
    P = np.median(sliding_window_view(np.pad(S, ((0, 0), (p, p)), mode="symmetric"), kernel_p, axis=1), axis=-1)
    return H.astype(np.float32), P.astype(np.float32)


def softmask(x, r, power, unit):
    """binary64, one rounding per operation, the powers by repeated multiplication from the left"""
    z = np.maximum(x, r)
    tiny = z < FLT_MIN
    zs = np.where(tiny, 1.0, z)
    qx, qr = x / zs, r / zs
    a, b = qx.copy(), qr.copy()
    for _ in range(power - 1):
        a, b = a * qx, b * qr
    return np.where(tiny, 0.5 if unit else 0.0, a / np.where(tiny, 1.0, a + b))


def masks(H, P, power=2, margin_h=1.0, margin_p=1.0):
    """float32 medians -> float32 M_h, M_p"""
    H, P = H.astype(np.float64), P.astype(np.float64)
    unit = margin_h == 1.0 and margin_p == 1.0
    return (softmask(H, np.float64(margin_h) * P, power, unit).astype(np.float32),
            softmask(P, np.float64(margin_p) * H, power, unit).astype(np.float32))


def hpss(x, kernel_h=31, kernel_p=31, power=2, margin_h=1.0, margin_p=1.0, residual=False, dtype=np.float64):
    """x (J, C, n) float32 -> (J, K, C, n) float32, K = 2 + residual: harmonic, percussive, residual"""
    n = x.shape[-1]
    D = stft(x, dtype)                                     # (J, C, T, F) complex64
    Mh, Mp = np.empty(D.shape, np.float32), np.empty(D.shape, np.float32)
    for j, c in np.ndindex(*D.shape[:2]):
        Mh[j, c], Mp[j, c] = masks(*medians(magnitudes(D[j, c]), kernel_h, kernel_p), power, margin_h, margin_p)
    kinds = [Mh, Mp] + ([(np.float32(1) - Mh) - Mp] if residual else [])
    Y = np.stack([(m * D.real + 1j * (m * D.imag)).astype(np.complex64) for m in kinds], axis=1)  # (J, K, C, T, F), fp32 products
    return istft(Y, n, dtype)
