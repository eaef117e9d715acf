"""Phase-vocoder time stretch and pitch shift of stems, restated in NumPy: the specification
csrc/stretch.hip is held to; librosa.phase_vocoder without angles. dtype=np.float64 is the reference; with np.float32 only the
STFT and the inverse run in single precision (scipy.fft keeps float32), which sizes the tolerance of tests/test_gpu_stretch.py.
The vocoder is binary64 and the converter's sum float64 in both."""
import os
import sys

import numpy as np

from wiener_spec import HOP, istft, stft

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import resample_oracle  # noqa: E402


def unit(z):
    m = np.abs(z)
    return np.where(m > 0, z / np.where(m > 0, m, 1.0), 1.0)


def vocoder(D, num, den, frames):
    """one plane: D (T, F) complex128 -> Y (frames, F) complex128; rows from T on read as zero"""
    D = np.concatenate([D, np.zeros((2, D.shape[1]), np.complex128)])
    t = np.arange(frames, dtype=np.int64)
    a, alpha = t * num // den, (t * num % den) / den
    U = unit(D)
    u = U[a + 1] * U[a].conj()
    ph = np.empty((frames, D.shape[1]), np.complex128)
    ph[0] = U[0]
    for i in range(frames - 1):                            # the running product, in frame order
        ph[i + 1] = ph[i] * u[i]
    return ((1 - alpha)[:, None] * np.abs(D[a]) + alpha[:, None] * np.abs(D[a + 1])) * ph


def stretch(x, num, den, pitch_num=1, pitch_den=1, taps=None, dtype=np.float64):
    """x (J, C, n) float32 -> (J, C, n'') float32. taps: the converter's filter as the library designs it (dmx_resample_filter)"""
    n = x.shape[-1]
    n2 = -(-n * den // num)
    D = stft(x, dtype).astype(np.complex128)               # (J, C, T, F), complex64 values
    Y = np.stack([[vocoder(Dc, num, den, 1 + n2 // HOP) for Dc in Dj] for Dj in D])
    y = istft(Y.astype(np.complex64), n2, dtype)
    if pitch_num == pitch_den:
        return y
    return resample_oracle.resample(y, pitch_num, pitch_den, taps).astype(np.float32)
