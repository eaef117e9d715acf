"""The log-mel stage restated in binary64 NumPy: the specification csrc/logmel.hip is pinned to.
spec: any object with the fields of dmx_logmel_spec (binding.LogmelSpec). Two routes to the power spectrum: np.fft.rfft and the
explicit product with the windowed cos / sin matrix; their distance is the yardstick D of tests/test_gpu_logmel.py."""
import numpy as np

SLANEY, HTK = 0, 1  # mel_scale; mel_norm: 0 Slaney, 1 none
LOG_NONE, LOG_DB, LOG_WHISPER = 0, 1, 2


def hz_to_mel(f, scale):
    f = np.asarray(f, np.float64)
    if scale == HTK:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    f_sp = 200.0 / 3.0
    return np.where(f >= 1000.0, 1000.0 / f_sp + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / f_sp)


def mel_to_hz(m, scale):
    m = np.asarray(m, np.float64)
    if scale == HTK:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp = 200.0 / 3.0
    return np.where(m >= 1000.0 / f_sp, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 1000.0 / f_sp)), f_sp * m)


def filters(spec):
    """librosa.filters.mel: W (n_mels, n_fft / 2 + 1)"""
    hz = mel_to_hz(np.linspace(hz_to_mel(spec.fmin, spec.mel_scale), hz_to_mel(spec.fmax, spec.mel_scale), spec.n_mels + 2), spec.mel_scale)
    bins = np.arange(spec.n_fft // 2 + 1) * float(spec.sr) / spec.n_fft
    lower = (bins[None, :] - hz[:-2, None]) / np.diff(hz)[:-1, None]
    upper = (hz[2:, None] - bins[None, :]) / np.diff(hz)[1:, None]
    W = np.maximum(0.0, np.minimum(lower, upper))
    return W * (2.0 / (hz[2:] - hz[:-2]))[:, None] if spec.mel_norm == 0 else W


def frames_of(spec, n):
    """(chunks, frames of a chunk, samples of a chunk)"""
    if spec.chunk_frames == 0:
        return 1, 1 + n // spec.hop, n
    size = spec.chunk_frames * spec.hop
    return -(-n // size), spec.chunk_frames, size


def power(spec, chunk, frames, route):
    """|STFT|^2 (bins, frames) of one chunk: centred, reflect padding, periodic Hann"""
    N, pad = spec.n_fft, spec.n_fft // 2
    x = np.pad(np.asarray(chunk, np.float64), pad, mode="reflect")
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    fr = np.stack([x[t * spec.hop:t * spec.hop + N] for t in range(frames)]) * w
    if route == "rfft":
        X = np.fft.rfft(fr, axis=1)
        return (X.real ** 2 + X.imag ** 2).T
    ph = 2.0 * np.pi * (np.outer(np.arange(N // 2 + 1), np.arange(N)) % N) / N
    return (np.cos(ph) @ fr.T) ** 2 + (np.sin(ph) @ fr.T) ** 2


def logmel(planes, spec, route="rfft"):
    """planes (P, n) float32 -> (P, chunks, n_mels, frames) float64, before the one rounding to fp32"""
    planes = np.asarray(planes, np.float32)
    P, n = planes.shape
    chunks, frames, size = frames_of(spec, n)
    W = filters(spec)
    out = np.empty((P, chunks, spec.n_mels, frames))
    for p in range(P):
        x = np.zeros(chunks * size, np.float32)
        x[:n] = planes[p]
        for c in range(chunks):
            M = W @ power(spec, x[c * size:(c + 1) * size], frames, route)
            if spec.log_mode == LOG_DB:
                M = 10.0 * np.log10(np.maximum(spec.amin, M))
                if spec.top_db > 0:
                    M = np.maximum(M, M.max() - spec.top_db)
            elif spec.log_mode == LOG_WHISPER:
                M = np.log10(np.maximum(1e-10, M))
                M = (np.maximum(M, M.max() - 8.0) + 4.0) / 4.0
            out[p, c] = M
    return out
