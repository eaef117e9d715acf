"""NumPy restatement of the PCM output stage (csrc/pcm.hip; include/demucs_hip.h dmx_tracks_infer_pcm; DESIGN.md section
2.9). There is no reference arithmetic (the reference writes float32 only), so this text is what the kernels are pinned
against, exactly: every operation below is one correctly rounded fp32 operation, and no product feeds an addition.

    outputs  stem = -1: the S stems. Else output 0 = v[stem], output 1 = the other stems added in increasing order,
             starting from the first of them.
    peak     per output, the largest |x| over both channels and all frames, NaN ignored, 0 if there is none.
    clip     none: y = x;  clamp: y = x < -0.99f ? -0.99f : x > 0.99f ? 0.99f : x  (a NaN stays one);
             rescale: d = max(1.01f * peak, 1.0f), y = x / d.
    encode   F32: y;  S16: rint(y * 32768.0f) saturated to [-32768, 32767];  S24: rint(y * 8388608.0f) saturated to
             [-8388608, 8388607], 3 bytes little-endian;  ties to even, NaN -> 0, +-inf saturates.
"""
import numpy as np

PCM_F32, PCM_S16, PCM_S24 = 0, 1, 2
CLIP_NONE, CLIP_RESCALE, CLIP_CLAMP = 0, 1, 2
F = np.float32


def outputs(v, stem=-1):
    """v (S, 2, n) float32 -> (n_out, 2, n) float32"""
    v = np.asarray(v, F)
    if stem < 0:
        return v.copy()
    others = [s for s in range(v.shape[0]) if s != stem]
    acc = v[others[0]].copy()
    with np.errstate(all="ignore"):
        for s in others[1:]:
            acc = (acc + v[s]).astype(F)
    return np.stack([v[stem], acc])


def peak(x):
    """the largest |x| of one output (2, n), NaN ignored, as float32"""
    a = np.abs(np.asarray(x, F)).ravel()
    a = a[~np.isnan(a)]
    return F(a.max()) if a.size else F(0)


def clip(x, mode, pk):
    x = np.asarray(x, F)
    if mode == CLIP_NONE:
        return x
    if mode == CLIP_CLAMP:
        return np.where(x < F(-0.99), F(-0.99), np.where(x > F(0.99), F(0.99), x)).astype(F)
    assert mode == CLIP_RESCALE
    with np.errstate(all="ignore"):
        dd = F(F(1.01) * F(pk))
        d = dd if dd > F(1) else F(1)
        return (x / d).astype(F)


def quantise(y, scale, lo, hi):
    with np.errstate(all="ignore"):
        t = np.rint(np.asarray(y, F) * F(scale)).astype(F)  # ties to even
    t = np.where(np.isnan(t), F(0), t)
    return np.clip(t, F(lo), F(hi)).astype(np.int32)


def encode_output(x, encoding, clip_mode, pk=None):
    """one output (2, n) float32 -> np.float32 (n, 2), np.int16 (n, 2) or np.uint8 (n, 2, 3)"""
    pk = peak(x) if pk is None else pk
    y = np.ascontiguousarray(clip(x, clip_mode, pk).T)
    if encoding == PCM_F32:
        return y
    if encoding == PCM_S16:
        return quantise(y, 32768.0, -32768.0, 32767.0).astype(np.int16)
    assert encoding == PCM_S24
    q = quantise(y, 8388608.0, -8388608.0, 8388607.0).astype(np.uint32) & np.uint32(0xFFFFFF)
    return np.stack([(q >> np.uint32(8 * b)).astype(np.uint8) for b in range(3)], axis=-1)


def encode(v, encoding, clip_mode, stem=-1):
    """v (S, 2, n) float32 -> (list of n_out encoded outputs, np.float32 (n_out,) peaks)"""
    outs = outputs(v, stem)
    peaks = np.array([peak(o) for o in outs], F)
    return [encode_output(o, encoding, clip_mode, p) for o, p in zip(outs, peaks)], peaks


def s24_to_int(b):
    """np.uint8 (..., 3) packed little-endian 24 bit -> np.int32"""
    b = np.asarray(b, np.uint8).astype(np.int32)
    q = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.where(q >= 1 << 23, q - (1 << 24), q).astype(np.int32)


def same(a, b):
    """exact equality of two encoded outputs: bytes for the integer formats, bit patterns for float32 (a NaN equals a NaN:
    IEEE 754 does not fix the sign and payload of a NaN that an operation produces, e.g. inf / inf under rescale)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
    return bool(np.array_equal(a, b))
