"""NumPy restatement of the bag of models on the track path (include/demucs_hip.h dmx_tracks_infer_bag / dmx_bag_weights,
csrc/tracks.hip track_ola_bag_kernel).

Notation: Q models of S stems, N shifted copies per model and track, weights w[q][s] >= 0. The shift of track t, model q,
copy k is shift_offsets[(t*Q + q)*N + k]; NULL or -1 entries are rand() % 22050 drawn in that row-major order.

Per output sample and plane (stem s, channel c), all fp32:
  1. v[q][k]: track_ola_ens_kernel's per-copy value acc / sw on copy (q, k)'s own shifted geometry.
  2. e[q] = v[q][0] when N = 1, else (v[q][0] + v[q][1] + ...) / (float)N, summed in increasing k.
  3. over the models with w[q][s] != 0 in increasing q: the first initialises a = w * e[q], each later one does
     a = fmaf(w, e[q], a); W is the fp32 sum of those weights in the same order, the first initialising it.
  4. x = a / W correctly rounded; out = fmaf(x, std, mean).
A model with w[q][s] == 0 is not read for stem s."""
import numpy as np

MAX_BAG = 8
MAX_COPIES = 256  # n_models * n_shifts
MAX_SHIFT = 22050

f32 = np.float32


def shift_index(t, q, k, Q, N):
    return (t * Q + q) * N + k


def effective_weights(n_models, n_sources, weights=None):
    """(w (Q, S) float32, W (S,) float32) or ValueError with the library's wording."""
    Q, S = int(n_models), int(n_sources)
    if not 1 <= Q <= MAX_BAG:
        raise ValueError(f"n_models must be in [1, {MAX_BAG}], got {Q}")
    if weights is None:
        if Q != S:
            raise ValueError("weights: NULL (the diagonal bag) needs n_models == n_sources")
        w = np.eye(Q, dtype=f32)
    else:
        w = np.asarray(weights, f32).reshape(Q, S)
    for q in range(Q):
        for s in range(S):
            if not (w[q, s] >= 0) or np.isinf(w[q, s]):
                raise ValueError(f"weights: model {q}, stem {s}: weight {w[q, s]} is negative or not finite")
    W = np.zeros(S, f32)
    for s in range(S):
        have = False
        for q in range(Q):
            if w[q, s] != 0:
                W[s] = f32(W[s] + w[q, s]) if have else w[q, s]
                have = True
        if not have:
            raise ValueError(f"weights: stem {s} has no model")
    for q in range(Q):
        if not w[q].any():
            raise ValueError(f"weights: model {q} has no non-zero weight")
    return w, W


def _fma(a, b, c):
    """fmaf on float32 arrays: a*b is exact in float64 (48 bits); the sum is rounded to float64, then to float32 - the double
    rounding differs from fmaf in about 2^-29 of the cases by one ulp, which the tolerance tests allow for"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def model_value(v):
    """step 2: v (N, ...) float32 per-copy values -> e"""
    v = np.asarray(v, f32)
    if v.shape[0] == 1:
        return v[0]
    e = v[0]
    for k in range(1, v.shape[0]):
        e = (e + v[k]).astype(f32)
    return (e / f32(v.shape[0])).astype(f32)


def combine(e, w, std, mean):
    """steps 3-4: e (Q, S, 2, n) float32 per-model normalised values, w (Q, S) effective weights -> out (S, 2, n) float32"""
    e = np.asarray(e, f32)
    w = np.asarray(w, f32)
    Q, S = w.shape
    out = np.zeros(e.shape[1:], f32)
    for s in range(S):
        a, W = None, None
        for q in range(Q):
            if w[q, s] == 0:
                continue
            if a is None:
                a, W = (w[q, s] * e[q, s]).astype(f32), w[q, s]
            else:
                a, W = _fma(w[q, s], e[q, s], a), f32(W + w[q, s])
        x = (a / W).astype(f32)
        out[s] = _fma(x, f32(std), f32(mean))
    return out


def recombine64(outs, w):
    """the float64 recombination sum_q w out_q / sum_q w of the models' own de-normalised results (de-normalisation is
    affine and the weights are divided by their sum, so this is the bag's value up to rounding); outs: Q arrays (S, 2, n)"""
    w = np.asarray(w, np.float64)
    ref = np.zeros(outs[0].shape, np.float64)
    for s in range(w.shape[1]):
        ref[s] = sum(w[q, s] * outs[q][s].astype(np.float64) for q in range(w.shape[0]) if w[q, s] != 0) / w[:, s].sum()
    return ref


def tolerance(outs, mean):
    """2^-20 (max |out_q| + |track mean|): at most Q + 5 roundings of 2^-24 each, Q <= 8, with room to spare"""
    return 2.0 ** -20 * (max(float(np.abs(o).max()) for o in outs) + abs(float(mean)))
