"""BSS Eval v4 (csrc/bss.hip) restated in NumPy binary64, by two routes.

Route A is the authority: the dense matrix of delayed references, numpy.linalg.lstsq on that basis itself (no normal
equations), projections by matrix product. Route B is the algorithm the GPU runs: correlations by FFT, a Toeplitz G,
numpy.linalg.solve, projections by np.convolve. What B loses against A is what binary64 normal equations legitimately cost.

A source whose reference is all zero is dropped: left out of every system, NaN everywhere, zero filters. The failure rule
(a Cholesky pivot that is not finite and positive: status 1, NaN everywhere) is, in exact arithmetic, "the basis is rank
deficient": route A reads it from the rank lstsq reports, route B from numpy.linalg.cholesky.

Both return {"sdr", "isr", "sir", "sar"}: (J, nwin), "status", "X": (J, J C L, C), "parts": (4, J, C, n) = s_true, e_spat,
e_interf, e_artif over [0, n).
"""
import numpy as np

OK, SINGULAR = 0, 1


def windows(n, W, H):
    return [(0, n)] if n < W else [(w * H, w * H + W) for w in range((n - W + H) // H)]


def kept_sources(refs):
    return [j for j in range(refs.shape[0]) if np.any(refs[j] != 0)]


def _db(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.inf if den == 0 else 10.0 * np.log10(num / den)


def _finish(refs, ests, p_all, p_own, X, W, H, status):
    J, C, n = refs.shape
    kept, win = kept_sources(refs), windows(n, W, H)
    parts = np.stack([refs, p_own - refs, p_all - p_own, ests - p_all])
    m = np.full((4, J, len(win)), np.nan)
    for w, (a, b) in enumerate(win):
        if status != OK or any(not np.any(refs[j, :, a:b]) or not np.any(ests[j, :, a:b]) for j in kept):
            continue
        for j in kept:
            e = lambda x: float((x[j, :, a:b] ** 2).sum())  # noqa: E731
            m[:, j, w] = (_db(e(refs), e(ests - refs)), _db(e(refs), e(parts[1])), _db(e(p_own), e(parts[2])), _db(e(p_all), e(parts[3])))
    return {"sdr": m[0], "isr": m[1], "sir": m[2], "sar": m[3], "status": status, "X": X, "parts": parts}


def _rows(j, C, L):
    return slice(j * C * L, (j + 1) * C * L)


def route_a(refs, ests, L, W, H):
    refs, ests = np.asarray(refs, np.float64), np.asarray(ests, np.float64)
    J, C, n = refs.shape
    P, kept = n + L - 1, kept_sources(refs)
    B = np.zeros((P, J * C * L))  # column (j, c, tau) = r_jc delayed by tau; a dropped source's columns stay zero and unused
    for j in kept:
        for c in range(C):
            for t in range(L):
                B[t:t + n, (j * C + c) * L + t] = refs[j, c]
    cols = np.concatenate([np.arange(J * C * L)[_rows(j, C, L)] for j in kept]) if kept else np.zeros(0, int)
    E = np.zeros((P, J, C))
    E[:n] = ests.transpose(2, 0, 1)
    X, Y, status = np.zeros((J, J * C * L, C)), np.zeros((J, J * C * L, C)), OK
    for i in kept:
        sol, _, rank, _ = np.linalg.lstsq(B[:, cols], E[:, i], rcond=None)
        X[i, cols] = sol
        sol_own, _, rank_own, _ = np.linalg.lstsq(B[:, _rows(i, C, L)], E[:, i], rcond=None)
        Y[i, _rows(i, C, L)] = sol_own
        if rank < len(cols) or rank_own < C * L:
            status = SINGULAR
    p_all = np.einsum("pk,ikc->icp", B, X)[:, :, :n]
    p_own = np.einsum("pk,ikc->icp", B, Y)[:, :, :n]
    return _finish(refs, ests, p_all, p_own, X, W, H, status)


def _corr(a, b, L):
    """rho_ab(k) = sum_m a[m] b[m + k], 0 <= k < L"""
    nfft = 1 << int(np.ceil(np.log2(2 * (len(a) + L))))
    return np.fft.irfft(np.conj(np.fft.rfft(a, nfft)) * np.fft.rfft(b, nfft), nfft)[:L]


def route_b(refs, ests, L, W, H):
    refs, ests = np.asarray(refs, np.float64), np.asarray(ests, np.float64)
    J, C, n = refs.shape
    kept, M = kept_sources(refs), J * C
    planes = refs.reshape(M, n)
    tt = np.arange(L)[:, None] - np.arange(L)[None, :]
    G = np.eye(M * L)
    for p in range(M):
        for q in range(M):
            if p // C in kept and q // C in kept:
                fwd, bwd = _corr(planes[p], planes[q], L), _corr(planes[q], planes[p], L)
                G[p * L:(p + 1) * L, q * L:(q + 1) * L] = np.where(tt >= 0, fwd[np.abs(tt)], bwd[np.abs(tt)])
    D = np.zeros((J, M * L, C))
    for i in kept:
        for p in range(M):
            if p // C in kept:
                for c in range(C):
                    D[i, p * L:(p + 1) * L, c] = _corr(planes[p], ests[i, c], L)
    X, Y, status = np.zeros_like(D), np.zeros_like(D), OK
    try:
        np.linalg.cholesky(G)
        for i in kept:
            X[i] = np.linalg.solve(G, D[i])
            Y[i, _rows(i, C, L)] = np.linalg.solve(G[_rows(i, C, L), _rows(i, C, L)], D[i, _rows(i, C, L)])
    except np.linalg.LinAlgError:
        status = SINGULAR
    p_all, p_own = np.zeros((J, C, n)), np.zeros((J, C, n))
    for i in kept:
        for c in range(C):
            for p in range(M):
                p_all[i, c] += np.convolve(planes[p], X[i, p * L:(p + 1) * L, c])[:n]
                if p // C == i:
                    p_own[i, c] += np.convolve(planes[p], Y[i, p * L:(p + 1) * L, c])[:n]
    return _finish(refs, ests, p_all, p_own, X, W, H, status)


def distance(a, b):
    """(d in dB over the entries finite in both, d of X relative to max |X| of a (0 unless both factorisations succeeded), the
    statuses, the NaN masks and the infinities agree)"""
    d = 0.0
    same = a["status"] == b["status"]
    for k in ("sdr", "isr", "sir", "sar"):
        fin = np.isfinite(a[k])
        same = same and np.array_equal(np.isnan(a[k]), np.isnan(b[k])) and np.array_equal(a[k][~fin], b[k][~fin], equal_nan=True)
        both = fin & np.isfinite(b[k])
        if both.any():
            d = max(d, float(np.abs(a[k][both] - b[k][both]).max()))
    scale = float(np.abs(a["X"]).max())
    dx = float(np.abs(a["X"] - b["X"]).max()) / scale if scale > 0 and a["status"] == OK and b["status"] == OK else 0.0
    return d, dx, same
