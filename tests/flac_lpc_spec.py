"""The FLAC output stage's compression levels (csrc/flac.hip; include/demucs_hip.h dmx_flac_encode_level; DESIGN.md section
2.11) restated in NumPy on top of tests/flac_spec.py, which stays the text of level 0.

Level 0 is flac_spec.encode. Level 1 adds an LPC candidate of order 8 to every non-CONSTANT subframe, level 2 orders 8 and
12. Everything flac_spec states holds (stream, frames, stereo candidates, Rice coding, partition orders <= 4 with
(bs >> p) > order, k limits, tie-breaks); for a signal x of width w in a block of bs > 32 samples (shorter blocks get no
LPC candidate) the following is added:

    window    W[i] = floor(131072 i (bs - 1 - i) / (bs - 1)^2) (Welch in Q15, int64); xw[i] = (x[i] W[i]) >> 15.
    autocorr  R[l] = sum xw[i] xw[i - l], l = 0..12, exact in int64. R[0] == 0: no candidate. g = max(0, bitlength(R[0])
              - 52); every lag >> g (arithmetic), then converted to binary64 exactly.
    Levinson  binary64, every operation rounded once, no contraction, in the order of levinson() below; the recursion
              stops at the first m whose error is not > 0 (orders >= m give no candidate).
    quantise  precision P = 12 (16 bit) / 15 (24 bit), lim = 2^(P-1) - 1, cmax = max |a[j]|; the shift s is the largest t in
              15..0 with floor(cmax 2^t + 0.5) <= lim (none: no candidate); q[j] = clamp(floor(v + 0.5), -lim - 1, lim) with
              v = a[j] 2^s + e, e = v - q[j] carried from one coefficient to the next (0 before the first).
    residual  r[i] = x[i] - ((sum q[j] x[i - 1 - j]) >> s), i >= m, int64; any r[i] outside [-2^29, 2^29) discards the
              candidate (u < 2^30 is what the kClamp argument of csrc/flac.hip assumes).
    cost      8 + m w + 4 + 5 + m P + 6 + the partitioned Rice total (the same method, k limits and partition rule with
              order = m). CONSTANT if all samples are equal; else the smallest of the FIXED orders, then LPC 8, then LPC
              12, in that order, ties to the earliest; VERBATIM only if strictly smaller than all of them.
    writing   subframe header 0 1ooooo 0, ooooo = m - 1; m warm-up samples at w bits; P - 1 in 4 bits, s in 5 bits, the q[j]
              as P-bit two's complement; the residual section as for FIXED.

The residual-range discard was NOT reached by any crafted signal. A residual of 2^29 needs |x| + |prediction| >= 2^29
with |x| <= 2^24 (the side channel at 24 bits), so a prediction 31 times the largest sample: sum |q| / 2^s >= 31, which
a predictor from Levinson-Durbin on a windowed autocorrelation (its reflection coefficients are below 1 in magnitude while
the error stays positive) reaches only on a signal it models as almost perfectly predictable - and then misses where the
window hid the evidence. Tried: a smooth tone with full-scale alternating bursts where the window is near zero, and
full-scale alternation confined to the first and last 24 samples of every block around a near-silent AR(2) middle
(crafted("edge_burst")): the largest |r| over all its candidates at 24 bits is 16778566 = 2^24.0, the burst itself. The
guard stays, and tests/test_flac_lpc_cpu.py calls lpc_candidate() with hand-made coefficients that overflow it and with
residuals at both edges of the range.
"""
import numpy as np

import flac_spec as fs

BLOCK = fs.BLOCK
ORDERS = {0: (), 1: (8,), 2: (8, 12)}
MAX_LAG = 12
RES_LIM = 1 << 29


# ------------------------------------------------------------------------------------------------ the LPC candidate
def window(bs):
    """W[i] as Python ints (bs > 1)"""
    d = (bs - 1) * (bs - 1)
    return [131072 * i * (bs - 1 - i) // d for i in range(bs)]


def autocorrelation(x):
    """x: int sequence (bs > 32) -> R[0..12] as Python ints (exact)"""
    bs = len(x)
    xw = np.array([(int(v) * w) >> 15 for v, w in zip(x, window(bs))], np.int64)  # |xw| <= 2^24: products < 2^48, sums < 2^60
    return [int(np.dot(xw[l:], xw[:bs - l])) for l in range(MAX_LAG + 1)]


def levinson(R, orders):
    """R[0..12] ints, R[0] > 0 -> {m: [a_0 .. a_{m-1}] as Python floats} for the m of `orders` that the recursion reaches"""
    g = max(0, R[0].bit_length() - 52)
    r = [float(v >> g) for v in R]  # |v >> g| < 2^53: exact
    err, a, out = r[0], [], {}
    for m in range(1, max(orders) + 1):
        acc = r[m]
        for j in range(1, m):
            acc = acc - a[j - 1] * r[m - j]
        if not err > 0:
            break
        k = acc / err
        a = [a[j - 1] - k * a[m - 1 - j] for j in range(1, m)] + [k]
        err = err * (1.0 - k * k)
        if m in orders:
            out[m] = list(a)
    return out


def quantise(a, bits):
    """-> (q list of ints, shift) or None"""
    P = 12 if bits == 16 else 15
    lim = (1 << (P - 1)) - 1
    with np.errstate(all="ignore"):
        cmax = np.float64(0.0)
        for v in a:
            if abs(np.float64(v)) > cmax:
                cmax = abs(np.float64(v))
        shift = None
        for t in range(15, -1, -1):
            if np.floor(cmax * np.float64(2.0 ** t) + np.float64(0.5)) <= lim:
                shift = t
                break
        if shift is None:
            return None
        q, e = [], np.float64(0.0)
        for v in a:
            v = np.float64(v) * np.float64(2.0 ** shift) + e
            qq = int(min(max(np.floor(v + np.float64(0.5)), -lim - 1), lim))
            q.append(qq)
            e = v - np.float64(qq)
    return q, shift


def lpc_residual(x, q, shift):
    """x int64 (bs,), q ints -> r int64 (bs - m,)"""
    m, bs = len(q), x.size
    pred = np.zeros(bs - m, np.int64)
    for j, c in enumerate(q):
        pred += np.int64(c) * x[m - 1 - j:bs - 1 - j]
    return x[m:] - (pred >> shift)


def rice_plan(r, order, bs, bits):
    """the partitioned Rice total of the residual r (bs - order values) without the 6 bits of method and partition order:
    -> (bits, p, [k per partition])"""
    kmax, pb = (14, 4) if bits == 16 else (30, 5)
    ks = np.arange(kmax + 1, dtype=np.int64)
    u = (r << 1) ^ (r >> 63)
    cs = np.concatenate([np.zeros((kmax + 1, 1), np.int64), np.cumsum(u[None, :] >> ks[:, None], axis=1)], axis=1)
    best = None
    for p in range(5):
        if bs % (1 << p) or (bs >> p) <= order:
            break
        ps = bs >> p
        tot, kk = 0, []
        for j in range(1 << p):
            lo, hi = max(j * ps - order, 0), (j + 1) * ps - order
            cost = (hi - lo) * (ks + 1) + cs[:, hi] - cs[:, lo]
            k = int(np.argmin(cost))
            kk.append(k)
            tot += pb + int(cost[k])
        if best is None or tot < best[0]:
            best = (tot, p, kk)
    return best


def lpc_candidate(x, w, bits, q, shift):
    """the cost and decision of the LPC subframe with these quantised coefficients, or None if a residual leaves
    [-2^29, 2^29)"""
    m, bs = len(q), x.size
    r = lpc_residual(x, q, shift)
    if r.min() < -RES_LIM or r.max() >= RES_LIM:
        return None
    P = 12 if bits == 16 else 15
    tot, p, kk = rice_plan(r, m, bs, bits)
    return 8 + m * w + 4 + 5 + m * P + 6 + tot, {"type": "LPC", "order": m, "q": list(q), "shift": shift, "p": p, "k": kk}


def lpc_candidates(x, w, bits, level):
    """x int64 (bs,) -> [(bits, decision)] in the order 8, 12 for the candidates that exist"""
    bs = x.size
    if level == 0 or bs <= 32:
        return []
    R = autocorrelation(x)
    if R[0] == 0:
        return []
    out = []
    for m, a in sorted(levinson(R, ORDERS[level]).items()):
        qs = quantise(a, bits)
        if qs is None:
            continue
        c = lpc_candidate(x, w, bits, *qs)
        if c is not None:
            out.append(c)
    return out


def plan_subframe(x, w, bits, level):
    """-> (bit count, decision, the orders whose LPC candidate existed)"""
    base = fs._plan_subframe(x, w, bits)
    if base[1]["type"] == "CONSTANT":
        return base[0], base[1], ()
    cands = lpc_candidates(x, w, bits, level)
    best = base  # the smallest FIXED, or VERBATIM when it is strictly smaller than every FIXED
    for c in cands:  # then LPC 8, then LPC 12; a tie with VERBATIM goes to the predictor
        if c[0] < best[0] or (best[1]["type"] == "VERBATIM" and c[0] == best[0]):
            best = c
    return best[0], best[1], tuple(c[1]["order"] for c in cands)


def write_subframe(x, w, bits, d):
    if d["type"] != "LPC":
        return fs._write_subframe(x, w, bits, d)
    m, p, kk, q, shift = d["order"], d["p"], d["k"], d["q"], d["shift"]
    P = 12 if bits == 16 else 15
    bs = x.size
    mask = (1 << w) - 1
    parts = [fs._fixed_width_bits([0b01000000 | ((m - 1) << 1)], 8), fs._fixed_width_bits(x[:m] & mask, w),
             fs._fixed_width_bits([P - 1], 4), fs._fixed_width_bits([shift], 5),
             fs._fixed_width_bits(np.array(q, np.int64) & ((1 << P) - 1), P),
             fs._fixed_width_bits([0 if bits == 16 else 1], 2), fs._fixed_width_bits([p], 4)]
    r = lpc_residual(x, q, shift)
    u = (r << 1) ^ (r >> 63)
    ps = bs >> p
    for j in range(1 << p):
        lo, hi = max(j * ps - m, 0), (j + 1) * ps - m
        k = kk[j]
        parts.append(fs._fixed_width_bits([k], 4 if bits == 16 else 5))
        uu = u[lo:hi]
        qq = uu >> k
        ln = qq + 1 + k
        start = np.cumsum(ln) - ln
        arr = np.zeros(int(ln.sum()), np.uint8)
        arr[start + qq] = 1
        for b in range(k):
            arr[start + qq + 1 + b] = (uu >> (k - 1 - b)) & 1
        parts.append(arr)
    return np.concatenate(parts)


# ------------------------------------------------------------------------------------------------ the encoder
def encode(pcm, bits, rate=44100, level=0):
    """pcm int (n, 2) -> (the .flac file's bytes, decisions: per frame {"channels", "sub": [d0, d1], "lpc_valid": [.., ..],
    "bytes": the frame's length}); level 0 is flac_spec.encode"""
    assert level in ORDERS
    if level == 0:
        return fs.encode(pcm, bits, rate)
    pcm = np.asarray(pcm).astype(np.int64)
    n = pcm.shape[0]
    assert pcm.ndim == 2 and pcm.shape[1] == 2 and 1 <= n < 1 << 36 and bits in (16, 24) and 1 <= rate <= 655350
    frames, decisions = [], []
    for f in range((n + BLOCK - 1) // BLOCK):
        blk = pcm[f * BLOCK:(f + 1) * BLOCK]
        bs = blk.shape[0]
        L, R = blk[:, 0], blk[:, 1]
        sig = {"L": (L, bits), "R": (R, bits), "M": ((L + R) >> 1, bits), "S": (L - R, bits + 1)}
        plans = {c: plan_subframe(x, w, bits, level) for c, (x, w) in sig.items()}
        pick = None
        for code, (a, b) in zip(fs.CHANNEL_CODES, (("L", "R"), ("L", "S"), ("S", "R"), ("M", "S"))):
            tot = plans[a][0] + plans[b][0]
            if pick is None or tot < pick[0]:
                pick = (tot, code, a, b)
        _, code, a, b = pick
        hdr = bytearray([0xFF, 0xF8])
        hdr.append(((0b1100 if bs == BLOCK else 0b0111) << 4) | (0b1001 if rate == 44100 else 0b1010 if rate == 48000 else 0))
        hdr.append((code << 4) | ((0b100 if bits == 16 else 0b110) << 1))
        hdr += fs._utf8_number(f)
        if bs != BLOCK:
            hdr += bytes([(bs - 1) >> 8, (bs - 1) & 0xFF])
        hdr.append(fs.enc_crc8(hdr))
        body = np.concatenate([write_subframe(sig[a][0], sig[a][1], bits, plans[a][1]),
                               write_subframe(sig[b][0], sig[b][1], bits, plans[b][1])])
        assert body.size == pick[0]
        frame = bytes(hdr) + np.packbits(body).tobytes()
        frame += fs.enc_crc16(frame).to_bytes(2, "big")
        frames.append(frame)
        decisions.append({"channels": code, "sub": [plans[a][1], plans[b][1]], "lpc_valid": [plans[a][2], plans[b][2]]})
    lens = [len(fr) for fr in frames]
    si = (BLOCK << 128) | (BLOCK << 112) | (min(lens) << 88) | (max(lens) << 64) | (rate << 44) | (1 << 41) | ((bits - 1) << 36) | n
    return b"fLaC" + bytes([0x80, 0, 0, 0x22]) + si.to_bytes(18, "big") + bytes(16) + b"".join(frames), decisions


def frame_sizes(data):
    """the byte lengths of the frames of a file this project wrote (fixed block size, frame numbers from 0): found by the
    sync code, the frame number and the CRC-8 of each header in turn"""
    data = bytes(data)
    n = int.from_bytes(data[8:26], "big") & ((1 << 36) - 1)
    starts, p = [], 42
    for f in range((n + BLOCK - 1) // BLOCK):
        num = fs._utf8_number(f)
        while True:
            p = data.index(b"\xff\xf8", p)
            hl = 4 + len(num) + (2 if data[p + 2] >> 4 == 0b0111 else 0)
            if data[p + 4:p + 4 + len(num)] == num and fs.enc_crc8(data[p:p + hl]) == data[p + hl]:
                break
            p += 1
        starts.append(p)
        p += hl + 1
    return [b - a for a, b in zip(starts, starts[1:] + [len(data)])]


# ------------------------------------------------------------------------------------------------ the crafted inputs
NEW_SIGNALS = ("ar2_resonance", "ar2_wide", "edge_burst", "quiet_tone")
SIGNALS = fs.SIGNALS + NEW_SIGNALS
LENGTHS = fs.LENGTHS


def _ar2(rng, n, scale):
    e = rng.standard_normal(n + 64)
    y = np.zeros(n + 64)
    for t in range(2, n + 64):
        y[t] = 1.8 * y[t - 1] - 0.95 * y[t - 2] + e[t]
    y = y[64:]
    return np.rint(y / max(np.abs(y).max(), 1e-9) * scale)


def crafted(name, n, bits, seed=0):
    """one crafted input as int32 (n, 2) within the bit depth: flac_spec's, and
    ar2_resonance  y[t] = 1.8 y[t-1] - 0.95 y[t-2] + noise at half of full scale; right: the same resonance, another noise
    ar2_wide       the resonance on the left, the left plus a small independent resonance on the right (side and mid differ)
    edge_burst     a near-silent resonance with full-scale alternation in the first and last 24 samples of each block
    quiet_tone     two tones a few steps high: small coefficients' shifts differ from the loud signals'"""
    if name in fs.SIGNALS:
        return fs.crafted(name, n, bits, seed)
    rng = np.random.default_rng([seed, 100 + NEW_SIGNALS.index(name), n, bits])
    full = 1 << (bits - 1)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((n, 2), np.int64)
    if name == "ar2_resonance":
        x[:, 0] = _ar2(rng, n, full // 2)
        x[:, 1] = _ar2(rng, n, full // 2)
    elif name == "ar2_wide":
        x[:, 0] = _ar2(rng, n, full // 2)
        x[:, 1] = x[:, 0] + _ar2(rng, n, full // 64)
    elif name == "edge_burst":
        x[:, 0] = _ar2(rng, n, full // 4096)
        x[:, 1] = _ar2(rng, n, full // 4096)
        pos = np.arange(n) % BLOCK
        edge = (pos < 24) | (pos >= BLOCK - 24) | (np.arange(n) >= n - 24)
        alt = np.where(np.arange(n) % 2 == 0, -full, full - 1)
        x[edge, 0] = alt[edge]
        x[edge, 1] = -alt[edge] - 1
    elif name == "quiet_tone":
        x[:, 0] = np.rint(6.0 * np.sin(2 * np.pi * 1000.0 / 44100.0 * t) + 3.0 * np.sin(2 * np.pi * 6100.0 / 44100.0 * t))
        x[:, 1] = np.rint(40.0 * np.sin(2 * np.pi * 300.0 / 44100.0 * t)) + rng.integers(-1, 2, n)
    else:
        raise KeyError(name)
    return np.clip(x, -full, full - 1).astype(np.int32)
