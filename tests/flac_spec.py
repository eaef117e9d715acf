"""The FLAC output stage (csrc/flac.hip; include/demucs_hip.h dmx_flac_encode) restated in NumPy,
and a decoder written from the format specification (RFC 9639) that shares no code with it.

The encoder makes every choice by exact bit counts with stated tie-breaks, so this text pins the kernels byte for byte:

    stream    "fLaC", one STREAMINFO block (last-block flag set): min = max block size 4096, the smallest / largest frame
              byte length of the stream, 20-bit sample rate, 2 channels, bits, 36-bit total samples, an all-zero MD5.
    frames    fixed block size 4096 (the last frame holds n mod 4096 frames when that is not zero). Header FF F8, block
              size nibble 1100 (4096) or 0111 (blocksize - 1 as 16 bits at the end of the header), sample rate nibble
              1001 (44100), 1010 (48000) or 0000 (from STREAMINFO: legal, outside the streamable subset), channel
              assignment, sample size 100 / 110, the frame number in the UTF-8 style coding, CRC-8 (0x07, init 0).
              Footer: zero bits to the byte boundary, CRC-16 (0x8005, init 0, not reflected) big-endian over the frame.
    stereo    candidates 0001 (L, R), 1000 (L, S), 1001 (S, R), 1010 (M, S), S = L - R at bits + 1, M = (L + R) >> 1 at
              bits: the smallest total bit count of the two subframes, ties to the earliest.
    subframe  CONSTANT if all samples are equal; else the FIXED order 0..min(4, blocksize - 1) of the smallest exact bit
              count (ties to the lowest order); VERBATIM only if strictly smaller than every FIXED.
    residual  method 00 / 4-bit parameters / k <= 14 at 16 bits, method 01 / 5-bit / k <= 30 at 24 bits, no escape code;
              partition order p in [0, 4] while blocksize mod 2^p == 0 and (blocksize >> p) > order; per partition the k
              minimising count * (k + 1) + sum(u >> k), u = (r << 1) ^ (r >> 31), ties to the lowest k; per subframe the p
              of the smallest total including the parameter bits, ties to the lowest p.
    bound     42 + 18 * ceil(n / 4096) + n * 2 * bits / 8, rounded up to 16.
"""
import numpy as np

BLOCK = 4096
CHANNEL_CODES = (0b0001, 0b1000, 0b1001, 0b1010)  # (L, R), (L, S), (S, R), (M, S)


def bound(bits, n):
    """dmx_flac_bound: no encoded stream is larger"""
    return (42 + 18 * ((n + BLOCK - 1) // BLOCK) + n * 2 * bits // 8 + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ the encoder
def _enc_crc(data, poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    crc = 0
    for byte in data:
        crc ^= byte << (width - 8)
        for _ in range(8):
            crc = ((crc << 1) ^ poly) & mask if crc & top else (crc << 1) & mask
    return crc


_ENC_T16 = [_enc_crc(bytes([i]), 0x8005, 16) for i in range(256)]


def enc_crc8(data):
    return _enc_crc(data, 0x07, 8)


def enc_crc16(data):
    crc = 0
    for byte in data:
        crc = ((crc << 8) & 0xFFFF) ^ _ENC_T16[(crc >> 8) ^ byte]
    return crc


def _fixed_width_bits(vals, w):
    """unsigned values -> their w-bit big-endian bit strings, concatenated"""
    vals = np.asarray(vals, np.int64)
    return ((vals[:, None] >> np.arange(w - 1, -1, -1)) & 1).astype(np.uint8).ravel()


def _plan_subframe(x, w, bits):
    """x int64 (blocksize,), w its width -> (bit count, decision)"""
    bs = x.size
    if np.all(x == x[0]):
        return 8 + w, {"type": "CONSTANT"}
    kmax, pb = (14, 4) if bits == 16 else (30, 5)
    ks = np.arange(kmax + 1, dtype=np.int64)
    best = None
    for order in range(min(4, bs - 1) + 1):
        r = x
        for _ in range(order):
            r = np.diff(r)  # 1 / 1,-1 / 1,-2,1 / 1,-3,3,-1 / 1,-4,6,-4,1
        u = (r << 1) ^ (r >> 63)
        cs = np.concatenate([np.zeros((kmax + 1, 1), np.int64), np.cumsum(u[None, :] >> ks[:, None], axis=1)], axis=1)
        bestp = None
        for p in range(5):
            if bs % (1 << p) or (bs >> p) <= order:
                break
            ps = bs >> p
            tot, kk = 6, []
            for j in range(1 << p):
                lo, hi = max(j * ps - order, 0), (j + 1) * ps - order
                cost = (hi - lo) * (ks + 1) + cs[:, hi] - cs[:, lo]
                k = int(np.argmin(cost))  # the first minimum: the lowest k
                kk.append(k)
                tot += pb + int(cost[k])
            if bestp is None or tot < bestp[0]:
                bestp = (tot, p, kk)
        total = 8 + order * w + bestp[0]
        if best is None or total < best[0]:
            best = (total, {"type": "FIXED", "order": order, "p": bestp[1], "k": bestp[2]})
    verbatim = 8 + bs * w
    if verbatim < best[0]:
        return verbatim, {"type": "VERBATIM"}
    return best


def _write_subframe(x, w, bits, d):
    mask = (1 << w) - 1
    if d["type"] == "CONSTANT":
        return np.concatenate([_fixed_width_bits([0], 8), _fixed_width_bits([int(x[0]) & mask], w)])
    if d["type"] == "VERBATIM":
        return np.concatenate([_fixed_width_bits([0b00000010], 8), _fixed_width_bits(x & mask, w)])
    order, p, kk = d["order"], d["p"], d["k"]
    bs = x.size
    parts = [_fixed_width_bits([0b00010000 | (order << 1)], 8), _fixed_width_bits(x[:order] & mask, w),
             _fixed_width_bits([0 if bits == 16 else 1], 2), _fixed_width_bits([p], 4)]
    r = x
    for _ in range(order):
        r = np.diff(r)
    u = (r << 1) ^ (r >> 63)
    ps = bs >> p
    for j in range(1 << p):
        lo, hi = max(j * ps - order, 0), (j + 1) * ps - order
        k = kk[j]
        parts.append(_fixed_width_bits([k], 4 if bits == 16 else 5))
        uu = u[lo:hi]
        q = uu >> k
        ln = q + 1 + k
        start = np.cumsum(ln) - ln
        arr = np.zeros(int(ln.sum()), np.uint8)
        arr[start + q] = 1
        for b in range(k):
            arr[start + q + 1 + b] = (uu >> (k - 1 - b)) & 1
        parts.append(arr)
    return np.concatenate(parts)


def _utf8_number(v):
    if v < 0x80:
        return bytes([v])
    nb = 2
    while v >= 1 << (5 * nb + 1):  # 2 bytes hold 11 bits, 3: 16, 4: 21, 5: 26, 6: 31
        nb += 1
    out = [((0xFF << (8 - nb)) & 0xFF) | (v >> (6 * (nb - 1)))]
    for i in range(nb - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


def encode(pcm, bits, rate=44100):
    """pcm int (n, 2), bits 16 | 24 -> (the .flac file's bytes, decisions: per frame {"channels": code, "sub": [d0, d1]})"""
    pcm = np.asarray(pcm).astype(np.int64)
    n = pcm.shape[0]
    assert pcm.ndim == 2 and pcm.shape[1] == 2 and 1 <= n < 1 << 36 and bits in (16, 24) and 1 <= rate <= 655350
    frames, decisions = [], []
    for f in range((n + BLOCK - 1) // BLOCK):
        blk = pcm[f * BLOCK:(f + 1) * BLOCK]
        bs = blk.shape[0]
        L, R = blk[:, 0], blk[:, 1]
        sig = {"L": (L, bits), "R": (R, bits), "M": ((L + R) >> 1, bits), "S": (L - R, bits + 1)}
        plans = {c: _plan_subframe(x, w, bits) for c, (x, w) in sig.items()}
        pick = None
        for code, (a, b) in zip(CHANNEL_CODES, (("L", "R"), ("L", "S"), ("S", "R"), ("M", "S"))):
            tot = plans[a][0] + plans[b][0]
            if pick is None or tot < pick[0]:
                pick = (tot, code, a, b)
        _, code, a, b = pick
        hdr = bytearray([0xFF, 0xF8])
        hdr.append(((0b1100 if bs == BLOCK else 0b0111) << 4) | (0b1001 if rate == 44100 else 0b1010 if rate == 48000 else 0))
        hdr.append((code << 4) | ((0b100 if bits == 16 else 0b110) << 1))
        hdr += _utf8_number(f)
        if bs != BLOCK:
            hdr += bytes([(bs - 1) >> 8, (bs - 1) & 0xFF])
        hdr.append(enc_crc8(hdr))
        body = np.concatenate([_write_subframe(sig[a][0], sig[a][1], bits, plans[a][1]),
                               _write_subframe(sig[b][0], sig[b][1], bits, plans[b][1])])
        assert body.size == pick[0]
        frame = bytes(hdr) + np.packbits(body).tobytes()  # zero bits to the byte boundary
        frame += enc_crc16(frame).to_bytes(2, "big")
        frames.append(frame)
        decisions.append({"channels": code, "sub": [plans[a][1], plans[b][1]]})
    lens = [len(fr) for fr in frames]
    si = (BLOCK << 128) | (BLOCK << 112) | (min(lens) << 88) | (max(lens) << 64) | (rate << 44) | (1 << 41) | ((bits - 1) << 36) | n
    return b"fLaC" + bytes([0x80, 0, 0, 0x22]) + si.to_bytes(18, "big") + bytes(16) + b"".join(frames), decisions


# ------------------------------------------------------------------------------------------------ the decoder
class FlacError(ValueError):
    pass


def dec_crc8(data):
    c = 0
    for v in data:
        c ^= v
        for _ in range(8):
            c = ((c << 1) ^ 0x107) if c & 0x80 else c << 1
    return c & 0xFF


def dec_crc16(data):
    c = 0
    for v in data:
        c ^= v << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x18005) if c & 0x8000 else c << 1
    return c & 0xFFFF


_DEC_T16 = None


def _dec_crc16_fast(data):
    global _DEC_T16
    if _DEC_T16 is None:
        _DEC_T16 = [dec_crc16(bytes([i])) for i in range(256)]
    c = 0
    for v in data:
        c = ((c & 0xFF) << 8) ^ _DEC_T16[(c >> 8) ^ v]
    return c


class _Bits:
    def __init__(self, s, pos):
        self.s = s  # the whole file as a string of '0' / '1'
        self.pos = pos

    def u(self, nbits):
        if nbits == 0:
            return 0
        if self.pos + nbits > len(self.s):
            raise FlacError("truncated stream")
        v = int(self.s[self.pos:self.pos + nbits], 2)
        self.pos += nbits
        return v

    def s_(self, nbits):
        v = self.u(nbits)
        return v - (1 << nbits) if v >> (nbits - 1) else v

    def unary(self):
        try:
            one = self.s.index("1", self.pos)
        except ValueError:
            raise FlacError("truncated unary code")
        q = one - self.pos
        self.pos = one + 1
        return q


_FIXED_COEF = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


def _dec_subframe(br, bs, w):
    if br.u(1):
        raise FlacError("subframe padding bit set")
    typ = br.u(6)
    wasted = 0
    if br.u(1):
        wasted = br.unary() + 1
        w -= wasted
    if typ == 0:
        out = [br.s_(w)] * bs
    elif typ == 1:
        out = [br.s_(w) for _ in range(bs)]
    elif 8 <= typ <= 12:
        order = typ - 8
        if order > bs:
            raise FlacError("fixed order above the block size")
        out = [br.s_(w) for _ in range(order)]
        method = br.u(2)
        if method > 1:
            raise FlacError("reserved residual coding method")
        pbits, esc = (4, 15) if method == 0 else (5, 31)
        p = br.u(4)
        if bs % (1 << p) or (bs >> p) < order:
            raise FlacError("partition order does not fit the block")
        res = []
        for j in range(1 << p):
            cnt = (bs >> p) - (order if j == 0 else 0)
            k = br.u(pbits)
            if k == esc:
                raw = br.u(5)
                res += [br.s_(raw) if raw else 0 for _ in range(cnt)]
            else:
                for _ in range(cnt):
                    v = (br.unary() << k) | br.u(k)
                    res.append((v >> 1) ^ -(v & 1))
        coef = _FIXED_COEF[order]
        for r in res:
            out.append(r + sum(c * out[-1 - i] for i, c in enumerate(coef)))
    else:
        raise FlacError(f"subframe type {typ:06b} (LPC and reserved types are not produced by this project)")
    return [v << wasted for v in out] if wasted else out


def decode(data):
    """the bytes of a .flac file -> (pcm int32 (n, 2), bits, rate); verifies every CRC and the STREAMINFO fields"""
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos, info = 4, None
    while True:
        last, typ, ln = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        if typ == 0:
            if ln != 34 or info is not None or pos != 4:
                raise FlacError("bad STREAMINFO block")
            info = int.from_bytes(data[pos + 4:pos + 22], "big")
        pos += 4 + ln
        if last:
            break
    if info is None:
        raise FlacError("no STREAMINFO")
    min_bs, max_bs = info >> 128, (info >> 112) & 0xFFFF
    min_fs, max_fs = (info >> 88) & 0xFFFFFF, (info >> 64) & 0xFFFFFF
    rate, nch, bits, total = (info >> 44) & 0xFFFFF, ((info >> 41) & 7) + 1, ((info >> 36) & 31) + 1, info & ((1 << 36) - 1)
    if nch != 2 or min_bs != max_bs or rate == 0:
        raise FlacError("not a fixed-block-size stereo stream")
    chans, got, sizes, want_no = ([], []), 0, [], 0
    allbits = (np.unpackbits(np.frombuffer(data, np.uint8)) + np.uint8(48)).tobytes().decode("ascii")
    while pos < len(data):
        start = pos
        br = _Bits(allbits, 8 * pos)
        if br.u(15) != 0x7FFC or br.u(1) != 0:
            raise FlacError(f"frame {want_no}: bad sync code or variable block size")
        bs_code, sr_code, ch_code, ss_code = br.u(4), br.u(4), br.u(4), br.u(3)
        if br.u(1):
            raise FlacError("reserved header bit set")
        first = br.u(8)
        nb = 0
        while first & (0x80 >> nb):
            nb += 1
        if nb == 1 or nb > 7:
            raise FlacError("bad frame number coding")
        number = first & (0x7F >> nb)
        for _ in range(max(nb - 1, 0)):
            c = br.u(8)
            if c >> 6 != 2:
                raise FlacError("bad frame number continuation byte")
            number = (number << 6) | (c & 0x3F)
        if bs_code == 6:
            bs = br.u(8) + 1
        elif bs_code == 7:
            bs = br.u(16) + 1
        elif bs_code == 1:
            bs = 192
        elif 2 <= bs_code <= 5:
            bs = 576 << (bs_code - 2)
        elif bs_code >= 8:
            bs = 256 << (bs_code - 8)
        else:
            raise FlacError("reserved block size code")
        frate = {0: rate, 1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000,
                 11: 96000}.get(sr_code)
        if frate is None:
            raise FlacError("sample rate code not handled")
        fbits = {0: bits, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24}.get(ss_code)
        if frate != rate or fbits != bits:
            raise FlacError("frame header disagrees with STREAMINFO")
        hlen = br.pos // 8 - start
        if dec_crc8(data[start:start + hlen]) != data[start + hlen]:
            raise FlacError(f"frame {number}: CRC-8 mismatch")
        if number != want_no:
            raise FlacError(f"frame number {number}, expected {want_no}")
        if bs > max_bs or got + bs > total or (bs != max_bs and got + bs != total):
            raise FlacError(f"frame {number}: block size {bs}")
        widths = {1: (bits, bits), 8: (bits, bits + 1), 9: (bits + 1, bits), 10: (bits, bits + 1)}.get(ch_code)
        if widths is None:
            raise FlacError("channel assignment is not stereo")
        br = _Bits(allbits, 8 * (start + hlen + 1))
        a = np.array(_dec_subframe(br, bs, widths[0]), np.int64)
        b = np.array(_dec_subframe(br, bs, widths[1]), np.int64)
        pad = -br.pos % 8
        if br.u(pad) != 0:
            raise FlacError("non-zero padding bits")
        end = br.pos // 8
        if _dec_crc16_fast(data[start:end]) != int.from_bytes(data[end:end + 2], "big"):
            raise FlacError(f"frame {number}: CRC-16 mismatch")
        if ch_code == 1:
            left, right = a, b
        elif ch_code == 8:
            left, right = a, a - b
        elif ch_code == 9:
            left, right = a + b, b
        else:
            mid = (a << 1) | (b & 1)
            left, right = (mid + b) >> 1, (mid - b) >> 1
        chans[0].append(left), chans[1].append(right)
        pos = end + 2
        sizes.append(pos - start)
        got += bs
        want_no += 1
    if got != total:
        raise FlacError(f"{got} samples decoded, STREAMINFO says {total}")
    if min(sizes) != min_fs or max(sizes) != max_fs:
        raise FlacError(f"frame sizes {min(sizes)}..{max(sizes)}, STREAMINFO says {min_fs}..{max_fs}")
    out = np.stack([np.concatenate(chans[0]), np.concatenate(chans[1])], axis=1)
    lim = 1 << (bits - 1)
    if out.min() < -lim or out.max() >= lim:
        raise FlacError("decoded sample outside the bit depth")
    return out.astype(np.int32), bits, rate


# ------------------------------------------------------------------------------------------------ the crafted inputs
LENGTHS = (1, 2, 15, 4095, 4096, 4097, 3 * 4096 + 123)
SIGNALS = ("silence", "dc_one_channel", "white_noise", "sine_noise", "ramp", "l_eq_r", "l_eq_minus_r", "loud_quiet",
           "alternating", "jump_40db")


def crafted(name, n, bits, seed=0):
    """one crafted input as int32 (n, 2) within the bit depth"""
    rng = np.random.default_rng([seed, SIGNALS.index(name), n, bits])
    full = 1 << (bits - 1)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((n, 2), np.int64)
    if name == "silence":
        pass
    elif name == "dc_one_channel":
        x[:, 0] = full // 3
    elif name == "white_noise":
        x = rng.integers(-full, full, (n, 2))
    elif name == "sine_noise":  # a smooth left channel (high fixed orders), a noisier right one (lower orders)
        x[:, 0] = np.rint(0.6 * full * np.sin(2 * np.pi * 440.0 / 44100.0 * t))
        x[:, 1] = np.rint(0.3 * full * np.sin(2 * np.pi * 2500.0 / 44100.0 * t)) + rng.integers(-full >> 8, (full >> 8) + 1, n)
    elif name == "ramp":  # left: a line; right: a random walk (order 1)
        x[:, 0] = -full // 2 + (t * (full // 8192)).astype(np.int64)
        x[:, 1] = np.clip(np.cumsum(rng.integers(-(full >> 9), (full >> 9) + 1, n)), -full, full - 1)
    elif name == "l_eq_r":
        x[:, 0] = x[:, 1] = rng.integers(-full >> 2, full >> 2, n)
    elif name == "l_eq_minus_r":
        x[:, 0] = rng.integers(-full >> 2, full >> 2, n)
        x[:, 1] = -x[:, 0]
    elif name == "loud_quiet":
        x[:, 0] = rng.integers(-full >> 1, full >> 1, n)
        x[:, 1] = x[:, 0] >> 1
    elif name == "alternating":
        x[0::2] = -full
        x[1::2] = full - 1
    elif name == "jump_40db":
        amp = np.where((np.arange(n) % BLOCK) < BLOCK // 2, full >> 10, (full >> 10) * 100)[:, None]
        x = np.rint(rng.uniform(-1, 1, (n, 2)) * amp).astype(np.int64)
    else:
        raise KeyError(name)
    return np.clip(x, -full, full - 1).astype(np.int32)


def pcm_bytes(x, bits):
    """int (n, 2) -> the interleaved little-endian bytes csrc/pcm.hip writes (np.uint8)"""
    x = np.asarray(x)
    if bits == 16:
        return x.astype("<i2").view(np.uint8).ravel()
    q = x.astype(np.int64) & 0xFFFFFF
    return np.stack([(q >> (8 * b)).astype(np.uint8) for b in range(3)], axis=-1).ravel()


def pcm_ints(buf, bits):
    """the inverse of pcm_bytes: np.uint8 -> int32 (n, 2)"""
    buf = np.ascontiguousarray(buf, np.uint8).ravel()
    if bits == 16:
        return buf.view("<i2").reshape(-1, 2).astype(np.int32)
    b = buf.reshape(-1, 2, 3).astype(np.int32)
    q = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.where(q >= 1 << 23, q - (1 << 24), q).astype(np.int32)
