"""The FLAC input stage (csrc/flac_in.hip; include/demucs_hip.h dmx_flac_probe / dmx_flac_decode):
a FLAC WRITER WITH FREE CHOICES and a sequential reference decoder, both from RFC 9639, sharing no code with the kernels.

The writer takes the integer samples and every decision an encoder is free to make - per stream: channels, depth, rate,
fixed or variable blocking, the block sizes, extra metadata blocks, an ID3v2 tag, trailing bytes; per frame: the channel
assignment and the header codes; per subframe: type, order, quantised coefficients, precision, shift, wasted bits,
partition order, each partition's Rice parameter or escape width, the method. The ground truth of a written stream is the
samples handed to the writer. Raw overrides (`type_code`, `shift_raw`, `prec_raw`, `porder_raw`, `order_raw`) write an illegal
field under valid CRCs, for the damaged-file cases.

The reference decoder is sequential: frame 0 at the first byte after the metadata, frame k + 1 where frame k ends, each
checked in full (header against STREAMINFO, CRC-8, subframes, zero padding, CRC-16, position == the running total). It
defines `status` and `good` for damaged files: samples [0, good) and zeros behind.

All sample arithmetic keeps the low 32 bits, as the kernels do: prediction (sum c[j] s[i-1-j]) >> shift in int64, plus the
residual; a Rice code's value (q << k | low) modulo 2^32; wasted-bit shifts; the stereo reconstruction.
"""
import numpy as np

from flac_spec import FlacError, _Bits, _dec_crc16_fast, _utf8_number, dec_crc8, enc_crc8, enc_crc16

OK, BROKEN, TOO_MANY_CANDIDATES = 0, 1, 2
FIXED_COEF = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}
_BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
_SR_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


class ProbeError(ValueError):
    pass


def wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


# ------------------------------------------------------------------------------------------------ the writer
class _BitWriter:
    def __init__(self):
        self.parts = []
        self.n = 0

    def u(self, v, nbits):
        if nbits:
            assert 0 <= v < (1 << nbits), (v, nbits)
            self.parts.append(format(v, "0%db" % nbits))
            self.n += nbits

    def s(self, v, nbits):
        if nbits:
            assert -(1 << (nbits - 1)) <= v < (1 << (nbits - 1)), (v, nbits)
            self.u(v & ((1 << nbits) - 1), nbits)

    def unary(self, q):
        self.parts.append("0" * q + "1")
        self.n += q + 1

    def tobytes(self):
        s = "".join(self.parts)
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def sub(type="VERBATIM", order=0, coefs=None, precision=None, shift=0, wasted=0, porder=0, params=None, method=0, **raw):
    """one subframe's decisions; params: per partition a Rice parameter or ("esc", width); None: the cheapest parameter"""
    d = dict(type=type, order=order, coefs=coefs, precision=precision, shift=shift, wasted=wasted, porder=porder, params=params,
             method=method)
    d.update(raw)
    return d


def best_k(res, kmax):
    u = [(r << 1) ^ (r >> 63) for r in res]
    best = None
    for k in range(kmax + 1):
        c = sum((v >> k) + 1 + k for v in u)
        if best is None or c < best[0]:
            best = (c, k)
    return best[1]


def residual_of(x, coefs, shift):
    order = len(coefs)
    return [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, len(x))]


def _write_subframe(bw, x, w, d):
    x = [int(v) for v in x]
    bs = len(x)
    wasted = d["wasted"]
    typ = d["type"]
    order = d["order"]
    code = {"CONSTANT": 0, "VERBATIM": 1, "FIXED": 8 + order, "LPC": 32 + order - 1}[typ]
    if "order_raw" in d:  # the order the type field CLAIMS (the body is written for d["order"])
        code = (8 if typ == "FIXED" else 31) + d["order_raw"]
    bw.u(0, 1)
    bw.u(d.get("type_code", code), 6)
    bw.u(1 if wasted else 0, 1)
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in x)
        bw.unary(wasted - 1)
        x = [v >> wasted for v in x]
        w -= wasted
    if typ == "CONSTANT":
        assert all(v == x[0] for v in x)
        bw.s(x[0], w)
        return
    if typ == "VERBATIM":
        for v in x:
            bw.s(v, w)
        return
    for v in x[:order]:
        bw.s(v, w)
    if typ == "LPC":
        coefs, shift, prec = list(d["coefs"]), d["shift"], d["precision"]
        assert len(coefs) == order
        bw.u(d.get("prec_raw", prec - 1), 4)
        bw.u(d.get("shift_raw", shift), 5)
        for c in coefs:
            bw.s(c, prec)
    else:
        coefs, shift = list(FIXED_COEF[order]), 0
    res = residual_of(x, coefs, shift)
    method, po = d["method"], d["porder"]
    pbits, kmax = (4, 14) if method == 0 else (5, 30)
    bw.u(d.get("method_raw", method), 2)
    bw.u(d.get("porder_raw", po), 4)
    assert bs % (1 << po) == 0 and (bs >> po) >= order
    psz, at = bs >> po, 0
    params = d["params"]
    for j in range(1 << po):
        cnt = psz - (order if j == 0 else 0)
        part = res[at:at + cnt]
        at += cnt
        p = params[j] if params is not None else best_k(part, kmax)
        if isinstance(p, tuple):
            bw.u((1 << pbits) - 1, pbits)
            bw.u(p[1], 5)
            for r in part:
                if p[1]:
                    bw.s(r, p[1])
                else:
                    assert r == 0
        else:
            bw.u(p, pbits)
            for r in part:
                v = (r << 1) ^ (r >> 63)
                bw.unary(v >> p)
                bw.u(v & ((1 << p) - 1), p)


def frame(samples, assignment=None, subs=None, **hdr):
    """samples int (bs, channels); assignment: the 4-bit code (None: independent); subs: one sub() per channel (None:
    VERBATIM); hdr: bs_code, rate_code, size_code, number, reserved (raw header fields)"""
    d = dict(samples=np.asarray(samples, np.int64), assignment=assignment, subs=subs)
    d.update(hdr)
    return d


def write(frames, channels, bits, rate=44100, variable=False, min_block=None, max_block=None, total=None, extra_meta=(), id3=b"",
          trailing=b""):
    """-> (the file's bytes, layout): layout["frames"][k] = (first byte, byte behind the frame), layout["first"] the first
    frame's byte offset"""
    sizes = [int(fr["samples"].shape[0]) for fr in frames]
    if max_block is None:
        max_block = max(max(sizes), 16)
    if min_block is None:
        min_block = max(min(sizes[:-1] or sizes), 16) if not variable else max(min(sizes), 16)
        min_block = min(min_block, max_block)
    blobs, pos = [], 0
    for k, fr in enumerate(frames):
        x = fr["samples"].reshape(sizes[k], channels)
        bs = sizes[k]
        code = fr["assignment"] if fr["assignment"] is not None else channels - 1
        if channels == 2:
            L, R = x[:, 0], x[:, 1]
            sig = {1: ((L, bits), (R, bits)), 8: ((L, bits), (L - R, bits + 1)), 9: ((L - R, bits + 1), (R, bits)),
                   10: (((L + R) >> 1, bits), (L - R, bits + 1))}[code]
        else:
            sig = ((x[:, 0], bits),)
        bs_code = fr.get("bs_code", _BS_CODES.get(bs, 6 if bs <= 256 else 7))
        rate_code = fr.get("rate_code", _SR_CODES.get(rate, 0))
        size_code = fr.get("size_code", _SS_CODES[bits])
        hdr = bytearray([0xFF, 0xF8 | (1 if variable else 0), (bs_code << 4) | rate_code,
                         (code << 4) | (size_code << 1) | fr.get("reserved", 0)])
        hdr += _utf8_number(fr.get("number", pos if variable else k))
        if bs_code == 6:
            hdr.append(bs - 1)
        elif bs_code == 7:
            hdr += (bs - 1).to_bytes(2, "big")
        if rate_code == 12:
            hdr.append(rate // 1000)
        elif rate_code == 13:
            hdr += rate.to_bytes(2, "big")
        elif rate_code == 14:
            hdr += (rate // 10).to_bytes(2, "big")
        hdr.append(enc_crc8(hdr))
        bw = _BitWriter()
        subs = fr["subs"] or [sub() for _ in range(channels)]
        for (sx, w), d in zip(sig, subs):
            _write_subframe(bw, sx, w, d)
        blob = bytes(hdr) + bw.tobytes()
        blob += enc_crc16(blob).to_bytes(2, "big")
        blobs.append(blob)
        pos += bs
    if total is None:
        total = pos
    lens = [len(b) for b in blobs]
    si = (min_block << 128) | (max_block << 112) | (min(lens) << 88) | (max(lens) << 64) | (rate << 44) | ((channels - 1) << 41) | \
        ((bits - 1) << 36) | total
    meta = [(0, si.to_bytes(18, "big") + bytes(16))] + list(extra_meta)
    out = bytearray(id3) + b"fLaC"
    for i, (t, body) in enumerate(meta):
        out += bytes([(0x80 if i == len(meta) - 1 else 0) | t]) + len(body).to_bytes(3, "big") + body
    layout = {"first": len(out), "frames": []}
    for b in blobs:
        layout["frames"].append((len(out), len(out) + len(b)))
        out += b
    out += trailing
    return bytes(out), layout


def id3v2(n):
    """an ID3v2.4 tag with n bytes of (zero) content"""
    return b"ID3\x04\x00\x00" + bytes([(n >> 21) & 127, (n >> 14) & 127, (n >> 7) & 127, n & 127]) + bytes(n)


# ------------------------------------------------------------------------------------------------ the reference decoder
def probe(data):
    """-> dict(rate, channels, bits, total, min_block, max_block, variable, first); ProbeError otherwise"""
    data = bytes(data)
    if len(data) < 4:
        raise ProbeError("shorter than any FLAC file")
    p = 0
    if data[:3] == b"ID3":
        if len(data) < 10:
            raise ProbeError("truncated ID3v2 header")
        if any(b & 0x80 for b in data[6:10]):
            raise ProbeError("malformed ID3v2 size")
        p = 10 + ((data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9]) + (10 if data[5] & 0x10 else 0)
        if p + 4 > len(data):
            raise ProbeError("ID3v2 tag runs past the end")
    if data[p:p + 4] == b"OggS":
        raise ProbeError("Ogg FLAC")
    if data[p:p + 4] != b"fLaC":
        raise ProbeError("no fLaC marker")
    p += 4
    first, last, si = True, False, None
    while not last:
        if p + 4 > len(data):
            raise ProbeError("metadata runs past the end")
        last, typ, ln = data[p] >> 7, data[p] & 0x7F, int.from_bytes(data[p + 1:p + 4], "big")
        if typ == 127:
            raise ProbeError("metadata block type 127")
        if first and (typ != 0 or ln != 34):
            raise ProbeError("STREAMINFO is not first")
        if not first and typ == 0:
            raise ProbeError("second STREAMINFO")
        if p + 4 + ln > len(data):
            raise ProbeError("metadata block runs past the end")
        if first:
            si = int.from_bytes(data[p + 4:p + 22], "big")
        first = False
        p += 4 + ln
    info = dict(min_block=si >> 128, max_block=(si >> 112) & 0xFFFF, rate=(si >> 44) & 0xFFFFF, channels=((si >> 41) & 7) + 1,
                bits=((si >> 36) & 31) + 1, total=si & ((1 << 36) - 1))
    if info["channels"] > 2:
        raise ProbeError("more than 2 channels")
    if info["bits"] == 32:
        raise ProbeError("32-bit samples")
    if info["bits"] not in (8, 12, 16, 20, 24):
        raise ProbeError("bits per sample")
    if info["rate"] == 0:
        raise ProbeError("sample rate 0")
    if info["total"] == 0:
        raise ProbeError("unknown length")
    if info["total"] > 0x7FFFFFFF:
        raise ProbeError("too many samples")
    if info["min_block"] < 16 or info["max_block"] < info["min_block"]:
        raise ProbeError("block size range")
    if p + 2 > len(data):
        raise ProbeError("no audio frame")
    if data[p] != 0xFF or (data[p + 1] & 0xFE) != 0xF8:
        raise ProbeError("no frame sync code")
    info["variable"], info["first"] = data[p + 1] & 1, p
    return info


def _ref_subframe(br, bs, w):
    if br.u(1):
        raise FlacError("subframe padding bit")
    typ = br.u(6)
    wasted = 0
    if br.u(1):
        wasted = br.unary() + 1
    if wasted >= w:
        raise FlacError("wasted bits leave no sample bits")
    w -= wasted
    if typ == 0:
        out = [br.s_(w)] * bs
    elif typ == 1:
        out = [br.s_(w) for _ in range(bs)]
    else:
        if typ >= 32:
            order = (typ & 31) + 1
        elif 8 <= typ <= 12:
            order = typ - 8
        else:
            raise FlacError("reserved subframe type")
        if order >= bs:
            raise FlacError("predictor order >= block size")
        out = [br.s_(w) for _ in range(order)]
        shift = 0
        if typ >= 32:
            prec = br.u(4) + 1
            shift = br.u(5)
            if prec == 16:
                raise FlacError("reserved coefficient precision")
            if shift & 16:
                raise FlacError("negative shift")
            coefs = [br.s_(prec) for _ in range(order)]
        else:
            coefs = list(FIXED_COEF[order])
        method = br.u(2)
        if method > 1:
            raise FlacError("reserved residual method")
        po = br.u(4)
        if bs % (1 << po) or (bs >> po) < order:
            raise FlacError("partition order does not fit")
        pbits, esc = (4, 15) if method == 0 else (5, 31)
        for j in range(1 << po):
            cnt = (bs >> po) - (order if j == 0 else 0)
            k = br.u(pbits)
            raw = br.u(5) if k == esc else 0
            for _ in range(cnt):
                if k == esc:
                    r = br.s_(raw) if raw else 0
                else:
                    u = ((br.unary() << k) | br.u(k)) & 0xFFFFFFFF
                    r = wrap32((u >> 1) ^ -(u & 1))
                pred = 0
                for jj in range(order):
                    pred += coefs[jj] * out[-1 - jj]
                out.append(wrap32((pred >> shift) + r))
    return [wrap32(v << wasted) for v in out] if wasted else out


def _ref_header(data, info, p):
    """the header at byte p as (block size, channel code, header bytes, sample position), FlacError if none of this stream"""
    k = [p]

    def nxt():
        if k[0] >= len(data):
            raise FlacError("header runs past the end")
        k[0] += 1
        return data[k[0] - 1]

    if p + 6 > len(data) or nxt() != 0xFF:
        raise FlacError("no sync")
    b1, b2, b3 = nxt(), nxt(), nxt()
    if (b1 & 0xFE) != 0xF8 or (b1 & 1) != info["variable"] or (b3 & 1):
        raise FlacError("sync / strategy / reserved bit")
    bsc, src, chc, ssc = b2 >> 4, b2 & 15, b3 >> 4, (b3 >> 1) & 7
    if bsc == 0 or src == 15 or chc > 10 or ssc == 3:
        raise FlacError("reserved code")
    first = nxt()
    nb = 0
    while nb < 8 and first & (0x80 >> nb):
        nb += 1
    if nb == 1 or nb == 8 or (not info["variable"] and nb == 7):
        raise FlacError("number coding")
    number = first & (0x7F >> nb) if nb else first
    for _ in range(1, nb):
        c = nxt()
        if c & 0xC0 != 0x80:
            raise FlacError("number continuation")
        number = (number << 6) | (c & 0x3F)
    if bsc == 1:
        bs = 192
    elif bsc <= 5:
        bs = 576 << (bsc - 2)
    elif bsc == 6:
        bs = nxt() + 1
    elif bsc == 7:
        bs = ((nxt() << 8) | nxt()) + 1
    else:
        bs = 256 << (bsc - 8)
    table = {v: kk for kk, v in _SR_CODES.items()}
    if src == 0:
        rate = info["rate"]
    elif src <= 11:
        rate = table[src]
    elif src == 12:
        rate = nxt() * 1000
    elif src == 13:
        rate = (nxt() << 8) | nxt()
    else:
        rate = ((nxt() << 8) | nxt()) * 10
    bits = {0: info["bits"], 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}[ssc]
    channels = chc + 1 if chc < 8 else 2
    if k[0] >= len(data) or dec_crc8(data[p:k[0]]) != data[k[0]]:
        raise FlacError("CRC-8")
    if rate != info["rate"] or bits != info["bits"] or channels != info["channels"] or bs > info["max_block"] or bs > 65535:
        raise FlacError("disagrees with STREAMINFO")
    pos = number if info["variable"] else number * info["max_block"]
    if pos + bs > info["total"] or (bs < 16 and pos + bs != info["total"]):
        raise FlacError("position / block size outside the stream")
    return bs, chc, k[0] + 1 - p, pos


def decode(data):
    """the bytes of a .flac file -> dict(info=..., status, good, samples int32 (n, 2): mono duplicated, zero from `good` on)"""
    data = bytes(data)
    info = probe(data)
    n, nch, bits = info["total"], info["channels"], info["bits"]
    allbits = (np.unpackbits(np.frombuffer(data, np.uint8)) + np.uint8(48)).tobytes().decode("ascii")
    out = np.zeros((n, 2), np.int64)
    good, p, status = 0, info["first"], BROKEN
    while True:
        try:
            bs, chc, hlen, pos = _ref_header(data, info, p)
            if pos != good:
                raise FlacError("not the frame that continues the stream")
            br = _Bits(allbits, 8 * (p + hlen))
            ch = []
            for c in range(nch):
                side = (chc == 8 and c == 1) or (chc == 9 and c == 0) or (chc == 10 and c == 1)
                ch.append(np.array(_ref_subframe(br, bs, bits + (1 if side else 0)), np.int64))
            if br.u(-br.pos % 8) != 0:
                raise FlacError("non-zero padding")
            end = br.pos // 8
            if end + 2 > len(data) or _dec_crc16_fast(data[p:end]) != int.from_bytes(data[end:end + 2], "big"):
                raise FlacError("CRC-16")
        except FlacError:
            break
        a = ch[0]
        b = ch[1] if nch == 2 else a
        if chc == 8:
            left, right = a, a - b
        elif chc == 9:
            left, right = a + b, b
        elif chc == 10:
            mid = a * 2 + (b & 1)
            left, right = (mid + b) >> 1, (mid - b) >> 1
        else:
            left, right = a, b
        out[good:good + bs, 0], out[good:good + bs, 1] = left, right
        good += bs
        p = end + 2
        if good == n:
            status = OK
            break
    out = ((out + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    return dict(info=info, status=status, good=good, samples=out.astype(np.int32))


def as_f32(samples, bits):
    """what DMX_PCM_F32 returns for these integers"""
    return (np.asarray(samples).astype(np.float32) / np.float32(1 << (bits - 1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the matrix of streams
def _signal(rng, n, channels, bits, kind="smooth"):
    full = 1 << (bits - 1)
    t = np.arange(n)
    if kind == "noise":
        x = rng.integers(-full, full, (n, channels))
    else:
        x = np.stack([np.rint(0.5 * full * np.sin(2 * np.pi * (0.01 + 0.007 * c) * t + c)) for c in range(channels)], axis=1)
        x = x + rng.integers(-(full >> 6) - 1, (full >> 6) + 2, (n, channels))
    return np.clip(x, -full, full - 1).astype(np.int64)


def _blocks(x, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(x[at:at + s])
        at += s
    assert at == x.shape[0]
    return out


def _fixed_sizes(n, bs):
    return [bs] * (n // bs) + ([n % bs] if n % bs else [])


def matrix():
    """name -> (file bytes, samples int64 (n, channels), bits, channels): every positive case of the issue's matrix, each
    stream small (<= 40 000 samples except the single 65535-sample frame)"""
    rng = np.random.default_rng(20240607)
    cases = {}

    def add(name, frames, channels, bits, **kw):
        data, lay = write(frames, channels, bits, **kw)
        x = np.concatenate([f["samples"].reshape(-1, channels) for f in frames])
        cases[name] = (data, x, bits, channels, lay)

    # depths x channels, FIXED order 2 with default Rice parameters, block size 192 and a short last frame
    for bits in (8, 12, 16, 20, 24):
        for channels in (1, 2):
            x = _signal(rng, 500, channels, bits)
            add(f"depth{bits}_ch{channels}", [frame(b, subs=[sub("FIXED", order=2, method=int(bits > 16)) for _ in range(channels)])
                                              for b in _blocks(x, _fixed_sizes(500, 192))], channels, bits)
    # block sizes (fixed blocking; 16 and 17 through the 8-bit field, 4096 / 4608 by their codes, 4096 also through the 16-bit field)
    for bs in (16, 17, 192, 4096, 4608):
        n = 3 * bs + min(bs - 1, 5)
        x = _signal(rng, n, 2, 16)
        add(f"bs{bs}", [frame(b, subs=[sub("FIXED", order=1), sub("FIXED", order=3)]) for b in _blocks(x, _fixed_sizes(n, bs))], 2, 16)
    x = _signal(rng, 2 * 4096, 2, 16)
    add("bs4096_code7", [frame(b, bs_code=7, subs=[sub("FIXED", order=4, porder=4), sub("FIXED", order=0, porder=8)])
                         for b in _blocks(x, [4096, 4096])], 2, 16)
    x = _signal(rng, 65535, 1, 16)
    add("single65535", [frame(x, subs=[sub("FIXED", order=2)])], 1, 16)
    x = _signal(rng, 1, 2, 16)
    add("n1", [frame(x)], 2, 16, max_block=4096, min_block=4096)
    # variable blocking with mixed sizes, sample numbers up to 3 bytes
    sizes = [16, 4096, 17, 192, 1000, 4608, 31, 256, 2500, 5]
    x = _signal(rng, sum(sizes), 2, 16)
    add("variable", [frame(b, assignment=(1, 8, 9, 10)[i % 4], subs=[sub("FIXED", order=i % 5), sub("FIXED", order=(i + 2) % 5)])
                     for i, b in enumerate(_blocks(x, sizes))], 2, 16, variable=True)
    # the four assignments, side channel at the full 25-bit range
    full = 1 << 23
    x = np.zeros((64, 2), np.int64)
    x[0::2, 0], x[0::2, 1] = full - 1, -full
    x[1::2, 0], x[1::2, 1] = -full, full - 1
    add("assign_full_range", [frame(x[16 * i:16 * i + 16], assignment=c, subs=[sub("VERBATIM"), sub("FIXED", order=0, method=1)])
                              for i, c in enumerate((1, 8, 9, 10))], 2, 24)
    # subframe types
    c = np.tile(np.array([[1234, -77]]), (192, 1))
    add("constant", [frame(c, subs=[sub("CONSTANT"), sub("CONSTANT")])], 2, 16)
    x = _signal(rng, 192, 2, 16, "noise")
    add("verbatim", [frame(x)], 2, 16)
    for o in range(5):
        x = _signal(rng, 384, 2, 16)
        add(f"fixed{o}", [frame(b, subs=[sub("FIXED", order=o), sub("FIXED", order=o, porder=2)]) for b in _blocks(x, [192, 192])], 2, 16)
    # LPC orders 1, 8, 32; precision 15 with shift 0 and 15 (the 5-bit shift is signed: 15 is the largest); precision 1 and 5
    for order in (1, 8, 32):
        for prec, shift in ((15, 0), (15, 15), (5, 7), (1, 0)):
            x = _signal(rng, 400, 2, 16) >> (4 if shift == 0 else 0)  # shift 0: big gains, keep the residual in range
            lim = 1 << (prec - 1)
            if shift == 0:
                coefs = [int(v) for v in rng.integers(-min(lim, 2), min(lim, 2), order)]
            else:
                coefs = [int(v) for v in rng.integers(-lim, lim, order)]
                scale = sum(abs(v) for v in coefs) / float(1 << min(shift, 30))
                if scale > 2.0:  # keep the prediction within 32 bits
                    coefs = [int(v / scale) for v in coefs]
            d = sub("LPC", order=order, coefs=coefs, precision=prec, shift=shift, method=1, porder=1)
            add(f"lpc{order}_p{prec}_s{shift}", [frame(b, subs=[d, dict(d)]) for b in _blocks(x, [200, 200])], 2, 16)
    # wasted bits 1 and 7
    for wb in (1, 7):
        x = (_signal(rng, 192, 2, 16) >> wb) << wb
        add(f"wasted{wb}", [frame(x, assignment=8 if wb == 1 else 1,
                                  subs=[sub("FIXED", order=2, wasted=wb), sub("VERBATIM", wasted=wb if wb == 7 else 0)])], 2, 16)
    # partition orders 0, 4, 8
    for po in (0, 4, 8):
        x = _signal(rng, 4096, 2, 16)
        add(f"porder{po}", [frame(x, subs=[sub("FIXED", order=2, porder=po), sub("FIXED", order=4, porder=po)])], 2, 16)
    # escaped partitions of width 0, 1 and 25
    x = np.zeros((64, 2), np.int64)
    x[:, 0] = 5  # order 1: residual 0
    x[32:, 1] = rng.integers(-1, 1, 32)
    add("escape_0_1", [frame(x, subs=[sub("FIXED", order=1, porder=1, params=[("esc", 0), ("esc", 0)]),
                                      sub("FIXED", order=0, porder=1, params=[("esc", 0), ("esc", 1)])])], 2, 16)
    x = rng.integers(-(1 << 23), 1 << 23, (64, 2))
    add("escape_25", [frame(x, assignment=8, subs=[sub("FIXED", order=0, porder=2, params=[("esc", 24), 22, ("esc", 24), 23], method=1),
                                                   sub("FIXED", order=0, porder=0, params=[("esc", 25)])])], 2, 24)
    # both methods with the largest parameters
    x = rng.integers(-(1 << 23), 1 << 23, (32, 2))
    add("rice_max", [frame(x, subs=[sub("FIXED", order=0, params=[14], method=0), sub("FIXED", order=0, params=[30], method=1)])], 2, 24)
    # frame numbers in the 1-, 2- and 3-byte forms
    for nf in (200, 2100):
        x = _signal(rng, 16 * nf, 2, 8)
        add(f"frames{nf}", [frame(b, subs=[sub("FIXED", order=1), sub("FIXED", order=1)]) for b in _blocks(x, [16] * nf)], 2, 8)
    # every other header code: rate through the 8-bit / 16-bit / tens fields, sample size "from STREAMINFO"
    for rate, rc in ((48000, 12), (44100, 13), (44100, 14), (12345, 0), (44100, 0)):
        x = _signal(rng, 100, 2, 16)
        add(f"rate{rate}_code{rc}", [frame(x, rate_code=rc, size_code=0)], 2, 16, rate=rate)
    # false candidates: a PADDING block and a VERBATIM payload that hold a whole valid frame header (CRC-8 included)
    hdr = bytearray([0xFF, 0xF8, 0x19, 0x18, 0x00])
    hdr.append(enc_crc8(hdr))  # block size 192, 44100, stereo, 16 bits, frame 0
    fake = bytes(hdr)
    x = _signal(rng, 192 * 2, 2, 16)
    vb = np.frombuffer(fake * 8, ">i2").astype(np.int64)  # 24 samples of 16 bits holding the header 8 times
    x[10:34, 0] = vb
    add("false_candidates", [frame(b) for b in _blocks(x, [192, 192])], 2, 16, extra_meta=[(1, bytes(7) + fake * 3 + bytes(5))])
    # an ID3v2 tag in front, metadata blocks, trailing bytes
    x = _signal(rng, 300, 2, 16)
    add("id3_trailing", [frame(b, subs=[sub("FIXED", order=2), sub("FIXED", order=2)]) for b in _blocks(x, [192, 108])], 2, 16,
        id3=id3v2(77), trailing=b"TAG" + bytes(125), extra_meta=[(4, b"\x00" * 40), (1, bytes(10))])
    return cases


# ------------------------------------------------------------------------------------------------ damaged files
def _base_frames(rng, n_frames=6, bs=192, tail=50, **raw):
    """a stereo 16-bit stream of n_frames blocks and a short last one; raw: overrides for the FIRST subframe of frame 3"""
    n = n_frames * bs + tail
    x = _signal(rng, n, 2, 16)
    lpc = sub("LPC", order=8, coefs=[900, -300, 120, -60, 30, -10, 5, -2], precision=12, shift=10, porder=2)
    frames = []
    for i, b in enumerate(_blocks(x, _fixed_sizes(n, bs))):
        d0 = dict(lpc) if i % 2 else sub("FIXED", order=2, porder=1)
        if i == 3:
            d0.update(raw)
        frames.append(frame(b, assignment=(1, 8, 9, 10)[i % 4], subs=[d0, sub("FIXED", order=1, method=1)]))
    return frames, x


def _flip(data, bit):
    b = bytearray(data)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def damaged():
    """name -> file bytes: 40 damaged files (and what they were made from is of no interest: the reference decoder says
    what a decoder must return for each)"""
    rng = np.random.default_rng(77)
    frames, x = _base_frames(rng)
    base, lay = write(frames, 2, 16)
    fr = lay["frames"]
    out = {}
    out["header_bit"] = _flip(base, 8 * fr[2][0] + 20)
    out["crc8_byte"] = _flip(base, 8 * (fr[3][0] + 5) + 3)
    out["crc16_byte"] = _flip(base, 8 * (fr[1][1] - 1) + 6)
    out["residual_bit"] = _flip(base, 8 * ((fr[4][0] + fr[4][1]) // 2) + 1)
    out["first_frame"] = _flip(base, 8 * (fr[0][0] + 40))
    out["last_frame"] = _flip(base, 8 * (fr[6][1] - 4))
    out["truncated_mid_frame"] = base[:(fr[5][0] + fr[5][1]) // 2]
    out["truncated_at_frame"] = base[:fr[5][0]]
    out["truncated_in_header"] = base[:fr[2][0] + 3]
    out["short_of_total"] = write(frames, 2, 16, total=x.shape[0] + 100)[0]
    out["overshoots_total"] = write(frames, 2, 16, total=x.shape[0] - 7)[0]
    out["unary_to_end_of_file"] = base[:(fr[6][0] + fr[6][1]) // 2] + bytes(300)
    out["unary_to_end_of_frame"] = base[:(fr[3][0] + fr[3][1]) // 2] + bytes(64) + base[fr[4][0]:]
    out["frame_removed"] = base[:fr[2][0]] + base[fr[3][0]:]
    out["frame_repeated"] = base[:fr[3][0]] + base[fr[2][0]:]
    out["garbage_between_frames"] = base[:fr[4][0]] + b"\x00\xff\xf8" + base[fr[4][0]:]
    for name, raw in (("illegal_partition_order", dict(porder_raw=7)), ("partition_smaller_than_order", dict(porder_raw=6)),
                      ("reserved_type", dict(type_code=0b000100)), ("reserved_type_fixed5", dict(type_code=0b001101)),
                      ("negative_shift", dict(shift_raw=0b10001)), ("reserved_precision", dict(prec_raw=15)),
                      ("reserved_method", dict(method_raw=2)), ("order_above_block_size", None)):
        if raw is not None:
            out[name] = write(_base_frames(np.random.default_rng(77), **raw)[0], 2, 16)[0]
    # predictor order above the block size: a 3-sample last frame whose type field claims FIXED order 4
    f2, x2 = _base_frames(np.random.default_rng(77), tail=3)
    f2[-1]["subs"] = [sub("FIXED", order=2, order_raw=4), sub("FIXED", order=1)]
    out["order_above_block_size"] = write(f2, 2, 16)[0]
    f2[-1]["subs"] = [sub("FIXED", order=2, order_raw=3), sub("FIXED", order=1)]
    out["order_equal_block_size"] = write(f2, 2, 16)[0]
    f3 = _base_frames(np.random.default_rng(77))[0]
    f3[3]["number"] = 4
    out["frame_number_skips"] = write(f3, 2, 16)[0]
    f3 = _base_frames(np.random.default_rng(77))[0]
    f3[3]["reserved"] = 1
    out["reserved_header_bit"] = write(f3, 2, 16)[0]
    f3 = _base_frames(np.random.default_rng(77))[0]
    f3[3]["size_code"] = 6
    out["frame_says_24_bits"] = write(f3, 2, 16)[0]
    f3 = _base_frames(np.random.default_rng(77))[0]
    f3[3]["rate_code"] = 10
    out["frame_says_48_khz"] = write(f3, 2, 16)[0]
    k = 0
    while len(out) < 40:
        out[f"bit_flip_{k}"] = _flip(base, int(rng.integers(8 * lay["first"], 8 * len(base))))
        k += 1
    assert len(out) == 40
    return out


def small_files():
    """two small files (every single-byte truncation of them is in the CPU corpus) - one mono with metadata, one stereo"""
    rng = np.random.default_rng(5)
    x = _signal(rng, 100, 1, 12)
    a = write([frame(b, subs=[sub("FIXED", order=2)]) for b in _blocks(x, [48, 48, 4])], 1, 12, extra_meta=[(1, bytes(9))], id3=id3v2(5))[0]
    y = _signal(rng, 80, 2, 16)
    d = sub("LPC", order=3, coefs=[50, -20, 7], precision=8, shift=6, porder=1)
    b = write([frame(c, assignment=10, subs=[d, sub("FIXED", order=1, params=[("esc", 14)])]) for c in _blocks(y, [32, 32, 16])], 2, 16,
              variable=True)[0]
    return a, b


def bit_flips(count=500, seed=11):
    """seeded single-bit flips of the second small file, anywhere in it (the stream header included)"""
    _, b = small_files()
    rng = np.random.default_rng(seed)
    return [_flip(b, int(v)) for v in rng.integers(0, 8 * len(b), count)]


def too_many_candidates():
    """a VALID one-frame stream whose VERBATIM payload holds 1100 whole frame headers of this stream: more header look-alikes
    than the candidate table's 2 * ceil(n / min block) + 1024 = 1026, which a decoder reports as TOO_MANY_CANDIDATES with
    good = 0 and silence (the sequential reference decoder, which keeps no table, reads the stream)"""
    hdr = bytearray([0xFF, 0xF8, 0x19, 0x18, 0x00])
    hdr.append(enc_crc8(hdr))
    rng = np.random.default_rng(3)
    x = rng.integers(-100, 100, (4096, 2))
    x[:3300, 0] = np.frombuffer(bytes(hdr) * 1100, ">i2").astype(np.int64)
    return write([frame(x)], 2, 16)[0]
