// flac_in.hip — the input stage in front of the track path: the bytes of a native FLAC file (RFC 9639) in HBM -> the track
// as interleaved stereo fp32 (or, for round trips, the PCM bytes pcm.hip writes). Specification: DESIGN.md section 2.12,
// restated with a free-choice writer and a sequential reference decoder in tests/flac_in_spec.py.
//
// Parsing a frame is a serial bit parse and frames carry no length, so the work is five launches on one stream:
//   1 candidates  every byte position from the first frame on is tested as a frame header (sync code, blocking strategy,
//                 legal codes, well-formed number, agreement with STREAMINFO, position + block size within the stream,
//                 CRC-8). One lane tests 32 consecutive positions and keeps one mask word; a workgroup covers 8192
//                 positions and leaves their survivor count.
//   2 scan        the same grid. A workgroup ranks its survivors behind those of all earlier workgroups (sum of the counts:
//                 no workgroup waits for another), so candidate k of the table is the k-th survivor IN POSITION ORDER; the
//                 lane that owns a survivor parses that frame to its end without storing samples, checks CRC-16 and
//                 records {start, end byte (0: did not parse), block size | channel code, sample position}. The table holds
//                 cap = 2 * ceil(n / min block size) + 1024 candidates; more are counted, not stored.
//   3 chain       one workgroup: more than cap candidates is status TOO_MANY_CANDIDATES. Else every parsed candidate finds
//                 the candidate that starts where it ends (binary search), and lane 0 walks from the candidate at the first
//                 frame's byte while the sample positions add up, writing the table of true frames, `good`, the status.
//   4 decode      one lane per true frame parses it again and writes warm-up, verbatim and predicted samples (wasted bits
//                 applied) into two int32 planes at the frame's sample position. Predictor coefficients and the last 32
//                 samples live in LDS (dynamic indexing without scratch); FIXED orders run as LPC with their binomial rows.
//   5 finish      per 4 samples, coalesced: find the frame (binary search in the true-frame table), undo the stereo
//                 decorrelation, zero [good, n), convert, store whole dwords as pcm.hip does.
// All loads of file bytes are checked against the file length; all arithmetic on samples is integer (the one conversion
// to float in launch 5 is exact: |v| < 2^24 for every legal depth).
//
// With DMX_FLAC_IN_HOST defined the same bodies compile as plain C++ (tests/flac_in_host_main.cpp): every kernel is a
// sequence of phases separated by workgroup barriers, each phase a function of (block, lane); the device kernels call the
// phases with __syncthreads() between them, the host driver at the end of this file runs each phase for all lanes in turn.
#ifdef DMX_FLAC_IN_HOST
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define FI_DEV static inline
#else
#include "kernels.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#define FI_DEV __device__ __forceinline__
#endif
#include "../../include/demucs_hip.h"

namespace dmx
{
typedef unsigned char fi_u8;
typedef unsigned long long fi_u64;

// what the kernels know of the stream (by value in the kernel arguments) and where the workspace's parts lie (int32 words)
struct FiInfo
{
    int rate, channels, bits, total, maxBlock, variable, first, bytes;
    int cap, nChunks;
    int decLanes; // launch 4: the lanes of a 64-lane workgroup that take a frame (the others leave at once)
    // word offsets into the workspace
    long long oMask, oCounts, oCand, oNext, oFrames, oHdr, oPlanes, words;
};
enum
{
    FI_CHUNK_LANES = 256,
    FI_CHUNK = FI_CHUNK_LANES * 32, // byte positions per workgroup of launches 1 and 2
    FI_DEC_LANES = 64,
    FI_DEC_ACTIVE = 1 // default of FiInfo::decLanes: measured best of 64 / 16 / 4 / 1 on a 4-minute track
};

static inline bool fi_layout(const dmx_flac_info &info, int64_t bytes, FiInfo &I)
{
    if (info.total_samples < 1 || info.total_samples > 0x7fffffff || bytes > 0x7fffffff || info.first_frame < 0 || info.first_frame >= bytes ||
        info.min_block < 16 || info.max_block < info.min_block || info.max_block > 65535 || info.channels < 1 || info.channels > 2)
        return false;
    I.rate = info.sample_rate, I.channels = info.channels, I.bits = info.bits, I.total = (int)info.total_samples;
    I.maxBlock = info.max_block, I.variable = info.variable_blocking, I.first = (int)info.first_frame, I.bytes = (int)bytes;
    const long long cap = 2 * ((info.total_samples + info.min_block - 1) / info.min_block) + 1024;
    I.cap = (int)cap;
    I.decLanes = FI_DEC_ACTIVE;
    I.nChunks = (int)((bytes - info.first_frame + FI_CHUNK - 1) / FI_CHUNK);
    long long o = 0;
    auto take = [&](long long w) {
        const long long at = o;
        o += (w + 3) / 4 * 4;
        return at;
    };
    I.oHdr = take(4);
    I.oMask = take((long long)I.nChunks * FI_CHUNK_LANES);
    I.oCounts = take(I.nChunks);
    I.oCand = take(cap * 4);
    I.oNext = take(cap);
    I.oFrames = take(cap * 4);
    I.oPlanes = take(2 * info.total_samples);
    I.words = o;
    return true;
}

// ------------------------------------------------------------------------------------------------ the probe (host, no GPU)
// 0 and *info, or -1 and a message
int flac_in_probe(const void *file, int64_t bytes, dmx_flac_info *info, char *msg, size_t msgLen)
{
    const fi_u8 *f = (const fi_u8 *)file;
#define FI_FAIL(...)                       \
    do                                     \
    {                                      \
        snprintf(msg, msgLen, __VA_ARGS__); \
        return -1;                         \
    } while (0)
    if (!f || !info)
        FI_FAIL("null %s pointer", !f ? "file" : "info");
    if (bytes < 4)
        FI_FAIL("%lld bytes: shorter than any FLAC file", (long long)bytes);
    if (bytes > 0x7fffffff)
        FI_FAIL("%lld bytes: files of 2 GiB and more are not supported", (long long)bytes);
    int64_t p = 0;
    if (f[0] == 'I' && f[1] == 'D' && f[2] == '3')
    {
        if (bytes < 10)
            FI_FAIL("truncated ID3v2 header");
        if ((f[6] | f[7] | f[8] | f[9]) & 0x80)
            FI_FAIL("ID3v2 tag with a malformed size");
        p = 10 + (((int64_t)f[6] << 21) | (f[7] << 14) | (f[8] << 7) | f[9]) + ((f[5] & 0x10) ? 10 : 0);
        if (p + 4 > bytes)
            FI_FAIL("the ID3v2 tag runs past the end of the file");
    }
    if (memcmp(f + p, "OggS", 4) == 0)
        FI_FAIL("Ogg FLAC is not supported (native FLAC streams only)");
    if (memcmp(f + p, "fLaC", 4) != 0)
        FI_FAIL("no fLaC marker");
    p += 4;
    bool first = true, last = false;
    while (!last)
    {
        if (p + 4 > bytes)
            FI_FAIL("the metadata runs past the end of the file");
        last = f[p] >> 7;
        const int type = f[p] & 0x7f;
        const int64_t len = ((int64_t)f[p + 1] << 16) | (f[p + 2] << 8) | f[p + 3];
        if (type == 127)
            FI_FAIL("metadata block type 127 is invalid");
        if (first && (type != 0 || len != 34))
            FI_FAIL("the first metadata block is not a STREAMINFO of 34 bytes");
        if (!first && type == 0)
            FI_FAIL("a second STREAMINFO block");
        if (p + 4 + len > bytes)
            FI_FAIL("metadata block of type %d runs past the end of the file", type);
        if (first)
        {
            const fi_u8 *s = f + p + 4;
            info->min_block = (s[0] << 8) | s[1], info->max_block = (s[2] << 8) | s[3];
            info->min_frame = (s[4] << 16) | (s[5] << 8) | s[6], info->max_frame = (s[7] << 16) | (s[8] << 8) | s[9];
            info->sample_rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
            info->channels = ((s[12] >> 1) & 7) + 1;
            info->bits = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
            info->total_samples = ((int64_t)(s[13] & 15) << 32) | ((int64_t)s[14] << 24) | (s[15] << 16) | (s[16] << 8) | s[17];
        }
        first = false;
        p += 4 + len;
    }
    if (info->channels > 2)
        FI_FAIL("%d channels (1 or 2 are supported)", info->channels);
    if (info->bits == 32)
        FI_FAIL("32-bit samples are not supported");
    if (info->bits != 8 && info->bits != 12 && info->bits != 16 && info->bits != 20 && info->bits != 24)
        FI_FAIL("%d bits per sample (8, 12, 16, 20 or 24)", info->bits);
    if (info->sample_rate == 0)
        FI_FAIL("sample rate 0");
    if (info->total_samples == 0)
        FI_FAIL("unknown length (total samples 0) is not supported");
    if (info->total_samples > 0x7fffffff)
        FI_FAIL("%lld samples: streams of 2^31 samples and more are not supported", (long long)info->total_samples);
    if (info->min_block < 16 || info->max_block < info->min_block)
        FI_FAIL("block size range %d..%d (16 <= min <= max)", info->min_block, info->max_block);
    if (p + 2 > bytes)
        FI_FAIL("no audio frame after the metadata");
    if (f[p] != 0xff || (f[p + 1] & 0xfe) != 0xf8)
        FI_FAIL("no frame sync code at the first byte after the metadata");
    info->variable_blocking = f[p + 1] & 1;
    info->first_frame = p;
    return 0;
#undef FI_FAIL
}

int64_t flac_in_workspace_bytes(const dmx_flac_info *info, int64_t bytes)
{
    FiInfo I;
    if (!info || !fi_layout(*info, bytes, I))
        return -1;
    return I.words * 4;
}

// ------------------------------------------------------------------------------------------------ bits
struct FiBits
{
    const fi_u8 *f;
    int bytes, pos; // the file's length, the next byte to load
    fi_u64 acc;     // unread bits, left-aligned; the bits below the cnt valid ones are zero
    int cnt;
    bool err; // a read went past the last byte of the file
};
FI_DEV void fi_open(FiBits &b, const fi_u8 *f, int bytes, int at)
{
    b.f = f, b.bytes = bytes, b.pos = at, b.acc = 0, b.cnt = 0, b.err = false;
}
FI_DEV void fi_refill(FiBits &b)
{
    if (b.cnt <= 32 && b.pos + 4 <= b.bytes) // four bytes in one (unaligned) load: a quarter of the dependent round trips
    {
        unsigned w;
        __builtin_memcpy(&w, b.f + b.pos, 4);
        b.acc |= (fi_u64)__builtin_bswap32(w) << (32 - b.cnt);
        b.pos += 4, b.cnt += 32;
    }
    while (b.cnt <= 56 && b.pos < b.bytes)
    {
        b.acc |= (fi_u64)b.f[b.pos++] << (56 - b.cnt);
        b.cnt += 8;
    }
}
FI_DEV unsigned fi_read(FiBits &b, int n) // 0 <= n <= 32
{
    if (n == 0)
        return 0;
    if (b.cnt < n)
        fi_refill(b);
    if (b.cnt < n)
    {
        b.err = true, b.acc = 0, b.cnt = 0;
        return 0;
    }
    const unsigned v = (unsigned)(b.acc >> (64 - n));
    b.acc <<= n, b.cnt -= n;
    return v;
}
FI_DEV int fi_reads(FiBits &b, int n) // two's complement of n bits, 0 <= n <= 32
{
    if (n == 0)
        return 0;
    const unsigned v = fi_read(b, n);
    return (int)(v << (32 - n)) >> (32 - n);
}
FI_DEV unsigned fi_unary(FiBits &b) // the number of zero bits before the next one bit, modulo 2^32
{
    unsigned q = 0;
    for (;;)
    {
        if (b.cnt == 0)
            fi_refill(b);
        if (b.cnt == 0)
        {
            b.err = true;
            return q;
        }
        if (b.acc)
        {
            const int z = __builtin_clzll(b.acc); // < cnt: the bits below the valid ones are zero
            b.acc <<= z;
            b.acc <<= 1;
            b.cnt -= z + 1;
            return q + (unsigned)z;
        }
        q += (unsigned)b.cnt;
        b.cnt = 0;
    }
}
FI_DEV unsigned fi_crc8(unsigned c, unsigned byte)
{
    c ^= byte;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xff : (c << 1) & 0xff;
    return c;
}
FI_DEV unsigned fi_crc16(unsigned c, unsigned byte)
{
    c ^= byte << 8;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xffff : (c << 1) & 0xffff;
    return c;
}

// ------------------------------------------------------------------------------------------------ the frame header
struct FiHdr
{
    int bs, ch, hlen, pos; // block size, channel assignment code, header bytes including CRC-8, position of the first sample
};
// is there a frame header of THIS stream at byte p ?
FI_DEV bool fi_header(const fi_u8 *f, const FiInfo &I, int p, FiHdr &h)
{
    if (p < 0 || p > I.bytes - 6) // the shortest header: 4 bytes, a 1-byte number, CRC-8
        return false;
    if (f[p] != 0xff)
        return false;
    const unsigned b1 = f[p + 1], b2 = f[p + 2], b3 = f[p + 3];
    if ((b1 & 0xfe) != 0xf8 || (int)(b1 & 1) != I.variable || (b3 & 1))
        return false;
    unsigned crc = fi_crc8(fi_crc8(fi_crc8(fi_crc8(0, 0xff), b1), b2), b3);
    int k = p + 4; // the next byte: checked against the length before every load
    bool ok = true;
    auto next = [&]() -> unsigned {
        if (k >= I.bytes)
        {
            ok = false;
            return 0;
        }
        const unsigned v = f[k++];
        crc = fi_crc8(crc, v);
        return v;
    };
    const int bsCode = b2 >> 4, srCode = b2 & 15, chCode = b3 >> 4, ssCode = (b3 >> 1) & 7;
    if (bsCode == 0 || srCode == 15 || chCode > 10 || ssCode == 3)
        return false;
    // the frame (fixed blocking) or sample (variable) number: 0xxxxxxx, or a first byte with 2 .. 7 leading ones and one
    // 10xxxxxx byte for each but the first
    const unsigned first = next();
    int nb = 0;
    while (nb < 8 && (first & (0x80u >> nb)))
        ++nb;
    if (nb == 1 || nb == 8 || (!I.variable && nb == 7))
        return false;
    fi_u64 number = nb ? (first & (0x7fu >> nb)) : first;
    for (int j = 1; j < nb; ++j)
    {
        const unsigned c = next();
        if ((c & 0xc0) != 0x80)
            return false;
        number = (number << 6) | (c & 0x3f);
    }
    int bs;
    if (bsCode == 1)
        bs = 192;
    else if (bsCode <= 5)
        bs = 576 << (bsCode - 2);
    else if (bsCode == 6)
        bs = (int)next() + 1;
    else if (bsCode == 7)
    {
        bs = (int)next() << 8;
        bs = (bs | (int)next()) + 1;
    }
    else
        bs = 256 << (bsCode - 8);
    int rate;
    switch (srCode)
    {
    case 0: rate = I.rate; break;
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = (int)next() * 1000; break;
    case 13:
        rate = (int)next() << 8;
        rate |= (int)next();
        break;
    default:
        rate = (int)next() << 8;
        rate = (rate | (int)next()) * 10;
        break;
    }
    const int bits = ssCode == 0 ? I.bits : ssCode == 1 ? 8 : ssCode == 2 ? 12 : ssCode == 4 ? 16 : ssCode == 5 ? 20 : ssCode == 6 ? 24 : 32;
    const int channels = chCode < 8 ? chCode + 1 : 2;
    if (!ok || k >= I.bytes || crc != f[k])
        return false;
    if (rate != I.rate || bits != I.bits || channels != I.channels || bs > I.maxBlock || bs > 65535)
        return false;
    const fi_u64 pos = I.variable ? number : number * (fi_u64)I.maxBlock;
    if (pos >= (fi_u64)I.total || pos + (fi_u64)bs > (fi_u64)I.total)
        return false;
    if (bs < 16 && pos + (fi_u64)bs != (fi_u64)I.total) // only a stream's last frame may be that short
        return false;
    h.bs = bs, h.ch = chCode, h.hlen = k + 1 - p, h.pos = (int)pos;
    return true;
}

// ------------------------------------------------------------------------------------------------ subframes and frames
// One subframe of bs samples of width w. STORE: the samples go to plane[0 .. bs) (the caller has checked the room), the
// predictor's coefficients and its last 32 samples to lc[j * ls] and lh[j * ls]. Returns false on anything invalid.
template <bool STORE>
FI_DEV bool fi_subframe(FiBits &b, int bs, int w, int *plane, int *lc, int *lh, int ls)
{
    if (fi_read(b, 1))
        return false;
    const int type = (int)fi_read(b, 6);
    int wasted = 0;
    if (fi_read(b, 1))
    {
        const unsigned q = fi_unary(b);
        if (q >= 32)
            return false;
        wasted = (int)q + 1;
    }
    if (b.err || wasted >= w)
        return false;
    w -= wasted;
    if (type == 0) // CONSTANT
    {
        const int v = fi_reads(b, w);
        if (STORE)
            for (int i = 0; i < bs; ++i)
                plane[i] = (int)((unsigned)v << wasted);
        return !b.err;
    }
    if (type == 1) // VERBATIM
    {
        for (int i = 0; i < bs; ++i)
        {
            const int v = fi_reads(b, w);
            if (b.err)
                return false;
            if (STORE)
                plane[i] = (int)((unsigned)v << wasted);
        }
        return true;
    }
    int order, shift = 0;
    const bool lpc = type >= 32;
    if (lpc)
        order = (type & 31) + 1;
    else if (type >= 8 && type <= 12)
        order = type - 8;
    else
        return false; // reserved
    if (order >= bs)
        return false;
    for (int i = 0; i < order; ++i) // warm-up
    {
        const int v = fi_reads(b, w);
        if (STORE)
        {
            plane[i] = (int)((unsigned)v << wasted);
            lh[(i & 31) * ls] = v;
        }
    }
    if (lpc)
    {
        const int prec = (int)fi_read(b, 4) + 1;
        shift = (int)fi_read(b, 5);
        if (prec == 16 || (shift & 16)) // the reserved precision, a negative shift
            return false;
        for (int j = 0; j < order; ++j)
        {
            const int c = fi_reads(b, prec);
            if (STORE)
                lc[j * ls] = c;
        }
    }
    else if (STORE)
    {
        // s[i] - (the order-th difference) = the rows 1 / 2,-1 / 3,-3,1 / 4,-6,4,-1
        const int c0 = order, c1 = order == 2 ? -1 : order == 3 ? -3 : -6, c2 = order == 3 ? 1 : 4;
        if (order > 0)
            lc[0] = c0;
        if (order > 1)
            lc[1 * ls] = c1;
        if (order > 2)
            lc[2 * ls] = c2;
        if (order > 3)
            lc[3 * ls] = -1;
    }
    if (b.err)
        return false;
    const int method = (int)fi_read(b, 2), po = (int)fi_read(b, 4);
    if (b.err || method > 1 || (bs & ((1 << po) - 1)) || (bs >> po) < order)
        return false;
    const int pbits = method ? 5 : 4, esc = method ? 31 : 15, psz = bs >> po;
    int i = order;
    for (int part = 0; part < (1 << po); ++part)
    {
        const int cnt = psz - (part == 0 ? order : 0);
        const int k = (int)fi_read(b, pbits);
        const int raw = k == esc ? (int)fi_read(b, 5) : 0;
        if (b.err)
            return false;
        for (int t = 0; t < cnt; ++t, ++i)
        {
            int r;
            if (k == esc)
                r = fi_reads(b, raw);
            else
            {
                const unsigned q = fi_unary(b);
                const unsigned u = (q << k) | fi_read(b, k);
                r = (int)(u >> 1) ^ -(int)(u & 1);
            }
            if (b.err)
                return false;
            if (STORE)
            {
                long long sum = 0;
                for (int j = 0; j < order; ++j)
                    sum += (long long)lc[j * ls] * (long long)lh[((i - 1 - j) & 31) * ls];
                const int v = (int)(unsigned)(fi_u64)((sum >> shift) + (long long)r);
                plane[i] = (int)((unsigned)v << wasted);
                lh[(i & 31) * ls] = v;
            }
        }
    }
    return true;
}

// the frame at byte `start`: its header, and with `end` the first byte behind its CRC-16. STORE: samples into the planes
// (without a CRC-16 check: launch 2 has made it); else nothing is stored and CRC-16 is verified.
template <bool STORE>
FI_DEV bool fi_frame(const fi_u8 *f, const FiInfo &I, int start, FiHdr &h, int &end, int *planeA, int *planeB, int *lc, int *lh, int ls)
{
    if (!fi_header(f, I, start, h))
        return false;
    FiBits b;
    fi_open(b, f, I.bytes, start + h.hlen);
    for (int c = 0; c < I.channels; ++c)
    {
        const int side = (h.ch == 8 && c == 1) || (h.ch == 9 && c == 0) || (h.ch == 10 && c == 1);
        int *plane = STORE ? (c ? planeB : planeA) + h.pos : nullptr;
        if (!fi_subframe<STORE>(b, h.bs, I.bits + side, plane, lc, lh, ls))
            return false;
    }
    if (fi_read(b, b.cnt & 7) != 0) // zero bits to the byte boundary (cnt counts from a byte boundary)
        return false;
    const int e = b.pos - (b.cnt >> 3);
    if (b.err || e + 2 > I.bytes)
        return false;
    if (!STORE)
    {
        unsigned crc = 0;
        for (int k = start; k < e; ++k)
            crc = fi_crc16(crc, f[k]);
        if (crc != (((unsigned)f[e] << 8) | f[e + 1]))
            return false;
    }
    end = e + 2;
    return true;
}

// ------------------------------------------------------------------------------------------------ the launches, as phases
// launch 1, phase a: lane l of workgroup g tests the 32 positions from first + (g * 256 + l) * 32; lds[l] = survivors
FI_DEV void fi_cand_a(const fi_u8 *f, const FiInfo I, int *work, int g, int l, int *lds)
{
    const long long p0 = (long long)I.first + ((long long)g * FI_CHUNK_LANES + l) * 32;
    unsigned word = 0;
    for (int j = 0; j < 32; ++j)
    {
        const long long p = p0 + j;
        FiHdr h;
        if (p + 6 <= I.bytes && f[p] == 0xff && fi_header(f, I, (int)p, h))
            word |= 1u << j;
    }
    work[I.oMask + (long long)g * FI_CHUNK_LANES + l] = (int)word;
    lds[l] = __builtin_popcount(word);
}
// phase b: the workgroup's count
FI_DEV void fi_cand_b(const FiInfo I, int *work, int g, int l, const int *lds)
{
    if (l != 0)
        return;
    int s = 0;
    for (int k = 0; k < FI_CHUNK_LANES; ++k)
        s += lds[k];
    work[I.oCounts + g] = s;
}
// launch 2, phase a: lds[l] = this lane's share of the counts of the workgroups before g, lds[256 + l] = its own survivors
FI_DEV void fi_scan_a(const FiInfo I, const int *work, int g, int l, int *lds)
{
    int s = 0;
    for (int k = l; k < g; k += FI_CHUNK_LANES)
        s += work[I.oCounts + k];
    lds[l] = s;
    lds[FI_CHUNK_LANES + l] = __builtin_popcount((unsigned)work[I.oMask + (long long)g * FI_CHUNK_LANES + l]);
}
// phase b: rank and parse
FI_DEV void fi_scan_b(const fi_u8 *f, const FiInfo I, int *work, int g, int l, const int *lds)
{
    unsigned word = (unsigned)work[I.oMask + (long long)g * FI_CHUNK_LANES + l];
    if (!word)
        return;
    long long idx = 0; // survivors before this lane's first (a damaged file may hold more than 2^31 / 6 of them: 64 bits)
    for (int k = 0; k < FI_CHUNK_LANES; ++k)
        idx += lds[k];
    for (int k = 0; k < l; ++k)
        idx += lds[FI_CHUNK_LANES + k];
    const int p0 = I.first + (g * FI_CHUNK_LANES + l) * 32;
    for (; word; word &= word - 1, ++idx)
    {
        if (idx >= I.cap)
            return;
        const int start = p0 + __builtin_ctz(word);
        FiHdr h;
        int end = 0;
        h.bs = h.ch = h.hlen = h.pos = 0;
        if (!fi_frame<false>(f, I, start, h, end, nullptr, nullptr, nullptr, nullptr, 0))
            end = 0;
        int *c = work + I.oCand + idx * 4;
        c[0] = start, c[1] = end, c[2] = h.bs | (h.ch << 16), c[3] = h.pos;
    }
}
// launch 3 (one workgroup), phase a: lds[l] = this lane's share of all counts
FI_DEV void fi_chain_a(const FiInfo I, const int *work, int l, long long *lds)
{
    long long s = 0;
    for (int k = l; k < I.nChunks; k += FI_CHUNK_LANES)
        s += work[I.oCounts + k];
    lds[l] = s;
}
// phase b: next[i] = the candidate that starts where candidate i ends, or -1
FI_DEV void fi_chain_b(const FiInfo I, int *work, int l, const long long *lds)
{
    long long total = 0;
    for (int k = 0; k < FI_CHUNK_LANES; ++k)
        total += lds[k];
    if (total > I.cap)
        return;
    const int *cand = work + I.oCand;
    for (int i = l; i < (int)total; i += FI_CHUNK_LANES)
    {
        const int end = cand[4 * (long long)i + 1];
        int nx = -1;
        if (end > 0)
        {
            int lo = i + 1, hi = (int)total; // the first candidate at or behind `end` (starts ascend; a frame ends behind its start)
            while (lo < hi)
            {
                const int mid = lo + ((hi - lo) >> 1);
                if (cand[4 * (long long)mid] < end)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < (int)total && cand[4 * (long long)lo] == end)
                nx = lo;
        }
        work[I.oNext + i] = nx;
    }
}
// phase c: lane 0 walks the stream
FI_DEV void fi_chain_c(const FiInfo I, int *work, long long *status, int l, const long long *lds)
{
    if (l != 0)
        return;
    long long total = 0;
    for (int k = 0; k < FI_CHUNK_LANES; ++k)
        total += lds[k];
    int nFrames = 0, good = 0, st = DMX_FLAC_BROKEN;
    if (total > I.cap)
        st = DMX_FLAC_TOO_MANY_CANDIDATES;
    else
    {
        const int *cand = work + I.oCand;
        int cur = total > 0 && cand[0] == I.first ? 0 : -1;
        while (cur >= 0)
        {
            const int *c = cand + 4 * (long long)cur;
            const int bs = c[2] & 0xffff;
            if (c[1] <= 0 || c[3] != good) // did not parse, or is not the frame that continues the stream (the header check
                break;                     // has bounded position + block size by the stream's length)
            int *fr = work + I.oFrames + 4 * (long long)nFrames;
            fr[0] = c[0], fr[1] = c[3], fr[2] = bs, fr[3] = c[2] >> 16;
            ++nFrames;
            good += bs;
            if (good == I.total)
            {
                st = DMX_FLAC_OK;
                break;
            }
            cur = work[I.oNext + cur];
        }
    }
    work[I.oHdr] = nFrames, work[I.oHdr + 1] = good;
    status[0] = st, status[1] = good;
}
// launch 4: lane l of workgroup g decodes true frame g * 64 + l; lc / lh: 32 x 64 words of LDS each
FI_DEV void fi_decode(const fi_u8 *f, const FiInfo I, int *work, int g, int l, int *lc, int *lh)
{
    const long long k = (long long)g * I.decLanes + l;
    if (l >= I.decLanes || k >= work[I.oHdr])
        return;
    FiHdr h;
    int end;
    int *planeA = work + I.oPlanes, *planeB = planeA + I.total; // the header check bounds pos + bs by I.total
    (void)fi_frame<true>(f, I, work[I.oFrames + 4 * k], h, end, planeA, planeB, lc + l, lh + l, FI_DEC_LANES);
}
// launch 5: samples [4 q, 4 q + 4) -> the output's dwords
template <int ENC>
FI_DEV void fi_finish(const FiInfo I, const int *work, unsigned *out, long long q)
{
    const long long i0 = q * 4;
    if (i0 >= I.total)
        return;
    const int cnt = I.total - i0 < 4 ? (int)(I.total - i0) : 4;
    const int nFrames = work[I.oHdr], good = work[I.oHdr + 1];
    const int *fr = work + I.oFrames, *planeA = work + I.oPlanes, *planeB = planeA + I.total;
    int k = 0;
    if (i0 < good)
    {
        int lo = 0, hi = nFrames; // the last frame that starts at or before i0
        while (hi - lo > 1)
        {
            const int mid = lo + ((hi - lo) >> 1);
            if (fr[4 * (long long)mid + 1] <= i0)
                lo = mid;
            else
                hi = mid;
        }
        k = lo;
    }
    int L[4], R[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const long long s = i0 + j;
        L[j] = R[j] = 0;
        if (j < cnt && s < good)
        {
            while (s >= fr[4 * (long long)k + 1] + fr[4 * (long long)k + 2])
                ++k; // s < good: a frame that holds it exists
            const int ch = fr[4 * (long long)k + 3];
            const long long a = planeA[s], b = I.channels == 2 ? planeB[s] : a;
            long long l = a, r = b;
            if (ch == 8)
                r = a - b;
            else if (ch == 9)
                l = a + b;
            else if (ch == 10)
            {
                const long long mid = a * 2 + (b & 1);
                l = (mid + b) >> 1, r = (mid - b) >> 1;
            }
            L[j] = (int)(unsigned)(fi_u64)l, R[j] = (int)(unsigned)(fi_u64)r;
        }
    }
    unsigned w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int frameBytes = ENC == DMX_PCM_F32 ? 8 : ENC == DMX_PCM_S16 ? 4 : 6;
    if (ENC == DMX_PCM_F32)
    {
        const float scale = 1.0f / (float)(1 << (I.bits - 1)); // a power of two: v * scale == v / 2^(bits-1), exactly
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            const float x = (float)L[j] * scale, y = (float)R[j] * scale;
            unsigned ux, uy;
            __builtin_memcpy(&ux, &x, 4), __builtin_memcpy(&uy, &y, 4);
            w[2 * j] = ux, w[2 * j + 1] = uy;
        }
    }
    else if (ENC == DMX_PCM_S16)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w[j] = ((unsigned)L[j] & 0xffffu) | ((unsigned)R[j] << 16);
    }
    else
    {
        unsigned v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[2 * j] = (unsigned)L[j] & 0xffffffu, v[2 * j + 1] = (unsigned)R[j] & 0xffffffu;
#pragma unroll
        for (int h = 0; h < 2; ++h)
        {
            w[3 * h] = v[4 * h] | (v[4 * h + 1] << 24);
            w[3 * h + 1] = (v[4 * h + 1] >> 8) | (v[4 * h + 2] << 16);
            w[3 * h + 2] = (v[4 * h + 2] >> 16) | (v[4 * h + 3] << 8);
        }
    }
    unsigned *dst = out + i0 * frameBytes / 4;
    const int nd = (cnt * frameBytes + 3) >> 2; // whole dwords: the output is padded to 16 bytes (DMX_OUTPUT_STRIDE)
#ifndef DMX_FLAC_IN_HOST
    if (cnt == 4 && ENC == DMX_PCM_F32)
    {
        reinterpret_cast<uint4 *>(dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
        reinterpret_cast<uint4 *>(dst)[1] = make_uint4(w[4], w[5], w[6], w[7]);
        return;
    }
    if (cnt == 4 && ENC == DMX_PCM_S16)
    {
        reinterpret_cast<uint4 *>(dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#endif
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < nd)
            dst[j] = w[j];
}

#ifndef DMX_FLAC_IN_HOST
// ------------------------------------------------------------------------------------------------ device: the five kernels
__global__ __launch_bounds__(FI_CHUNK_LANES) void flac_in_candidates_kernel(const fi_u8 *f, FiInfo I, int *work)
{
    __shared__ int lds[FI_CHUNK_LANES];
    fi_cand_a(f, I, work, blockIdx.x, threadIdx.x, lds);
    __syncthreads();
    fi_cand_b(I, work, blockIdx.x, threadIdx.x, lds);
}
__global__ __launch_bounds__(FI_CHUNK_LANES) void flac_in_scan_kernel(const fi_u8 *f, FiInfo I, int *work)
{
    __shared__ int lds[2 * FI_CHUNK_LANES];
    fi_scan_a(I, work, blockIdx.x, threadIdx.x, lds);
    __syncthreads();
    fi_scan_b(f, I, work, blockIdx.x, threadIdx.x, lds);
}
__global__ __launch_bounds__(FI_CHUNK_LANES) void flac_in_chain_kernel(FiInfo I, int *work, long long *status)
{
    __shared__ long long lds[FI_CHUNK_LANES];
    fi_chain_a(I, work, threadIdx.x, lds);
    __syncthreads();
    fi_chain_b(I, work, threadIdx.x, lds);
    __syncthreads(); // next[] is written to global memory by this workgroup and read by its lane 0
    fi_chain_c(I, work, status, threadIdx.x, lds);
}
__global__ __launch_bounds__(FI_DEC_LANES) void flac_in_decode_kernel(const fi_u8 *f, FiInfo I, int *work)
{
    __shared__ int lc[32 * FI_DEC_LANES], lh[32 * FI_DEC_LANES];
    fi_decode(f, I, work, blockIdx.x, threadIdx.x, lc, lh);
}
template <int ENC>
__global__ __launch_bounds__(256) void flac_in_finish_kernel(FiInfo I, const int *work, unsigned *out)
{
    fi_finish<ENC>(I, work, out, (long long)blockIdx.x * 256 + threadIdx.x);
}

int launch_flac_decode(const unsigned char *file, long long bytes, const dmx_flac_info *info, int encoding, void *out, long long *status,
                       void *work, hipStream_t s, hipEvent_t *marks)
{
    auto mark = [&](int k) { // tools/flac_in_bench.py: six events around the five launches
        if (marks)
            (void)hipEventRecord(marks[k], s);
    };
    FiInfo I;
    if (!fi_layout(*info, bytes, I))
        return -1;
    int *w = (int *)work;
    mark(0);
    hipLaunchKernelGGL(flac_in_candidates_kernel, dim3(I.nChunks), dim3(FI_CHUNK_LANES), 0, s, file, I, w);
    mark(1);
    hipLaunchKernelGGL(flac_in_scan_kernel, dim3(I.nChunks), dim3(FI_CHUNK_LANES), 0, s, file, I, w);
    mark(2);
    hipLaunchKernelGGL(flac_in_chain_kernel, dim3(1), dim3(FI_CHUNK_LANES), 0, s, I, w, status);
    mark(3);
    if (const char *e = getenv("DMX_FLAC_IN_LANES")) // measurement switch (tools/flac_in_bench.py): 1 .. 64
        I.decLanes = atoi(e) >= 1 && atoi(e) <= FI_DEC_LANES ? atoi(e) : I.decLanes;
    hipLaunchKernelGGL(flac_in_decode_kernel, dim3((I.cap + I.decLanes - 1) / I.decLanes), dim3(FI_DEC_LANES), 0, s, file, I, w);
    mark(4);
    const unsigned gx = (unsigned)(((long long)I.total + 1023) / 1024);
    if (encoding == DMX_PCM_F32)
        hipLaunchKernelGGL(flac_in_finish_kernel<DMX_PCM_F32>, dim3(gx), dim3(256), 0, s, I, (const int *)w, (unsigned *)out);
    else if (encoding == DMX_PCM_S16)
        hipLaunchKernelGGL(flac_in_finish_kernel<DMX_PCM_S16>, dim3(gx), dim3(256), 0, s, I, (const int *)w, (unsigned *)out);
    else
        hipLaunchKernelGGL(flac_in_finish_kernel<DMX_PCM_S24>, dim3(gx), dim3(256), 0, s, I, (const int *)w, (unsigned *)out);
    mark(5);
    return 0;
}
#else
// ------------------------------------------------------------------------------------------------ host: the same phases
// every phase for all lanes of all workgroups in turn: what a barrier and a launch boundary guarantee
int flac_in_host_decode(const unsigned char *file, long long bytes, const dmx_flac_info *info, int encoding, void *out, long long *status,
                        void *work)
{
    FiInfo I;
    if (!fi_layout(*info, bytes, I))
        return -1;
    int *w = (int *)work;
    std::vector<int> lds(2 * FI_CHUNK_LANES), lc(32 * FI_DEC_LANES), lh(32 * FI_DEC_LANES);
    std::vector<long long> lds64(FI_CHUNK_LANES);
    for (int g = 0; g < I.nChunks; ++g)
    {
        for (int l = 0; l < FI_CHUNK_LANES; ++l)
            fi_cand_a(file, I, w, g, l, lds.data());
        for (int l = 0; l < FI_CHUNK_LANES; ++l)
            fi_cand_b(I, w, g, l, lds.data());
    }
    for (int g = 0; g < I.nChunks; ++g)
    {
        for (int l = 0; l < FI_CHUNK_LANES; ++l)
            fi_scan_a(I, w, g, l, lds.data());
        for (int l = 0; l < FI_CHUNK_LANES; ++l)
            fi_scan_b(file, I, w, g, l, lds.data());
    }
    for (int l = 0; l < FI_CHUNK_LANES; ++l)
        fi_chain_a(I, w, l, lds64.data());
    for (int l = 0; l < FI_CHUNK_LANES; ++l)
        fi_chain_b(I, w, l, lds64.data());
    for (int l = 0; l < FI_CHUNK_LANES; ++l)
        fi_chain_c(I, w, status, l, lds64.data());
    for (int g = 0; g < (I.cap + I.decLanes - 1) / I.decLanes; ++g)
        for (int l = 0; l < FI_DEC_LANES; ++l)
            fi_decode(file, I, w, g, l, lc.data(), lh.data());
    for (long long q = 0; q < ((long long)I.total + 3) / 4; ++q)
    {
        if (encoding == DMX_PCM_F32)
            fi_finish<DMX_PCM_F32>(I, w, (unsigned *)out, q);
        else if (encoding == DMX_PCM_S16)
            fi_finish<DMX_PCM_S16>(I, w, (unsigned *)out, q);
        else
            fi_finish<DMX_PCM_S24>(I, w, (unsigned *)out, q);
    }
    return 0;
}
#endif

} // namespace dmx
