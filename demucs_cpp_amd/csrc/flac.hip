// flac.hip — lossless frames behind the PCM stage: the interleaved 16 / 24 bit stereo PCM that pcm.hip writes -> a complete
// .flac file on the device (demucs's --flac; the reference has no encoder, vendor/libnyquist is empty, so there is no
// reference arithmetic: the specification is this project's own, DESIGN.md section 2.11, restated in NumPy in
// tests/flac_spec.py, whose independent decoder checks losslessness).
//
// Every choice is made by EXACT bit counts with stated tie-breaks, integer arithmetic only:
//   frames    fixed block size 4096 (the last frame: n mod 4096 when not zero); header FF F8, CRC-8; footer CRC-16
//   stereo    candidates (L,R) (L,S) (S,R) (M,S), S = L - R, M = (L + R) >> 1: the smallest total, ties to the earliest
//   subframe  CONSTANT if all samples are equal, else the FIXED order 0..min(4, bs - 1) of the smallest count (ties to the
//             lowest), VERBATIM only if strictly smaller than every FIXED
//   residual  Rice, k <= 14 (16 bit, 4-bit parameters) / k <= 30 (24 bit, 5-bit), no escape; partition order p <= 4 while
//             bs mod 2^p == 0 and (bs >> p) > order; per partition the k minimising count (k + 1) + sum(u >> k), ties to the
//             lowest k; per subframe the p of the smallest total, ties to the lowest p
// Three launches, none of which waits on another workgroup:
//   flac_frame_kernel   one workgroup per (frame, output): L and R staged once in LDS as int32 (M and S formed on the fly);
//                       per channel and order every lane sums min(u >> k, kClamp) over its samples for every k, the sums meet
//                       in an LDS table per finest partition, coarser partitions are sums of those; the decisions follow,
//                       then the chosen frame is bit-packed into a zeroed LDS buffer (per-lane code lengths, a block prefix
//                       sum of bit positions, LDS OR), given its CRCs and stored to a bound-sized slot of the workspace,
//                       its byte length to a table.
//   flac_scan_kernel    one workgroup per output: frame offsets, the total, min / max frame size; writes the 42 header bytes
//                       and the file's byte count.
//   flac_compact_kernel one workgroup per (frame, output): slot -> its place behind the header (whole dwords in the middle,
//                       bytes at the unaligned edges).
// kClamp: sum(u >> k) can pass 2^32 (u < 2^30, 4096 samples). A term is clamped to 2^20 - 64: a sum holding a clamped term is
// at least that, and the cost at k = kmax is at most 4096 * (15 + 128) = 585728 (16 bit; 4096 * 31 at 24 bit) - so neither
// the exact nor the clamped cost of such a k is ever the minimum, and the argmin and the minimum are the exact ones; and
// 4096 * (kClamp + 31) < 2^32.
// CRC-16 with zero initial value is linear: lane t takes the bytes [len - (t + 1) C, len - t C) (leading zeros do not change a
// CRC, so chunks are counted from the END), multiplies its CRC by x^(8 C t) mod P, and the lanes' values are XORed.
#include "kernels.h"

#include <cstdint>

namespace dmx
{
namespace
{
constexpr int kFlacBlock = 4096;
constexpr unsigned kClamp = (1u << 20) - 64;
constexpr int kNodes = 31; // partitions of orders 0..4: 1 + 2 + 4 + 8 + 16

constexpr i64 align16(i64 v) { return (v + 15) / 16 * 16; }
constexpr int flac_slot_bytes(int bits) { return (int)align16(18 + 2 * kFlacBlock * bits / 8); }
struct FlacLayout // one output's part of the workspace
{
    i64 nFrames, offOffs, offSlots, stride;
};
FlacLayout flac_layout(int bits, i64 n)
{
    FlacLayout l;
    l.nFrames = (n + kFlacBlock - 1) / kFlacBlock;
    l.offOffs = align16(4 * l.nFrames);
    l.offSlots = l.offOffs + align16(8 * l.nFrames);
    l.stride = l.offSlots + l.nFrames * flac_slot_bytes(bits);
    return l;
}

// bits [pos, pos + n) of the big-endian bit stream := v (1 <= n <= 32, v < 2^n); buf is zero there
__device__ __forceinline__ void put_bits(unsigned *buf, unsigned pos, int n, unsigned v)
{
    const unsigned w = pos >> 5;
    const int room = 32 - (int)(pos & 31);
    if (n <= room)
        atomicOr(&buf[w], v << (room - n));
    else
    {
        atomicOr(&buf[w], v >> (n - room));
        atomicOr(&buf[w + 1], v << (32 - (n - room)));
    }
}
__device__ __forceinline__ unsigned get_byte(const unsigned *buf, int b) { return (buf[b >> 2] >> (24 - 8 * (b & 3))) & 0xffu; }

template <int C>
__device__ __forceinline__ int chan_at(const int *L, const int *R, int i)
{
    return C == 0 ? L[i] : C == 1 ? R[i] : C == 2 ? (L[i] + R[i]) >> 1 : L[i] - R[i];
}
__device__ __forceinline__ int chan_rt(int c, const int *L, const int *R, int i)
{
    return c == 0 ? L[i] : c == 1 ? R[i] : c == 2 ? (L[i] + R[i]) >> 1 : L[i] - R[i];
}
__device__ __forceinline__ unsigned zigzag(int r) { return ((unsigned)r << 1) ^ (unsigned)(r >> 31); }

// a * b mod x^16 + x^15 + x^2 + 1 (bit j = x^j)
__device__ __forceinline__ unsigned gf16_mul(unsigned a, unsigned b)
{
    unsigned r = 0;
    for (int i = 15; i >= 0; --i)
    {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : r << 1;
        if ((b >> i) & 1u)
            r ^= a;
    }
    return r;
}
__device__ __forceinline__ unsigned gf16_xpow(unsigned e)
{
    unsigned r = 1, b = 2;
    for (; e; e >>= 1)
    {
        if (e & 1u)
            r = gf16_mul(r, b);
        b = gf16_mul(b, b);
    }
    return r;
}

// exclusive prefix sum over the block's 256 lanes; total: the block's sum. sWave: 4 words, free between calls
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned *sWave, unsigned &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
    {
        const unsigned y = (unsigned)__shfl_up((int)inc, off, 64);
        if (lane >= off)
            inc += y;
    }
    __syncthreads();
    if (lane == 63)
        sWave[wave] = inc;
    __syncthreads();
    unsigned add = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
    {
        add += w < wave ? sWave[w] : 0u;
        total += sWave[w];
    }
    return add + inc - v;
}

// channel C, order O: every lane's sums over its samples of one finest partition, added to tab[(O * 16 + q) * NK + k]
template <int NK, int C, int O>
__device__ __forceinline__ void flac_stats_pass(const int *sL, const int *sR, unsigned *tab, unsigned *nonConst, int bs, int ps, int q,
                                                int j, int tpp)
{
    if (O >= bs) // the order does not exist in a block this short (uniform)
        return;
    unsigned acc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k)
        acc[k] = 0;
    bool differs = false;
    const int x00 = O == 0 ? chan_at<C>(sL, sR, 0) : 0;
    for (int m = j; m < ps; m += tpp)
    {
        const int i = q * ps + m;
        if (i < O)
            continue;
        const int x0 = chan_at<C>(sL, sR, i);
        int r = x0;
        if (O == 0)
            differs = differs || x0 != x00;
        if (O == 1)
            r = x0 - chan_at<C>(sL, sR, i - 1);
        if (O == 2)
            r = x0 - 2 * chan_at<C>(sL, sR, i - 1) + chan_at<C>(sL, sR, i - 2);
        if (O == 3)
            r = x0 - 3 * chan_at<C>(sL, sR, i - 1) + 3 * chan_at<C>(sL, sR, i - 2) - chan_at<C>(sL, sR, i - 3);
        if (O == 4)
            r = x0 - 4 * chan_at<C>(sL, sR, i - 1) + 6 * chan_at<C>(sL, sR, i - 2) - 4 * chan_at<C>(sL, sR, i - 3) +
                chan_at<C>(sL, sR, i - 4);
        const unsigned u = zigzag(r);
#pragma unroll
        for (int k = 0; k < NK; ++k)
        {
            const unsigned v = u >> k;
            acc[k] += v < kClamp ? v : kClamp;
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (acc[k])
            atomicAdd(&tab[(O * 16 + q) * NK + k], acc[k]);
    if (O == 0 && differs)
        atomicOr(&nonConst[C], 1u);
}

template <int BITS>
struct FlacShared
{
    static constexpr int NK = BITS == 16 ? 15 : 31;
    static constexpr int kSlotWords = flac_slot_bytes(BITS) / 4;
    static constexpr int kTabWords = 5 * 16 * NK;
    int L[kFlacBlock], R[kFlacBlock];
    unsigned buf[kSlotWords > kTabWords ? kSlotWords : kTabWords]; // the statistics table, then the frame's bits
    unsigned cost[4][5][kNodes];                                   // per channel, order, partition node: the smallest cost
    unsigned char kBest[4][5][kNodes];
    unsigned fixedBits[4][5];
    int fixedP[4][5];
    unsigned nonConst[4];
    int type[4]; // 0 CONSTANT, 1 VERBATIM, 2 + order FIXED
    unsigned subBits[4];
    int ch[2];
    unsigned start[2], totalBits;
    unsigned wave[4];
};

template <int BITS, int C>
__device__ __forceinline__ void flac_channel_stats(FlacShared<BITS> &sh, int bs, int pmax)
{
    constexpr int NK = FlacShared<BITS>::NK;
    const int t = threadIdx.x;
    for (int w = t; w < FlacShared<BITS>::kTabWords; w += 256)
        sh.buf[w] = 0;
    __syncthreads();
    const int ps = bs >> pmax, tpp = 256 >> pmax, q = t >> (8 - pmax), j = t & (tpp - 1);
    flac_stats_pass<NK, C, 0>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 1>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 2>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 3>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 4>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    __syncthreads();
    // node (p, idx) of order o: the sum of its finest partitions, the best k
    if (t < 5 * kNodes)
    {
        const int o = t / kNodes, node = t % kNodes;
        const int p = 31 - __clz(node + 1), idx = node + 1 - (1 << p);
        unsigned best = 0xffffffffu;
        int bk = 0;
        if (o < bs && p <= pmax && (bs >> p) > o)
        {
            const int span = 1 << (pmax - p);
            const unsigned cnt = (unsigned)((bs >> p) - (idx == 0 ? o : 0));
            for (int k = 0; k < NK; ++k)
            {
                unsigned s = cnt * (unsigned)(k + 1);
                for (int f = 0; f < span; ++f)
                    s += sh.buf[(o * 16 + idx * span + f) * NK + k];
                if (s < best)
                    best = s, bk = k;
            }
        }
        sh.cost[C][o][node] = best;
        sh.kBest[C][o][node] = (unsigned char)bk;
    }
    __syncthreads();
}

} // namespace

// grid (frames, outputs), block 256
template <int BITS>
__global__ __launch_bounds__(256) void flac_frame_kernel(const unsigned char *pcm, i64 pcmStride, i64 n, unsigned char *work,
                                                         FlacLayout lay, int rateNibble)
{
    constexpr int PB = BITS == 16 ? 4 : 5;
    __shared__ FlacShared<BITS> sh;
    const int t = threadIdx.x;
    const i64 f = blockIdx.x;
    const i64 i0 = f * kFlacBlock;
    const int bs = n - i0 < kFlacBlock ? (int)(n - i0) : kFlacBlock;
    unsigned char *wk = work + (i64)blockIdx.y * lay.stride;
    const unsigned char *src = pcm + (i64)blockIdx.y * pcmStride + i0 * (BITS == 16 ? 4 : 6);
    for (int i = t; i < bs; i += 256)
    {
        if (BITS == 16)
        {
            const unsigned w = reinterpret_cast<const unsigned *>(src)[i];
            sh.L[i] = (int)(short)(w & 0xffffu);
            sh.R[i] = (int)w >> 16;
        }
        else
        {
            const unsigned short *h = reinterpret_cast<const unsigned short *>(src) + 3 * i;
            const unsigned h0 = h[0], h1 = h[1], h2 = h[2];
            sh.L[i] = (int)((h0 | (h1 << 16)) << 8) >> 8;
            sh.R[i] = (int)(((h1 >> 8) | (h2 << 8)) << 8) >> 8;
        }
    }
    if (t < 4)
        sh.nonConst[t] = 0;
    int pmax = 0;
    while (pmax < 4 && (bs & ((2 << pmax) - 1)) == 0)
        ++pmax;
    // (flac_channel_stats starts with a barrier behind its own zeroing: the loads above are ordered before the reads)
    flac_channel_stats<BITS, 0>(sh, bs, pmax);
    flac_channel_stats<BITS, 1>(sh, bs, pmax);
    flac_channel_stats<BITS, 2>(sh, bs, pmax);
    flac_channel_stats<BITS, 3>(sh, bs, pmax);
    // the table is dead: zero the bit buffer; per (channel, order) the partition order
    for (int w = t; w < FlacShared<BITS>::kSlotWords; w += 256)
        sh.buf[w] = 0;
    if (t < 20)
    {
        const int c = t / 5, o = t % 5;
        unsigned best = 0xffffffffu;
        int bp = 0;
        if (o < bs)
        {
            for (int p = 0; p <= pmax && (bs >> p) > o; ++p)
            {
                unsigned tot = (unsigned)PB << p;
                for (int idx = 0; idx < (1 << p); ++idx)
                    tot += sh.cost[c][o][(1 << p) - 1 + idx];
                if (tot < best)
                    best = tot, bp = p;
            }
            best += 8u + (unsigned)o * (unsigned)(BITS + (c == 3)) + 6u;
        }
        sh.fixedBits[c][o] = best;
        sh.fixedP[c][o] = bp;
    }
    __syncthreads();
    if (t < 4)
    {
        const unsigned w = BITS + (t == 3);
        if (!sh.nonConst[t])
            sh.type[t] = 0, sh.subBits[t] = 8 + w;
        else
        {
            unsigned best = 0xffffffffu;
            int bo = 0;
            for (int o = 0; o < 5; ++o)
                if (sh.fixedBits[t][o] < best)
                    best = sh.fixedBits[t][o], bo = o;
            const unsigned verbatim = 8u + (unsigned)bs * w;
            if (verbatim < best)
                sh.type[t] = 1, sh.subBits[t] = verbatim;
            else
                sh.type[t] = 2 + bo, sh.subBits[t] = best;
        }
    }
    __syncthreads();
    if (t == 0)
    {
        const int ca[4] = {0, 0, 3, 2}, cb[4] = {1, 3, 1, 3};
        const unsigned code[4] = {1, 8, 9, 10};
        int pick = 0;
        for (int a = 1; a < 4; ++a)
            if (sh.subBits[ca[a]] + sh.subBits[cb[a]] < sh.subBits[ca[pick]] + sh.subBits[cb[pick]])
                pick = a;
        unsigned char hdr[16];
        int hl = 0;
        hdr[hl++] = 0xff, hdr[hl++] = 0xf8;
        hdr[hl++] = (unsigned char)(((bs == kFlacBlock ? 0xc : 0x7) << 4) | rateNibble);
        hdr[hl++] = (unsigned char)((code[pick] << 4) | ((BITS == 16 ? 4u : 6u) << 1));
        const unsigned fn = (unsigned)f; // < 2^24
        if (fn < 0x80u)
            hdr[hl++] = (unsigned char)fn;
        else
        {
            int nb = 2;
            while (fn >= (1u << (5 * nb + 1)))
                ++nb;
            hdr[hl++] = (unsigned char)(((0xffu << (8 - nb)) & 0xffu) | (fn >> (6 * (nb - 1))));
            for (int i = nb - 2; i >= 0; --i)
                hdr[hl++] = (unsigned char)(0x80u | ((fn >> (6 * i)) & 0x3fu));
        }
        if (bs != kFlacBlock)
            hdr[hl++] = (unsigned char)((bs - 1) >> 8), hdr[hl++] = (unsigned char)((bs - 1) & 0xff);
        unsigned crc = 0;
        for (int i = 0; i < hl; ++i)
        {
            crc ^= hdr[i];
            for (int b = 0; b < 8; ++b)
                crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xffu : (crc << 1) & 0xffu;
        }
        hdr[hl++] = (unsigned char)crc;
        for (int i = 0; i < hl; ++i)
            put_bits(sh.buf, 8u * i, 8, hdr[i]);
        sh.ch[0] = ca[pick], sh.ch[1] = cb[pick];
        sh.start[0] = 8u * hl;
        sh.start[1] = sh.start[0] + sh.subBits[ca[pick]];
        sh.totalBits = sh.start[1] + sh.subBits[cb[pick]];
    }
    __syncthreads();
    // the two subframes
    for (int s = 0; s < 2; ++s)
    {
        const int c = sh.ch[s], type = sh.type[c], w = BITS + (c == 3);
        const unsigned base = sh.start[s], mask = (1u << w) - 1u; // w <= 25
        if (t == 0)
            put_bits(sh.buf, base, 8, type == 0 ? 0u : type == 1 ? 2u : 0x10u | ((unsigned)(type - 2) << 1));
        if (type == 0)
        {
            if (t == 0)
                put_bits(sh.buf, base + 8, w, (unsigned)chan_rt(c, sh.L, sh.R, 0) & mask);
        }
        else if (type == 1)
        {
            for (int i = t; i < bs; i += 256)
                put_bits(sh.buf, base + 8 + (unsigned)i * w, w, (unsigned)chan_rt(c, sh.L, sh.R, i) & mask);
        }
        else
        {
            const int o = type - 2, p = sh.fixedP[c][o], psp = bs >> p;
            const int c1 = o == 1 ? -1 : o == 2 ? -2 : o == 3 ? -3 : o == 4 ? -4 : 0;
            const int c2 = o == 2 ? 1 : o == 3 ? 3 : o == 4 ? 6 : 0;
            const int c3 = o == 3 ? -1 : o == 4 ? -4 : 0;
            const int c4 = o == 4 ? 1 : 0;
            unsigned val[16];         // the warm-up sample, or u
            unsigned short meta[16];  // k | pre << 8 (pre: the bits in front of the code: method, partition order, parameter)
            unsigned sum = 0;
            int part = (16 * t) / psp, rem = (16 * t) % psp;
#pragma unroll
            for (int e = 0; e < 16; ++e)
            {
                const int i = 16 * t + e;
                val[e] = 0, meta[e] = 0;
                if (i < bs)
                {
                    const int x0 = chan_rt(c, sh.L, sh.R, i);
                    if (i < o)
                    {
                        val[e] = (unsigned)x0 & mask;
                        sum += w;
                    }
                    else
                    {
                        int r = x0;
                        if (o >= 1)
                            r += c1 * chan_rt(c, sh.L, sh.R, i - 1);
                        if (o >= 2)
                            r += c2 * chan_rt(c, sh.L, sh.R, i - 2);
                        if (o >= 3)
                            r += c3 * chan_rt(c, sh.L, sh.R, i - 3);
                        if (o >= 4)
                            r += c4 * chan_rt(c, sh.L, sh.R, i - 4);
                        const unsigned u = zigzag(r);
                        const unsigned k = sh.kBest[c][o][(1 << p) - 1 + part];
                        const unsigned pre = i == o ? 6 + PB : rem == 0 ? PB : 0;
                        val[e] = u, meta[e] = (unsigned short)(k | (pre << 8));
                        sum += pre + (u >> k) + 1 + k;
                    }
                }
                if (++rem == psp)
                    rem = 0, ++part;
            }
            unsigned total;
            unsigned pos = base + 8 + block_scan_excl(sum, sh.wave, total);
#pragma unroll
            for (int e = 0; e < 16; ++e)
            {
                const int i = 16 * t + e;
                if (i >= bs)
                    continue;
                if (i < o)
                {
                    put_bits(sh.buf, pos, w, val[e]);
                    pos += w;
                    continue;
                }
                const unsigned k = meta[e] & 0xffu, pre = meta[e] >> 8, u = val[e];
                if (pre == 6 + PB)
                    put_bits(sh.buf, pos, 6 + PB, ((BITS == 16 ? 0u : 1u) << (4 + PB)) | ((unsigned)p << PB) | k);
                else if (pre)
                    put_bits(sh.buf, pos, PB, k);
                pos += pre;
                const unsigned q = u >> k;
                put_bits(sh.buf, pos + q, (int)k + 1, (1u << k) | (u & ((1u << k) - 1u)));
                pos += q + 1 + k;
            }
        }
    }
    __syncthreads();
    // CRC-16 over the padded frame
    // (the selection rules keep a frame within 18 + the verbatim payload; the clamp only keeps a wrong count inside the slot)
    const int maxBytes = 16 + bs * 2 * BITS / 8;
    const int nBytes = (int)((sh.totalBits + 7) >> 3) < maxBytes ? (int)((sh.totalBits + 7) >> 3) : maxBytes, len = nBytes + 2;
    {
        const int C = (nBytes + 255) >> 8;
        const int hi = nBytes - t * C, lo = hi - C > 0 ? hi - C : 0;
        unsigned crc = 0;
        for (int b = lo; b < hi; ++b)
        {
            crc ^= get_byte(sh.buf, b) << 8;
#pragma unroll
            for (int x = 0; x < 8; ++x)
                crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xffffu : crc << 1;
        }
        if (crc && t)
            crc = gf16_mul(crc, gf16_xpow(8u * (unsigned)C * (unsigned)t));
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            crc ^= (unsigned)__shfl_xor((int)crc, off, 64);
        if ((t & 63) == 0)
            sh.wave[t >> 6] = crc;
        __syncthreads();
        if (t == 0)
            put_bits(sh.buf, 8u * (unsigned)nBytes, 16, sh.wave[0] ^ sh.wave[1] ^ sh.wave[2] ^ sh.wave[3]);
        __syncthreads();
    }
    // the slot holds the byte stream: big-endian words -> memory order
    unsigned *slot = reinterpret_cast<unsigned *>(wk + lay.offSlots + f * flac_slot_bytes(BITS));
    for (int w = t; w < (len + 3) >> 2; w += 256)
        slot[w] = __builtin_bswap32(sh.buf[w]);
    if (t == 0)
        reinterpret_cast<unsigned *>(wk)[f] = (unsigned)len;
}

// grid (outputs), block 256: offsets of the frames, STREAMINFO, the file's byte count
__global__ __launch_bounds__(256) void flac_scan_kernel(unsigned char *work, FlacLayout lay, unsigned char *out, i64 outStride,
                                                        long long *sizes, i64 n, int bits, int rate)
{
    __shared__ unsigned sWave[4], sMin[4], sMax[4];
    const int t = threadIdx.x;
    unsigned char *wk = work + (i64)blockIdx.x * lay.stride;
    const unsigned *lens = reinterpret_cast<const unsigned *>(wk);
    unsigned long long *offs = reinterpret_cast<unsigned long long *>(wk + lay.offOffs);
    unsigned long long carry = 0;
    unsigned mn = 0xffffffffu, mx = 0;
    for (i64 base = 0; base < lay.nFrames; base += 256)
    {
        const i64 i = base + t;
        const unsigned v = i < lay.nFrames ? lens[i] : 0u;
        if (i < lay.nFrames)
        {
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        unsigned total;
        const unsigned ex = block_scan_excl(v, sWave, total);
        if (i < lay.nFrames)
            offs[i] = carry + ex;
        carry += total;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
    {
        const unsigned a = (unsigned)__shfl_xor((int)mn, off, 64), b = (unsigned)__shfl_xor((int)mx, off, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((t & 63) == 0)
        sMin[t >> 6] = mn, sMax[t >> 6] = mx;
    __syncthreads();
    if (t == 0)
    {
        for (int w = 1; w < 4; ++w)
        {
            mn = sMin[w] < mn ? sMin[w] : mn;
            mx = sMax[w] > mx ? sMax[w] : mx;
        }
        unsigned char *h = out + (i64)blockIdx.x * outStride;
        const unsigned long long un = (unsigned long long)n;
        const unsigned char hd[42] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 0x22,
                                      kFlacBlock >> 8, kFlacBlock & 0xff, kFlacBlock >> 8, kFlacBlock & 0xff,
                                      (unsigned char)(mn >> 16), (unsigned char)(mn >> 8), (unsigned char)mn,
                                      (unsigned char)(mx >> 16), (unsigned char)(mx >> 8), (unsigned char)mx,
                                      (unsigned char)(rate >> 12), (unsigned char)(rate >> 4),
                                      (unsigned char)(((rate & 0xf) << 4) | (1 << 1) | (((bits - 1) >> 4) & 1)),
                                      (unsigned char)((((bits - 1) & 0xf) << 4) | (unsigned)((un >> 32) & 0xf)),
                                      (unsigned char)(un >> 24), (unsigned char)(un >> 16), (unsigned char)(un >> 8), (unsigned char)un,
                                      0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 42; ++i)
            h[i] = hd[i];
        sizes[blockIdx.x] = (long long)(42 + carry);
    }
}

// grid (frames, outputs), block 256: slot -> out + 42 + offset
__global__ __launch_bounds__(256) void flac_compact_kernel(const unsigned char *work, FlacLayout lay, int slotBytes, unsigned char *out,
                                                           i64 outStride)
{
    const int t = threadIdx.x;
    const i64 f = blockIdx.x;
    const unsigned char *wk = work + (i64)blockIdx.y * lay.stride;
    const int len = (int)reinterpret_cast<const unsigned *>(wk)[f];
    const unsigned long long off = reinterpret_cast<const unsigned long long *>(wk + lay.offOffs)[f];
    const unsigned char *src = wk + lay.offSlots + f * slotBytes;
    const unsigned *src32 = reinterpret_cast<const unsigned *>(src);
    unsigned char *dst = out + (i64)blockIdx.y * outStride + 42 + (i64)off;
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    head = head < len ? head : len;
    const int nW = (len - head) >> 2, tail0 = head + 4 * nW;
    if (t < head)
        dst[t] = src[t];
    if (t >= 64 && t - 64 < len - tail0)
        dst[tail0 + t - 64] = src[tail0 + t - 64];
    unsigned *dst32 = reinterpret_cast<unsigned *>(dst + head);
    const int sh = head & 3; // source byte of dword j: head + 4 j
    for (int j = t; j < nW; j += 256)
    {
        const unsigned w0 = src32[j + (head >> 2)];
        dst32[j] = sh ? (w0 >> (8 * sh)) | (src32[j + (head >> 2) + 1] << (32 - 8 * sh)) : w0;
    }
}

i64 flac_bound(int bits, i64 n)
{
    if ((bits != 16 && bits != 24) || n < 1 || n >= (i64)1 << 36)
        return -1;
    return align16(42 + 18 * ((n + kFlacBlock - 1) / kFlacBlock) + n * 2 * bits / 8);
}
i64 flac_workspace_bytes(int bits, i64 n)
{
    if ((bits != 16 && bits != 24) || n < 1 || n >= (i64)1 << 36)
        return -1;
    return flac_layout(bits, n).stride;
}

void launch_flac_encode(const unsigned char *pcm, i64 pcmStride, int bits, i64 n, int rate, int nOut, unsigned char *out, i64 outStride,
                        long long *sizes, unsigned char *work, hipStream_t s)
{
    const FlacLayout lay = flac_layout(bits, n);
    const int nib = rate == 44100 ? 9 : rate == 48000 ? 10 : 0;
    const dim3 grid((unsigned)lay.nFrames, (unsigned)nOut);
    if (bits == 16)
        hipLaunchKernelGGL(flac_frame_kernel<16>, grid, dim3(256), 0, s, pcm, pcmStride, n, work, lay, nib);
    else
        hipLaunchKernelGGL(flac_frame_kernel<24>, grid, dim3(256), 0, s, pcm, pcmStride, n, work, lay, nib);
    hipLaunchKernelGGL(flac_scan_kernel, dim3(nOut), dim3(256), 0, s, work, lay, out, outStride, sizes, n, bits, rate);
    hipLaunchKernelGGL(flac_compact_kernel, grid, dim3(256), 0, s, work, lay, flac_slot_bytes(bits), out, outStride);
}

} // namespace dmx
