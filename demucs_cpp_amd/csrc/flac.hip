// flac.hip — lossless frames behind the PCM stage: the interleaved 16 / 24 bit stereo PCM that pcm.hip writes -> a complete
// .flac file on the device (demucs's --flac; the reference has no encoder, vendor/libnyquist is empty, so there is no
// reference arithmetic: the specification is this project's own, DESIGN.md section 2.11, restated in NumPy in
// tests/flac_spec.py (level 0) and tests/flac_lpc_spec.py (levels 1 and 2), whose independent decoders check losslessness).
//
// Every choice is made by EXACT bit counts with stated tie-breaks; level 0 is integer arithmetic only:
//   frames    fixed block size 4096 (the last frame: n mod 4096 when not zero); header FF F8, CRC-8; footer CRC-16
//   stereo    candidates (L,R) (L,S) (S,R) (M,S), S = L - R, M = (L + R) >> 1: the smallest total, ties to the earliest
//   subframe  CONSTANT if all samples are equal, else the FIXED order 0..min(4, bs - 1) of the smallest count (ties to the
//             lowest), VERBATIM only if strictly smaller than every FIXED
//   residual  Rice, k <= 14 (16 bit, 4-bit parameters) / k <= 30 (24 bit, 5-bit), no escape; partition order p <= 4 while
//             bs mod 2^p == 0 and (bs >> p) > order; per partition the k minimising count (k + 1) + sum(u >> k), ties to the
//             lowest k; per subframe the p of the smallest total, ties to the lowest p
//   levels    level 1 adds an LPC candidate of order 8 to every non-CONSTANT subframe of a block of more than 32 samples,
//             level 2 orders 8 and 12 (behind the FIXED orders in the tie-break): an integer Welch window in Q15, the
//             autocorrelation exact in int64, Levinson-Durbin in binary64 with every operation rounded once (contraction off)
//             in a fixed order, coefficients quantised to 12 (16 bit) / 15 (24 bit) bits with error feedback, the residual in
//             int64; a candidate with a residual outside [-2^29, 2^29) is discarded, which keeps u < 2^30 below
// Three launches, none of which waits on another workgroup:
//   flac_frame_kernel   one workgroup per (frame, output): L and R staged once in LDS as int32 (M and S formed on the fly);
//                       per channel and order every lane sums min(u >> k, kClamp) over its samples for every k, the sums meet
//                       in an LDS table per finest partition, coarser partitions are sums of those; the decisions follow,
//                       then the chosen frame is bit-packed into a zeroed LDS buffer (per-lane code lengths, a block prefix
//                       sum of bit positions, LDS OR), given its CRCs and stored to a bound-sized slot of the workspace,
//                       its byte length to a table. LEVEL is a template parameter: level 0 instantiates none of the LPC
//                       phases (window -> LDS, 13 lags per lane and signal -> wave and LDS reduction, Levinson and
//                       quantisation on four lanes -> LDS, one or two more statistics passes per signal).
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
//
// With DMX_FLAC_HOST defined the same bodies compile as plain C++ (tests/flac_host_main.cpp): every kernel is a sequence of
// phases separated by workgroup barriers, each phase a function of (workgroup, lane); what a lane carries over a barrier in
// registers is a small struct. The device kernels call the phases with __syncthreads() between them, the host driver at
// the end of this file runs each phase for all lanes in turn. The three cross-lane register exchanges (the block prefix
// sum, the XOR / min / max / sum reductions over a wave) are the only device-only text: the host driver forms them directly.
#ifdef DMX_FLAC_HOST
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
typedef int64_t i64;
#define FL_DEV static inline
static inline unsigned atomicOr(unsigned *p, unsigned v)
{
    const unsigned o = *p;
    *p = o | v;
    return o;
}
static inline unsigned atomicAdd(unsigned *p, unsigned v)
{
    const unsigned o = *p;
    *p = o + v;
    return o;
}
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }
#else
#include "kernels.h"
#define FL_DEV __device__ __forceinline__
#endif

#include <cstdint>

namespace dmx
{
namespace
{
constexpr int kFlacBlock = 4096;
constexpr unsigned kClamp = (1u << 20) - 64;
constexpr int kNodes = 31; // partitions of orders 0..4: 1 + 2 + 4 + 8 + 16
constexpr int kLags = 13;  // autocorrelation lags 0..12

constexpr i64 align16(i64 v) { return (v + 15) / 16 * 16; }
constexpr int flac_slot_bytes(int bits) { return (int)align16(18 + 2 * kFlacBlock * bits / 8); }
struct FlacLayout // one output's part of the workspace
{
    i64 nFrames, offOffs, offSlots, stride;
};
inline FlacLayout flac_layout(int bits, i64 n)
{
    FlacLayout l;
    l.nFrames = (n + kFlacBlock - 1) / kFlacBlock;
    l.offOffs = align16(4 * l.nFrames);
    l.offSlots = l.offOffs + align16(8 * l.nFrames);
    l.stride = l.offSlots + l.nFrames * flac_slot_bytes(bits);
    return l;
}

// bits [pos, pos + n) of the big-endian bit stream := v (1 <= n <= 32, v < 2^n); buf is zero there
FL_DEV void put_bits(unsigned *buf, unsigned pos, int n, unsigned v)
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
FL_DEV unsigned get_byte(const unsigned *buf, int b) { return (buf[b >> 2] >> (24 - 8 * (b & 3))) & 0xffu; }

template <int C>
FL_DEV int chan_at(const int *L, const int *R, int i)
{
    return C == 0 ? L[i] : C == 1 ? R[i] : C == 2 ? (L[i] + R[i]) >> 1 : L[i] - R[i];
}
FL_DEV int chan_rt(int c, const int *L, const int *R, int i)
{
    return c == 0 ? L[i] : c == 1 ? R[i] : c == 2 ? (L[i] + R[i]) >> 1 : L[i] - R[i];
}
FL_DEV unsigned zigzag(int r) { return ((unsigned)r << 1) ^ (unsigned)(r >> 31); }

// a * b mod x^16 + x^15 + x^2 + 1 (bit j = x^j)
FL_DEV unsigned gf16_mul(unsigned a, unsigned b)
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
FL_DEV unsigned gf16_xpow(unsigned e)
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

#ifndef DMX_FLAC_HOST
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
#endif

// the order behind entry oi of the per-(signal, order) tables: FIXED 0..4, then LPC 8, then LPC 12
template <int LEVEL>
FL_DEV int order_of(int oi)
{
    return LEVEL == 0 || oi < 5 ? oi : oi == 5 ? 8 : 12;
}

// channel C, order O: every lane's sums over its samples of one finest partition, added to tab[(O * 16 + q) * NK + k]
template <int NK, int C, int O>
FL_DEV void flac_stats_pass(const int *sL, const int *sR, unsigned *tab, unsigned *nonConst, int bs, int ps, int q, int j, int tpp)
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

// channel C, the LPC predictor of order M (table entry OI) with the quantised coefficients qc and shift: the same sums over
// the residual x[i] - ((sum qc[j] x[i - 1 - j]) >> shift) in int64; a residual outside [-2^29, 2^29) sets *bad
template <int NK, int C, int M, int OI>
FL_DEV void flac_lpc_stats_pass(const int *sL, const int *sR, unsigned *tab, const int *qc, int shift, unsigned *bad, int ps, int q,
                                int j, int tpp)
{
    unsigned acc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k)
        acc[k] = 0;
    bool out = false;
    for (int m = j; m < ps; m += tpp)
    {
        const int i = q * ps + m;
        if (i < M)
            continue;
        i64 pred = 0;
#pragma unroll
        for (int jj = 0; jj < M; ++jj)
            pred += (i64)qc[jj] * (i64)chan_at<C>(sL, sR, i - 1 - jj);
        const i64 r = (i64)chan_at<C>(sL, sR, i) - (pred >> shift);
        out = out || r < -((i64)1 << 29) || r >= ((i64)1 << 29);
        const unsigned u = zigzag((int)r); // (a residual out of range: the candidate is discarded, its sums are not used)
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
            atomicAdd(&tab[(OI * 16 + q) * NK + k], acc[k]);
    if (out)
        atomicOr(bad, 1u);
}

template <int LEVEL>
struct FlacLpcShared
{
    i64 ac[4][4][kLags];  // per signal and wave: the autocorrelation
    int q[4][LEVEL][12];  // per signal and candidate (order 8, order 12): the quantised coefficients
    int shift[4][LEVEL];
    unsigned ok[4][LEVEL];  // the candidate exists
    unsigned bad[4][LEVEL]; // a residual left [-2^29, 2^29)
};
template <>
struct FlacLpcShared<0>
{
};

template <int BITS, int LEVEL>
struct FlacShared
{
    static constexpr int NK = BITS == 16 ? 15 : 31;
    static constexpr int NO = 5 + LEVEL; // entries per signal: FIXED 0..4, LPC 8, LPC 12
    static constexpr int kSlotWords = flac_slot_bytes(BITS) / 4;
    static constexpr int kTabWords = NO * 16 * NK;
    int L[kFlacBlock], R[kFlacBlock];
    unsigned buf[kSlotWords > kTabWords ? kSlotWords : kTabWords]; // (the window,) the statistics table, then the frame's bits
    unsigned cost[4][NO][kNodes];                                  // per channel, order, partition node: the smallest cost
    unsigned char kBest[4][NO][kNodes];
    unsigned fixedBits[4][NO];
    int fixedP[4][NO];
    unsigned nonConst[4];
    int type[4]; // 0 CONSTANT, 1 VERBATIM, 2 + entry: FIXED (entries 0..4) and LPC (5, 6)
    unsigned subBits[4];
    int ch[2];
    unsigned start[2], totalBits;
    unsigned wave[4];
    FlacLpcShared<LEVEL> lpc;
};

// what a lane carries from the first half of the bit-packer over the prefix sum to the second
struct FlacLane
{
    unsigned val[16];        // the warm-up sample, or u
    unsigned short meta[16]; // k | pre << 8 (pre: the bits in front of the code: coefficients, method, partition order, parameter)
    unsigned sum;
};

// ------------------------------------------------------------------------------------------------ the frame kernel's phases
template <int BITS, int LEVEL>
FL_DEV void fl_load(FlacShared<BITS, LEVEL> &sh, const unsigned char *src, int bs, int t)
{
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
}

// W[i] = floor(131072 i (bs - 1 - i) / (bs - 1)^2) -> buf[i] (bs > 32)
template <int BITS, int LEVEL>
FL_DEV void fl_window(FlacShared<BITS, LEVEL> &sh, int bs, int t)
{
    const unsigned long long d = (unsigned long long)(bs - 1) * (unsigned long long)(bs - 1);
    for (int i = t; i < bs; i += 256)
        sh.buf[i] = (unsigned)(131072ull * (unsigned long long)i * (unsigned long long)(bs - 1 - i) / d);
}

// signal C: this lane's 16 samples times 13 lags
template <int BITS, int LEVEL, int C>
FL_DEV void fl_autocorr(const FlacShared<BITS, LEVEL> &sh, int bs, int t, i64 acc[kLags])
{
    int xw[28]; // the windowed samples 16 t - 12 .. 16 t + 15
#pragma unroll
    for (int e = 0; e < 28; ++e)
    {
        const int i = 16 * t - 12 + e;
        xw[e] = i >= 0 && i < bs ? (int)(((i64)chan_at<C>(sh.L, sh.R, i) * (i64)sh.buf[i]) >> 15) : 0;
    }
#pragma unroll
    for (int l = 0; l < kLags; ++l)
    {
        i64 s = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            s += (i64)xw[12 + e] * (i64)xw[12 + e - l];
        acc[l] = s;
    }
}

// the lanes' lags -> sh.lpc.ac[C][wave] (integer sums: any tree gives the same value)
template <int BITS, int LEVEL>
FL_DEV void fl_autocorr_reduce(FlacShared<BITS, LEVEL> &sh, int C, int t, i64 acc[kLags])
{
#ifdef DMX_FLAC_HOST
    if (t == 0)
        for (int w = 0; w < 4; ++w)
            for (int l = 0; l < kLags; ++l)
                sh.lpc.ac[C][w][l] = 0;
    for (int l = 0; l < kLags; ++l)
        sh.lpc.ac[C][t >> 6][l] += acc[l];
#else
#pragma unroll
    for (int l = 0; l < kLags; ++l)
    {
        i64 v = acc[l];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            v += __shfl_xor(v, off, 64);
        if ((t & 63) == 0)
            sh.lpc.ac[C][t >> 6][l] = v;
    }
#endif
}

// coefficients a[0..M) -> candidate e of signal c: the shift, the quantised coefficients with error feedback
template <int BITS, int LEVEL, int M>
FL_DEV void fl_quantise(FlacShared<BITS, LEVEL> &sh, int c, int e, const double *a)
{
#ifndef DMX_FLAC_HOST
#pragma clang fp contract(off)
#endif
    constexpr int P = BITS == 16 ? 12 : 15;
    constexpr int lim = (1 << (P - 1)) - 1;
    double cmax = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j)
    {
        const double v = fabs(a[j]);
        if (v > cmax)
            cmax = v;
    }
    int s = -1;
#pragma unroll
    for (int tt = 15; tt >= 0; --tt)
        if (s < 0 && floor(cmax * (double)(1 << tt) + 0.5) <= (double)lim)
            s = tt;
    if (s < 0)
        return;
    const double scale = (double)(1 << s);
    double err = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j)
    {
        const double v = a[j] * scale + err;
        double fl = floor(v + 0.5);
        fl = !(fl >= (double)(-lim - 1)) ? (double)(-lim - 1) : fl > (double)lim ? (double)lim : fl; // (|a[j]| <= cmax: never NaN)
        sh.lpc.q[c][e][j] = (int)fl;
        err = v - fl;
    }
    sh.lpc.shift[c][e] = s;
    sh.lpc.ok[c][e] = 1u;
}

// one lane per signal: the waves' lags summed, scaled into 53 bits, Levinson-Durbin in binary64 in the order of the
// specification (every operation rounded once), the coefficients of orders 8 and 12 quantised
template <int BITS, int LEVEL>
FL_DEV void fl_levinson(FlacShared<BITS, LEVEL> &sh, int c)
{
#ifndef DMX_FLAC_HOST
#pragma clang fp contract(off)
#endif
    constexpr int MMAX = LEVEL == 1 ? 8 : 12;
#pragma unroll
    for (int e = 0; e < LEVEL; ++e)
        sh.lpc.ok[c][e] = 0u, sh.lpc.bad[c][e] = 0u;
    i64 R[kLags];
#pragma unroll
    for (int l = 0; l < kLags; ++l)
        R[l] = sh.lpc.ac[c][0][l] + sh.lpc.ac[c][1][l] + sh.lpc.ac[c][2][l] + sh.lpc.ac[c][3][l];
    if (R[0] == 0)
        return;
    int g = 64 - __clzll(R[0]) - 52;
    g = g < 0 ? 0 : g;
    double r[kLags];
#pragma unroll
    for (int l = 0; l < kLags; ++l)
        r[l] = (double)(R[l] >> g);
    double a[12], err = r[0];
#pragma unroll
    for (int j = 0; j < 12; ++j)
        a[j] = 0.0;
    bool alive = true;
#pragma unroll
    for (int m = 1; m <= MMAX; ++m)
    {
        double acc = r[m];
#pragma unroll
        for (int j = 1; j < m; ++j)
            acc = acc - a[j - 1] * r[m - j];
        alive = alive && err > 0.0;
        if (alive)
        {
            const double k = acc / err;
            double nw[12];
#pragma unroll
            for (int j = 1; j < m; ++j)
                nw[j - 1] = a[j - 1] - k * a[m - 1 - j];
            nw[m - 1] = k;
#pragma unroll
            for (int j = 0; j < m; ++j)
                a[j] = nw[j];
            err = err * (1.0 - k * k);
            if (m == 8)
                fl_quantise<BITS, LEVEL, 8>(sh, c, 0, a);
            if (LEVEL == 2 && m == 12)
                fl_quantise<BITS, LEVEL, 12>(sh, c, LEVEL - 1, a);
        }
    }
}

template <int BITS, int LEVEL>
FL_DEV void fl_stats_zero(FlacShared<BITS, LEVEL> &sh, int t)
{
    for (int w = t; w < FlacShared<BITS, LEVEL>::kTabWords; w += 256)
        sh.buf[w] = 0;
}
template <int BITS, int LEVEL, int C>
FL_DEV void fl_stats_passes(FlacShared<BITS, LEVEL> &sh, int bs, int pmax, int t)
{
    constexpr int NK = FlacShared<BITS, LEVEL>::NK;
    const int ps = bs >> pmax, tpp = 256 >> pmax, q = t >> (8 - pmax), j = t & (tpp - 1);
    flac_stats_pass<NK, C, 0>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 1>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 2>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 3>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    flac_stats_pass<NK, C, 4>(sh.L, sh.R, sh.buf, sh.nonConst, bs, ps, q, j, tpp);
    if constexpr (LEVEL > 0)
    {
        if (bs > 32) // (uniform, as are the candidates' flags)
        {
            if (sh.lpc.ok[C][0])
                flac_lpc_stats_pass<NK, C, 8, 5>(sh.L, sh.R, sh.buf, sh.lpc.q[C][0], sh.lpc.shift[C][0], &sh.lpc.bad[C][0], ps, q, j, tpp);
            if constexpr (LEVEL > 1)
                if (sh.lpc.ok[C][1])
                    flac_lpc_stats_pass<NK, C, 12, 6>(sh.L, sh.R, sh.buf, sh.lpc.q[C][1], sh.lpc.shift[C][1], &sh.lpc.bad[C][1], ps, q, j,
                                                      tpp);
        }
    }
}
// node (p, idx) of entry o: the sum of its finest partitions, the best k
template <int BITS, int LEVEL, int C>
FL_DEV void fl_stats_nodes(FlacShared<BITS, LEVEL> &sh, int bs, int pmax, int t)
{
    constexpr int NK = FlacShared<BITS, LEVEL>::NK;
    if (t < FlacShared<BITS, LEVEL>::NO * kNodes)
    {
        const int o = t / kNodes, node = t % kNodes, ord = order_of<LEVEL>(o);
        const int p = 31 - __clz(node + 1), idx = node + 1 - (1 << p);
        unsigned best = 0xffffffffu;
        int bk = 0;
        if (ord < bs && p <= pmax && (bs >> p) > ord)
        {
            const int span = 1 << (pmax - p);
            const unsigned cnt = (unsigned)((bs >> p) - (idx == 0 ? ord : 0));
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
}

// the table is dead: zero the bit buffer; per (channel, entry) the partition order and the subframe's bit count
template <int BITS, int LEVEL>
FL_DEV void fl_decide_orders(FlacShared<BITS, LEVEL> &sh, int bs, int pmax, int t)
{
    constexpr int PB = BITS == 16 ? 4 : 5;
    constexpr int NO = FlacShared<BITS, LEVEL>::NO;
    for (int w = t; w < FlacShared<BITS, LEVEL>::kSlotWords; w += 256)
        sh.buf[w] = 0;
    if (t < 4 * NO)
    {
        const int c = t / NO, o = t % NO, ord = order_of<LEVEL>(o);
        unsigned best = 0xffffffffu;
        int bp = 0;
        bool exists = ord < bs;
        if constexpr (LEVEL > 0)
            if (o >= 5)
                exists = bs > 32 && sh.lpc.ok[c][o - 5] && !sh.lpc.bad[c][o - 5];
        if (exists)
        {
            for (int p = 0; p <= pmax && (bs >> p) > ord; ++p)
            {
                unsigned tot = (unsigned)PB << p;
                for (int idx = 0; idx < (1 << p); ++idx)
                    tot += sh.cost[c][o][(1 << p) - 1 + idx];
                if (tot < best)
                    best = tot, bp = p;
            }
            best += 8u + (unsigned)ord * (unsigned)(BITS + (c == 3)) + 6u;
            if (LEVEL > 0 && o >= 5)
                best += 9u + (unsigned)ord * (BITS == 16 ? 12u : 15u);
        }
        sh.fixedBits[c][o] = best;
        sh.fixedP[c][o] = bp;
    }
}
template <int BITS, int LEVEL>
FL_DEV void fl_decide_types(FlacShared<BITS, LEVEL> &sh, int bs, int t)
{
    if (t < 4)
    {
        const unsigned w = BITS + (t == 3);
        if (!sh.nonConst[t])
            sh.type[t] = 0, sh.subBits[t] = 8 + w;
        else
        {
            unsigned best = 0xffffffffu;
            int bo = 0;
            for (int o = 0; o < FlacShared<BITS, LEVEL>::NO; ++o)
                if (sh.fixedBits[t][o] < best)
                    best = sh.fixedBits[t][o], bo = o;
            const unsigned verbatim = 8u + (unsigned)bs * w;
            if (verbatim < best)
                sh.type[t] = 1, sh.subBits[t] = verbatim;
            else
                sh.type[t] = 2 + bo, sh.subBits[t] = best;
        }
    }
}
template <int BITS, int LEVEL>
FL_DEV void fl_frame_header(FlacShared<BITS, LEVEL> &sh, int bs, i64 f, int rateNibble, int t)
{
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
}

// subframe s: its header byte; a CONSTANT or VERBATIM subframe whole
template <int BITS, int LEVEL>
FL_DEV void fl_sub_head(FlacShared<BITS, LEVEL> &sh, int s, int bs, int t)
{
    const int c = sh.ch[s], type = sh.type[c], w = BITS + (c == 3);
    const unsigned base = sh.start[s], mask = (1u << w) - 1u; // w <= 25
    if (t == 0)
    {
        unsigned head = type == 0 ? 0u : type == 1 ? 2u : 0x10u | ((unsigned)(type - 2) << 1);
        if (LEVEL > 0 && type >= 7)
            head = 0x40u | ((unsigned)(order_of<LEVEL>(type - 2) - 1) << 1);
        put_bits(sh.buf, base, 8, head);
    }
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
}
// a predicted subframe, first half: this lane's 16 samples as warm-up values or Rice codes, their bit count
template <int BITS, int LEVEL>
FL_DEV void fl_sub_codes(const FlacShared<BITS, LEVEL> &sh, int s, int bs, int t, FlacLane &ln)
{
    constexpr int PB = BITS == 16 ? 4 : 5;
    const int c = sh.ch[s], w = BITS + (c == 3);
    const unsigned mask = (1u << w) - 1u;
    const int oi = sh.type[c] - 2, o = order_of<LEVEL>(oi), p = sh.fixedP[c][oi], psp = bs >> p;
    const int c1 = o == 1 ? -1 : o == 2 ? -2 : o == 3 ? -3 : o == 4 ? -4 : 0;
    const int c2 = o == 2 ? 1 : o == 3 ? 3 : o == 4 ? 6 : 0;
    const int c3 = o == 3 ? -1 : o == 4 ? -4 : 0;
    const int c4 = o == 4 ? 1 : 0;
    const bool lpc = LEVEL > 0 && oi >= 5;
    unsigned sum = 0;
    int part = (16 * t) / psp, rem = (16 * t) % psp;
#pragma unroll
    for (int e = 0; e < 16; ++e)
    {
        const int i = 16 * t + e;
        ln.val[e] = 0, ln.meta[e] = 0;
        if (i < bs)
        {
            const int x0 = chan_rt(c, sh.L, sh.R, i);
            if (i < o)
            {
                ln.val[e] = (unsigned)x0 & mask;
                sum += w;
            }
            else
            {
                int r = x0;
                if (!lpc)
                {
                    if (o >= 1)
                        r += c1 * chan_rt(c, sh.L, sh.R, i - 1);
                    if (o >= 2)
                        r += c2 * chan_rt(c, sh.L, sh.R, i - 2);
                    if (o >= 3)
                        r += c3 * chan_rt(c, sh.L, sh.R, i - 3);
                    if (o >= 4)
                        r += c4 * chan_rt(c, sh.L, sh.R, i - 4);
                }
                if constexpr (LEVEL > 0)
                    if (lpc)
                    {
                        i64 pred = 0;
                        for (int jj = 0; jj < o; ++jj)
                            pred += (i64)sh.lpc.q[c][oi - 5][jj] * (i64)chan_rt(c, sh.L, sh.R, i - 1 - jj);
                        r = (int)((i64)x0 - (pred >> sh.lpc.shift[c][oi - 5]));
                    }
                const unsigned u = zigzag(r);
                const unsigned k = sh.kBest[c][oi][(1 << p) - 1 + part];
                unsigned pre = i == o ? 6 + PB : rem == 0 ? PB : 0;
                if (lpc && i == o)
                    pre += 9u + (unsigned)o * (BITS == 16 ? 12u : 15u); // <= 200
                ln.val[e] = u, ln.meta[e] = (unsigned short)(k | (pre << 8));
                sum += pre + (u >> k) + 1 + k;
            }
        }
        if (++rem == psp)
            rem = 0, ++part;
    }
    ln.sum = sum;
}
// second half: the lane's bits from bit position pos on
template <int BITS, int LEVEL>
FL_DEV void fl_sub_pack(FlacShared<BITS, LEVEL> &sh, int s, int bs, int t, const FlacLane &ln, unsigned pos)
{
    constexpr int PB = BITS == 16 ? 4 : 5;
    constexpr int P = BITS == 16 ? 12 : 15;
    const int c = sh.ch[s], w = BITS + (c == 3);
    const int oi = sh.type[c] - 2, o = order_of<LEVEL>(oi), p = sh.fixedP[c][oi];
#pragma unroll
    for (int e = 0; e < 16; ++e)
    {
        const int i = 16 * t + e;
        if (i >= bs)
            continue;
        if (i < o)
        {
            put_bits(sh.buf, pos, w, ln.val[e]);
            pos += w;
            continue;
        }
        const unsigned k = ln.meta[e] & 0xffu, pre = ln.meta[e] >> 8, u = ln.val[e];
        if (pre >= 6 + PB)
        {
            unsigned at = pos;
            if constexpr (LEVEL > 0)
                if (oi >= 5)
                {
                    put_bits(sh.buf, at, 9, ((unsigned)(P - 1) << 5) | (unsigned)sh.lpc.shift[c][oi - 5]);
                    at += 9;
                    for (int jj = 0; jj < o; ++jj, at += P)
                        put_bits(sh.buf, at, P, (unsigned)sh.lpc.q[c][oi - 5][jj] & ((1u << P) - 1u));
                }
            put_bits(sh.buf, at, 6 + PB, ((BITS == 16 ? 0u : 1u) << (4 + PB)) | ((unsigned)p << PB) | k);
        }
        else if (pre)
            put_bits(sh.buf, pos, PB, k);
        pos += pre;
        const unsigned q = u >> k;
        put_bits(sh.buf, pos + q, (int)k + 1, (1u << k) | (u & ((1u << k) - 1u)));
        pos += q + 1 + k;
    }
}

// the byte count of the frame without its CRC-16
// (the selection rules keep a frame within 18 + the verbatim payload; the clamp only keeps a wrong count inside the slot)
template <int BITS, int LEVEL>
FL_DEV int fl_frame_bytes(const FlacShared<BITS, LEVEL> &sh, int bs)
{
    const int maxBytes = 16 + bs * 2 * BITS / 8;
    return (int)((sh.totalBits + 7) >> 3) < maxBytes ? (int)((sh.totalBits + 7) >> 3) : maxBytes;
}
// CRC-16 over the padded frame: this lane's chunk, moved to its place
template <int BITS, int LEVEL>
FL_DEV unsigned fl_crc_lane(const FlacShared<BITS, LEVEL> &sh, int nBytes, int t)
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
    return crc;
}
template <int BITS, int LEVEL>
FL_DEV void fl_crc_put(FlacShared<BITS, LEVEL> &sh, int nBytes, int t)
{
    if (t == 0)
        put_bits(sh.buf, 8u * (unsigned)nBytes, 16, sh.wave[0] ^ sh.wave[1] ^ sh.wave[2] ^ sh.wave[3]);
}
// the slot holds the byte stream: big-endian words -> memory order
template <int BITS, int LEVEL>
FL_DEV void fl_store(const FlacShared<BITS, LEVEL> &sh, unsigned char *wk, const FlacLayout &lay, i64 f, int len, int t)
{
    unsigned *slot = reinterpret_cast<unsigned *>(wk + lay.offSlots + f * flac_slot_bytes(BITS));
    for (int w = t; w < (len + 3) >> 2; w += 256)
        slot[w] = __builtin_bswap32(sh.buf[w]);
    if (t == 0)
        reinterpret_cast<unsigned *>(wk)[f] = (unsigned)len;
}
FL_DEV int fl_pmax(int bs)
{
    int pmax = 0;
    while (pmax < 4 && (bs & ((2 << pmax) - 1)) == 0)
        ++pmax;
    return pmax;
}

// ------------------------------------------------------------------------------------------------ the scan kernel's phases
struct FlacScanLane
{
    unsigned long long carry;
    unsigned mn, mx, v;
};
FL_DEV void fl_scan_take(const unsigned char *wk, const FlacLayout &lay, i64 base, int t, FlacScanLane &ln)
{
    const unsigned *lens = reinterpret_cast<const unsigned *>(wk);
    const i64 i = base + t;
    ln.v = i < lay.nFrames ? lens[i] : 0u;
    if (i < lay.nFrames)
    {
        ln.mn = ln.v < ln.mn ? ln.v : ln.mn;
        ln.mx = ln.v > ln.mx ? ln.v : ln.mx;
    }
}
FL_DEV void fl_scan_put(unsigned char *wk, const FlacLayout &lay, i64 base, int t, FlacScanLane &ln, unsigned ex, unsigned total)
{
    unsigned long long *offs = reinterpret_cast<unsigned long long *>(wk + lay.offOffs);
    const i64 i = base + t;
    if (i < lay.nFrames)
        offs[i] = ln.carry + ex;
    ln.carry += total;
}
// STREAMINFO and the file's byte count (one lane)
FL_DEV void fl_scan_header(unsigned char *h, long long *size, unsigned mn, unsigned mx, unsigned long long carry, i64 n, int bits, int rate)
{
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
    *size = (long long)(42 + carry);
}

// ------------------------------------------------------------------------------------------------ the compact kernel's body
FL_DEV void fl_compact(const unsigned char *wk, const FlacLayout &lay, int slotBytes, unsigned char *outFile, i64 f, int t)
{
    const int len = (int)reinterpret_cast<const unsigned *>(wk)[f];
    const unsigned long long off = reinterpret_cast<const unsigned long long *>(wk + lay.offOffs)[f];
    const unsigned char *src = wk + lay.offSlots + f * slotBytes;
    const unsigned *src32 = reinterpret_cast<const unsigned *>(src);
    unsigned char *dst = outFile + 42 + (i64)off;
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

} // namespace

#ifndef DMX_FLAC_HOST
// ------------------------------------------------------------------------------------------------ device: the three kernels
// grid (frames, outputs), block 256
template <int BITS, int LEVEL>
__global__ __launch_bounds__(256) void flac_frame_kernel(const unsigned char *pcm, i64 pcmStride, i64 n, unsigned char *work,
                                                         FlacLayout lay, int rateNibble)
{
    __shared__ FlacShared<BITS, LEVEL> sh;
    const int t = threadIdx.x;
    const i64 f = blockIdx.x;
    const i64 i0 = f * kFlacBlock;
    const int bs = n - i0 < kFlacBlock ? (int)(n - i0) : kFlacBlock;
    unsigned char *wk = work + (i64)blockIdx.y * lay.stride;
    const unsigned char *src = pcm + (i64)blockIdx.y * pcmStride + i0 * (BITS == 16 ? 4 : 6);
    fl_load(sh, src, bs, t);
    const int pmax = fl_pmax(bs);
    if constexpr (LEVEL > 0)
    {
        if (bs > 32)
        {
            fl_window(sh, bs, t);
            __syncthreads();
            i64 acc[kLags];
            fl_autocorr<BITS, LEVEL, 0>(sh, bs, t, acc);
            fl_autocorr_reduce(sh, 0, t, acc);
            fl_autocorr<BITS, LEVEL, 1>(sh, bs, t, acc);
            fl_autocorr_reduce(sh, 1, t, acc);
            fl_autocorr<BITS, LEVEL, 2>(sh, bs, t, acc);
            fl_autocorr_reduce(sh, 2, t, acc);
            fl_autocorr<BITS, LEVEL, 3>(sh, bs, t, acc);
            fl_autocorr_reduce(sh, 3, t, acc);
            __syncthreads();
            if (t < 4)
                fl_levinson(sh, t);
            __syncthreads(); // the window is dead: the table's zeroing below may overwrite it
        }
    }
    // (the zeroing is followed by a barrier: the loads above are ordered before the reads)
#define DMX_FLAC_CHANNEL(C)                          \
    fl_stats_zero(sh, t);                            \
    __syncthreads();                                 \
    fl_stats_passes<BITS, LEVEL, C>(sh, bs, pmax, t); \
    __syncthreads();                                 \
    fl_stats_nodes<BITS, LEVEL, C>(sh, bs, pmax, t);  \
    __syncthreads();
    DMX_FLAC_CHANNEL(0)
    DMX_FLAC_CHANNEL(1)
    DMX_FLAC_CHANNEL(2)
    DMX_FLAC_CHANNEL(3)
#undef DMX_FLAC_CHANNEL
    fl_decide_orders(sh, bs, pmax, t);
    __syncthreads();
    fl_decide_types(sh, bs, t);
    __syncthreads();
    fl_frame_header(sh, bs, f, rateNibble, t);
    __syncthreads();
    // the two subframes
    for (int s = 0; s < 2; ++s)
    {
        fl_sub_head(sh, s, bs, t);
        if (sh.type[sh.ch[s]] >= 2)
        {
            FlacLane ln;
            fl_sub_codes(sh, s, bs, t, ln);
            unsigned total;
            const unsigned pos = sh.start[s] + 8 + block_scan_excl(ln.sum, sh.wave, total);
            fl_sub_pack(sh, s, bs, t, ln, pos);
        }
    }
    __syncthreads();
    const int nBytes = fl_frame_bytes(sh, bs), len = nBytes + 2;
    {
        unsigned crc = fl_crc_lane(sh, nBytes, t);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            crc ^= (unsigned)__shfl_xor((int)crc, off, 64);
        if ((t & 63) == 0)
            sh.wave[t >> 6] = crc;
        __syncthreads();
        fl_crc_put(sh, nBytes, t);
        __syncthreads();
    }
    fl_store(sh, wk, lay, f, len, t);
}

// grid (outputs), block 256: offsets of the frames, STREAMINFO, the file's byte count
__global__ __launch_bounds__(256) void flac_scan_kernel(unsigned char *work, FlacLayout lay, unsigned char *out, i64 outStride,
                                                        long long *sizes, i64 n, int bits, int rate)
{
    __shared__ unsigned sWave[4], sMin[4], sMax[4];
    const int t = threadIdx.x;
    unsigned char *wk = work + (i64)blockIdx.x * lay.stride;
    FlacScanLane ln = {0, 0xffffffffu, 0, 0};
    for (i64 base = 0; base < lay.nFrames; base += 256)
    {
        fl_scan_take(wk, lay, base, t, ln);
        unsigned total;
        const unsigned ex = block_scan_excl(ln.v, sWave, total);
        fl_scan_put(wk, lay, base, t, ln, ex, total);
    }
    unsigned mn = ln.mn, mx = ln.mx;
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
        fl_scan_header(out + (i64)blockIdx.x * outStride, sizes + blockIdx.x, mn, mx, ln.carry, n, bits, rate);
    }
}

// grid (frames, outputs), block 256: slot -> out + 42 + offset
__global__ __launch_bounds__(256) void flac_compact_kernel(const unsigned char *work, FlacLayout lay, int slotBytes, unsigned char *out,
                                                           i64 outStride)
{
    fl_compact(work + (i64)blockIdx.y * lay.stride, lay, slotBytes, out + (i64)blockIdx.y * outStride, blockIdx.x, threadIdx.x);
}
#endif

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

#ifndef DMX_FLAC_HOST
void launch_flac_encode(const unsigned char *pcm, i64 pcmStride, int bits, i64 n, int rate, int nOut, unsigned char *out, i64 outStride,
                        long long *sizes, unsigned char *work, hipStream_t s, int level, hipEvent_t *marks)
{
    auto mark = [&](int k) { // tools/flac_bench.py: four events around the three launches
        if (marks)
            (void)hipEventRecord(marks[k], s);
    };
    const FlacLayout lay = flac_layout(bits, n);
    const int nib = rate == 44100 ? 9 : rate == 48000 ? 10 : 0;
    const dim3 grid((unsigned)lay.nFrames, (unsigned)nOut);
    mark(0);
#define DMX_FLAC_FRAME(B, LV) hipLaunchKernelGGL((flac_frame_kernel<B, LV>), grid, dim3(256), 0, s, pcm, pcmStride, n, work, lay, nib)
    if (bits == 16)
    {
        if (level == 0)
            DMX_FLAC_FRAME(16, 0);
        else if (level == 1)
            DMX_FLAC_FRAME(16, 1);
        else
            DMX_FLAC_FRAME(16, 2);
    }
    else
    {
        if (level == 0)
            DMX_FLAC_FRAME(24, 0);
        else if (level == 1)
            DMX_FLAC_FRAME(24, 1);
        else
            DMX_FLAC_FRAME(24, 2);
    }
#undef DMX_FLAC_FRAME
    mark(1);
    hipLaunchKernelGGL(flac_scan_kernel, dim3(nOut), dim3(256), 0, s, work, lay, out, outStride, sizes, n, bits, rate);
    mark(2);
    hipLaunchKernelGGL(flac_compact_kernel, grid, dim3(256), 0, s, work, lay, flac_slot_bytes(bits), out, outStride);
    mark(3);
}
#else
// ------------------------------------------------------------------------------------------------ host: the same phases
// every phase for all lanes of a workgroup in turn, the workgroups and the launches one after another: what a barrier and a
// launch boundary guarantee
template <int BITS, int LEVEL>
static void flac_host_frame(const unsigned char *pcm, i64 n, unsigned char *wk, const FlacLayout &lay, int rateNibble, i64 f)
{
    typedef FlacShared<BITS, LEVEL> SH;
    std::vector<unsigned char> mem(sizeof(SH)); // not initialised by a constructor, as LDS is not
    memset(mem.data(), 0xa5, mem.size());
    SH &sh = *reinterpret_cast<SH *>(mem.data());
    const i64 i0 = f * kFlacBlock;
    const int bs = n - i0 < kFlacBlock ? (int)(n - i0) : kFlacBlock;
    const unsigned char *src = pcm + i0 * (BITS == 16 ? 4 : 6);
#define FL_ALL(...)               \
    for (int t = 0; t < 256; ++t) \
    {                             \
        __VA_ARGS__;              \
    }
    FL_ALL(fl_load(sh, src, bs, t))
    const int pmax = fl_pmax(bs);
    if constexpr (LEVEL > 0)
    {
        if (bs > 32)
        {
            FL_ALL(fl_window(sh, bs, t))
            i64 acc[kLags];
            FL_ALL(fl_autocorr<BITS, LEVEL, 0>(sh, bs, t, acc); fl_autocorr_reduce(sh, 0, t, acc))
            FL_ALL(fl_autocorr<BITS, LEVEL, 1>(sh, bs, t, acc); fl_autocorr_reduce(sh, 1, t, acc))
            FL_ALL(fl_autocorr<BITS, LEVEL, 2>(sh, bs, t, acc); fl_autocorr_reduce(sh, 2, t, acc))
            FL_ALL(fl_autocorr<BITS, LEVEL, 3>(sh, bs, t, acc); fl_autocorr_reduce(sh, 3, t, acc))
            for (int t = 0; t < 4; ++t)
                fl_levinson(sh, t);
        }
    }
#define FL_CHANNEL(C)                                           \
    FL_ALL(fl_stats_zero(sh, t))                                \
    FL_ALL(fl_stats_passes<BITS, LEVEL, C>(sh, bs, pmax, t))     \
    FL_ALL(fl_stats_nodes<BITS, LEVEL, C>(sh, bs, pmax, t))
    FL_CHANNEL(0)
    FL_CHANNEL(1)
    FL_CHANNEL(2)
    FL_CHANNEL(3)
#undef FL_CHANNEL
    FL_ALL(fl_decide_orders(sh, bs, pmax, t))
    FL_ALL(fl_decide_types(sh, bs, t))
    FL_ALL(fl_frame_header(sh, bs, f, rateNibble, t))
    std::vector<FlacLane> lanes(256);
    for (int s = 0; s < 2; ++s)
    {
        FL_ALL(fl_sub_head(sh, s, bs, t))
        if (sh.type[sh.ch[s]] >= 2)
        {
            FL_ALL(fl_sub_codes(sh, s, bs, t, lanes[t]))
            unsigned pos = sh.start[s] + 8;
            for (int t = 0; t < 256; ++t) // the block prefix sum
            {
                fl_sub_pack(sh, s, bs, t, lanes[t], pos);
                pos += lanes[t].sum;
            }
        }
    }
    const int nBytes = fl_frame_bytes(sh, bs), len = nBytes + 2;
    unsigned crc = 0;
    FL_ALL(crc ^= fl_crc_lane(sh, nBytes, t))
    sh.wave[0] = crc, sh.wave[1] = sh.wave[2] = sh.wave[3] = 0;
    FL_ALL(fl_crc_put(sh, nBytes, t))
    FL_ALL(fl_store(sh, wk, lay, f, len, t))
}

// one output: pcm (16-byte aligned, as pcm.hip writes it) -> out (flac_bound bytes), *size; work: flac_workspace_bytes
int flac_host_encode(const unsigned char *pcm, int bits, i64 n, int rate, int level, unsigned char *out, long long *size,
                     unsigned char *work)
{
    if (flac_bound(bits, n) < 0 || level < 0 || level > 2)
        return -1;
    const FlacLayout lay = flac_layout(bits, n);
    const int nib = rate == 44100 ? 9 : rate == 48000 ? 10 : 0;
    for (i64 f = 0; f < lay.nFrames; ++f)
    {
        if (bits == 16)
            level == 0   ? flac_host_frame<16, 0>(pcm, n, work, lay, nib, f)
            : level == 1 ? flac_host_frame<16, 1>(pcm, n, work, lay, nib, f)
                         : flac_host_frame<16, 2>(pcm, n, work, lay, nib, f);
        else
            level == 0   ? flac_host_frame<24, 0>(pcm, n, work, lay, nib, f)
            : level == 1 ? flac_host_frame<24, 1>(pcm, n, work, lay, nib, f)
                         : flac_host_frame<24, 2>(pcm, n, work, lay, nib, f);
    }
    std::vector<FlacScanLane> lanes(256, FlacScanLane{0, 0xffffffffu, 0, 0});
    for (i64 base = 0; base < lay.nFrames; base += 256)
    {
        FL_ALL(fl_scan_take(work, lay, base, t, lanes[t]))
        unsigned total = 0;
        FL_ALL(total += lanes[t].v)
        unsigned ex = 0;
        for (int t = 0; t < 256; ++t)
        {
            fl_scan_put(work, lay, base, t, lanes[t], ex, total);
            ex += lanes[t].v;
        }
    }
    unsigned mn = 0xffffffffu, mx = 0;
    FL_ALL(mn = lanes[t].mn < mn ? lanes[t].mn : mn; mx = lanes[t].mx > mx ? lanes[t].mx : mx)
    fl_scan_header(out, size, mn, mx, lanes[0].carry, n, bits, rate);
    for (i64 f = 0; f < lay.nFrames; ++f)
        FL_ALL(fl_compact(work, lay, flac_slot_bytes(bits), out, f, t))
#undef FL_ALL
    return 0;
}
#endif

} // namespace dmx
