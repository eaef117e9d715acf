// limiter.hip — the look-ahead peak limiter behind the output stages' gain (the specification is
// restated in tests/limiter_spec.py). It is exact: the same bits as the specification whatever the cut into tiles, because all
// that depends on time runs in integers in the log domain (one octave is 65536 units) and only maxima carry state.
//   level     p[j] = max over the channels of |g x[c][j]|, NaN ignored; with the true-peak filter also of |g y_p[j]| for the
//             F - 1 interpolated phases of meters.hip at frame j (tp_lane_frames: the same taps in the same order)
//   required  M[j] = min(U e + LUT[m >> 11], 24 U) where p[j] > c, from the exponent e and the mantissa m of the correctly
//             rounded quotient p[j] / c; else 0
//   envelope  D[i] = max(0, max_{j <= i} M[j] - qr (i - j), max_{j >= i} M[j] - qa (j - i)): a prefix maximum of M[j] + qr j and
//             a suffix maximum of M[j] - qa j in int64
//   gain      G(D) = THI[D >> 12] * TLO[D & 4095], one fp32 product; y = (g x) G(D), two products in that order
// Three launches over tiles of 2048 frames, a workgroup of 256 whose lanes take 8 consecutive frames; no workgroup waits on
// another and nothing ordered goes through an atomic:
//   lim_detect_kernel<F>  gathers the envelope's outputs (GatherRemix: 16-byte loads, a plane with gain 0 is not read; for F > 1
//      through the staged tile and the lane window of the true-peak launch), writes M and the tile's two aggregates,
//      max(M[j] + qr j) and max(M[j] - qa j)
//   lim_carry_kernel      one wave per envelope: lane l sweeps the aggregates of the tiles [l u, (l + 1) u), u = ceil(tiles / 64),
//      the wave scans the 64 units forward and backward by shuffles, and the lanes sweep again to leave with every tile what
//      the tiles in front of it and behind it carry in
//   lim_envelope_kernel   a lane scans its 8 frames, the wave scans its lanes by shuffles, the 4 waves meet in LDS; D, the gain
//      plane, and in the same pass the limited sample peak of every output (a second gather), the largest D and the frames with
//      D > 0: maxima and integer sums, published by atomics as the peak kernel publishes its maximum
//   lim_tp_kernel<F>      under the true-peak filter: the true-peak launch's body over the limited signal, (g x) G(D)
// The tables are read from global memory where a frame needs them: LUT only over the ceiling, THI and TLO only where D > 0.
//
// With DMX_LIMITER_HOST defined the same bodies compile as plain C++ (tests/limiter_host_main.cpp): the phases are functions of
// (tile, thread), and the host driver at the end of this file runs each phase for all threads in turn. The scans over lanes
// are maxima, so the driver takes them in a plain loop.
#ifdef DMX_LIMITER_HOST
#include "limiter_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
namespace dmx
{
typedef int64_t i64;
}
#ifndef MT_DEV
#define MT_DEV static inline
#define MT_HD static inline
#endif
#define LIM_DIV(p, c) ((p) / (c))
#define LIM_MEMBER inline
#else
#include "kernels.h"
#include "pcm_gather.h"

#include "../../include/demucs_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#define MT_DEV __device__ __forceinline__
#define MT_HD __host__ __device__ __forceinline__
#define LIM_DIV(p, c) __fdiv_rn(p, c)
#define LIM_MEMBER __device__ __forceinline__
#endif
#include "tp_phases.h"

namespace dmx
{
// ------------------------------------------------------------------------------------------------ host: the plan
void lim_tables(int32_t *lut, float *thi, float *tlo)
{
    const auto towardZero = [](double d) {
        float f = (float)d;
        return (double)f > d ? std::nextafterf(f, 0.0f) : f;
    };
    for (int k = 0; k < kLimLut; ++k)
        lut[k] = (int32_t)std::ceil(kLimUnit * std::log2(1.0 + (k + 1) / 4096.0)) + 2;
    for (int a = 0; a < kLimHi; ++a)
        thi[a] = towardZero(std::pow(2.0, -a / 16.0));
    for (int b = 0; b < kLimLo; ++b)
        tlo[b] = towardZero(std::pow(2.0, -b / 65536.0));
}

int lim_slopes(int rate, double attackMs, double releaseMs, int *qa, int *qr)
{
    if (rate < 1)
        return -1;
    const double ms[2] = {attackMs, releaseMs};
    int q[2];
    for (int k = 0; k < 2; ++k)
    {
        if (!std::isfinite(ms[k]) || ms[k] < kLimMinMs || ms[k] > kLimMaxMs)
            return -1;
        const double v = std::rint(kLimUnit * std::log2(std::pow(10.0, 0.5)) * 1000.0 / (ms[k] * rate));
        q[k] = (int)std::min(std::max(v, 1.0), (double)kLimMaxSlope);
    }
    *qa = q[0], *qr = q[1];
    return 0;
}

int64_t lim_workspace_bytes(int64_t n) { return n < 1 ? -1 : lim_ws_bytes(n); }

namespace
{
// ------------------------------------------------------------------------------------------------ the phases
constexpr i64 kLimNone = -((i64)1 << 62); // below every M[j] + qr j and M[j] - qa j: |q j| < 2^56
struct LimTables
{
    const int32_t *lut;
    const float *thi, *tlo;
};
MT_DEV LimTables lim_tables_at(const int32_t *words)
{
    return LimTables{words, reinterpret_cast<const float *>(words + kLimLut), reinterpret_cast<const float *>(words + kLimLut + kLimHiPad)};
}
MT_DEV i64 lim_max(i64 a, i64 b) { return a > b ? a : b; }
// a tile's 64 bytes of the workspace: its two aggregates, and what the tiles in front of it and behind it carry in
struct LimTile
{
    i64 fwd, bwd, carryF, carryB, pad[4];
};

// the level of the thread's 8 frames from f0 on, straight from the gather: p[r] = max(p[r], |g x|) over both channels
template <class Piece, class Gather>
MT_DEV void lim_level(const Piece &pc, const Gather &gather, int o, i64 n, i64 f0, float g, float p[kLimRun])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int h = 0; h < kLimRun / 4; ++h)
    {
        const i64 i = f0 + 4 * h;
        const int cnt = n - i >= 4 ? 4 : (n > i ? (int)(n - i) : 0);
        if (cnt <= 0)
            continue;
        float L[4], R[4];
        gather(pc, o, i, cnt, L, R);
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const float a = fabsf(g * L[k]), b = fabsf(g * R[k]);
            float m = p[4 * h + k];
            m = a > m ? a : m;
            m = b > m ? b : m;
            p[4 * h + k] = m;
        }
    }
}
// the required reduction of a level
MT_DEV int32_t lim_required_of(float p, float c, const int32_t *lut)
{
    if (!(p > c))
        return 0;
    const float r = LIM_DIV(p, c);
    uint32_t u;
    memcpy(&u, &r, sizeof u);
    const i64 M = (i64)kLimUnit * ((int)(u >> 23) - 127) + lut[(u & 0x7fffffu) >> 11];
    return (int32_t)(M < kLimCap ? M : kLimCap);
}
// M of the thread's 8 frames (0 from frame n on) and its share of the tile's aggregates
MT_DEV void lim_required(const float p[kLimRun], float c, const int32_t *lut, i64 f0, i64 n, int qa, int qr, int32_t M[kLimRun], i64 &fwd,
                         i64 &bwd)
{
    fwd = bwd = kLimNone;
#pragma unroll
    for (int r = 0; r < kLimRun; ++r)
    {
        const i64 j = f0 + r;
        M[r] = j < n ? lim_required_of(p[r], c, lut) : 0;
        if (j < n)
        {
            fwd = lim_max(fwd, M[r] + (i64)qr * j);
            bwd = lim_max(bwd, M[r] - (i64)qa * j);
        }
    }
}
// 8 words of a plane of the workspace from frame f0 (a multiple of 8) on; the plane is 16-byte aligned and holds n rounded
// up to 4 words
struct alignas(16) LimVec4
{
    uint32_t w[4];
};
template <class T>
MT_DEV void lim_store8(T *plane, i64 f0, i64 n, const T v[kLimRun])
{
    static_assert(sizeof(T) == 4, "4-byte words");
#pragma unroll
    for (int h = 0; h < kLimRun / 4; ++h)
    {
        const i64 i = f0 + 4 * h;
        if (i + 4 <= n)
        {
            LimVec4 q;
            memcpy(q.w, v + 4 * h, 16);
            *reinterpret_cast<LimVec4 *>(plane + i) = q;
        }
        else
            for (int k = 0; k < 4; ++k)
                if (i + k < n)
                    plane[i + k] = v[4 * h + k];
    }
}
template <class T>
MT_DEV void lim_load8(const T *plane, i64 f0, i64 n, T v[kLimRun])
{
    static_assert(sizeof(T) == 4, "4-byte words");
#pragma unroll
    for (int h = 0; h < kLimRun / 4; ++h)
    {
        const i64 i = f0 + 4 * h;
        if (i + 4 <= n)
        {
            const LimVec4 q = *reinterpret_cast<const LimVec4 *>(plane + i);
            memcpy(v + 4 * h, q.w, 16);
        }
        else
            for (int k = 0; k < 4; ++k)
                v[4 * h + k] = i + k < n ? plane[i + k] : T(0);
    }
}
// lane `lane` of the carry launch over its unit of u tiles: the unit's two aggregates (write false), or, from what the units
// in front of it (inF) and behind it (inB) carry, every tile's carryF and carryB (write true)
MT_DEV void lim_unit_sweep(LimTile *tiles, i64 nTiles, i64 u, int lane, bool write, i64 &inF, i64 &inB)
{
    const i64 a = lane * u, b = a + u < nTiles ? a + u : nTiles;
    i64 f = write ? inF : kLimNone, w = write ? inB : kLimNone;
    for (i64 t = a; t < b; ++t)
    {
        if (write)
            tiles[t].carryF = f;
        f = lim_max(f, tiles[t].fwd);
    }
    for (i64 t = b - 1; t >= a; --t)
    {
        if (write)
            tiles[t].carryB = w;
        w = lim_max(w, tiles[t].bwd);
    }
    if (!write)
        inF = f, inB = w;
}
// the thread's 8 frames: a[r] the maximum of M[j] + qr j over its frames up to r, b[r] that of M[j] - qa j from r on
MT_DEV void lim_local(const int32_t M[kLimRun], i64 f0, i64 n, int qa, int qr, i64 a[kLimRun], i64 b[kLimRun])
{
#pragma unroll
    for (int r = 0; r < kLimRun; ++r)
    {
        const i64 j = f0 + r, v = j < n ? M[r] + (i64)qr * j : kLimNone;
        a[r] = r ? lim_max(a[r - 1], v) : v;
    }
#pragma unroll
    for (int r = kLimRun - 1; r >= 0; --r)
    {
        const i64 j = f0 + r, v = j < n ? M[r] - (i64)qa * j : kLimNone;
        b[r] = r < kLimRun - 1 ? lim_max(b[r + 1], v) : v;
    }
}
// D and the gain of the thread's 8 frames from what the lanes and tiles in front (inF) and behind (inB) carry
MT_DEV void lim_gain(const i64 a[kLimRun], const i64 b[kLimRun], i64 inF, i64 inB, i64 f0, i64 n, int qa, int qr, const LimTables &T,
                     int32_t D[kLimRun], float G[kLimRun])
{
#pragma unroll
    for (int r = 0; r < kLimRun; ++r)
    {
        const i64 j = f0 + r;
        const i64 d = lim_max(lim_max(a[r], inF) - (i64)qr * j, lim_max(b[r], inB) + (i64)qa * j);
        D[r] = j < n && d > 0 ? (int32_t)d : 0;
        G[r] = D[r] > 0 ? T.thi[D[r] >> 12] * T.tlo[D[r] & 4095] : 1.0f; // THI[0] TLO[0] = 1
    }
}
// the largest |(g x) G| of output o over the thread's 8 frames, NaN ignored
template <class Piece, class Gather>
MT_DEV float lim_peak(const Piece &pc, const Gather &gather, int o, i64 n, i64 f0, float g, const float G[kLimRun])
{
#pragma clang fp contract(off)
    float m = 0.0f;
#pragma unroll
    for (int h = 0; h < kLimRun / 4; ++h)
    {
        const i64 i = f0 + 4 * h;
        const int cnt = n - i >= 4 ? 4 : (n > i ? (int)(n - i) : 0);
        if (cnt <= 0)
            continue;
        float L[4], R[4];
        gather(pc, o, i, cnt, L, R);
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            if (k >= cnt)
                continue;
            const float gl = g * L[k], gr = g * R[k];
            const float a = fabsf(gl * G[4 * h + k]), b = fabsf(gr * G[4 * h + k]);
            m = a > m ? a : m;
            m = b > m ? b : m;
        }
    }
    return m;
}
// the limited signal as the true-peak stage gathers it: (g x) G(D), two products
template <class Gather>
struct LimGatherLimited
{
    const Gather &inner;
    float g;
    const float *plane;
    template <class Piece>
    LIM_MEMBER void operator()(const Piece &pc, int o, i64 i, int cnt, float L[4], float R[4]) const
    {
#pragma clang fp contract(off)
        inner(pc, o, i, cnt, L, R);
        for (int k = 0; k < 4; ++k)
        {
            const float G = k < cnt ? plane[i + k] : 0.0f;
            const float gl = g * L[k], gr = g * R[k];
            L[k] = k < cnt ? gl * G : 0.0f;
            R[k] = k < cnt ? gr * G : 0.0f;
        }
    }
};
} // namespace

#ifndef DMX_LIMITER_HOST
// ------------------------------------------------------------------------------------------------ device: the kernels
namespace
{
__device__ __forceinline__ i64 lim_shfl(i64 v, int from)
{
    const int lo = __shfl((int)(unsigned)(v & 0xffffffff), from, 64), hi = __shfl((int)(v >> 32), from, 64);
    return (i64)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// the maximum over the workgroup's 256 threads; every thread returns it (red: 4 words of LDS, free on entry)
__device__ __forceinline__ i64 lim_block_max(i64 v, i64 *red, int tid)
{
    const int lane = tid & 63;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v = lim_max(v, lim_shfl(v, lane ^ off));
    if (lane == 0)
        red[tid >> 6] = v;
    __syncthreads();
    v = lim_max(lim_max(red[0], red[1]), lim_max(red[2], red[3]));
    __syncthreads();
    return v;
}
__device__ __forceinline__ float lim_gain_at(const LimJob &J, int o) { return J.gains ? J.gains[o] : J.gainImm; }
__device__ __forceinline__ unsigned char *lim_env(const LimJob &J, int e) { return J.work + (i64)e * lim_ws_bytes(J.pc.n); }
} // namespace

// grid (tiles, envelopes), block 256. F: 1 the samples alone, 2 or 4 the interpolated phases too
template <int F>
__global__ __launch_bounds__(256) void lim_detect_kernel(LimJob J, TpFilter f)
{
    __shared__ TpLds sh;
    __shared__ i64 red[4];
    const int tid = threadIdx.x, e = blockIdx.y;
    const i64 n = J.pc.n, t0 = (i64)blockIdx.x * kLimTile, f0 = t0 + (i64)tid * kLimRun;
    const int o0 = J.link ? 0 : e, o1 = J.link ? J.G.nOut : e + 1;
    float p[kLimRun];
#pragma unroll
    for (int r = 0; r < kLimRun; ++r)
        p[r] = 0.0f;
    for (int o = o0; o < o1; ++o)
    {
        const float g = lim_gain_at(J, o);
        if (F > 1)
        {
            if (o > o0)
                __syncthreads(); // the lanes have read the output before
            tp_stage(J.pc, GatherRemix{J.G}, o, n, t0, tid, sh);
            __syncthreads();
            float m[kLimRun];
            tp_lane_frames<F>(sh, f, tid, g, m);
#pragma unroll
            for (int r = 0; r < kLimRun; ++r)
                p[r] = m[r] > p[r] ? m[r] : p[r];
        }
        else
            lim_level(J.pc, GatherRemix{J.G}, o, n, f0, g, p);
    }
    unsigned char *env = lim_env(J, e);
    int32_t M[kLimRun];
    i64 fwd, bwd;
    lim_required(p, J.ceiling, J.tables, f0, n, J.qa, J.qr, M, fwd, bwd);
    lim_store8(reinterpret_cast<int32_t *>(env), f0, n, M);
    fwd = lim_block_max(fwd, red, tid);
    bwd = lim_block_max(bwd, red, tid);
    if (tid == 0)
    {
        LimTile *tile = reinterpret_cast<LimTile *>(env + lim_ws_tiles_offset(n)) + blockIdx.x;
        tile->fwd = fwd, tile->bwd = bwd;
    }
}

// grid (envelopes), block 64
__global__ __launch_bounds__(64) void lim_carry_kernel(LimJob J)
{
    const int lane = threadIdx.x;
    const i64 n = J.pc.n, nTiles = (n + kLimTile - 1) / kLimTile, u = (nTiles + 63) / 64;
    LimTile *tiles = reinterpret_cast<LimTile *>(lim_env(J, blockIdx.x) + lim_ws_tiles_offset(n));
    i64 uf, ub;
    lim_unit_sweep(tiles, nTiles, u, lane, false, uf, ub);
    // inclusive scans over the lanes: forward for uf, backward for ub
    i64 sf = uf, sb = ub;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const i64 vf = lim_shfl(sf, lane - d < 0 ? lane : lane - d), vb = lim_shfl(sb, lane + d > 63 ? lane : lane + d);
        sf = lim_max(sf, vf), sb = lim_max(sb, vb);
    }
    i64 inF = lim_shfl(sf, lane > 0 ? lane - 1 : lane), inB = lim_shfl(sb, lane < 63 ? lane + 1 : lane);
    if (lane == 0)
        inF = kLimNone;
    if (lane == 63)
        inB = kLimNone;
    lim_unit_sweep(tiles, nTiles, u, lane, true, inF, inB);
}

// grid (tiles, envelopes), block 256
__global__ __launch_bounds__(256) void lim_envelope_kernel(LimJob J)
{
    __shared__ i64 red[4];
    __shared__ i64 wF[4], wB[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = blockIdx.y;
    const i64 n = J.pc.n, t0 = (i64)blockIdx.x * kLimTile, f0 = t0 + (i64)tid * kLimRun;
    unsigned char *env = lim_env(J, e);
    const LimTile *tile = reinterpret_cast<const LimTile *>(env + lim_ws_tiles_offset(n)) + blockIdx.x;
    int32_t M[kLimRun];
    lim_load8(reinterpret_cast<const int32_t *>(env), f0, n, M);
    i64 a[kLimRun], b[kLimRun];
    lim_local(M, f0, n, J.qa, J.qr, a, b);
    // inclusive scans of the lanes' totals over the wave, then exclusive with the waves and the tile's carry in front
    i64 sf = a[kLimRun - 1], sb = b[0];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const i64 vf = lim_shfl(sf, lane - d < 0 ? lane : lane - d), vb = lim_shfl(sb, lane + d > 63 ? lane : lane + d);
        sf = lim_max(sf, vf), sb = lim_max(sb, vb);
    }
    if (lane == 63)
        wF[wave] = sf;
    if (lane == 0)
        wB[wave] = sb;
    i64 inF = lim_shfl(sf, lane > 0 ? lane - 1 : lane), inB = lim_shfl(sb, lane < 63 ? lane + 1 : lane);
    if (lane == 0)
        inF = kLimNone;
    if (lane == 63)
        inB = kLimNone;
    __syncthreads();
    inF = lim_max(inF, tile->carryF), inB = lim_max(inB, tile->carryB);
    for (int w = 0; w < 4; ++w)
    {
        if (w < wave)
            inF = lim_max(inF, wF[w]);
        if (w > wave)
            inB = lim_max(inB, wB[w]);
    }
    int32_t D[kLimRun];
    float G[kLimRun];
    lim_gain(a, b, inF, inB, f0, n, J.qa, J.qr, lim_tables_at(J.tables), D, G);
    lim_store8(reinterpret_cast<float *>(env + lim_ws_gain_offset(n)), f0, n, G);
    int dMax = 0, cnt = 0;
#pragma unroll
    for (int r = 0; r < kLimRun; ++r)
        dMax = D[r] > dMax ? D[r] : dMax, cnt += D[r] > 0;
    // the workgroup's largest D (upper word) and its frames with D > 0 (lower word: at most 2048)
    const i64 both = lim_block_max((i64)dMax << 32, red, tid);
    i64 total = cnt;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        total += lim_shfl(total, lane ^ off);
    if (lane == 0)
        red[wave] = total;
    __syncthreads();
    total = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    dmx_limit_result *res = (dmx_limit_result *)J.res;
    const int o0 = J.link ? 0 : e, o1 = J.link ? J.G.nOut : e + 1;
    for (int o = o0; o < o1; ++o)
    {
        const float m = lim_peak(J.pc, GatherRemix{J.G}, o, n, f0, lim_gain_at(J, o), G);
        const i64 pk = lim_block_max((i64)__float_as_uint(m), red, tid);
        if (tid == 0)
        {
            if (pk)
                atomicMax(reinterpret_cast<unsigned *>(&res[o].peak_out), (unsigned)pk);
            if (total)
            {
                atomicMax(&res[o].max_reduction, (int)(both >> 32));
                atomicAdd(reinterpret_cast<unsigned long long *>(&res[o].limited_frames), (unsigned long long)total);
            }
        }
    }
}

// grid (tiles, outputs), block 256: the true peak of the limited output
template <int F>
__global__ __launch_bounds__(256) void lim_tp_kernel(LimJob J, TpFilter f)
{
    __shared__ TpLds sh;
    __shared__ i64 red[4];
    const int tid = threadIdx.x, o = blockIdx.y;
    const i64 n = J.pc.n, t0 = (i64)blockIdx.x * kLimTile;
    const float *plane = reinterpret_cast<const float *>(lim_env(J, J.link ? 0 : o) + lim_ws_gain_offset(n));
    const GatherRemix inner{J.G};
    tp_stage(J.pc, LimGatherLimited<GatherRemix>{inner, lim_gain_at(J, o), plane}, o, n, t0, tid, sh);
    __syncthreads();
    const float m = tp_lane<F>(sh, f, tid, t0, 0, n);
    const i64 pk = lim_block_max((i64)__float_as_uint(m), red, tid);
    if (tid == 0 && pk)
        atomicMax(reinterpret_cast<unsigned *>(&((dmx_limit_result *)J.res)[o].true_peak_out), (unsigned)pk);
}

void launch_limit(const LimJob &job, const TpFilter &f, bool truePeak, hipStream_t s, hipEvent_t *marks)
{
    const i64 n = job.pc.n;
    const unsigned tiles = (unsigned)lim_tiles(n), envs = job.link ? 1u : (unsigned)job.G.nOut;
    const int F = truePeak ? f.F : 1;
    (void)hipMemsetAsync(job.res, 0, sizeof(dmx_limit_result) * (size_t)job.G.nOut, s);
    if (marks)
        (void)hipEventRecord(marks[0], s);
    if (F == 4)
        hipLaunchKernelGGL(lim_detect_kernel<4>, dim3(tiles, envs), dim3(256), 0, s, job, f);
    else if (F == 2)
        hipLaunchKernelGGL(lim_detect_kernel<2>, dim3(tiles, envs), dim3(256), 0, s, job, f);
    else
        hipLaunchKernelGGL(lim_detect_kernel<1>, dim3(tiles, envs), dim3(256), 0, s, job, f);
    if (marks)
        (void)hipEventRecord(marks[1], s);
    hipLaunchKernelGGL(lim_carry_kernel, dim3(envs), dim3(64), 0, s, job);
    if (marks)
        (void)hipEventRecord(marks[2], s);
    hipLaunchKernelGGL(lim_envelope_kernel, dim3(tiles, envs), dim3(256), 0, s, job);
    if (marks)
        (void)hipEventRecord(marks[3], s);
    if (truePeak)
    {
        const dim3 grid(tiles, (unsigned)job.G.nOut);
        if (F == 4)
            hipLaunchKernelGGL(lim_tp_kernel<4>, grid, dim3(256), 0, s, job, f);
        else if (F == 2)
            hipLaunchKernelGGL(lim_tp_kernel<2>, grid, dim3(256), 0, s, job, f);
        else
            hipLaunchKernelGGL(lim_tp_kernel<1>, grid, dim3(256), 0, s, job, f);
    }
    if (marks)
        (void)hipEventRecord(marks[4], s);
}
#else
// ------------------------------------------------------------------------------------------------ host: the driver
struct LimHostPiece
{
    const float *x; // planar [2][n] or interleaved [n][2]
    i64 n;
    bool interleaved;
};
struct LimHostGather
{
    void operator()(const LimHostPiece &pc, int, i64 i, int cnt, float L[4], float R[4]) const
    {
        for (int k = 0; k < 4; ++k)
        {
            L[k] = k < cnt ? (pc.interleaved ? pc.x[2 * (i + k)] : pc.x[i + k]) : 0.0f;
            R[k] = k < cnt ? (pc.interleaved ? pc.x[2 * (i + k) + 1] : pc.x[pc.n + i + k]) : 0.0f;
        }
    }
};
struct LimHostResult
{
    float peakOut, truePeakOut;
    int32_t maxReduction;
    i64 limitedFrames;
};
// the launches on one signal: work receives M and the gain plane as the device's workspace does
static void lim_host_run(const float *x, bool interleaved, i64 n, int rate, float g, float c, bool truePeak, int qa, int qr,
                         std::vector<unsigned char> &work, LimHostResult *res)
{
    std::vector<int32_t> words(kLimTableWords);
    lim_tables(words.data(), reinterpret_cast<float *>(words.data() + kLimLut), reinterpret_cast<float *>(words.data() + kLimLut + kLimHiPad));
    const LimTables T = lim_tables_at(words.data());
    TpFilter f;
    tp_filter(rate, &f);
    const int F = truePeak ? f.F : 1;
    work.assign((size_t)lim_workspace_bytes(n), 0xcd);
    int32_t *Mp = reinterpret_cast<int32_t *>(work.data());
    float *Gp = reinterpret_cast<float *>(work.data() + lim_ws_gain_offset(n));
    LimTile *tiles = reinterpret_cast<LimTile *>(work.data() + lim_ws_tiles_offset(n));
    const i64 nTiles = lim_tiles(n), u = (nTiles + 63) / 64;
    const LimHostPiece pc{x, n, interleaved};
    std::vector<TpLds> lds(1);
    TpLds &sh = lds[0];
    *res = LimHostResult{0.0f, 0.0f, 0, 0};
    // detect
    for (i64 t = 0; t < nTiles; ++t)
    {
        const i64 t0 = t * kLimTile;
        if (F > 1)
            for (int tid = 0; tid < 256; ++tid)
                tp_stage(pc, LimHostGather{}, 0, n, t0, tid, sh);
        i64 fwd = kLimNone, bwd = kLimNone;
        for (int tid = 0; tid < 256; ++tid)
        {
            const i64 f0 = t0 + (i64)tid * kLimRun;
            float p[kLimRun] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (F == 4)
                tp_lane_frames<4>(sh, f, tid, g, p);
            else if (F == 2)
                tp_lane_frames<2>(sh, f, tid, g, p);
            else
                lim_level(pc, LimHostGather{}, 0, n, f0, g, p);
            int32_t M[kLimRun];
            i64 a, b;
            lim_required(p, c, T.lut, f0, n, qa, qr, M, a, b);
            lim_store8(Mp, f0, n, M);
            fwd = lim_max(fwd, a), bwd = lim_max(bwd, b);
        }
        tiles[t].fwd = fwd, tiles[t].bwd = bwd;
    }
    // carry: the units' aggregates, the scans over the 64 lanes as plain loops (maxima), the second sweep
    {
        i64 uf[64], ub[64], inF[64], inB[64];
        for (int lane = 0; lane < 64; ++lane)
            lim_unit_sweep(tiles, nTiles, u, lane, false, uf[lane], ub[lane]);
        i64 run = kLimNone;
        for (int lane = 0; lane < 64; ++lane)
            inF[lane] = run, run = lim_max(run, uf[lane]);
        run = kLimNone;
        for (int lane = 63; lane >= 0; --lane)
            inB[lane] = run, run = lim_max(run, ub[lane]);
        for (int lane = 63; lane >= 0; --lane) // a lane's sweep writes its own tiles only: any order
            lim_unit_sweep(tiles, nTiles, u, lane, true, inF[lane], inB[lane]);
    }
    // envelope
    for (i64 t = nTiles - 1; t >= 0; --t) // tiles are independent: any order
    {
        const i64 t0 = t * kLimTile;
        std::vector<i64> a(256 * kLimRun), b(256 * kLimRun), inF(256), inB(256);
        for (int tid = 0; tid < 256; ++tid)
        {
            int32_t M[kLimRun];
            lim_load8(Mp, t0 + (i64)tid * kLimRun, n, M);
            lim_local(M, t0 + (i64)tid * kLimRun, n, qa, qr, &a[tid * kLimRun], &b[tid * kLimRun]);
        }
        i64 run = tiles[t].carryF;
        for (int tid = 0; tid < 256; ++tid)
            inF[tid] = run, run = lim_max(run, a[tid * kLimRun + kLimRun - 1]);
        run = tiles[t].carryB;
        for (int tid = 255; tid >= 0; --tid)
            inB[tid] = run, run = lim_max(run, b[tid * kLimRun]);
        for (int tid = 0; tid < 256; ++tid)
        {
            const i64 f0 = t0 + (i64)tid * kLimRun;
            int32_t D[kLimRun];
            float G[kLimRun];
            lim_gain(&a[tid * kLimRun], &b[tid * kLimRun], inF[tid], inB[tid], f0, n, qa, qr, T, D, G);
            lim_store8(Gp, f0, n, G);
            for (int r = 0; r < kLimRun; ++r)
            {
                res->maxReduction = std::max(res->maxReduction, D[r]);
                res->limitedFrames += D[r] > 0;
            }
            const float m = lim_peak(pc, LimHostGather{}, 0, n, f0, g, G);
            res->peakOut = m > res->peakOut ? m : res->peakOut;
        }
    }
    if (!truePeak)
        return;
    const LimHostGather inner{};
    for (i64 t = 0; t < nTiles; ++t)
    {
        const i64 t0 = t * kLimTile;
        for (int tid = 0; tid < 256; ++tid)
            tp_stage(pc, LimGatherLimited<LimHostGather>{inner, g, Gp}, 0, n, t0, tid, sh);
        for (int tid = 0; tid < 256; ++tid)
        {
            const float m = F == 4 ? tp_lane<4>(sh, f, tid, t0, 0, n) : F == 2 ? tp_lane<2>(sh, f, tid, t0, 0, n) : tp_lane<1>(sh, f, tid, t0, 0, n);
            res->truePeakOut = m > res->truePeakOut ? m : res->truePeakOut;
        }
    }
}
#endif

} // namespace dmx
