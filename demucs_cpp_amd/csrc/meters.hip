// meters.hip — the meters of EBU R 128 that the loudness stage (loudness.hip) left out: true peak, loudness range, and the
// maxima of momentary and short-term loudness (the specification is restated in tests/meters_spec.py).
//
// True peak is the largest |y| of the signal oversampled F times (4 below 96 kHz, 2 below 192 kHz, else 1): a Hann-windowed
// sinc of 12 taps per phase, made on the host in binary64 and rounded once to fp32 (tp_filter), passed in the kernel
// arguments. Phase 0 is the sample itself; phase p at frame i is the sum over j = 0 .. 11 of h[p + F j] * x[i + 6 - j] in
// fp32, every product rounded and then added with a rounding of its own, j ascending (the rule of remix_acc, pcm_gather.h:
// contraction is off in tp_lane). A maximum does not depend on the order it is taken in, so TP is the same bits whatever the
// cut into tiles and pieces.
//   true_peak_kernel<F>  a workgroup of 256 takes the tile of 2048 frames at a multiple of 2048 of one signal (an output row
//      of a gain table through GatherRemix: 16-byte loads, a plane with gain 0 is not read) and stages both channels in LDS
//      with 8 frames of halo on either side (6 are used; 8 keeps every group of 4 frames aligned) - the neighbouring tiles'
//      gathered values, zeros before frame 0 and from frame n on. A lane then walks 8 consecutive frames of a channel from a
//      window of 19 staged values in registers: 8 + 11 LDS reads for 8 frames of F - 1 phases. Staged frame s lies at word
//      s + s / 8: lane l's k-th read is word 9 l + const(k), and 9 is odd - the 32 lanes of a half wave meet 32 banks.
//      |y| is reduced over the wave by shuffles, over the 4 waves in LDS, and published by an atomicMax on the bit pattern
//      of a non-negative float, as launch_pcm_peak does. NaN is ignored (a > m is false).
//      A piece [i0, i1) of a track evaluates the frames [max(0, i0 - 6), i1 - 6), up to n behind the track's last piece: the
//      frames whose 12 inputs the pieces so far hold. Piece by piece a track gives the whole track's TP.
//   meters_kernel        one workgroup of 256 per signal, behind loud_final_kernel: thread b forms the momentary block l[b]
//      (loudness.hip's block) and the short-term block S[b] (30 hops, summed in increasing order, channel 0 then channel 1 of
//      a hop) from the hop energies in the workspace, quantises them to hundredths of a LU, takes the two maxima with integer
//      LDS atomics and counts min(s_c, 2000) > -7000 in a histogram of 9001 LDS bins with integer atomics: order-free. The
//      threads list the occupied bins in ascending order (a count per range of 36 bins, offsets, a write), and one lane then
//      walks that list: the mean of the absolutely gated blocks, the relative gate 20 LU under it,
//      the nearest-rank 10th and 95th percentiles of what is left (EBU Tech 3342). No workgroup waits on another.
// The ceiling by true peak (DMX_LOUD_TRUE_PEAK) is loudness.hip's launch_loud_gain_tp: the gain rule reads TP where it read P.
//
// With DMX_METERS_HOST defined the same bodies compile as plain C++ (tests/meters_host_main.cpp): the stage and lane phases
// are functions of (tile, thread), the LDS atomics become plain integer operations, and the host driver at the end of this
// file runs each phase for all threads in turn.
#ifdef DMX_METERS_HOST
#include "meters_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
namespace dmx
{
typedef int64_t i64;
}
#define MT_DEV static inline
#define MT_HD static inline
#define MT_ATOMIC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define MT_ATOMIC_ADD(p, v) (*(p) += (v))
#else
#include "kernels.h"
#include "pcm_gather.h"

#include "../../include/demucs_hip.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
#define MT_DEV __device__ __forceinline__
#define MT_HD __host__ __device__ __forceinline__
#define MT_ATOMIC_MAX(p, v) atomicMax(p, v)
#define MT_ATOMIC_ADD(p, v) atomicAdd(p, v)
#endif

namespace dmx
{
// ------------------------------------------------------------------------------------------------ host: the plan
int tp_factor(int rate) { return rate < 96000 ? 4 : (rate < 192000 ? 2 : 1); }

void tp_filter(int rate, TpFilter *f)
{
    const double pi = 3.14159265358979323846;
    const int F = tp_factor(rate);
    f->F = F;
    for (float &v : f->h)
        v = 0.0f;
    for (int k = 0; k <= kTpTaps * F; ++k)
    {
        const double t = (double)(k - kTpHalo * F) / (double)F;
        const double sinc = k == kTpHalo * F ? 1.0 : std::sin(pi * t) / (pi * t);
        const double w = 0.5 * (1.0 - std::cos(2.0 * pi * k / (12.0 * F)));
        f->h[k] = (float)(sinc * w);
    }
}

int64_t meters_workspace_bytes(int64_t n) { return n < 1 ? -1 : meters_ws_bytes(n); }

} // namespace dmx
#include "tp_phases.h"
namespace dmx
{
namespace
{

// ------------------------------------------------------------------------------------------------ the hop meters: the phases
struct MetersLds
{
    int hist[kMetersBins];
    unsigned short occ[kMetersBins]; // the occupied bins in ascending order, nOcc of them (meters_compact)
    int part[256];                   // occupied bins in a thread's range
    int nOcc;
    int maxM, maxS, badM, badS; // the maxima in hundredths of a LU (INT_MIN: no block yet); a block that is not finite
};
struct MetersOut
{
    int lraC, maxMC, maxSC;
};
MT_DEV void meters_init(MetersLds &sh, int tid, int nThreads)
{
    for (int k = tid; k < kMetersBins; k += nThreads)
        sh.hist[k] = 0;
    if (tid == 0)
        sh.maxM = INT_MIN, sh.maxS = INT_MIN, sh.badM = 0, sh.badS = 0;
}
// a block of mean square z in hundredths of a LU: false for a block of zero energy (it is -inf and never wins); a block
// that is not finite raises *bad
MT_DEV bool meters_quantum(double z, int *bad, int &c)
{
    if (z == 0.0)
        return false;
    const double v = -0.691 + 10.0 * log10(z);
    if (!(v - v == 0.0))
    {
        MT_ATOMIC_MAX(bad, 1);
        return false;
    }
    c = (int)rint(100.0 * v);
    return true;
}
// the thread's blocks b = tid, tid + nThreads ..
MT_DEV void meters_blocks(const double *e, int hop, int H, int tid, int nThreads, MetersLds &sh)
{
    const double *e0 = e, *e1 = e + H;
    for (int b = tid; b < H - 3; b += nThreads)
    {
        const double s0 = e0[b] + e1[b], s1 = e0[b + 1] + e1[b + 1], s2 = e0[b + 2] + e1[b + 2], s3 = e0[b + 3] + e1[b + 3];
        int c;
        if (meters_quantum((((s0 + s1) + s2) + s3) / (4.0 * hop), &sh.badM, c))
            MT_ATOMIC_MAX(&sh.maxM, c);
    }
    for (int b = tid; b < H - (kMetersShort - 1); b += nThreads)
    {
        double acc = 0.0;
        for (int j = 0; j < kMetersShort; ++j)
        {
            acc += e0[b + j];
            acc += e1[b + j];
        }
        int c;
        if (!meters_quantum(acc / (30.0 * hop), &sh.badS, c))
            continue;
        MT_ATOMIC_MAX(&sh.maxS, c);
        const int sc = c > 2000 ? 2000 : c;
        if (sc > -7000)
            MT_ATOMIC_ADD(&sh.hist[sc + 7000], 1);
    }
}
// the occupied bins as a list in ascending order, so that the one lane of meters_finish walks tens of entries and not three
// times 9000 words of LDS: thread tid of nThreads <= 256 counts those of its range of bins, then (behind a barrier) writes them
// behind the ranges in front of it
constexpr int kMetersRange = (kMetersBins - 1 + 255) / 256; // bins of a thread's range: 36
MT_DEV void meters_compact_count(MetersLds &sh, int tid)
{
    int c = 0;
    for (int k = 1 + tid * kMetersRange; k < 1 + (tid + 1) * kMetersRange && k < kMetersBins; ++k)
        c += sh.hist[k] != 0;
    sh.part[tid] = c;
}
MT_DEV void meters_compact_write(MetersLds &sh, int tid)
{
    int at = 0;
    for (int t = 0; t < tid; ++t)
        at += sh.part[t];
    for (int k = 1 + tid * kMetersRange; k < 1 + (tid + 1) * kMetersRange && k < kMetersBins; ++k)
        if (sh.hist[k] != 0)
            sh.occ[at++] = (unsigned short)k;
    if (tid == 255)
        sh.nOcc = at;
}
// one thread, behind the list
MT_DEV MetersOut meters_finish(const MetersLds &sh, int H)
{
    MetersOut r;
    r.maxMC = sh.badM ? INT_MIN : sh.maxM;
    r.maxSC = sh.badS ? INT_MIN : sh.maxS;
    r.lraC = INT_MIN;
    if (H < kMetersShort || sh.badS)
        return r;
    long long tot = 0;
    double sum = 0.0;
    for (int x = 0; x < sh.nOcc; ++x)
    {
        const int k = sh.occ[x], c = sh.hist[k];
        tot += c;
        sum += (double)c * pow(10.0, (double)(k - 7000) / 1000.0);
    }
    if (tot == 0)
        return r;
    const double mean = sum / (double)tot;
    const long long rc = (long long)floor(100.0 * (10.0 * log10(mean))) - 2000;
    long long m = 0;
    for (int x = 0; x < sh.nOcc; ++x)
        if (sh.occ[x] - 7000 > rc)
            m += sh.hist[sh.occ[x]];
    if (m == 0)
        return r;
    const long long i10 = ((m - 1) * 10 + 50) / 100, i95 = ((m - 1) * 95 + 50) / 100;
    long long cum = 0;
    int v10 = 0, v95 = 0;
    bool have10 = false;
    for (int x = 0; x < sh.nOcc; ++x)
    {
        const int k = sh.occ[x];
        if (!(k - 7000 > rc))
            continue;
        cum += sh.hist[k];
        if (!have10 && cum > i10)
            v10 = k - 7000, have10 = true;
        if (cum > i95)
        {
            v95 = k - 7000;
            break;
        }
    }
    r.lraC = v95 - v10;
    return r;
}
} // namespace

#ifndef DMX_METERS_HOST
// ------------------------------------------------------------------------------------------------ device: the kernels
// grid (tiles, G.nOut, pieces), block 256; pc.peaks[o] receives the true peak
template <int F>
__global__ __launch_bounds__(256) void true_peak_kernel(RemixTable t, PcmGains G, TpFilter f)
{
    __shared__ TpLds sh;
    const RemixPiece &pc = t.p[blockIdx.z];
    const int o = blockIdx.y, tid = threadIdx.x;
    i64 lo, hi;
    tp_range(pc.i0, pc.i1, pc.n, lo, hi);
    const i64 t0 = (lo / kTpTile + blockIdx.x) * kTpTile;
    if (t0 >= hi) // the whole workgroup: a shorter piece of the table
        return;
    tp_stage(pc, GatherRemix{G}, o, pc.n, t0, tid, sh);
    __syncthreads();
    const float m = tp_lane<F>(sh, f, tid, t0, lo, hi);
    unsigned u = __float_as_uint(m);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
    {
        const unsigned v = (unsigned)__shfl_xor((int)u, off, 64);
        u = v > u ? v : u;
    }
    __shared__ unsigned wmax[4];
    if ((tid & 63) == 0)
        wmax[tid >> 6] = u;
    __syncthreads();
    if (tid == 0)
    {
        for (int w = 1; w < 4; ++w)
            u = wmax[w] > u ? wmax[w] : u;
        if (u)
            atomicMax(pc.peaks + o, u);
    }
}

// grid (signals), block 256: signal o reads the hop energies of slot slot0 + o and tp[o], and fills out[o]
__global__ __launch_bounds__(256) void meters_kernel(const unsigned char *work, i64 slotBytes, int slot0, i64 eOffset, int hop, int H,
                                                     const unsigned *tp, dmx_meters_result *out)
{
    __shared__ MetersLds sh;
    const int tid = threadIdx.x, o = blockIdx.x;
    const double *e = reinterpret_cast<const double *>(work + (i64)(slot0 + o) * slotBytes + eOffset);
    meters_init(sh, tid, 256);
    __syncthreads();
    meters_blocks(e, hop, H, tid, 256, sh);
    __syncthreads();
    meters_compact_count(sh, tid);
    __syncthreads();
    meters_compact_write(sh, tid);
    __syncthreads();
    if (tid == 0)
    {
        const MetersOut r = meters_finish(sh, H);
        out[o].true_peak = __uint_as_float(tp[o]);
        out[o].lra_c = r.lraC, out[o].max_momentary_c = r.maxMC, out[o].max_short_c = r.maxSC;
    }
}

void launch_true_peak(const RemixPiece *pieces, int P, const PcmGains &G, const TpFilter &f, hipStream_t s)
{
    for (int p0 = 0; p0 < P; p0 += RemixTable::kMax)
    {
        RemixTable t{};
        int nt = 0;
        i64 tiles = 0;
        for (int k = p0; k < P && k < p0 + RemixTable::kMax; ++k)
        {
            i64 lo, hi;
            tp_range(pieces[k].i0, pieces[k].i1, pieces[k].n, lo, hi);
            if (hi <= lo)
                continue;
            t.p[nt++] = pieces[k];
            tiles = std::max(tiles, (hi - 1) / kTpTile - lo / kTpTile + 1);
        }
        if (!nt)
            continue;
        const dim3 grid((unsigned)tiles, (unsigned)G.nOut, (unsigned)nt);
        if (f.F == 4)
            hipLaunchKernelGGL(true_peak_kernel<4>, grid, dim3(256), 0, s, t, G, f);
        else if (f.F == 2)
            hipLaunchKernelGGL(true_peak_kernel<2>, grid, dim3(256), 0, s, t, G, f);
        else
            hipLaunchKernelGGL(true_peak_kernel<1>, grid, dim3(256), 0, s, t, G, f);
    }
}

void launch_meters(const unsigned char *work, int slot0, int nSignals, const LoudPlan &lp, const unsigned *tp, void *out, hipStream_t s)
{
    hipLaunchKernelGGL(meters_kernel, dim3((unsigned)nSignals), dim3(256), 0, s, work, (i64)loud_workspace_bytes(lp.n), slot0,
                       (i64)loud_ws_e_offset(lp), lp.hop, lp.H, tp, (dmx_meters_result *)out);
}
#else
// ------------------------------------------------------------------------------------------------ host: the driver
struct TpHostPiece
{
    const float *x; // planar [2][n] or interleaved [n][2]
    i64 n;
    bool interleaved;
    i64 i0, i1;
};
struct TpHostGather
{
    void operator()(const TpHostPiece &pc, int, i64 i, int cnt, float L[4], float R[4]) const
    {
        for (int k = 0; k < 4; ++k)
        {
            L[k] = k < cnt ? (pc.interleaved ? pc.x[2 * (i + k)] : pc.x[i + k]) : 0.0f;
            R[k] = k < cnt ? (pc.interleaved ? pc.x[2 * (i + k) + 1] : pc.x[pc.n + i + k]) : 0.0f;
        }
    }
};
static float tp_lane_any(const TpLds &sh, const TpFilter &f, int tid, i64 t0, i64 lo, i64 hi)
{
    return f.F == 4 ? tp_lane<4>(sh, f, tid, t0, lo, hi) : f.F == 2 ? tp_lane<2>(sh, f, tid, t0, lo, hi) : tp_lane<1>(sh, f, tid, t0, lo, hi);
}
// the true-peak launch on one signal cut into the pieces [0, cut) and [cut, n) (cut a multiple of 4; 0: one piece)
static float tp_host_measure(const float *x, bool interleaved, i64 n, int rate, i64 cut)
{
    TpFilter f;
    tp_filter(rate, &f);
    std::vector<TpLds> lds(1);
    TpLds &sh = lds[0];
    float m = 0.0f;
    const i64 cuts[3] = {0, cut > 0 && cut < n ? cut : n, n};
    for (int q = 0; q < 2; ++q)
    {
        const TpHostPiece pc{x, n, interleaved, cuts[q], cuts[q + 1]};
        if (pc.i1 <= pc.i0)
            continue;
        i64 lo, hi;
        tp_range(pc.i0, pc.i1, n, lo, hi);
        for (i64 t0 = lo / kTpTile * kTpTile; t0 < hi; t0 += kTpTile)
        {
            for (int tid = 0; tid < 256; ++tid)
                tp_stage(pc, TpHostGather{}, 0, n, t0, tid, sh);
            for (int tid = 0; tid < 256; ++tid)
            {
                const float v = tp_lane_any(sh, f, tid, t0, lo, hi);
                m = v > m ? v : m;
            }
        }
    }
    return m;
}
// the meters launch on one signal's hop energies e[2][H]
static void meters_host(const double *e, int hop, int H, int *lraC, int *maxMC, int *maxSC)
{
    std::vector<MetersLds> lds(1);
    MetersLds &sh = lds[0];
    for (int tid = 0; tid < 256; ++tid)
        meters_init(sh, tid, 256);
    for (int tid = 0; tid < 256; ++tid)
        meters_blocks(e, hop, H, tid, 256, sh);
    for (int tid = 0; tid < 256; ++tid)
        meters_compact_count(sh, tid);
    for (int tid = 0; tid < 256; ++tid)
        meters_compact_write(sh, tid);
    const MetersOut r = meters_finish(sh, H);
    *lraC = r.lraC, *maxMC = r.maxMC, *maxSC = r.maxSC;
}
#endif

} // namespace dmx
