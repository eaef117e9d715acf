// loudness.hip — integrated loudness (ITU-R BS.1770-4 / EBU R 128) of the track path's outputs and of the mixture, and the
// gain that brings them to a target (the specification is restated in tests/loudness_spec.py).
//
// The measurement is an IIR filter, serial in time: two biquads (the K-weighting's shelf and high-pass, coefficients computed
// on the host for the rate) in transposed direct form II, i.e. a linear recurrence s[i+1] = A s[i] + B x[i] over four states.
// It is evaluated exactly, in binary64, as a chunked scan with NO wait of one workgroup on another - every carry between
// workgroups crosses a launch boundary:
//   1  loud_tile_kernel<false>  a workgroup takes a tile of 4096 frames of one signal (an output row of a gain table, through
//      the same GatherRemix functor the peak and encode kernels use, so a plane with gain 0 is not read), stages both channels
//      in LDS with coalesced loads (rows of 64 frames, padded to 65 words: a lane walking its row meets no bank conflict), and
//      one wave per channel runs 64 chunks of 64 frames from zero state. A Hillis-Steele scan over the lanes with the
//      host-supplied powers A^64, A^128 .. A^2048 gives the state at the tile's end for zero state at its start.
//   2  loud_scan_kernel         one wave per signal and channel turns the tiles' end states into the tiles' true initial
//      states: each lane sweeps a unit of U = ceil(tiles / 64) consecutive tiles with A^4096, a scan over the lanes with
//      A^(4096 U 2^j) joins the units, a second sweep writes the result. Trip counts are known at launch.
//   3  loud_tile_kernel<true>   stages the tile again, lane 0 starts from the tile's true state, the same scan gives every
//      lane its true initial state, and the lanes run their chunks a second time accumulating y^2 into the one or two 100 ms
//      hops a chunk touches. The tile's lanes are summed per hop in lane order by one lane per hop.
//   4  loud_final_kernel        one workgroup per signal: the hop energies as sums over the tiles in tile order, the 400 ms
//      blocks, the two gates, L and its quantum lufs_c = rint(100 L) - fixed-order sums of 256 strided partials and a tree.
// There are no floating-point atomics: L is the same bits from run to run, whatever else the call holds.
// Then loud_gain_kernel (one launch, no host round trip) reads lufs_c and the peaks the peak kernel formed, looks the gain up
// in the host-made table T[k + 6000] = (float)10^(k / 2000), applies the ceiling, and leaves per output the gain for the
// encode kernel (pcm.hip, the GAIN form) and the peak of the gained samples g * P.
// Workspace: per signal 64 bytes, per tile 64 bytes of states and 8 bytes per hop it can touch, 16 bytes per hop: the host sizes it
// for the smallest hop (400 frames), 64 + 256 per tile + 16 per 400 frames, about n / 10 bytes.
// The bodies are templates over the gather functor (the host driver brings its own); the kernels are instantiated for GatherRemix
// alone. An output spec (GatherStems) is measured as its 0/1 gain matrix, which gathers the same bits (1 * x is exact).
//
// True peak, loudness range and the momentary and short-term maxima are meters.hip's (they read the hop energies left here);
// loud_gain_tp_kernel is the ceiling by true peak. Out of scope: ReplayGain tags, the engine.
//
// With DMX_LOUDNESS_HOST defined the same bodies compile as plain C++ (tests/loudness_host_main.cpp): each kernel is a
// sequence of phases, each a function of (tile, lane); the device kernels call them with barriers between, the host driver at
// the end of this file runs each phase for all lanes in turn. The cross-lane exchanges (the scan's shuffles, the final
// kernel's tree) are the only device-only text; the host driver performs the same steps in the same order on arrays.
#ifdef DMX_LOUDNESS_HOST
#include "loudness_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
namespace dmx
{
typedef int64_t i64;
}
#define LD_DEV static inline
#else
#include "kernels.h"
#include "pcm_gather.h"

#include "../../include/demucs_hip.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
#define LD_DEV __device__ __forceinline__
#endif

namespace dmx
{
// ------------------------------------------------------------------------------------------------ host: the plan
void loud_coefficients(int rate, double coef[10])
{
    const double pi = 3.14159265358979323846;
    double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    double K = std::tan(pi * f0 / rate);
    const double Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    double a0 = 1.0 + K / Q + K * K;
    coef[0] = (Vh + Vb * K / Q + K * K) / a0;
    coef[1] = 2.0 * (K * K - Vh) / a0;
    coef[2] = (Vh - Vb * K / Q + K * K) / a0;
    coef[3] = 2.0 * (K * K - 1.0) / a0;
    coef[4] = (1.0 - K / Q + K * K) / a0;
    f0 = 38.13547087602444, Q = 0.5003270373238773;
    K = std::tan(pi * f0 / rate);
    a0 = 1.0 + K / Q + K * K;
    coef[5] = 1.0, coef[6] = -2.0, coef[7] = 1.0;
    coef[8] = 2.0 * (K * K - 1.0) / a0;
    coef[9] = (1.0 - K / Q + K * K) / a0;
}

namespace
{
// one frame through both biquads: s = (shelf z1, z2, high-pass z1, z2); returns the K-weighted sample
#ifdef DMX_LOUDNESS_HOST
static inline
#else
__host__ __device__ __forceinline__
#endif
    double
    loud_step(const double *k, double s[4], double x)
{
    const double y1 = k[0] * x + s[0];
    s[0] = k[1] * x - k[3] * y1 + s[1];
    s[1] = k[2] * x - k[4] * y1;
    const double y2 = y1 + s[2];
    s[2] = -2.0 * y1 - k[5] * y2 + s[3];
    s[3] = y1 - k[6] * y2;
    return y2;
}
void loud_mat_mul(const double *a, const double *b, double *c) // c = a b, row-major 4 x 4; c may be a or b
{
    double t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
        {
            double v = 0.0;
            for (int l = 0; l < 4; ++l)
                v += a[4 * i + l] * b[4 * l + j];
            t[4 * i + j] = v;
        }
    for (int i = 0; i < 16; ++i)
        c[i] = t[i];
}
void loud_mat_pow(const double *a, i64 e, double *r) // r = a^e, e >= 1
{
    double base[16], acc[16];
    bool have = false;
    for (int i = 0; i < 16; ++i)
        base[i] = a[i];
    for (; e > 0; e >>= 1)
    {
        if (e & 1)
        {
            if (have)
                loud_mat_mul(acc, base, acc);
            else
                for (int i = 0; i < 16; ++i)
                    acc[i] = base[i];
            have = true;
        }
        loud_mat_mul(base, base, base);
    }
    for (int i = 0; i < 16; ++i)
        r[i] = acc[i];
}
// A^e, A the filter's state matrix: column j is the state e steps behind the unit state e_j with no input. Up to kStepCap
// steps it is formed BY STEPPING, the way the filter itself runs: the high-pass has a double pole next to 1, the entries of
// A^e are differences of much larger terms, and repeated squaring of A loses in them what a signal with a DC offset then
// shows in its energies (1e-8 relative at 96 kHz; stepping: the rounding of the sequential filter). Past the cap the entries
// are below 1e-9 of a state and products of stepped powers serve.
constexpr i64 kStepCap = 16 * kLoudTile;
// out[x] = A^(exps[x]) for all x, in one stepping pass of the four unit states
void loud_state_powers(const double *k, const i64 *exps, int nE, double (*out)[16])
{
    struct Want
    {
        i64 steps;
        double *dst;
    };
    std::vector<Want> want;
    std::vector<double> low((size_t)16 * nE);
    double cap[16];
    bool needCap = false;
    for (int x = 0; x < nE; ++x)
    {
        if (exps[x] <= kStepCap)
            want.push_back(Want{exps[x], out[x]});
        else
        {
            needCap = true;
            want.push_back(Want{exps[x] % kStepCap, &low[(size_t)16 * x]});
        }
    }
    if (needCap)
        want.push_back(Want{kStepCap, cap});
    std::sort(want.begin(), want.end(), [](const Want &a, const Want &b) { return a.steps < b.steps; });
    double s[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}}; // s[j]: from e_j
    i64 done = 0;
    for (const Want &w : want)
    {
        for (; done < w.steps; ++done)
            for (int j = 0; j < 4; ++j)
                loud_step(k, s[j], 0.0);
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 4; ++i)
                w.dst[4 * i + j] = s[j][i];
    }
    for (int x = 0; x < nE; ++x)
        if (exps[x] > kStepCap)
        {
            loud_mat_pow(cap, exps[x] / kStepCap, out[x]);
            if (exps[x] % kStepCap)
                loud_mat_mul(out[x], &low[(size_t)16 * x], out[x]);
        }
}
} // namespace

int loud_plan(int rate, int64_t n, LoudPlan *p)
{
    if (rate < kLoudMinRate || n < 1 || n >= (int64_t)1 << 36)
        return -1;
    double c[10];
    loud_coefficients(rate, c);
    p->k[0] = c[0], p->k[1] = c[1], p->k[2] = c[2], p->k[3] = c[3], p->k[4] = c[4], p->k[5] = c[8], p->k[6] = c[9];
    p->n = n;
    p->hop = (rate + 5) / 10;
    p->H = (int)(n / p->hop);
    p->nTiles = (int)((n + kLoudTile - 1) / kLoudTile);
    p->kHops = kLoudTile / p->hop + 2;
    p->U = (p->nTiles + 63) / 64;
    p->absThr = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    i64 exps[13];
    double pw[13][16];
    for (int j = 0; j < 6; ++j)
        exps[j] = (i64)kLoudChunk << j, exps[7 + j] = ((i64)kLoudTile * p->U) << j;
    exps[6] = kLoudTile;
    loud_state_powers(p->k, exps, 13, pw);
    for (int j = 0; j < 6; ++j)
    {
        std::memcpy(p->lane[j], pw[j], sizeof pw[j]);
        std::memcpy(p->unit[j], pw[7 + j], sizeof pw[j]);
    }
    std::memcpy(p->tile, pw[6], sizeof pw[6]);
    return 0;
}

int64_t loud_workspace_bytes(int64_t n) { return n < 1 ? -1 : loud_ws_bytes(n); }

void loud_gain_table(float *T)
{
    for (int i = 0; i < kLoudGainSteps; ++i)
        T[i] = (float)std::pow(10.0, (i - 6000) / 2000.0);
}

namespace
{
// ------------------------------------------------------------------------------------------------ the workspace of a signal
struct LoudRes
{
    double L;   // NaN: unmeasurable
    int lufsC;  // INT_MIN: unmeasurable
    int pad;
};
LD_DEV LoudRes *loud_ws_res(unsigned char *slot) { return reinterpret_cast<LoudRes *>(slot); }
LD_DEV double *loud_ws_states(unsigned char *slot) { return reinterpret_cast<double *>(slot + 64); } // [2][nTiles][4]
LD_DEV double *loud_ws_part(unsigned char *slot, const LoudPlan &lp) { return loud_ws_states(slot) + (i64)8 * lp.nTiles; } // [2][nTiles][kHops]
LD_DEV double *loud_ws_e(unsigned char *slot, const LoudPlan &lp) { return reinterpret_cast<double *>(slot + loud_ws_e_offset(lp)); } // [2][H]

constexpr int kLoudRow = kLoudChunk + 1; // words of a staged row: lane l's row starts at bank (l * 65) % 32 = l % 32
struct LoudLds
{
    float x[2][64 * kLoudRow]; // the tile, channel by channel, a row of 64 frames per lane
    double p[2][64][2];        // a lane's two hop partials
    int kk[2][64];             // the hop of a lane's first frame, counted from the tile's first hop
};

// ------------------------------------------------------------------------------------------------ phases of the tile kernels
// thread tid of 128 stages its share of the tile starting at frame t0 (frames at and past n are zeros)
template <class Piece, class Gather>
LD_DEV void loud_stage(const Piece &pc, const Gather &gather, int o, i64 n, i64 t0, int tid, LoudLds &sh)
{
    for (int it = 0; it < kLoudTile / 4 / 128; ++it)
    {
        const int f = 4 * (it * 128 + tid); // 4 frames of one row: 4 divides 64
        const i64 i = t0 + f;
        const int cnt = n - i >= 4 ? 4 : (n > i ? (int)(n - i) : 0);
        float L[4] = {0.0f, 0.0f, 0.0f, 0.0f}, R[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (cnt > 0)
            gather(pc, o, i, cnt, L, R);
        const int at = (f >> 6) * kLoudRow + (f & 63);
        for (int k = 0; k < 4; ++k)
            sh.x[0][at + k] = L[k], sh.x[1][at + k] = R[k];
    }
}
// the lane's chunk from state s; s becomes the state behind it
LD_DEV void loud_chunk_state(const LoudPlan &lp, const LoudLds &sh, int tid, double s[4])
{
    const float *row = sh.x[tid >> 6] + (tid & 63) * kLoudRow;
    for (int i = 0; i < kLoudChunk; ++i)
        loud_step(lp.k, s, (double)row[i]);
}
// v += P u
LD_DEV void loud_apply(const double *P, const double u[4], double v[4])
{
    for (int i = 0; i < 4; ++i)
        v[i] += ((P[4 * i] * u[0] + P[4 * i + 1] * u[1]) + P[4 * i + 2] * u[2]) + P[4 * i + 3] * u[3];
}
// the lane's chunk from its true state: y^2 into the hop of its first frame and, behind a hop boundary, into the next one
LD_DEV void loud_chunk_energy(const LoudPlan &lp, LoudLds &sh, int tid, i64 t, const double init[4])
{
    const int c = tid >> 6, lane = tid & 63;
    const float *row = sh.x[c] + lane * kLoudRow;
    const i64 f0 = t * kLoudTile + (i64)lane * kLoudChunk;
    const i64 j0 = f0 / lp.hop, jf = t * kLoudTile / lp.hop;
    const i64 left = (j0 + 1) * lp.hop - f0; // frames of hop j0 from f0 on: >= 1
    const int nFirst = left < kLoudChunk ? (int)left : kLoudChunk;
    double s[4] = {init[0], init[1], init[2], init[3]};
    double p0 = 0.0, p1 = 0.0;
    for (int i = 0; i < kLoudChunk; ++i)
    {
        const double y = loud_step(lp.k, s, (double)row[i]);
        const double q = y * y;
        if (i < nFirst)
            p0 += q;
        else
            p1 += q;
    }
    sh.p[c][lane][0] = p0, sh.p[c][lane][1] = p1;
    sh.kk[c][lane] = (int)(j0 - jf);
}
// lane k of a channel's wave sums the tile's partials of the tile's k-th hop, in lane order
LD_DEV void loud_tile_reduce(const LoudPlan &lp, const LoudLds &sh, int tid, i64 t, double *part)
{
    const int c = tid >> 6, k = tid & 63;
    if (k >= lp.kHops)
        return;
    double acc = 0.0;
    for (int l = 0; l < 64; ++l)
    {
        const int kk = sh.kk[c][l];
        if (kk == k)
            acc += sh.p[c][l][0];
        if (kk + 1 == k)
            acc += sh.p[c][l][1];
    }
    part[((i64)c * lp.nTiles + t) * lp.kHops + k] = acc;
}
// ------------------------------------------------------------------------------------------------ phases of the scan kernel
// lane's unit of U tiles from state s: with `write`, a tile's slot receives the state in front of it
LD_DEV void loud_unit_sweep(const LoudPlan &lp, double *st, int lane, bool write, double s[4])
{
    for (int k = 0; k < lp.U; ++k)
    {
        const i64 t = (i64)lane * lp.U + k;
        if (t >= lp.nTiles)
            break;
        double w[4], v[4];
        for (int j = 0; j < 4; ++j)
            w[j] = st[4 * t + j], v[j] = w[j];
        if (write)
            for (int j = 0; j < 4; ++j)
                st[4 * t + j] = s[j];
        loud_apply(lp.tile, s, v); // v = w + A^4096 s
        for (int j = 0; j < 4; ++j)
            s[j] = v[j];
    }
}
// ------------------------------------------------------------------------------------------------ phases of the final kernel
// hop j of channel c: the tiles that overlap it, in tile order
LD_DEV double loud_hop_energy(const LoudPlan &lp, const double *part, int c, int j)
{
    const i64 t0 = (i64)j * lp.hop / kLoudTile, t1 = ((i64)(j + 1) * lp.hop - 1) / kLoudTile;
    double acc = 0.0;
    for (i64 t = t0; t <= t1; ++t)
    {
        const i64 jf = t * kLoudTile / lp.hop; // <= j, and j - jf < kHops: the tile holds a frame of hop j
        acc += part[((i64)c * lp.nTiles + t) * lp.kHops + (j - jf)];
    }
    return acc;
}
LD_DEV double loud_block_z(const LoudPlan &lp, const double *e, int b)
{
    const double *e0 = e, *e1 = e + lp.H;
    const double s0 = e0[b] + e1[b], s1 = e0[b + 1] + e1[b + 1], s2 = e0[b + 2] + e1[b + 2], s3 = e0[b + 3] + e1[b + 3];
    return (((s0 + s1) + s2) + s3) / (4.0 * lp.hop);
}
// the thread's blocks b = tid, tid + nThreads ..: those past both thresholds (a NaN passes: it must reach L)
LD_DEV void loud_gate_partial(const LoudPlan &lp, const double *e, int tid, int nThreads, double thrA, double thrB, double &sum, int &cnt)
{
    sum = 0.0, cnt = 0;
    for (int b = tid; b < lp.H - 3; b += nThreads)
    {
        const double z = loud_block_z(lp, e, b);
        if (!(z <= thrA) && !(z <= thrB))
            sum += z, ++cnt;
    }
}
LD_DEV void loud_finish(double sum, int cnt, LoudRes *res)
{
    double L = 0.0;
    bool ok = cnt > 0;
    if (ok)
    {
        L = -0.691 + 10.0 * log10(sum / cnt);
        ok = L - L == 0.0; // finite
    }
    res->L = ok ? L : (double)NAN;
    res->lufsC = ok ? (int)rint(100.0 * L) : INT_MIN;
    res->pad = 0;
}
// the fp32 gain of a signal of lufsC whose sample peak is P
LD_DEV float loud_gain_of(int lufsC, int targetC, float P, float maxPeak, const float *T)
{
    if (lufsC == INT_MIN)
        return 1.0f;
    long long k = (long long)targetC - lufsC;
    k = k < -6000 ? -6000 : (k > 6000 ? 6000 : k);
    float g = T[k + 6000];
    if (P > 0.0f && g * P > maxPeak)
        g = maxPeak / P;
    return g;
}
} // namespace

#ifndef DMX_LOUDNESS_HOST
// ------------------------------------------------------------------------------------------------ device: the kernels
namespace
{
// inclusive scan over the wave's lanes: s_l <- s_l + A^c s_(l-1) + A^2c s_(l-2) + .., P[j] = A^(c 2^j)
__device__ __forceinline__ void loud_wave_scan(const double P[6][16], double s[4], int lane)
{
#pragma unroll
    for (int j = 0; j < 6; ++j)
    {
        double u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            u[i] = __shfl_up(s[i], 1u << j, 64);
        if (lane >= (1 << j))
            loud_apply(P[j], u, s);
    }
}
} // namespace

// grid (tiles, signals), block 128: wave 0 the left channel, wave 1 the right one
template <bool ENERGY>
__global__ __launch_bounds__(128) void loud_tile_kernel(RemixPiece pc, PcmGains G, LoudPlan lp, unsigned char *work, i64 slotBytes, int slot0)
{
    __shared__ LoudLds sh;
    const int tid = threadIdx.x, lane = tid & 63, c = tid >> 6, o = blockIdx.y;
    const i64 t = blockIdx.x;
    unsigned char *slot = work + (i64)(slot0 + o) * slotBytes;
    double *st = loud_ws_states(slot) + ((i64)c * lp.nTiles + t) * 4;
    loud_stage(pc, GatherRemix{G}, o, lp.n, t * kLoudTile, tid, sh);
    __syncthreads();
    double s[4] = {0.0, 0.0, 0.0, 0.0}, carry[4] = {0.0, 0.0, 0.0, 0.0};
    if (ENERGY)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            carry[j] = st[j];
        if (lane == 0)
        {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                s[j] = carry[j];
        }
    }
    loud_chunk_state(lp, sh, tid, s);
    loud_wave_scan(lp.lane, s, lane);
    if (!ENERGY)
    {
        if (lane == 63)
        {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                st[j] = s[j];
        }
        return;
    }
    double init[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const double u = __shfl_up(s[j], 1u, 64);
        init[j] = lane == 0 ? carry[j] : u;
    }
    loud_chunk_energy(lp, sh, tid, t, init);
    __syncthreads();
    loud_tile_reduce(lp, sh, tid, t, loud_ws_part(slot, lp));
}

// grid (2, signals), block 64
__global__ __launch_bounds__(64) void loud_scan_kernel(LoudPlan lp, unsigned char *work, i64 slotBytes, int slot0)
{
    const int lane = threadIdx.x, c = blockIdx.x;
    unsigned char *slot = work + (i64)(slot0 + blockIdx.y) * slotBytes;
    double *st = loud_ws_states(slot) + (i64)c * lp.nTiles * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    loud_unit_sweep(lp, st, lane, false, s);
    loud_wave_scan(lp.unit, s, lane);
    double init[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const double u = __shfl_up(s[j], 1u, 64);
        init[j] = lane == 0 ? 0.0 : u;
    }
    loud_unit_sweep(lp, st, lane, true, init);
}

namespace
{
// sum and count over the block's 256 threads in a fixed order; every thread returns the totals
__device__ __forceinline__ void loud_block_sum(double *a, int *cN, int tid, double &sum, int &cnt)
{
    __syncthreads(); // the arrays are free
    a[tid] = sum, cN[tid] = cnt;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1)
    {
        if (tid < off)
            a[tid] += a[tid + off], cN[tid] += cN[tid + off];
        __syncthreads();
    }
    sum = a[0], cnt = cN[0];
}
} // namespace

// grid (signals), block 256
__global__ __launch_bounds__(256) void loud_final_kernel(LoudPlan lp, unsigned char *work, i64 slotBytes, int slot0, double *eOut,
                                                         dmx_loudness_result *resOut)
{
    __shared__ double a[256];
    __shared__ int cN[256];
    const int tid = threadIdx.x, o = blockIdx.x;
    unsigned char *slot = work + (i64)(slot0 + o) * slotBytes;
    const double *part = loud_ws_part(slot, lp);
    double *e = loud_ws_e(slot, lp);
    for (i64 idx = tid; idx < (i64)2 * lp.H; idx += 256)
    {
        const int c = idx >= lp.H, j = (int)(idx - (i64)c * lp.H);
        const double v = loud_hop_energy(lp, part, c, j);
        e[idx] = v;
        if (eOut)
            eOut[(i64)o * 2 * lp.H + idx] = v;
    }
    __syncthreads();
    double sum;
    int cnt;
    loud_gate_partial(lp, e, tid, 256, lp.absThr, -1.0, sum, cnt);
    loud_block_sum(a, cN, tid, sum, cnt);
    if (cnt > 0)
    {
        const double rel = sum / cnt * 0.1; // 10 LU under the mean of the absolutely gated blocks
        loud_gate_partial(lp, e, tid, 256, lp.absThr, rel, sum, cnt);
        loud_block_sum(a, cN, tid, sum, cnt);
    }
    if (tid == 0)
    {
        LoudRes *res = loud_ws_res(slot);
        loud_finish(sum, cnt, res);
        if (resOut)
        {
            resOut[o].lufs_c = res->lufsC;
            resOut[o].gain = 0.0f;
            resOut[o].lufs = res->L;
        }
    }
}

// one block of 64: thread o < nOut is an output, thread nOut the mixture
__global__ __launch_bounds__(64) void loud_gain_kernel(const unsigned char *work, i64 slotBytes, int nOut, unsigned *peaks, int mode, int targetC,
                                                       float maxPeak, const float *T, float *gains, dmx_loudness_result *report)
{
    __shared__ float sP[PcmGains::kMaxOut];
    const int o = threadIdx.x;
    if (o < nOut)
        sP[o] = __uint_as_float(peaks[o]);
    __syncthreads();
    if (o > nOut)
        return;
    const LoudRes own = *reinterpret_cast<const LoudRes *>(work + (i64)o * slotBytes);
    if (o == nOut)
    {
        report[o].lufs_c = own.lufsC, report[o].gain = 0.0f, report[o].lufs = own.L;
        return;
    }
    float g = 1.0f;
    if (mode == DMX_LOUD_MIXTURE)
    {
        float P = 0.0f;
        for (int q = 0; q < nOut; ++q)
            P = sP[q] > P ? sP[q] : P;
        const LoudRes mix = *reinterpret_cast<const LoudRes *>(work + (i64)nOut * slotBytes);
        g = loud_gain_of(mix.lufsC, targetC, P, maxPeak, T);
    }
    else if (mode == DMX_LOUD_EACH)
        g = loud_gain_of(own.lufsC, targetC, sP[o], maxPeak, T);
    gains[o] = g;
    if (mode != DMX_LOUD_MEASURE)
        peaks[o] = __float_as_uint(g * sP[o]);
    report[o].lufs_c = own.lufsC, report[o].gain = g, report[o].lufs = own.L;
}

// the same with the ceiling by true peak (DMX_LOUD_TRUE_PEAK): the gain rule reads tp[o], the true peaks
// the true-peak kernel formed, where it read the sample peaks; peaks[o] still becomes the gained SAMPLE peak g * P
__global__ __launch_bounds__(64) void loud_gain_tp_kernel(const unsigned char *work, i64 slotBytes, int nOut, unsigned *peaks, const unsigned *tp,
                                                          int mode, int targetC, float maxPeak, const float *T, float *gains,
                                                          dmx_loudness_result *report)
{
    __shared__ float sP[PcmGains::kMaxOut], sTP[PcmGains::kMaxOut];
    const int o = threadIdx.x;
    if (o < nOut)
        sP[o] = __uint_as_float(peaks[o]), sTP[o] = __uint_as_float(tp[o]);
    __syncthreads();
    if (o > nOut)
        return;
    const LoudRes own = *reinterpret_cast<const LoudRes *>(work + (i64)o * slotBytes);
    if (o == nOut)
    {
        report[o].lufs_c = own.lufsC, report[o].gain = 0.0f, report[o].lufs = own.L;
        return;
    }
    float g = 1.0f;
    if (mode == DMX_LOUD_MIXTURE)
    {
        float P = 0.0f;
        for (int q = 0; q < nOut; ++q)
            P = sTP[q] > P ? sTP[q] : P;
        const LoudRes mix = *reinterpret_cast<const LoudRes *>(work + (i64)nOut * slotBytes);
        g = loud_gain_of(mix.lufsC, targetC, P, maxPeak, T);
    }
    else if (mode == DMX_LOUD_EACH)
        g = loud_gain_of(own.lufsC, targetC, sTP[o], maxPeak, T);
    gains[o] = g;
    if (mode != DMX_LOUD_MEASURE)
        peaks[o] = __float_as_uint(g * sP[o]);
    report[o].lufs_c = own.lufsC, report[o].gain = g, report[o].lufs = own.L;
}

void launch_loud_measure(const RemixPiece &pc, const PcmGains &G, const LoudPlan &lp, unsigned char *work, int slot0, double *eOut,
                         void *resOut, hipStream_t s, hipEvent_t *marks)
{
    auto mark = [&](int k) {
        if (marks)
            (void)hipEventRecord(marks[k], s);
    };
    const i64 slotBytes = loud_workspace_bytes(lp.n);
    const dim3 tiles((unsigned)lp.nTiles, (unsigned)G.nOut);
    mark(0);
    hipLaunchKernelGGL(loud_tile_kernel<false>, tiles, dim3(128), 0, s, pc, G, lp, work, slotBytes, slot0);
    mark(1);
    hipLaunchKernelGGL(loud_scan_kernel, dim3(2, (unsigned)G.nOut), dim3(64), 0, s, lp, work, slotBytes, slot0);
    mark(2);
    hipLaunchKernelGGL(loud_tile_kernel<true>, tiles, dim3(128), 0, s, pc, G, lp, work, slotBytes, slot0);
    mark(3);
    hipLaunchKernelGGL(loud_final_kernel, dim3((unsigned)G.nOut), dim3(256), 0, s, lp, work, slotBytes, slot0, eOut,
                       (dmx_loudness_result *)resOut);
    mark(4);
}

void launch_loud_gain(const unsigned char *work, i64 slotBytes, int nOut, unsigned *peaks, int mode, int targetC, float maxPeak,
                      const float *table, float *gains, void *report, hipStream_t s)
{
    hipLaunchKernelGGL(loud_gain_kernel, dim3(1), dim3(64), 0, s, work, slotBytes, nOut, peaks, mode, targetC, maxPeak, table, gains,
                       (dmx_loudness_result *)report);
}
void launch_loud_gain_tp(const unsigned char *work, i64 slotBytes, int nOut, unsigned *peaks, const unsigned *tp, int mode, int targetC,
                         float maxPeak, const float *table, float *gains, void *report, hipStream_t s)
{
    hipLaunchKernelGGL(loud_gain_tp_kernel, dim3(1), dim3(64), 0, s, work, slotBytes, nOut, peaks, tp, mode, targetC, maxPeak, table, gains,
                       (dmx_loudness_result *)report);
}
#else
// ------------------------------------------------------------------------------------------------ host: the driver
struct LoudHostPiece
{
    const float *x; // planar [2][n] or interleaved [n][2]
    i64 n;
    bool interleaved;
};
struct LoudHostGather
{
    void operator()(const LoudHostPiece &pc, int, i64 i, int cnt, float L[4], float R[4]) const
    {
        for (int k = 0; k < 4; ++k)
        {
            L[k] = k < cnt ? (pc.interleaved ? pc.x[2 * (i + k)] : pc.x[i + k]) : 0.0f;
            R[k] = k < cnt ? (pc.interleaved ? pc.x[2 * (i + k) + 1] : pc.x[pc.n + i + k]) : 0.0f;
        }
    }
};
// the device's loud_wave_scan, step for step, on the 64 lanes' states
static void loud_host_scan(const double P[6][16], double S[64][4])
{
    for (int j = 0; j < 6; ++j)
    {
        double U[64][4];
        std::memcpy(U, S, sizeof U);
        for (int lane = 1 << j; lane < 64; ++lane)
            loud_apply(P[j], U[lane - (1 << j)], S[lane]);
    }
}
// the four launches on one signal; e receives [2][H]. 0, or -1 (rate, n)
static int loud_host_measure(const float *x, bool interleaved, i64 n, int rate, double *L, int *lufsC, std::vector<double> &eOut)
{
    LoudPlan lp;
    if (loud_plan(rate, n, &lp) != 0)
        return -1;
    std::vector<unsigned char> work((size_t)loud_workspace_bytes(n));
    unsigned char *slot = work.data();
    const LoudHostPiece pc{x, n, interleaved};
    std::vector<LoudLds> lds(1);
    LoudLds &sh = lds[0];
    for (int pass = 0; pass < 2; ++pass)
    {
        for (i64 t = 0; t < lp.nTiles; ++t)
        {
            for (int tid = 0; tid < 128; ++tid)
                loud_stage(pc, LoudHostGather{}, 0, n, t * kLoudTile, tid, sh);
            double S[2][64][4], carry[2][4];
            for (int tid = 0; tid < 128; ++tid)
            {
                const int c = tid >> 6, lane = tid & 63;
                double *st = loud_ws_states(slot) + ((i64)c * lp.nTiles + t) * 4;
                for (int j = 0; j < 4; ++j)
                {
                    carry[c][j] = pass ? st[j] : 0.0;
                    S[c][lane][j] = pass && lane == 0 ? st[j] : 0.0;
                }
                loud_chunk_state(lp, sh, tid, S[c][lane]);
            }
            for (int c = 0; c < 2; ++c)
                loud_host_scan(lp.lane, S[c]);
            if (!pass)
            {
                for (int c = 0; c < 2; ++c)
                    for (int j = 0; j < 4; ++j)
                        loud_ws_states(slot)[((i64)c * lp.nTiles + t) * 4 + j] = S[c][63][j];
                continue;
            }
            for (int tid = 0; tid < 128; ++tid)
            {
                const int c = tid >> 6, lane = tid & 63;
                loud_chunk_energy(lp, sh, tid, t, lane == 0 ? carry[c] : S[c][lane - 1]);
            }
            for (int tid = 0; tid < 128; ++tid)
                loud_tile_reduce(lp, sh, tid, t, loud_ws_part(slot, lp));
        }
        if (!pass)
            for (int c = 0; c < 2; ++c)
            {
                double *st = loud_ws_states(slot) + (i64)c * lp.nTiles * 4;
                double S[64][4];
                std::memset(S, 0, sizeof S);
                for (int lane = 0; lane < 64; ++lane)
                    loud_unit_sweep(lp, st, lane, false, S[lane]);
                loud_host_scan(lp.unit, S);
                for (int lane = 63; lane >= 0; --lane) // a lane's sweep writes its own tiles only: any order
                {
                    double init[4] = {0.0, 0.0, 0.0, 0.0};
                    if (lane > 0)
                        std::memcpy(init, S[lane - 1], sizeof init);
                    loud_unit_sweep(lp, st, lane, true, init);
                }
            }
    }
    double *e = loud_ws_e(slot, lp);
    for (i64 idx = 0; idx < (i64)2 * lp.H; ++idx)
    {
        const int c = idx >= lp.H, j = (int)(idx - (i64)c * lp.H);
        e[idx] = loud_hop_energy(lp, loud_ws_part(slot, lp), c, j);
    }
    eOut.assign(e, e + (size_t)2 * lp.H);
    // the final kernel's sums: 256 strided partials, then the tree
    auto total = [&](double thrB, double &sum, int &cnt) {
        double a[256];
        int cN[256];
        for (int tid = 0; tid < 256; ++tid)
            loud_gate_partial(lp, e, tid, 256, lp.absThr, thrB, a[tid], cN[tid]);
        for (int off = 128; off >= 1; off >>= 1)
            for (int tid = 0; tid < off; ++tid)
                a[tid] += a[tid + off], cN[tid] += cN[tid + off];
        sum = a[0], cnt = cN[0];
    };
    double sum;
    int cnt;
    total(-1.0, sum, cnt);
    if (cnt > 0)
        total(sum / cnt * 0.1, sum, cnt);
    LoudRes res;
    loud_finish(sum, cnt, &res);
    *L = res.L, *lufsC = res.lufsC;
    return 0;
}
#endif

} // namespace dmx
