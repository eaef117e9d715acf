// hpss.hip — median-filter harmonic/percussive separation of stems for gfx950 (specification: DESIGN.md section 2.23, restated
// in tests/hpss_spec.py; Fitzgerald 2010 with Driedger's margins, what librosa.decompose.hpss computes; geometry and workspace:
// hpss_plan.h). Every plane on its own. D[t][k] is the Wiener stage's STFT (wiener_stft.h, the J stems as the plane sets).
//   S[t][k] = fp32(sqrt(re^2 + im^2)), the squares, the sum and the root in binary64
//   H[t][k] = median of S[t - h .. t + h][k], kernel_h = 2 h + 1;  P[t][k] = median of S[t][k - p .. k + p], kernel_p = 2 p + 1
//   an index outside the plane is folded by half-sample symmetric reflection, d c b a | a b c d | d c b a (hpss_fold), as
//   often as it takes
//   softmask(x, r), in binary64 without contraction: z = max(x, r); a = (x / z)^power, b = (r / z)^power by repeated
//   multiplication from the left; a / (a + b); where z < FLT_MIN: 0.5 if both margins are 1, else 0
//   M_h = fp32(softmask(H, margin_h P)), M_p = fp32(softmask(P, margin_p H))
//   the outputs: the Wiener stage's inverse of M_h D, of M_p D and, with `residual`, of ((1 - M_h) - M_p) D, products in fp32
// Two kernels:
//   filter    one workgroup of 256 threads per tile of 64 bins x 32 frames of a plane. It takes the magnitudes of the tile and
//             of a halo of 15 cells on all four sides once per cell, folding by index arithmetic, into 62 rows of 94 (+ 1)
//             words of LDS (23.6 KB). A thread is a bin lane and 8 consecutive frames. Time: the 38 values of its column go
//             to registers once and the 31-wide window slides over them with static indices. Frequency: the 31 neighbours of
//             a cell come from LDS; the lanes of a wave are consecutive bins, so no bank is asked twice. Both medians go
//             through median31 below; a window of k < 31 is padded with (31 - k) / 2 times -inf and as many +inf, which
//             leaves the median where it was. The masks follow in registers: S, H and P never reach HBM.
//   inverse   wiener_istft_body with the masked spectrum as its source, launched once per kind of output over the same D.
// median31: Batcher's merge exchange (Knuth 5.2.2, Algorithm M) for 31 keys, 186 comparators, pruned to output 15: the
// comparators that no path joins to that output are dropped (152 remain) and of the others only the half that something
// reads is computed (274 v_min_i32 / v_max_i32 in all, on the bits of the magnitudes; the counts are asserted below). The
// network is made at compile time and applied with constant indices, so the 31 keys stay in registers. With both windows at
// 31 the kernel is the variant without the padding's instructions.
// No atomics, every decision in a fixed order: equal inputs, equal bits. Magnitudes are taken to be finite.
// Out of scope: hard masks (an infinite power), windows above 31, other STFT sizes, more than 2 channels, the multi-track
// entry points, an HPSS-aware --tempo.
#include "wiener_stft.h"
#include "hpss_plan.h"
#include <cfloat>
#include <climits>
#include <utility>

namespace dmx
{
namespace
{
// ------------------------------------------------------------------------------------------------ the selection network
struct MedianNet
{
    static constexpr int kMax = 192;
    int a[kMax] = {}, b[kMax] = {}; // comparator c leaves min at a[c] and max at b[c], a[c] < b[c]
    bool lo[kMax] = {}, hi[kMax] = {}; // which of the two something reads
    int all = 0, kept = 0, ops = 0;
};
constexpr MedianNet median_net()
{
    MedianNet m{};
    constexpr int N = kHpssMaxKernel, t = 5; // 2^(t - 1) < N <= 2^t
    for (int p = 1 << (t - 1); p > 0; p >>= 1)
    {
        int q = 1 << (t - 1), r = 0, d = p;
        while (true)
        {
            for (int i = 0; i < N - d; ++i)
                if ((i & p) == r)
                    m.a[m.all] = i, m.b[m.all] = i + d, ++m.all;
            if (q == p)
                break;
            d = q - p, q >>= 1, r = p;
        }
    }
    bool live[N] = {};
    live[N / 2] = true;
    for (int c = m.all - 1; c >= 0; --c)
    {
        m.lo[c] = live[m.a[c]], m.hi[c] = live[m.b[c]];
        if (m.lo[c] || m.hi[c])
        {
            live[m.a[c]] = live[m.b[c]] = true;
            ++m.kept, m.ops += (m.lo[c] ? 1 : 0) + (m.hi[c] ? 1 : 0);
        }
    }
    return m;
}
constexpr MedianNet kMedianNet = median_net();
static_assert(kMedianNet.all == 186 && kMedianNet.kept == 152 && kMedianNet.ops == 274, "Batcher's merge exchange for 31 keys, pruned");

// The keys are the bits of the magnitudes as int32: a magnitude is +0 or above (the root of a sum of squares), and such floats
// order as their bits do, so v_min_i32 / v_max_i32 select what v_min_f32 / v_max_f32 would, without the quieting of the
// operands that the float forms need in IEEE mode (a v_max_f32 v, v, v per key of every window).
template <int c>
__device__ __forceinline__ void median_step(int (&v)[kHpssMaxKernel])
{
    constexpr int a = kMedianNet.a[c], b = kMedianNet.b[c];
    if (kMedianNet.lo[c] || kMedianNet.hi[c])
    {
        const int x = v[a], y = v[b];
        if (kMedianNet.lo[c])
            v[a] = min(x, y);
        if (kMedianNet.hi[c])
            v[b] = max(x, y);
    }
}
template <int... c>
__device__ __forceinline__ float median31_of(int (&v)[kHpssMaxKernel], std::integer_sequence<int, c...>)
{
    (median_step<c>(v), ...);
    return __int_as_float(v[kHpssMaxKernel / 2]);
}
// the median of the 31 keys of v, which it destroys
__device__ __forceinline__ float median31(int (&v)[kHpssMaxKernel])
{
    return median31_of(v, std::make_integer_sequence<int, kMedianNet.all>{});
}
// Key i of a window of 2 half + 1 values centred on key 15: outside it the lowest key below and the highest above (-inf and
// +inf of the padding). One v_min_i32 or v_max_i32 with a scalar that is uniform over the launch; the centre is always inside.
// FULL: half is 15 and every key is inside.
template <bool FULL>
__device__ __forceinline__ int window_key(int i, int half, int x)
{
    if (FULL || i == kHpssHalo)
        return x;
    if (i < kHpssHalo)
        return min(x, i < kHpssHalo - half ? INT_MIN : INT_MAX);
    return max(x, i > kHpssHalo + half ? INT_MAX : INT_MIN);
}

// ------------------------------------------------------------------------------------------------ the masks
__device__ __forceinline__ float softmask(double x, double r, int power, bool unit)
{
#pragma clang fp contract(off)
    const double z = x > r ? x : r;
    if (z < (double)FLT_MIN)
        return unit ? 0.5f : 0.f;
    const double qx = x / z, qr = r / z;
    double a = qx, b = qr;
    for (int i = 1; i < power; ++i)
        a = a * qx, b = b * qr;
    return (float)(a / (a + b));
}

struct HpssFilterArgs
{
    const float2 *D; // [planes][frames][row]
    float *A, *B;    // [planes][frames][row]: M_h and M_p, or H and P
    i64 plane;       // frames row
    int frames, bins, row;
    int halfH, halfP, power;
    double mh, mp;
};

// grid (tiles of 32 frames, tiles of 64 bins, planes). FULL: both windows are 31 wide, nothing is padded
template <int WHAT, bool FULL>
__global__ __launch_bounds__(256) void hpss_filter_kernel(const HpssFilterArgs p)
{
    __shared__ int S[kHpssLdsRows * kHpssLdsStride]; // the bits of the magnitudes
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int t0 = blockIdx.x * kHpssTileFrames, k0 = blockIdx.y * kHpssTileBins;
    const float2 *d = p.D + (i64)blockIdx.z * p.plane;
    for (int i = tid; i < kHpssLdsRows * kHpssLdsCols; i += 256)
    {
        const int r = i / kHpssLdsCols, c = i - r * kHpssLdsCols;
        const int t = hpss_fold(t0 - kHpssHalo + r, p.frames), k = hpss_fold(k0 - kHpssHalo + c, p.bins); // both inside the plane
        const float2 z = d[(i64)t * p.row + k];
        S[r * kHpssLdsStride + c] = __float_as_int((float)sqrt((double)z.x * z.x + (double)z.y * z.y));
    }
    __syncthreads();
    const int k = k0 + lane, tBeg = t0 + grp * 8;
    if (k >= p.bins || tBeg >= p.frames)
        return;
    int col[8 + 2 * kHpssHalo]; // the thread's column: rows grp 8 .. grp 8 + 37 of the image
#pragma unroll
    for (int i = 0; i < 8 + 2 * kHpssHalo; ++i)
        col[i] = S[(grp * 8 + i) * kHpssLdsStride + kHpssHalo + lane];
    const bool unit = p.mh == 1.0 && p.mp == 1.0;
    float *oa = p.A + (i64)blockIdx.z * p.plane + (i64)tBeg * p.row + k, *ob = p.B + (i64)blockIdx.z * p.plane + (i64)tBeg * p.row + k;
#pragma unroll
    for (int j = 0; j < 8; ++j)
    {
        int v[kHpssMaxKernel];
#pragma unroll
        for (int i = 0; i < kHpssMaxKernel; ++i)
            v[i] = window_key<FULL>(i, p.halfH, col[j + i]);
        const float H = median31(v);
        const int *row = S + (grp * 8 + j + kHpssHalo) * kHpssLdsStride + lane;
#pragma unroll
        for (int i = 0; i < kHpssMaxKernel; ++i)
            v[i] = window_key<FULL>(i, p.halfP, row[i]);
        const float P = median31(v);
        if (tBeg + j < p.frames)
        {
            if (WHAT == kHpssMedians)
                oa[(i64)j * p.row] = H, ob[(i64)j * p.row] = P;
            else
            {
                oa[(i64)j * p.row] = softmask((double)H, p.mh * (double)P, p.power, unit);
                ob[(i64)j * p.row] = softmask((double)P, p.mp * (double)H, p.power, unit);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the inverse
// the spectrum source of the inverse (wiener_stft.h): the rows of D times a mask row; KIND 0 M_h, 1 M_p, 2 (1 - M_h) - M_p
template <int C, int KIND>
struct MaskedSpectrum
{
    const float2 *d0, *r0;
    const float *h0, *p0, *rh, *rp;
    i64 plane;
    __device__ MaskedSpectrum(const float2 *D, const float *mh, const float *mp, i64 plane_, int src)
        : d0(D + (i64)src * C * plane_), r0(nullptr), h0(mh + (i64)src * C * plane_), p0(mp + (i64)src * C * plane_), rh(nullptr), rp(nullptr),
          plane(plane_)
    {
    }
    __device__ __forceinline__ void seek(i64 f) { r0 = d0 + f * kWienerRow, rh = h0 + f * kWienerRow, rp = p0 + f * kWienerRow; }
    __device__ __forceinline__ float2 masked(i64 at) const
    {
        const float m = KIND == 0 ? rh[at] : KIND == 1 ? rp[at] : (1.f - rh[at]) - rp[at];
        const float2 z = r0[at];
        return make_float2(m * z.x, m * z.y);
    }
    __device__ __forceinline__ void bin(int, int k, float2 &a, float2 &b) const
    {
        a = masked(k), b = C == 2 ? masked(plane + k) : make_float2(0.f, 0.f);
    }
};

// grid (chunks, J)
template <int C, int KIND>
__global__ __launch_bounds__(256) void hpss_istft_kernel(const WienerArgs p, const float *mh, const float *mp, int kinds)
{
    MaskedSpectrum<C, KIND> spectrum(p.ispec, mh, mp, p.plane, blockIdx.y);
    wiener_istft_body<C>(p, spectrum, kinds, KIND);
}
template <int C, int KIND>
void launch_hpss_istft(const WienerArgs &v, const float *mh, const float *mp, int kinds, hipStream_t s)
{
    hipLaunchKernelGGL((hpss_istft_kernel<C, KIND>), dim3((unsigned)v.chunks, v.J), dim3(256), 0, s, v, mh, mp, kinds);
}
} // namespace

void launch_hpss_filter(const float2 *D, int planes, int frames, int bins, int row, const HpssSpec &spec, int what, float *A, float *B, hipStream_t s)
{
    HpssFilterArgs a{};
    a.D = D, a.A = A, a.B = B, a.plane = (i64)frames * row, a.frames = frames, a.bins = bins, a.row = row;
    a.halfH = spec.kh / 2, a.halfP = spec.kp / 2, a.power = spec.power, a.mh = spec.mh, a.mp = spec.mp;
    const dim3 grid((frames + kHpssTileFrames - 1) / kHpssTileFrames, (bins + kHpssTileBins - 1) / kHpssTileBins, planes);
    const bool full = a.halfH == kHpssHalo && a.halfP == kHpssHalo;
    if (what == kHpssMedians)
        hipLaunchKernelGGL((full ? hpss_filter_kernel<kHpssMedians, true> : hpss_filter_kernel<kHpssMedians, false>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((full ? hpss_filter_kernel<kHpssMasks, true> : hpss_filter_kernel<kHpssMasks, false>), grid, dim3(256), 0, s, a);
}

void launch_hpss(const HpssJob &job, hipStream_t s, hipEvent_t *marks)
{
    const HpssLayout l = hpss_layout(job.J, job.C, job.n);
    WienerArgs w{}; // the forward transform: plane set j is stem j
    w.mix = job.x, w.ests = job.x + (i64)job.C * job.stride;
    w.tw = (float2 *)(job.work + l.tw), w.win = (float *)(job.work + l.win), w.fmax = (double *)(job.work + l.fmax);
    w.spec = (float2 *)(job.work + l.D);
    w.n = job.n, w.stride = job.stride, w.T = l.T, w.plane = l.plane, w.J = job.J;
    WienerArgs v = w; // the inverse
    v.ispec = w.spec, v.out = job.out, v.stride = job.outStride, v.chunks = l.chunks;
    float *mh = (float *)(job.work + l.mh), *mp = (float *)(job.work + l.mp);
    const int kinds = 2 + job.spec.residual;
    Marks mark{marks, s};
    mark();
    hipLaunchKernelGGL(wiener_tables_kernel, dim3(16), dim3(256), 0, s, w.tw, w.win);
    if (job.C == 2)
        hipLaunchKernelGGL((wiener_stft_kernel<2, false>), dim3((unsigned)l.T, job.J), dim3(256), 0, s, w);
    else
        hipLaunchKernelGGL((wiener_stft_kernel<1, false>), dim3((unsigned)l.T, job.J), dim3(256), 0, s, w);
    mark();
    launch_hpss_filter(w.spec, job.J * job.C, (int)l.T, kWienerBins, kWienerRow, job.spec, kHpssMasks, mh, mp, s);
    mark();
    if (job.C == 2)
    {
        launch_hpss_istft<2, 0>(v, mh, mp, kinds, s);
        launch_hpss_istft<2, 1>(v, mh, mp, kinds, s);
        if (job.spec.residual)
            launch_hpss_istft<2, 2>(v, mh, mp, kinds, s);
    }
    else
    {
        launch_hpss_istft<1, 0>(v, mh, mp, kinds, s);
        launch_hpss_istft<1, 1>(v, mh, mp, kinds, s);
        if (job.spec.residual)
            launch_hpss_istft<1, 2>(v, mh, mp, kinds, s);
    }
    mark();
}

} // namespace dmx
