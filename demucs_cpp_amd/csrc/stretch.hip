// stretch.hip — time stretch and pitch shift of stems by the phase vocoder for gfx950 (specification: DESIGN.md section 2.22,
// restated in tests/stretch_spec.py; what librosa.phase_vocoder computes; geometry and workspace: stretch_plan.h). The forward
// transform is the Wiener stage's (wiener_stft.h) with the J stems as the plane sets and leaves D[plane][a][k]; the converter
// behind the inverse is resample.hip's. Output frame t reads the rows a_t = (t num) div den and a_t + 1 with the weight
// alpha_t = ((t num) mod den) / den, both exact in int64; rows from T on read as zero. With unit(z) = z / |z| (1 where z = 0) and
// u[a] = unit(D[a + 1]) conj(unit(D[a])), the phasor is the running product ph[0] = unit(D[0]), ph[t + 1] = ph[t] u[a_t] of
// unit complex numbers in binary64 (no angle, no transcendental function), and Y[t] = ((1 - alpha_t) |D[a_t]| + alpha_t
// |D[a_t + 1]|) ph[t] rounded to complex64. The running product is a scan over t, done in three launches:
//   live      beside the forward transform: the frames of a plane whose samples are all zero (stretch_live_kernel says why)
//   products  one workgroup per (range of output frames, tile of 64 bins, stem), a lane per bin and a wave per channel, so a
//             wave reads whole contiguous segments of a row. Range c is [stretch_first(c), stretch_first(c + 1)): what takes
//             the phasor from the first frame chunk c of the inverse forms to the first of chunk c + 1. A lane walks its frames
//             with unit(D[a]) and unit(D[a + 1]) in registers and fetches a row only when a_t advances: below rate 1 a row is
//             read once per range, above it the skipped rows are never touched. The product goes to carry[plane][c + 1][k].
//   carry     a lane per (plane, bin) multiplies the products in range order, seeded with unit(D[0]), and leaves in their
//             place the phasor at stretch_first(c) for every chunk c
//   inverse   the Wiener stage's inverse (wiener_istft_body) with the vocoder as its spectrum source: the frame loop is
//             sequential in t and each of the 256 threads owns 8 bins (thread 0 the Nyquist bin too) of both channels, so the
//             phasors of a chunk stay in registers, 2 x 9 double2 a thread, from the carry on; Y[t] is formed from the two rows
//             and handed to the loop, which writes it into the LDS image of the inverse transform. Y never exists in HBM.
// No atomics, no workgroup waits on another, every product in a fixed order: equal inputs, equal bits.
// Out of scope: phase locking and transient handling, other STFT sizes, more than 2 channels, the multi-track entry points.
#include "wiener_stft.h"
#include "stretch_plan.h"

namespace dmx
{
namespace
{
struct StretchArgs
{
    const float2 *D; // [J][C][T][kWienerRow]
    int *live;       // [J C][T]: 0 where the frame's windowed samples are all zero
    double2 *carry;  // [J C][chunks][kWienerRow]
    i64 T, plane, chunks, num, den;
    int C;
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// b conj(a)
__device__ __forceinline__ double2 cmul_conj(double2 b, double2 a) { return make_double2(b.x * a.x + b.y * a.y, b.y * a.x - b.x * a.y); }
// |z| in binary64 (the squares of fp32 values are exact there) and unit(z)
__device__ __forceinline__ double2 unit_of(float2 z, double &mag)
{
    mag = sqrt((double)z.x * z.x + (double)z.y * z.y);
    return mag > 0.0 ? make_double2(z.x / mag, z.y / mag) : make_double2(1.0, 0.0);
}
// unit(D[a][k]) of the column d = D + k of a plane whose frames' flags are `live`; rows from T on are zero
__device__ __forceinline__ double2 unit_at(const float2 *d, const int *live, i64 a, i64 T)
{
    double mag;
    return unit_of(a < T && live[a] ? d[a * kWienerRow] : make_float2(0.f, 0.f), mag);
}

// The forward kernel sends both channels of a stem through one complex transform, so a channel that is silent beside one that
// is not comes out as rounding residue with a phase of its own, where the spectrum of zeros is zero and unit(0) = 1. This
// marks the frames of a plane whose windowed samples (the forward kernel's products) are all zero; they read as zero rows.
// grid (T, J C)
__global__ __launch_bounds__(256) void stretch_live_kernel(const WienerArgs p, int *live)
{
    __shared__ int any[4];
    const i64 t = blockIdx.x, pl = blockIdx.y;
    const float *src = p.mix + pl * p.stride;
    bool nz = false;
    for (int i = threadIdx.x; i < FFT_N; i += 256)
    {
        i64 m = t * kWienerHop + i - kWienerPad; // the forward kernel's reflect padding
        if (m < 0)
            m = -m;
        if (m >= p.n)
            m = 2 * (p.n - 1) - m;
        nz |= src[m] * p.win[i] != 0.f;
    }
    const bool wave = __any(nz);
    if ((threadIdx.x & 63) == 0)
        any[threadIdx.x >> 6] = wave;
    __syncthreads();
    if (threadIdx.x == 0)
        live[pl * p.T + t] = any[0] | any[1] | any[2] | any[3];
}

// grid (chunks - 1, kWienerTiles, J), 64 C threads
__global__ __launch_bounds__(128) void stretch_products_kernel(const StretchArgs p)
{
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6, k = blockIdx.y * kWienerTile + lane;
    if (k >= kWienerBins)
        return;
    const i64 r = blockIdx.x, pl = (i64)blockIdx.z * p.C + c;
    const float2 *d = p.D + pl * p.plane + k;
    const int *live = p.live + pl * p.T;
    const i64 tBeg = stretch_first(r), tEnd = stretch_first(r + 1);
    const i64 step = p.num / p.den, frac = p.num - step * p.den; // a and the remainder move by these from frame to frame
    i64 a = tBeg * p.num / p.den, rem = tBeg * p.num - a * p.den;
    double2 ua = unit_at(d, live, a, p.T), ub = unit_at(d, live, a + 1, p.T);
    double2 prod = make_double2(1.0, 0.0);
    for (i64 t = tBeg; t < tEnd; ++t)
    {
        prod = cmul(prod, cmul_conj(ub, ua));
        i64 an = a + step;
        rem += frac;
        if (rem >= p.den)
            rem -= p.den, ++an;
        if (an != a && t + 1 < tEnd)
        {
            ua = an == a + 1 ? ub : unit_at(d, live, an, p.T);
            ub = unit_at(d, live, an + 1, p.T);
        }
        a = an;
    }
    p.carry[(pl * p.chunks + r + 1) * kWienerRow + k] = prod;
}

// grid (kWienerTiles, J C), 64 threads
__global__ __launch_bounds__(64) void stretch_carry_kernel(const StretchArgs p)
{
    const int k = blockIdx.x * kWienerTile + threadIdx.x;
    if (k >= kWienerBins)
        return;
    const i64 pl = blockIdx.y;
    double2 acc = unit_at(p.D + pl * p.plane + k, p.live + pl * p.T, 0, p.T);
    double2 *w = p.carry + pl * p.chunks * kWienerRow + k;
    w[0] = acc;
#pragma unroll 4
    for (i64 c = 1; c < p.chunks; ++c)
    {
        acc = cmul(acc, w[c * kWienerRow]);
        w[c * kWienerRow] = acc;
    }
}

// the vocoder as the spectrum source of the inverse (wiener_stft.h): the phasors of the thread's bins, from the chunk's carry on
template <int C>
struct VocoderSpectrum
{
    double2 ph[C][9];
    const float2 *d0, *row;
    const int *live;
    i64 plane, T, num, den;
    double alpha;
    bool hasA[C], hasB[C];
    __device__ VocoderSpectrum(const StretchArgs &q, int src, i64 ch, int tid)
        : d0(q.D + (i64)src * C * q.plane), row(nullptr), live(q.live + (i64)src * C * q.T), plane(q.plane), T(q.T), num(q.num), den(q.den),
          alpha(0.0)
    {
#pragma unroll
        for (int c = 0; c < C; ++c)
        {
            const double2 *w = q.carry + (((i64)src * C + c) * q.chunks + ch) * kWienerRow;
#pragma unroll
            for (int m = 0; m < 8; ++m)
                ph[c][m] = w[tid + 256 * m];
            ph[c][8] = tid == 0 ? w[2048] : make_double2(1.0, 0.0);
        }
    }
    __device__ __forceinline__ void seek(i64 t)
    {
        const i64 x = t * num, a = x / den;
        alpha = (double)(x - a * den) / (double)den;
        row = d0 + a * kWienerRow;
#pragma unroll
        for (int c = 0; c < C; ++c)
            hasA[c] = a < T && live[c * T + a], hasB[c] = a + 1 < T && live[c * T + a + 1];
    }
    __device__ __forceinline__ void bin(int m, int k, float2 &a, float2 &b)
    {
        float2 y[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
#pragma unroll
        for (int c = 0; c < C; ++c)
        {
            const float2 *r = row + c * plane + k;
            double ma, mb;
            const double2 ua = unit_of(hasA[c] ? r[0] : make_float2(0.f, 0.f), ma);
            const double2 ub = unit_of(hasB[c] ? r[kWienerRow] : make_float2(0.f, 0.f), mb);
            const double mag = (1.0 - alpha) * ma + alpha * mb;
            y[c] = make_float2((float)(mag * ph[c][m].x), (float)(mag * ph[c][m].y));
            ph[c][m] = cmul(ph[c][m], cmul_conj(ub, ua));
        }
        a = y[0], b = y[1];
    }
};

// grid (chunks, J): the inverse of wiener_stft.h on the vocoder's frames; p carries the output's geometry (n', T', chunks)
template <int C>
__global__ __launch_bounds__(256) void stretch_istft_kernel(const WienerArgs p, const StretchArgs q)
{
    VocoderSpectrum<C> spectrum(q, blockIdx.y, blockIdx.x, threadIdx.x);
    wiener_istft_body<C>(p, spectrum);
}
} // namespace

void launch_stretch(const StretchJob &job, hipStream_t s, hipEvent_t *marks)
{
    const StretchLayout l = stretch_layout(job.J, job.C, job.n, job.spec);
    WienerArgs w{}; // the forward transform: plane set j is stem j
    w.mix = job.x, w.ests = job.x + (i64)job.C * job.stride;
    w.tw = (float2 *)(job.work + l.tw), w.win = (float *)(job.work + l.win), w.fmax = (double *)(job.work + l.fmax);
    w.spec = (float2 *)(job.work + l.D);
    w.n = job.n, w.stride = job.stride, w.T = l.T, w.plane = l.plane, w.J = job.J;
    WienerArgs v{}; // the inverse: T' frames to n' samples, into `out` or, ahead of a converter, into the workspace
    const bool conv = stretch_converts(job.spec);
    v.out = conv ? (float *)(job.work + l.tmp) : job.out;
    v.tw = w.tw, v.win = w.win;
    v.n = l.n2, v.stride = conv ? l.mid : job.outStride, v.T = l.T2, v.chunks = l.chunks, v.J = job.J;
    StretchArgs a{};
    a.D = w.spec, a.live = (int *)(job.work + l.live), a.carry = (double2 *)(job.work + l.carry);
    a.T = l.T, a.plane = l.plane, a.chunks = l.chunks, a.num = job.spec.num, a.den = job.spec.den, a.C = job.C;
    Marks mark{marks, s};
    mark();
    hipLaunchKernelGGL(wiener_tables_kernel, dim3(16), dim3(256), 0, s, w.tw, w.win);
    const dim3 gs((unsigned)l.T, job.J), gi((unsigned)l.chunks, job.J);
    if (job.C == 2)
        hipLaunchKernelGGL((wiener_stft_kernel<2, false>), gs, dim3(256), 0, s, w);
    else
        hipLaunchKernelGGL((wiener_stft_kernel<1, false>), gs, dim3(256), 0, s, w);
    hipLaunchKernelGGL(stretch_live_kernel, dim3((unsigned)l.T, job.J * job.C), dim3(256), 0, s, w, a.live);
    mark();
    if (l.chunks > 1)
        hipLaunchKernelGGL(stretch_products_kernel, dim3((unsigned)(l.chunks - 1), kWienerTiles, job.J), dim3(64 * job.C), 0, s, a);
    hipLaunchKernelGGL(stretch_carry_kernel, dim3(kWienerTiles, job.J * job.C), dim3(64), 0, s, a);
    mark();
    if (job.C == 2)
        hipLaunchKernelGGL(stretch_istft_kernel<2>, gi, dim3(256), 0, s, v, a);
    else
        hipLaunchKernelGGL(stretch_istft_kernel<1>, gi, dim3(256), 0, s, v, a);
    mark();
}

} // namespace dmx
