// dereverb.hip — Weighted Prediction Error de-reverberation of stems for gfx950 (specification: DESIGN.md section 2.21,
// restated in tests/dereverb_spec.py; geometry and workspace: dereverb_plan.h). The transforms are the Wiener stage's
// (wiener_stft.h) with the J stems as the plane sets; the WPE core is binary64. No atomics, no workgroup waits on another,
// every sum in a fixed order: equal inputs, equal bits.
//   peak    one workgroup per stem: the largest |Y|^2 from the per-frame maxima the forward transform left (floor = eps peak;
//           a stem whose peak is 0 is skipped by every kernel below and comes out as zeros)
//   lam0    lam of the first iteration, from Y
//   corr    one workgroup per (tile of 8 adjacent bins, range of frames, stem), a wave per bin. With the complex vectors
//           embedded as reals, S(t) = [Re Yt; Im Yt; Re Y; Im Y] (2 M + 2 C rows, padded to NT tiles of 16), the real symmetric
//           S diag(1 / lam) S^T carries R and P. It runs on v_mfma_f64_16x16x4_f64 with t as the K dimension: lane (lo, hi) gives
//           row 16 I + lo at frame t + hi as the A operand of tile row I and the same value times 1 / lam(t + hi) as the B
//           operand of tile column I; the NT (NT + 1) / 2 tiles on and below the diagonal keep their accumulators in registers
//           over the whole range. The frames [t - D - K + 1, t + 64) of the 8 bins sit in LDS as [frame][bin][channel][re | im]
//           floats; the K delayed copies are the Toeplitz view of that slab, read with overlapping addresses: row (part, k, c)
//           of frame t is the float at pitch (t - D - k) + 2 C bin + 2 c + part. Each range leaves its tiles as they lie in
//           the registers.
//   solve   one wave per (bin, stem): the ranges' partials meet in range order as the entries of the Hermitian R (lower
//           triangle, in LDS) and of P are formed; diagonal loading; right-looking Cholesky, a row per lane and the trailing
//           columns dealt to the two half waves; the two substitutions run in registers, lane (c, i) holds row i of right-hand
//           side c and the pivot row's value goes round by a lane shuffle
//   filter  one workgroup per (tile of 8 bins, 64 frames, stem): Z = Y - G^H Yt from the same slab with G in LDS, a thread per
//           (frame, bin), on the vector ALU (the output is 2 C rows wide: an MFMA tile would be 3 / 4 padding or more). Writes
//           lam of the next iteration from the binary64 Z; the last launch writes Z as complex64 instead, to planes of its own
#include "wiener_stft.h"

namespace dmx
{
namespace
{
typedef double v4d __attribute__((ext_vector_type(4)));

// D = A (16 x 4) B (4 x 16) + C. Lane l gives A[l % 16][l / 16] and B[l / 16][l % 16] and holds D[4 r + l / 16][l % 16] in element r
__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

struct DrvArgs
{
    const float2 *Y; // [J][C][T][kWienerRow]
    float2 *Z;
    double *lam;     // [J][T][kWienerRow]
    double *part;    // [J][bins][ranges][lower][4][64]
    double2 *G;      // [J][bins][M][C]
    const double *fmax;
    double *peak;    // [J]
    i64 T, plane, range;
    int ranges, C, K, D, M, lower, last;
    double eps, reg;
};

__global__ __launch_bounds__(256) void dereverb_peak_kernel(const DrvArgs p)
{
    __shared__ double red[4];
    const int tid = threadIdx.x, j = blockIdx.x;
    double m = 0.0;
    for (i64 t = tid; t < p.T; t += 256)
        m = fmax(m, p.fmax[j * p.T + t]);
    m = wave_max(m);
    if ((tid & 63) == 0)
        red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0)
        p.peak[j] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// grid (T, J)
__global__ __launch_bounds__(256) void dereverb_lam0_kernel(const DrvArgs p)
{
    const int j = blockIdx.y;
    const i64 t = blockIdx.x;
    const double peak = p.peak[j];
    if (peak == 0.0)
        return;
    const double floor = p.eps * peak;
    const float2 *y = p.Y + (i64)j * p.C * p.plane + t * kWienerRow;
    for (int f = threadIdx.x; f < kWienerBins; f += 256)
    {
        double s = 0.0;
        for (int c = 0; c < p.C; ++c)
        {
            const float2 v = y[c * p.plane + f];
            s += (double)v.x * v.x + (double)v.y * v.y;
        }
        p.lam[(i64)j * p.plane + t * kWienerRow + f] = fmax(s / p.C, floor);
    }
}

// The slab of a tile of bins: frames [t0 - halo, t0 + frames) as rows of kDrvPitch floats, zero outside [0, T) and behind the
// Nyquist bin. Every thread of the workgroup (NTHR of them) takes part.
template <int NTHR>
__device__ __forceinline__ void dereverb_stage(const DrvArgs &p, float *slab, int j, int f0, i64 t0, int halo, int frames, int tid)
{
    const int C = p.C, per = kDrvBinTile * C;
    for (int e = tid; e < (frames + halo) * per; e += NTHR)
    {
        const int i = e / per, c = (e % per) / kDrvBinTile, b = e % kDrvBinTile;
        const i64 t = t0 - halo + i;
        float2 v = make_float2(0.f, 0.f);
        if (t >= 0 && t < p.T && f0 + b < kWienerBins)
            v = p.Y[((i64)j * C + c) * p.plane + t * kWienerRow + f0 + b];
        float *d = slab + i * kDrvPitch + (b * C + c) * 2;
        d[0] = v.x, d[1] = v.y;
    }
}

// ------------------------------------------------------------------------------------------------ correlation
// grid (kDrvBinTiles, ranges, J), 8 waves
template <int NT>
__global__ __launch_bounds__(512) void dereverb_corr_kernel(const DrvArgs p)
{
    __shared__ float slab[kDrvSlabRows * kDrvPitch];
    __shared__ double winv[kDrvSlab][kDrvBinTile]; // 1 / lam, 0 behind the range
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const int j = blockIdx.z, f0 = blockIdx.x * kDrvBinTile;
    if (p.peak[j] == 0.0)
        return;
    const int C = p.C, M = p.M, halo = p.D + p.K - 1;
    const i64 r0 = blockIdx.y * p.range, r1 = min(p.T, r0 + p.range);

    // where row 16 I + lo of S(t) lies relative to the slab row of frame t: [Re Yt; Im Yt; Re Y; Im Y], row (k, c) of Yt is
    // Y_c(t - D - k); the rows behind 2 M + 2 C are zero
    int off[NT];
    double keep[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I)
    {
        const int r = 16 * I + lo;
        off[I] = 0, keep[I] = 1.0;
        if (r < 2 * M)
            off[I] = (halo - p.D - (r % M) / C) * kDrvPitch + (wave * C + (r % M) % C) * 2 + r / M;
        else if (r < 2 * M + 2 * C)
            off[I] = halo * kDrvPitch + (wave * C + (r - 2 * M) % C) * 2 + (r - 2 * M) / C;
        else
            keep[I] = 0.0;
    }
    v4d acc[NT * (NT + 1) / 2];
#pragma unroll
    for (int q = 0; q < NT * (NT + 1) / 2; ++q)
        acc[q] = v4d{0.0, 0.0, 0.0, 0.0};

    for (i64 s0 = r0; s0 < r1; s0 += kDrvSlab)
    {
        dereverb_stage<512>(p, slab, j, f0, s0, halo, kDrvSlab, tid);
        {
            const int tt = tid >> 3, b = tid & 7; // 64 frames x 8 bins
            const i64 t = s0 + tt;
            winv[tt][b] = t < r1 && f0 + b < kWienerBins ? 1.0 / p.lam[(i64)j * p.plane + t * kWienerRow + f0 + b] : 0.0;
        }
        __syncthreads();
        const int lim = (int)min((i64)kDrvSlab, (r1 - s0 + 3) & ~(i64)3);
        for (int tt = 0; tt < lim; tt += 4)
        {
            const double w = winv[tt + hi][wave];
            double a[NT], b[NT];
#pragma unroll
            for (int I = 0; I < NT; ++I)
            {
                a[I] = (double)slab[off[I] + (tt + hi) * kDrvPitch] * keep[I];
                b[I] = a[I] * w;
            }
#pragma unroll
            for (int I = 0; I < NT; ++I)
#pragma unroll
                for (int Jt = 0; Jt <= I; ++Jt)
                    acc[I * (I + 1) / 2 + Jt] = mfma_f64(a[I], b[Jt], acc[I * (I + 1) / 2 + Jt]);
        }
        __syncthreads(); // the slab is rewritten by the next sweep
    }
    const int f = f0 + wave;
    if (f >= kWienerBins)
        return;
    double *out = p.part + (((i64)j * kWienerBins + f) * p.ranges + blockIdx.y) * p.lower * 256;
#pragma unroll
    for (int q = 0; q < NT * (NT + 1) / 2; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            out[q * 256 + r * 64 + lane] = acc[q][r];
}

// ------------------------------------------------------------------------------------------------ solve
// grid (kWienerBins, J), one wave
__global__ __launch_bounds__(64) void dereverb_solve_kernel(const DrvArgs p)
{
    __shared__ double2 A[32][33]; // the lower triangle of R, then of its Cholesky factor below the diagonal
    __shared__ double diag[32];   // the factor's diagonal
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int f = blockIdx.x, j = blockIdx.y, M = p.M, C = p.C;
    if (p.peak[j] == 0.0)
        return;
    const double *pt = p.part + ((i64)j * kWienerBins + f) * p.ranges * p.lower * 256;
    // entry (a, b), a >= b, of S diag(1 / lam) S^T: the ranges' partials in range order
    auto T = [&](int a, int b) {
        const int o = ((a >> 4) * ((a >> 4) + 1) / 2 + (b >> 4)) * 256 + ((a & 15) >> 2) * 64 + (a & 3) * 16 + (b & 15);
        double s = 0.0;
        for (int r = 0; r < p.ranges; ++r)
            s += pt[(i64)r * p.lower * 256 + o];
        return s;
    };
    // R(m, n) = sum Yt_m conj(Yt_n) / lam, m >= n
    for (int e = lane; e < M * M; e += 64)
    {
        const int m = e / M, n = e % M;
        if (n <= m)
            A[m][n] = make_double2(T(m, n) + T(M + m, M + n), T(M + m, n) - T(M + n, m));
    }
    // P(m, c) = sum Yt_m conj(Y_c) / lam: row i of right-hand side h in this lane
    double2 b = make_double2(0.0, 0.0);
    if (i < M && h < C)
        b = make_double2(T(2 * M + h, i) + T(2 * M + C + h, M + i), T(2 * M + h, M + i) - T(2 * M + C + h, i));
    __syncthreads();
    double tr = 0.0;
    for (int m = 0; m < M; ++m)
        tr += A[m][m].x;
    __syncthreads();
    if (lane < M)
        A[lane][lane].x += p.reg * tr / M;
    for (int c = 0; c < M; ++c)
    {
        __syncthreads();
        const double d = sqrt(A[c][c].x);
        if (h == 0 && i > c && i < M)
            A[i][c] = make_double2(A[i][c].x / d, A[i][c].y / d);
        if (lane == 0)
            diag[c] = d;
        __syncthreads();
        if (i > c && i < M)
        {
            const double2 u = A[i][c];
            for (int k = c + 1 + h; k <= i; k += 2) // A[i][k] -= L[i][c] conj(L[k][c])
            {
                const double2 v = A[k][c];
                A[i][k] = make_double2(A[i][k].x - (u.x * v.x + u.y * v.y), A[i][k].y - (u.y * v.x - u.x * v.y));
            }
        }
    }
    __syncthreads();
    for (int k = 0; k < M; ++k) // L y = P
    {
        const double d = diag[k];
        const double2 y = make_double2(__shfl(b.x, (lane & 32) + k) / d, __shfl(b.y, (lane & 32) + k) / d);
        if (i == k)
            b = y;
        else if (i > k && i < M)
        {
            const double2 l = A[i][k];
            b = make_double2(b.x - (l.x * y.x - l.y * y.y), b.y - (l.x * y.y + l.y * y.x));
        }
    }
    for (int k = M - 1; k >= 0; --k) // L^H g = y
    {
        const double d = diag[k];
        const double2 g = make_double2(__shfl(b.x, (lane & 32) + k) / d, __shfl(b.y, (lane & 32) + k) / d);
        if (i == k)
            b = g;
        else if (i < k)
        {
            const double2 l = A[k][i]; // conj(l) g
            b = make_double2(b.x - (l.x * g.x + l.y * g.y), b.y - (l.x * g.y - l.y * g.x));
        }
    }
    if (i < M && h < C)
        p.G[(((i64)j * kWienerBins + f) * M + i) * C + h] = b;
}

// ------------------------------------------------------------------------------------------------ filter
// grid (kDrvBinTiles, ceil(T / kDrvFilterFrames), J)
__global__ __launch_bounds__(256) void dereverb_filter_kernel(const DrvArgs p)
{
    constexpr int kRows = kDrvFilterFrames + kDrvMaxDelay + kDrvMaxTaps - 1;
    __shared__ float slab[kRows * kDrvPitch];
    __shared__ double2 Gs[kDrvBinTile][2 * kDrvMaxTaps * 2 + 1]; // [bin][m C + c], a pitch that spreads the bins over the banks
    const int tid = threadIdx.x, b = tid & 7, j = blockIdx.z, f0 = blockIdx.x * kDrvBinTile, f = f0 + b;
    const int C = p.C, M = p.M, halo = p.D + p.K - 1;
    const i64 t0 = (i64)blockIdx.y * kDrvFilterFrames;
    const double peak = p.peak[j];
    if (peak != 0.0)
    {
        dereverb_stage<256>(p, slab, j, f0, t0, halo, kDrvFilterFrames, tid);
        for (int e = tid; e < kDrvBinTile * M * C; e += 256)
        {
            const int bb = e / (M * C), r = e % (M * C);
            Gs[bb][r] = f0 + bb < kWienerBins ? p.G[((i64)j * kWienerBins + f0 + bb) * M * C + r] : make_double2(0.0, 0.0);
        }
        __syncthreads();
    }
    if (f >= kWienerBins)
        return;
    const double floor = p.eps * peak;
    for (int tt = tid >> 3; tt < kDrvFilterFrames; tt += 32)
    {
        const i64 t = t0 + tt;
        if (t >= p.T)
            break;
        double zr[2] = {0.0, 0.0}, zi[2] = {0.0, 0.0};
        if (peak != 0.0)
        {
            const float *now = slab + (tt + halo) * kDrvPitch + b * C * 2;
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (c < C)
                    zr[c] = now[2 * c], zi[c] = now[2 * c + 1];
            for (int k = 0; k < p.K; ++k)
            {
                const float *past = now - (p.D + k) * kDrvPitch;
                for (int c2 = 0; c2 < C; ++c2)
                {
                    const double yr = past[2 * c2], yi = past[2 * c2 + 1];
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        if (c < C)
                        {
                            const double2 g = Gs[b][(k * C + c2) * C + c]; // z_c -= conj(g) y
                            zr[c] -= g.x * yr + g.y * yi;
                            zi[c] -= g.x * yi - g.y * yr;
                        }
                }
            }
        }
        if (p.last)
        {
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (c < C)
                    p.Z[((i64)j * C + c) * p.plane + t * kWienerRow + f] = make_float2((float)zr[c], (float)zi[c]);
        }
        else if (peak != 0.0)
        {
            const double s = (zr[0] * zr[0] + zi[0] * zi[0]) + (zr[1] * zr[1] + zi[1] * zi[1]);
            p.lam[(i64)j * p.plane + t * kWienerRow + f] = fmax(s / C, floor);
        }
    }
}

template <int NT>
void corr(const DrvArgs &a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL(dereverb_corr_kernel<NT>, grid, dim3(512), 0, s, a);
}
} // namespace

void launch_dereverb(const DereverbJob &job, hipStream_t s, hipEvent_t *marks)
{
    const DrvLayout l = dereverb_layout(job.J, job.C, job.n, job.spec.taps);
    WienerArgs w{};
    w.mix = job.x, w.ests = job.x + (i64)job.C * job.stride, w.out = job.out; // plane set j is stem j
    w.tw = (float2 *)(job.work + l.tw), w.win = (float *)(job.work + l.win), w.fmax = (double *)(job.work + l.fmax);
    w.spec = (float2 *)(job.work + l.Y), w.ispec = (const float2 *)(job.work + l.Z);
    w.n = job.n, w.stride = job.stride, w.T = l.T, w.plane = l.plane, w.chunks = l.chunks, w.J = job.J;
    DrvArgs a{};
    a.Y = w.spec, a.Z = (float2 *)(job.work + l.Z), a.lam = (double *)(job.work + l.lam), a.part = (double *)(job.work + l.part);
    a.G = (double2 *)(job.work + l.G), a.fmax = w.fmax, a.peak = (double *)(job.work + l.peak);
    a.T = l.T, a.plane = l.plane, a.range = l.range, a.ranges = (int)l.ranges;
    a.C = job.C, a.K = job.spec.taps, a.D = job.spec.delay, a.M = l.M, a.lower = l.lower;
    a.eps = job.spec.eps, a.reg = job.spec.reg;
    Marks mark{marks, s};
    mark();
    hipLaunchKernelGGL(wiener_tables_kernel, dim3(16), dim3(256), 0, s, w.tw, w.win);
    const dim3 gs((unsigned)l.T, job.J), gi((unsigned)l.chunks, job.J);
    if (job.C == 2)
        hipLaunchKernelGGL((wiener_stft_kernel<2, true>), gs, dim3(256), 0, s, w);
    else
        hipLaunchKernelGGL((wiener_stft_kernel<1, true>), gs, dim3(256), 0, s, w);
    hipLaunchKernelGGL(dereverb_peak_kernel, dim3(job.J), dim3(256), 0, s, a);
    hipLaunchKernelGGL(dereverb_lam0_kernel, gs, dim3(256), 0, s, a);
    mark();
    const dim3 gc(kDrvBinTiles, (unsigned)l.ranges, job.J), gv(kWienerBins, job.J);
    const dim3 gf(kDrvBinTiles, (unsigned)((l.T + kDrvFilterFrames - 1) / kDrvFilterFrames), job.J);
    for (int it = 0; it < job.spec.iterations; ++it)
    {
        a.last = it == job.spec.iterations - 1;
        switch (l.nt)
        {
        case 1: corr<1>(a, gc, s); break;
        case 2: corr<2>(a, gc, s); break;
        case 3: corr<3>(a, gc, s); break;
        case 4: corr<4>(a, gc, s); break;
        default: corr<5>(a, gc, s); break;
        }
        hipLaunchKernelGGL(dereverb_solve_kernel, gv, dim3(64), 0, s, a);
        hipLaunchKernelGGL(dereverb_filter_kernel, gf, dim3(256), 0, s, a);
        mark();
    }
    if (job.C == 2)
        hipLaunchKernelGGL(wiener_istft_kernel<2>, gi, dim3(256), 0, s, w);
    else
        hipLaunchKernelGGL(wiener_istft_kernel<1>, gi, dim3(256), 0, s, w);
    mark();
}

} // namespace dmx
