// wiener.hip — the multichannel Wiener post-filter with EM re-estimation for gfx950 (specification: DESIGN.md section 2.19,
// restated in tests/wiener_spec.py; geometry and workspace: wiener_plan.h).
//
// Four kernels, no atomics, no workgroup waits on another, every sum in a fixed order. The tables, the forward transform
// (the mixture's workgroups also leave max |X|^2 of their frame) and the inverse are those of wiener_stft.h, shared with
// dereverb.hip; this file adds
//   wiener_em_kernel     one launch per iteration, one workgroup per (block of win_len frames, tile of 64 bins): a lane owns a
//                         bin, the four waves deal the block's frames. Pass A keeps the J (C^2 + 1) sums of the lane's bin in
//                         binary64 registers, the waves' partials meet in LDS in wave order, pass B re-reads x and y, inverts
//                         Cxx in closed form and overwrites y. The first launch forms the initial estimate (and the residual
//                         source) from X and E on the fly, in both passes, and writes y over E; the last applies the scale.
// Matrix instructions have no place here: the work is radix-16 butterflies and 2 x 2 Hermitian algebra per bin.
#include "wiener_stft.h"

namespace dmx
{

constexpr int kWS = kWienerMaxSources + 1; // sources of the EM kernel with the residual

// ------------------------------------------------------------------------------------------------ EM
// y of every source and X at (frame, bin) `off` as the complex64 values the iteration starts from. FIRST: formed from X and
// E (the estimate's magnitude with the mixture's phase, the residual X - sum, both over s, rounded), else read back.
template <int C, bool FIRST>
__device__ __forceinline__ void wiener_fetch(const WienerArgs &p, i64 off, double s, bool needX, float2 (&y)[kWS][C], float2 (&X)[C])
{
    if (FIRST || needX)
#pragma unroll
        for (int c = 0; c < C; ++c)
            X[c] = p.spec[c * p.plane + off];
    if (!FIRST)
    {
#pragma unroll
        for (int j = 0; j < kWS; ++j)
            if (j < p.S)
#pragma unroll
                for (int c = 0; c < C; ++c)
                    y[j][c] = p.spec[((1 + j) * C + c) * p.plane + off];
        return;
    }
    double phr[C], phi[C], rr[C], ri[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
    {
        const double xr = X[c].x, xi = X[c].y, a = sqrt(xr * xr + xi * xi);
        phr[c] = a > 0.0 ? xr / a : 1.0;
        phi[c] = a > 0.0 ? xi / a : 0.0;
        rr[c] = xr, ri[c] = xi;
    }
#pragma unroll
    for (int j = 0; j < kWS; ++j)
    {
        if (j < p.J)
        {
#pragma unroll
            for (int c = 0; c < C; ++c)
            {
                const float2 E = p.spec[((1 + j) * C + c) * p.plane + off];
                const double er = E.x, ei = E.y, m = sqrt(er * er + ei * ei);
                const double yr = m * phr[c], yi = m * phi[c];
                rr[c] -= yr, ri[c] -= yi;
                y[j][c] = make_float2((float)(yr / s), (float)(yi / s));
            }
        }
        else if (j == p.J && p.residual)
        {
#pragma unroll
            for (int c = 0; c < C; ++c)
                y[j][c] = make_float2((float)(rr[c] / s), (float)(ri[c] / s));
        }
    }
}

template <int C, bool FIRST>
__global__ __launch_bounds__(256) void wiener_em_kernel(const WienerArgs p)
{
    constexpr int NS = C * C + 1; // running sums of a source: a = sum |y0|^2, [d = sum |y1|^2, Re b, Im b of sum y0 conj(y1)], sum v
    __shared__ double meet[kWS * NS][64];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 blk = blockIdx.x / kWienerTiles;
    const int f = (int)(blockIdx.x % kWienerTiles) * kWienerTile + lane;
    const bool live = f < kWienerBins;
    const int fl = live ? f : kWienerBins - 1; // the lanes behind the Nyquist bin repeat its work and store nothing
    const i64 t0 = blk * p.win_len, t1 = min(p.T, t0 + p.win_len);
    const double eps = 1e-10, reg = __builtin_sqrt(1e-10);

    // the block's scale s = max(1, max |X| / 10) from the per-frame maxima the forward transform left
    double m2 = 0.0;
    for (i64 t = t0 + tid; t < t1; t += 256)
        m2 = fmax(m2, p.fmax[t]);
    m2 = wave_max(m2);
    if (lane == 0)
        red[wave] = m2;
    __syncthreads();
    const double s = fmax(1.0, sqrt(fmax(fmax(red[0], red[1]), fmax(red[2], red[3]))) / 10.0);

    float2 y[kWS][C], X[C];
    // pass A: this wave's frames of the block
    double sum[kWS][NS];
#pragma unroll
    for (int j = 0; j < kWS; ++j)
#pragma unroll
        for (int k = 0; k < NS; ++k)
            sum[j][k] = 0.0;
    for (i64 t = t0 + wave; t < t1; t += 4)
    {
        wiener_fetch<C, FIRST>(p, t * kWienerRow + fl, s, false, y, X);
#pragma unroll
        for (int j = 0; j < kWS; ++j)
            if (j < p.S)
            {
                const double ar = y[j][0].x, ai = y[j][0].y, p0 = ar * ar + ai * ai;
                if (C == 2)
                {
                    const double br = y[j][C - 1].x, bi = y[j][C - 1].y, p1 = br * br + bi * bi;
                    sum[j][0] += p0;
                    sum[j][1] += p1;
                    sum[j][2] += ar * br + ai * bi; // y0 conj(y1)
                    sum[j][3] += ai * br - ar * bi;
                    sum[j][NS - 1] += (p0 + p1) / 2.0;
                }
                else
                {
                    sum[j][0] += p0;
                    sum[j][NS - 1] += p0;
                }
            }
    }
    // the waves' partials meet in wave order: ((w0 + w1) + w2) + w3
#pragma unroll 1
    for (int w = 0; w < 4; ++w)
    {
        if (wave == w)
        {
#pragma unroll
            for (int j = 0; j < kWS; ++j)
                if (j < p.S)
#pragma unroll
                    for (int k = 0; k < NS; ++k)
                        meet[j * NS + k][lane] = w == 0 ? sum[j][k] : meet[j * NS + k][lane] + sum[j][k];
        }
        __syncthreads();
    }
    double R[kWS][NS - 1]; // R_j(f) = sum_t y y^H / (eps + sum_t v): a, [d, Re b, Im b]
#pragma unroll
    for (int j = 0; j < kWS; ++j)
        if (j < p.S)
        {
            const double den = eps + meet[j * NS + NS - 1][lane];
#pragma unroll
            for (int k = 0; k < NS - 1; ++k)
                R[j][k] = meet[j * NS + k][lane] / den;
        }

    // pass B: y_j = v_j R_j Cxx^-1 x with Cxx = sum_j v_j R_j + sqrt(eps) I
    for (i64 t = t0 + wave; t < t1; t += 4)
    {
        const i64 off = t * kWienerRow + fl;
        wiener_fetch<C, FIRST>(p, off, s, true, y, X);
        double v[kWS];
        double A = reg, D = reg, Br = 0.0, Bi = 0.0;
#pragma unroll
        for (int j = 0; j < kWS; ++j)
            if (j < p.S)
            {
                const double ar = y[j][0].x, ai = y[j][0].y, p0 = ar * ar + ai * ai;
                if (C == 2)
                {
                    const double br = y[j][C - 1].x, bi = y[j][C - 1].y, p1 = br * br + bi * bi;
                    v[j] = (p0 + p1) / 2.0;
                    D += v[j] * R[j][1 % (NS - 1)];
                    Br += v[j] * R[j][2 % (NS - 1)];
                    Bi += v[j] * R[j][3 % (NS - 1)];
                }
                else
                    v[j] = p0;
                A += v[j] * R[j][0];
            }
        double g0r, g0i, g1r = 0.0, g1i = 0.0; // g = Cxx^-1 x
        const double x0r = (double)X[0].x / s, x0i = (double)X[0].y / s;
        if (C == 2)
        {
            const double x1r = (double)X[C - 1].x / s, x1i = (double)X[C - 1].y / s;
            const double det = A * D - (Br * Br + Bi * Bi);
            // adj = [[D, -B], [-conj B, A]]
            g0r = (D * x0r - (Br * x1r - Bi * x1i)) / det;
            g0i = (D * x0i - (Br * x1i + Bi * x1r)) / det;
            g1r = (A * x1r - (Br * x0r + Bi * x0i)) / det;
            g1i = (A * x1i - (Br * x0i - Bi * x0r)) / det;
        }
        else
        {
            g0r = x0r / A;
            g0i = x0i / A;
        }
#pragma unroll
        for (int j = 0; j < kWS; ++j)
            if (j < p.S)
            {
                double u0r, u0i, u1r = 0.0, u1i = 0.0; // R_j g
                if (C == 2)
                {
                    const double a = R[j][0], d = R[j][1 % (NS - 1)], br = R[j][2 % (NS - 1)], bi = R[j][3 % (NS - 1)];
                    u0r = a * g0r + (br * g1r - bi * g1i);
                    u0i = a * g0i + (br * g1i + bi * g1r);
                    u1r = (br * g0r + bi * g0i) + d * g1r;
                    u1i = (br * g0i - bi * g0r) + d * g1i;
                }
                else
                {
                    u0r = R[j][0] * g0r;
                    u0i = R[j][0] * g0i;
                }
                float2 o0 = make_float2((float)(v[j] * u0r), (float)(v[j] * u0i));
                float2 o1 = make_float2((float)(v[j] * u1r), (float)(v[j] * u1i));
                if (p.last)
                {
                    o0 = make_float2((float)((double)o0.x * s), (float)((double)o0.y * s));
                    o1 = make_float2((float)((double)o1.x * s), (float)((double)o1.y * s));
                }
                if (live)
                {
                    p.spec[((1 + j) * C) * p.plane + off] = o0;
                    if (C == 2)
                        p.spec[((1 + j) * C + 1) * p.plane + off] = o1;
                }
            }
    }
}

void launch_wiener(const WienerJob &job, hipStream_t s, hipEvent_t *marks)
{
    const WienerLayout l = wiener_layout(job.J, job.C, job.n, job.residual, job.win_len);
    WienerArgs a{};
    a.mix = job.mix, a.ests = job.ests, a.out = job.out;
    a.tw = (float2 *)(job.work + l.tw), a.win = (float *)(job.work + l.win), a.fmax = (double *)(job.work + l.fmax);
    a.spec = (float2 *)(job.work + l.spec);
    a.ispec = a.spec + (i64)job.C * l.plane; // y of the sources: behind X
    a.n = job.n, a.stride = job.stride, a.T = l.T, a.plane = l.plane, a.chunks = l.chunks;
    a.J = job.J, a.S = job.J + (job.residual ? 1 : 0), a.residual = job.residual, a.win_len = job.win_len;
    Marks mark{marks, s};
    mark();
    hipLaunchKernelGGL(wiener_tables_kernel, dim3(16), dim3(256), 0, s, a.tw, a.win);
    const dim3 gs((unsigned)l.T, 1 + job.J), ge((unsigned)(l.blocks * kWienerTiles)), gi((unsigned)l.chunks, job.J);
    if (job.C == 2)
        hipLaunchKernelGGL(wiener_stft_kernel<2>, gs, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(wiener_stft_kernel<1>, gs, dim3(256), 0, s, a);
    mark();
    for (int it = 0; it < job.iterations; ++it)
    {
        a.first = it == 0, a.last = it == job.iterations - 1;
        if (job.C == 2 && a.first)
            hipLaunchKernelGGL((wiener_em_kernel<2, true>), ge, dim3(256), 0, s, a);
        else if (job.C == 2)
            hipLaunchKernelGGL((wiener_em_kernel<2, false>), ge, dim3(256), 0, s, a);
        else if (a.first)
            hipLaunchKernelGGL((wiener_em_kernel<1, true>), ge, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((wiener_em_kernel<1, false>), ge, dim3(256), 0, s, a);
        mark();
    }
    if (job.C == 2)
        hipLaunchKernelGGL(wiener_istft_kernel<2>, gi, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(wiener_istft_kernel<1>, gi, dim3(256), 0, s, a);
    mark();
}

} // namespace dmx
