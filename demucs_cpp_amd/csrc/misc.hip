// misc.hip — normalisation / statistics kernels and small copies for gfx950 (HBM-bound,
// wave64 shuffle reductions, fixed summation order => bit-reproducible results). The track-level kernels are in tracks.hip.
//
// Reference semantics (/root/reference):
//   layer_norm      src/layers.cpp:121-150   (UNBIASED variance, Q3: layers.hpp:76-95)
//   group_norm      src/layers.cpp:9-49      (1 group; statistics come from the producing
//                                             GEMM's per-row partials, reduced here in fp64)
//   z-norm          src/model_inference.cpp:115-124,138-144 : (x-mean)/(std+1e-5)
#include "kernels.h"

namespace dmx
{

// --------------------------------------------------------------------------- stats reduce
// rowstat [B][R][NB][2] -> out [B*G][4] = {mean, scale, std, 0}; G = max(G0,1).
// grid (ceil(G/GX), B); block 256 = GX groups x SL slices.
template <int GX>
__global__ __launch_bounds__(256) void stats_reduce_kernel(const ReduceArgs p)
{
    constexpr int SL = 256 / GX;
    __shared__ double sh[SL][GX][2];
    const int G = p.G0 > 1 ? p.G0 : 1;
    const int gx = threadIdx.x % GX, sl = threadIdx.x / GX;
    const int gi = blockIdx.x * GX + gx, b = blockIdx.y;
    double s = 0.0, q = 0.0;
    if (gi < G)
    {
        const int rowsPerGroup = (p.R - gi + G - 1) / G;
        for (int i = sl; i < rowsPerGroup; i += SL)
        {
            const int r = gi + i * G;
            const float2 *src = reinterpret_cast<const float2 *>(p.rowstat) + ((i64)b * p.R + r) * p.NB;
            for (int nb = 0; nb < p.NB; ++nb)
            {
                const float2 v = src[nb];
                s += (double)v.x;
                q += (double)v.y;
            }
        }
    }
    sh[sl][gx][0] = s;
    sh[sl][gx][1] = q;
    __syncthreads();
    if (sl == 0 && gi < G)
    {
        double S = 0.0, Q = 0.0;
        for (int i = 0; i < SL; ++i)
        {
            S += sh[i][gx][0];
            Q += sh[i][gx][1];
        }
        const double mean = S / p.count;
        double var = (Q - p.count * mean * mean) / (p.count - 1.0);
        if (var < 0.0)
            var = 0.0;
        float4 o;
        o.x = (float)mean;
        o.z = (float)sqrt(var);
        o.y = p.mode == MODE_RSTD ? (float)(1.0 / sqrt(var + (double)p.eps)) : (float)(1.0 / (sqrt(var) + (double)p.eps));
        o.w = 0.f;
        reinterpret_cast<float4 *>(p.out)[(i64)b * G + gi] = o;
    }
}

// G0 <= 1 (one group per batch element, up to 86k rows): two stages.
// stage 1: grid (nchunk, B); each workgroup sums a contiguous chunk of the [R*NB] float2 entries
__global__ __launch_bounds__(256) void stats_partial_kernel(const ReduceArgs p)
{
    __shared__ double red[4][2];
    const int b = blockIdx.y;
    const i64 entries = (i64)p.R * p.NB;
    const i64 per = (entries + p.nchunk - 1) / p.nchunk;
    const i64 lo = (i64)blockIdx.x * per, hi = lo + per < entries ? lo + per : entries;
    const float2 *src = reinterpret_cast<const float2 *>(p.rowstat) + (i64)b * entries;
    double s = 0.0, q = 0.0;
    for (i64 i = lo + threadIdx.x; i < hi; i += 256)
    {
        const float2 v = src[i];
        s += (double)v.x;
        q += (double)v.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
        s += __shfl_xor(s, off);
        q += __shfl_xor(q, off);
    }
    if ((threadIdx.x & 63) == 0)
    {
        red[threadIdx.x >> 6][0] = s;
        red[threadIdx.x >> 6][1] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double *dst = p.scratch + ((i64)b * p.nchunk + blockIdx.x) * 2;
        dst[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        dst[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    }
}
// stage 2: one wave per batch element sums the nchunk partials in index order
__global__ __launch_bounds__(64) void stats_final_kernel(const ReduceArgs p)
{
    const int b = blockIdx.x;
    if (threadIdx.x != 0)
        return;
    double S = 0.0, Q = 0.0;
    for (int i = 0; i < p.nchunk; ++i)
    {
        S += p.scratch[((i64)b * p.nchunk + i) * 2];
        Q += p.scratch[((i64)b * p.nchunk + i) * 2 + 1];
    }
    const double mean = S / p.count;
    double var = (Q - p.count * mean * mean) / (p.count - 1.0);
    if (var < 0.0)
        var = 0.0;
    float4 o;
    o.x = (float)mean;
    o.z = (float)sqrt(var);
    o.y = p.mode == MODE_RSTD ? (float)(1.0 / sqrt(var + (double)p.eps)) : (float)(1.0 / (sqrt(var) + (double)p.eps));
    o.w = 0.f;
    reinterpret_cast<float4 *>(p.out)[b] = o;
}

void launch_stats_reduce(const ReduceArgs &a, hipStream_t s)
{
    const int G = a.G0 > 1 ? a.G0 : 1;
    if (G >= 32)
        hipLaunchKernelGGL(stats_reduce_kernel<32>, dim3((G + 31) / 32, a.B), dim3(256), 0, s, a);
    else if (G > 1)
        hipLaunchKernelGGL(stats_reduce_kernel<8>, dim3((G + 7) / 8, a.B), dim3(256), 0, s, a);
    else
    {
        hipLaunchKernelGGL(stats_partial_kernel, dim3(a.nchunk, a.B), dim3(256), 0, s, a);
        hipLaunchKernelGGL(stats_final_kernel, dim3(a.B), dim3(64), 0, s, a);
    }
}

// --------------------------------------------------------------------------- LayerNorm
// one wave64 per row; two-pass (mean, then sum of squared deviations) in registers.
__global__ __launch_bounds__(256) void layernorm_kernel(const LnArgs p)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows)
        return;
    const float *x = p.x + (i64)row * p.D;
    float v[8]; // D <= 512
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
    {
        const int c = lane + i * 64;
        v[i] = c < p.D ? x[c] : 0.f;
        s += v[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        s += __shfl_xor(s, off);
    const float mean = s / (float)p.D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
    {
        const int c = lane + i * 64;
        const float d = c < p.D ? v[i] - mean : 0.f;
        q += d * d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        q += __shfl_xor(q, off);
    const float rstd = 1.0f / sqrtf(q / (float)(p.D - 1) + p.eps);
    float *y = p.y + (i64)row * p.D;
    const float *pe = p.pe ? p.pe + (i64)(row % p.rowsPerBatch) * p.D : nullptr;
#pragma unroll
    for (int i = 0; i < 8; ++i)
    {
        const int c = lane + i * 64;
        if (c < p.D)
        {
            float o = (v[i] - mean) * rstd * p.w[c] + p.b[c];
            if (pe)
                o += pe[c];
            y[c] = o;
        }
    }
}

void launch_layernorm(const LnArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(layernorm_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
}

// --------------------------------------------------------------------------- GroupNorm apply / add
__global__ __launch_bounds__(256) void gn_apply_kernel(const GnArgs p)
{
    const int b = blockIdx.y;
    const i64 per = (i64)p.rows * p.C; // multiple of 4
    float mean = 0.f, sc = 1.f;
    if (p.stats)
    {
        mean = p.stats[b * 4];
        sc = p.stats[b * 4 + 1];
    }
    const float4 *x = reinterpret_cast<const float4 *>(p.x + (i64)b * per);
    const float4 *res = p.res ? reinterpret_cast<const float4 *>(p.res + (i64)b * per) : nullptr;
    float4 *y = reinterpret_cast<float4 *>(p.y + (i64)b * per);
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < per / 4; i += (i64)gridDim.x * 256)
    {
        float4 v = x[i];
        if (p.stats)
        {
            const int c = (int)((i * 4) % p.C);
            const float4 w = *reinterpret_cast<const float4 *>(p.w + c);
            const float4 bb = *reinterpret_cast<const float4 *>(p.b + c);
            v.x = (v.x - mean) * sc * w.x + bb.x;
            v.y = (v.y - mean) * sc * w.y + bb.y;
            v.z = (v.z - mean) * sc * w.z + bb.z;
            v.w = (v.w - mean) * sc * w.w + bb.w;
        }
        if (res)
        {
            const float4 r = res[i];
            v.x += r.x, v.y += r.y, v.z += r.z, v.w += r.w;
        }
        y[i] = v;
    }
}

void launch_gn_apply(const GnArgs &a, hipStream_t s)
{
    i64 n4 = (i64)a.rows * a.C / 4;
    int gx = (int)((n4 + 255) / 256);
    if (gx > 2048)
        gx = 2048;
    hipLaunchKernelGGL(gn_apply_kernel, dim3(gx, a.B), dim3(256), 0, s, a);
}

// rows x width floats between two pitched images (packing / unpacking the segment tails the OWNER finish mode exchanges)
__global__ __launch_bounds__(256) void copy_rows_kernel(float *dst, i64 dpitch, const float *src, i64 spitch, i64 width)
{
    const i64 r = blockIdx.y;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < width; i += (i64)gridDim.x * 256)
        dst[r * dpitch + i] = src[r * spitch + i];
}
void launch_copy_rows(float *dst, i64 dpitch, const float *src, i64 spitch, i64 width, int rows, hipStream_t s)
{
    if (width <= 0 || rows <= 0)
        return;
    int gx = (int)((width + 255) / 256);
    if (gx > 1024)
        gx = 1024;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(gx, rows), dim3(256), 0, s, dst, dpitch, src, spitch, width);
}

__global__ void planar_to_interleaved_kernel(const float *src, float *dst, i64 n)
{
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x)
        reinterpret_cast<float2 *>(dst)[i] = make_float2(src[i], src[n + i]);
}
void launch_planar_to_interleaved(const float *src, float *dst, i64 n, hipStream_t s)
{
    int gx = (int)((n + 255) / 256);
    if (gx > 4096)
        gx = 4096;
    hipLaunchKernelGGL(planar_to_interleaved_kernel, dim3(gx), dim3(256), 0, s, src, dst, n);
}

__global__ void f32_to_f16_kernel(const float *src, unsigned short *dst, i64 n)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
    {
        const _Float16 h = (_Float16)src[i];
        dst[i] = __builtin_bit_cast(unsigned short, h);
    }
}
void launch_f32_to_f16(const float *src, unsigned short *dst, i64 n, hipStream_t s)
{
    if (n > 0)
        hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n);
}

} // namespace dmx
