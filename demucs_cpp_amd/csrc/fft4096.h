// fft4096.h — the 4096-point radix-16 transform in LDS that the STFT / ISTFT kernels (fft.hip) and the Wiener
// post-filter (wiener.hip) share: one text, so both families compute the same bits. Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace dmx
{

#define FFT_N 4096
#define FFT_LOG 12

// twiddle w_N^idx of the requested direction: tw[k] = exp(-2 pi i k / 4096), k < 2048; exponents in
// [2048, 4096) use w^(k) = -w^(k - 2048)
template <int SIGN>
__device__ __forceinline__ float2 fft_tw(const float2 *__restrict__ tw, int idx)
{
    float2 w = tw[idx & 2047];
    if (idx & 2048)
        w = make_float2(-w.x, -w.y);
    if (SIGN > 0)
        w.y = -w.y;
    return w;
}
__device__ __forceinline__ float2 cmul(const float2 a, const float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// LDS position of element i: a XOR swizzle of the low 4 bits with the next 4. Every access pattern of the three
// radix-16 stages below (reads x[j + 256 k] / 16-element blocks, writes y[16 p + k] / y[q + 256 p + 16 k] /
// y[j + 256 k]) then puts the 16 lanes of a ds_read/write_b64 group on 16 distinct bank pairs.
#define FSW(i) ((i) ^ (((i) >> 4) & 15))

// in place 4-point DFT X_d = sum_e w4^(e d) x_e, w4 = -i (forward) / +i (inverse)
template <int SIGN>
__device__ __forceinline__ void dft4(float2 &x0, float2 &x1, float2 &x2, float2 &x3)
{
    const float2 s02 = make_float2(x0.x + x2.x, x0.y + x2.y), d02 = make_float2(x0.x - x2.x, x0.y - x2.y);
    const float2 s13 = make_float2(x1.x + x3.x, x1.y + x3.y), d13 = make_float2(x1.x - x3.x, x1.y - x3.y);
    const float2 j13 = SIGN < 0 ? make_float2(d13.y, -d13.x) : make_float2(-d13.y, d13.x); // w4 * d13
    x0 = make_float2(s02.x + s13.x, s02.y + s13.y);
    x1 = make_float2(d02.x + j13.x, d02.y + j13.y);
    x2 = make_float2(s02.x - s13.x, s02.y - s13.y);
    x3 = make_float2(d02.x - j13.x, d02.y - j13.y);
}
template <int SIGN>
__device__ __forceinline__ float2 mulw16(const float2 v, const float c, const float sn) // v * (c + i SIGN sn)
{
    const float si = SIGN < 0 ? -sn : sn;
    return make_float2(v.x * c - v.y * si, v.x * si + v.y * c);
}

// In-LDS Stockham radix-16 FFT of FFT_N = 16^3 complex points: 3 autosort stages, every thread does ONE 16-point DFT per
// stage in registers (4 x 4 decomposition, constants w16^(c d)). Half the LDS traffic of the 6-stage radix-4 form it
// replaced. IN PLACE since round 5: a stage reads its 16 inputs into registers, all threads meet at a barrier, then the
// outputs go back into the same 32 KB image (the autosort permutation moves every element, hence the barrier between the
// reads and the writes; a second one publishes the stage). One image instead of two: 32 KB per transform, so five
// (STFT) / three (fused ISTFT, with its twiddle table) workgroups share a CU instead of two - the kernels are bound by
// the latency of their barrier-separated stages, which more resident workgroups hide (stft 0.46 -> see DESIGN.md, same bits).
// Input and result: a[FSW(i)]. sign = -1 forward (w = exp(-2 pi i p/n)), +1 inverse. tw[k] = exp(-2 pi i k / 4096), k < 2048.
// Stage with stride s (= 16^st), sub-transform length n = N/s, m = n/16, p < m, q < s:
//   y[q + s (16 p + k)] = w_n^(p k) * sum_j w16^(j k) x[q + s (p + j m)]
template <int SIGN>
__device__ __forceinline__ void fft4096(float2 *a, const float2 *__restrict__ tw, int tid)
{
    float2 *x = a, *y = a;
#pragma unroll 1
    for (int st = 0; st < FFT_LOG; st += 4)
    {
        const int s = 1 << st, m = 256 >> st;
        const int p = tid >> st, q = tid & (s - 1);
        float2 v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
        {
            const int i = q + s * (p + k * m);
            v[k] = x[FSW(i)];
        }
        // 16-point DFT: b_{c,d} = DFT4 over e of v[c + 4e] (in place -> v[c + 4d]); times w16^(c d); Y_{d + 4f} =
        // DFT4 over c (in place -> v[f + 4d])
#pragma unroll
        for (int c = 0; c < 4; ++c)
            dft4<SIGN>(v[c], v[c + 4], v[c + 8], v[c + 12]);
        v[1 + 4] = mulw16<SIGN>(v[1 + 4], 0.92387953251128674f, 0.38268343236508977f);   // w16^1
        v[2 + 4] = mulw16<SIGN>(v[2 + 4], 0.70710678118654752f, 0.70710678118654752f);   // w16^2
        v[3 + 4] = mulw16<SIGN>(v[3 + 4], 0.38268343236508977f, 0.92387953251128674f);   // w16^3
        v[1 + 8] = mulw16<SIGN>(v[1 + 8], 0.70710678118654752f, 0.70710678118654752f);   // w16^2
        v[2 + 8] = mulw16<SIGN>(v[2 + 8], 0.0f, 1.0f);                                   // w16^4
        v[3 + 8] = mulw16<SIGN>(v[3 + 8], -0.70710678118654752f, 0.70710678118654752f);  // w16^6
        v[1 + 12] = mulw16<SIGN>(v[1 + 12], 0.38268343236508977f, 0.92387953251128674f); // w16^3
        v[2 + 12] = mulw16<SIGN>(v[2 + 12], -0.70710678118654752f, 0.70710678118654752f); // w16^6
        v[3 + 12] = mulw16<SIGN>(v[3 + 12], -0.92387953251128674f, -0.38268343236508977f); // w16^9
#pragma unroll
        for (int d = 0; d < 4; ++d)
            dft4<SIGN>(v[4 * d], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3]);
        const int o = q + s * 16 * p;
        __syncthreads(); // every thread holds its inputs: the image may be overwritten
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int f = 0; f < 4; ++f)
            {
                const int k = d + 4 * f;
                float2 r = v[f + 4 * d];
                if (st < 8 && k > 0) // the last stage has p = 0
                    r = cmul(r, fft_tw<SIGN>(tw, (p * k) << st));
                const int i = o + s * k;
                y[FSW(i)] = r;
            }
        __syncthreads();
    }
}

} // namespace dmx
