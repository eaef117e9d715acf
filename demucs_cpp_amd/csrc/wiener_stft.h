// wiener_stft.h — the whole-track STFT and its inverse that the Wiener post-filter (wiener.hip) and the de-reverberation
// (dereverb.hip) share: one text, so both stages compute the same bits. nfft 4096, hop 1024, periodic Hann, centred with
// reflect padding, complex64 rows of kWienerRow elements (geometry: wiener_plan.h). Device code only.
//   wiener_tables_kernel  the twiddles and the periodic Hann window into the workspace (the stages own no context)
//   wiener_stft_kernel    one workgroup per (frame, plane set): both channels of a set share one 4096-point complex transform
//                         (fft4096.h, the routine of fft.hip); reflect padding by index arithmetic. Set 0 is `mix`, set 1 + j is
//                         `ests` + j C planes. Set 0's workgroups leave max |X|^2 of their frame in fmax[t]; with ALLMAX every
//                         set does, in fmax[set T + t]
//   wiener_istft_kernel   one workgroup per (source, chunk of frames): inverse transform of both channels of `ispec` + src C
//                         planes at once, the windowed frames go to a ring of four hops in LDS, each finished hop is divided by
//                         its window-square sum and written; the frames never reach HBM. Chunks start 3 frames early, so every
//                         hop is summed in frame order whatever the cut. Its text is wiener_istft_body, whose frame loop takes
//                         the spectrum from a source: PlainSpectrum here, the phase vocoder's in stretch.hip, the masked
//                         spectrum of hpss.hip, which also writes several kinds of output per source.
#pragma once
#include "kernels.h"
#include "fft4096.h"

namespace dmx
{
struct WienerArgs
{
    const float *mix, *ests;
    float *out;
    float2 *tw;     // [2048]
    float *win;     // [4096]
    double *fmax;   // [T]
    float2 *spec;   // [sets][C][T][kWienerRow]
    const float2 *ispec; // what the inverse reads: [sources][C][T][kWienerRow]
    i64 n, stride, T, plane, chunks;
    int J, S, residual, win_len; // S = J + residual
    int first, last;
};

static __global__ __launch_bounds__(256) void wiener_tables_kernel(float2 *tw, float *win)
{
    const int i = blockIdx.x * 256 + threadIdx.x; // < 4096
    const double c = cospi(i / 2048.0), s = sinpi(i / 2048.0);
    win[i] = (float)(0.5 - 0.5 * c);
    if (i < 2048)
        tw[i] = make_float2((float)c, (float)-s);
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmax(v, __shfl_xor(v, off));
    return v;
}

// ------------------------------------------------------------------------------------------------ forward STFT
template <int C, bool ALLMAX = false>
__global__ __launch_bounds__(256) void wiener_stft_kernel(const WienerArgs p)
{
    __shared__ float2 buf[FFT_N];
    __shared__ double red[4];
    const int tid = threadIdx.x, set = blockIdx.y;
    const i64 t = blockIdx.x;
    const float *src = set == 0 ? p.mix : p.ests + (i64)(set - 1) * C * p.stride;
    for (int i = tid; i < FFT_N; i += 256)
    {
        i64 m = t * kWienerHop + i - kWienerPad; // reflect padding: n > 2048, so one fold is enough at either end
        if (m < 0)
            m = -m;
        if (m >= p.n)
            m = 2 * (p.n - 1) - m;
        const float w = p.win[i];
        buf[FSW(i)] = make_float2(src[m] * w, C == 2 ? src[p.stride + m] * w : 0.f);
    }
    __syncthreads();
    fft4096<-1>(buf, p.tw, tid);
    float2 *o0 = p.spec + (i64)set * C * p.plane + t * kWienerRow;
    double m2 = 0.0;
    for (int k = tid; k < kWienerBins; k += 256)
    {
        const float2 zk = buf[FSW(k)];
        float2 x0 = zk, x1 = make_float2(0.f, 0.f);
        if (C == 2)
        {
            // X0 = (Z[k] + conj(Z[N-k]))/2 ; X1 = -i (Z[k] - conj(Z[N-k]))/2
            const float2 zn = buf[FSW((FFT_N - k) & (FFT_N - 1))];
            x0 = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
            x1 = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
            o0[p.plane + k] = x1;
        }
        o0[k] = x0;
        m2 = fmax(m2, fmax((double)x0.x * x0.x + (double)x0.y * x0.y, (double)x1.x * x1.x + (double)x1.y * x1.y));
    }
    if (ALLMAX || set == 0)
    {
        m2 = wave_max(m2);
        if ((tid & 63) == 0)
            red[tid >> 6] = m2;
        __syncthreads();
        if (tid == 0)
            p.fmax[(ALLMAX ? set * p.T : 0) + t] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    }
}

// ------------------------------------------------------------------------------------------------ inverse STFT + overlap-add
// The spectrum source of the inverse's frame loop: seek(f) once per frame, in ascending order, then bin(m, k, a, b) once per
// bin the thread owns (k = tid + 256 m for m = 0 .. 7; thread 0 also the Nyquist bin 2048 as m = 8, last): the two channels'
// values. m is a constant of the unrolled loop, so a source may keep a state per owned bin in registers. The plain source
// reads the rows of `ispec`. Where a stage leaves `kinds` outputs per source, the call for kind `kind` writes the planes
// (src kinds + kind) C + channel; the defaults are the one output per source of the other stages.
template <int C>
struct PlainSpectrum
{
    const float2 *y0, *r0;
    i64 plane;
    __device__ PlainSpectrum(const WienerArgs &p, int src) : y0(p.ispec + (i64)src * C * p.plane), r0(nullptr), plane(p.plane) {}
    __device__ __forceinline__ void seek(i64 f) { r0 = y0 + f * kWienerRow; }
    __device__ __forceinline__ void bin(int, int k, float2 &a, float2 &b) const
    {
        a = r0[k], b = C == 2 ? r0[plane + k] : make_float2(0.f, 0.f);
    }
};

template <int C, class Source>
__device__ __forceinline__ void wiener_istft_body(const WienerArgs &p, Source &spectrum, int kinds = 1, int kind = 0)
{
    __shared__ float2 buf[FFT_N];
    __shared__ float2 ring[FFT_N]; // the four hops that still collect frames; position (1024 f + i) & 4095, each owned by the
                                   // thread i & 255 in every frame: no barrier between the add and the emit
    __shared__ float2 twS[2048];
    const int tid = threadIdx.x, src = blockIdx.y * kinds + kind; // the first output plane is src C
    const i64 ch = blockIdx.x;
    for (int k = tid; k < 2048; k += 256)
        twS[k] = p.tw[k];
    float wreg[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        wreg[j] = p.win[tid + 256 * j];
        ring[tid + 256 * j] = make_float2(0.f, 0.f);
    }
    const i64 t0 = ch * kWienerChunk, t1 = min(p.T, t0 + kWienerChunk);
    const i64 fBeg = max((i64)0, t0 - 3), fEnd = ch == p.chunks - 1 ? p.T + 3 : t1;
    __syncthreads();
    for (i64 f = fBeg; f < fEnd; ++f)
    {
        if (f < p.T)
        {
            // Z[k] = Y0[k] + i Y1[k] with the Hermitian extension; the imaginary parts of DC and Nyquist are ignored
            spectrum.seek(f);
#pragma unroll
            for (int m = 0; m < 8; ++m)
            {
                const int k = tid + 256 * m;
                float2 a, b;
                spectrum.bin(m, k, a, b);
                if (k == 0)
                    a.y = 0.f, b.y = 0.f;
                buf[FSW(k)] = make_float2(a.x - b.y, a.y + b.x);
                if (k > 0)
                    buf[FSW(FFT_N - k)] = make_float2(a.x + b.y, b.x - a.y);
            }
            if (tid == 0)
            {
                float2 a, b;
                spectrum.bin(8, 2048, a, b);
                buf[FSW(2048)] = make_float2(a.x, b.x);
            }
            __syncthreads();
            fft4096<+1>(buf, twS, tid); // ends with a barrier
#pragma unroll
            for (int j = 0; j < 16; ++j)
            {
                const int i = tid + 256 * j;
                const float2 z = buf[FSW(i)];
                const float w = wreg[j] * (1.0f / 4096.0f); // the inverse transform's 1/n, exact
                float2 &a = ring[(int)((f * kWienerHop + i) & (FFT_N - 1))];
                a.x += z.x * w;
                a.y += z.y * w;
            }
        }
        // hop f has its last frame: divide by the window-square sum over the frames that exist, crop, write, clear
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
        {
            const i64 n = f * kWienerHop + tid + 256 * jj, i = n - kWienerPad;
            float2 &a = ring[(int)(n & (FFT_N - 1))];
            if (f >= t0 && i >= 0 && i < p.n)
            {
                float wss = 0.f;
#pragma unroll
                for (int m = 3; m >= 0; --m) // frame f - m, in frame order
                    if (f - m >= 0 && f - m < p.T)
                        wss += wreg[jj + 4 * m] * wreg[jj + 4 * m];
                p.out[(i64)(src * C) * p.stride + i] = a.x / wss;
                if (C == 2)
                    p.out[(i64)(src * C + 1) * p.stride + i] = a.y / wss;
            }
            a = make_float2(0.f, 0.f);
        }
        __syncthreads(); // the image is rewritten by the next frame's spectrum
    }
}

template <int C>
__global__ __launch_bounds__(256) void wiener_istft_kernel(const WienerArgs p)
{
    PlainSpectrum<C> spectrum(p, blockIdx.y);
    wiener_istft_body<C>(p, spectrum);
}

} // namespace dmx
