// pcm.hip — the output stage behind the track path: finished fp32 stems in HBM -> the bytes of a WAV `data` chunk
// (demucs's --two-stems, --clip-mode and --int24 / --float32; the reference writes float32 only, cli-apps/demucs.cpp:100-102,
// so there is no reference arithmetic: the specification is this project's own, DESIGN.md section 2.8, restated in NumPy in
// tests/pcm_spec.py).
//
// Everything is fp32 and no product feeds an addition, so contraction cannot change a bit:
//   outputs  stem < 0: the S stems. Else output 0 = v[stem], output 1 = the other stems added in increasing order,
//            starting from the first of them;
//   peak     per output, the largest |x| over both channels and all frames, NaN ignored (x > m is false for a NaN);
//   clip     none: y = x;  clamp: y = x < -0.99f ? -0.99f : x > 0.99f ? 0.99f : x (a NaN stays one);
//            rescale: d = max(1.01f * peak, 1.0f), y = x / d, correctly rounded (v_div_scale / v_div_fmas / v_div_fixup);
//   encode   F32: y;  S16: rint(y * 32768.0f);  S24: rint(y * 8388608.0f), ties to even, saturated, NaN -> 0;
//            interleaved L0 R0 L1 R1 ..., little-endian, 24 bit packed in 3 bytes.
// Both kernels are HBM-bound: one lane takes 4 consecutive frames of one output, reads each plane it needs as one
// 16-byte load when that plane's base is 16-byte aligned (planes are n-strided and n is arbitrary, so this is decided per
// plane) and as four dword loads otherwise, and stores 16 (S16), 24 (S24) or 32 (F32) bytes as whole dwords. The last
// group of a track may hold 1-3 frames: the same lane takes the scalar edge path (guarded loads, dword stores; a 24-bit
// track of odd length ends in two zero bytes of the output's padding).
//
// The remix pair (dmx_remix_spec; DESIGN.md section 2.10, restated in tests/remix_spec.py) shares everything above but the
// gather: output o is a row of gains over the S stems and the mixture (the caller's track, interleaved, un-normalised).
// Sources are visited in increasing index, a source with gain 0 is NOT read (a uniform branch: the table sits in the kernel
// arguments), the first visited source gives a = g * x and each later one p = g * x, a = a + p - every product and every sum
// its own correctly rounded fp32 operation. hipcc contracts device code by default, so the gather is compiled with
// contraction off (remix_acc, pcm_gather.h); no fused multiply-add may appear in it. The mixture's 4 frames are 32 contiguous
// bytes: two 16-byte loads when aligned, dword loads otherwise and in the edge group.
#include "kernels.h"
#include "pcm_gather.h"

#include "../../include/demucs_hip.h"

#include <algorithm>
#include <cstdint>

namespace dmx
{
namespace
{
__device__ __forceinline__ int pcm_quant(float y, float scale, float lo, float hi)
{
    float t = rintf(y * scale); // v_rndne_f32: ties to even
    t = t != t ? 0.0f : t;
    t = t < lo ? lo : t;
    t = t > hi ? hi : t;
    return (int)t;
}

template <class Table, class Gather>
__device__ __forceinline__ void pcm_peak_body(const Table &t, const Gather &gather)
{
    const auto &pc = t.p[blockIdx.z];
    const int o = blockIdx.y;
    const i64 g0 = pc.i0 >> 2, g1 = (pc.i1 + 3) >> 2;
    float m = 0.0f;
    for (i64 g = g0 + (i64)blockIdx.x * 256 + threadIdx.x; g < g1; g += (i64)gridDim.x * 256)
    {
        const i64 i = g << 2;
        const int cnt = pc.i1 - i < 4 ? (int)(pc.i1 - i) : 4;
        float L[4], R[4];
        gather(pc, o, i, cnt, L, R);
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const float a = fabsf(L[k]), b = fabsf(R[k]); // the padding of a short group is 0: no effect on a maximum
            m = a > m ? a : m;
            m = b > m ? b : m;
        }
    }
    // non-negative floats order as their bit patterns: reduce those (wave64 shuffles, then LDS over the 4 waves)
    unsigned u = __float_as_uint(m);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
    {
        const unsigned v = (unsigned)__shfl_xor((int)u, off, 64);
        u = v > u ? v : u;
    }
    __shared__ unsigned wmax[4];
    if ((threadIdx.x & 63) == 0)
        wmax[threadIdx.x >> 6] = u;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < 4; ++w)
            u = wmax[w] > u ? wmax[w] : u;
        if (u)
            atomicMax(pc.peaks + o, u);
    }
}

// GAIN (the loudness stage): the gathered value is multiplied by the output's gain pc.gains[o], one
// fp32 product per sample, before clip; pc.peaks[o] then holds the peak of the gained samples (loud_gain_kernel). GAIN == 2 (the
// limiter): that product is multiplied by the frame's gain from the plane pc.gplane, a second fp32
// product; pc.peaks[o] then holds the peak of the limited samples
template <int ENC, int GAIN = 0, class Table, class Gather>
__device__ __forceinline__ void pcm_encode_body(const Table &t, int clip, const Gather &gather)
{
    const auto &pc = t.p[blockIdx.z];
    const int o = blockIdx.y;
    const i64 g0 = pc.i0 >> 2, g1 = (pc.i1 + 3) >> 2;
    float d = 1.0f;
    if (clip == DMX_CLIP_RESCALE)
    {
        const float dd = 1.01f * __uint_as_float(pc.peaks[o]);
        d = dd > 1.0f ? dd : 1.0f;
    }
    const int frameBytes = ENC == DMX_PCM_F32 ? 8 : ENC == DMX_PCM_S16 ? 4 : 6;
    unsigned char *outBase = pc.pcm + (i64)o * pc.outStride;
    for (i64 g = g0 + (i64)blockIdx.x * 256 + threadIdx.x; g < g1; g += (i64)gridDim.x * 256)
    {
        const i64 i = g << 2;
        const int cnt = pc.i1 - i < 4 ? (int)(pc.i1 - i) : 4;
        float L[4], R[4];
        gather(pc, o, i, cnt, L, R);
        float y[8];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            y[2 * k] = L[k], y[2 * k + 1] = R[k];
        if constexpr (GAIN != 0)
        {
            const float gn = pc.gains[o];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                y[k] = gn * y[k];
        }
        if constexpr (GAIN == 2)
        {
            float gl[4];
            pcm_load4(pc.gplane + (i64)o * pc.gplaneStride, i, cnt, gl);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                y[k] = y[k] * gl[k >> 1];
        }
        if (clip == DMX_CLIP_CLAMP)
        {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                y[k] = y[k] < -0.99f ? -0.99f : (y[k] > 0.99f ? 0.99f : y[k]);
        }
        else if (clip == DMX_CLIP_RESCALE)
        {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                y[k] = y[k] / d;
        }
        // the group's dwords (8 for F32, 4 for S16, 6 for S24)
        unsigned w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ENC == DMX_PCM_F32)
        {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                w[k] = __float_as_uint(y[k]);
        }
        else if (ENC == DMX_PCM_S16)
        {
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const unsigned l = (unsigned)pcm_quant(y[2 * k], 32768.0f, -32768.0f, 32767.0f) & 0xffffu;
                const unsigned r = (unsigned)pcm_quant(y[2 * k + 1], 32768.0f, -32768.0f, 32767.0f) & 0xffffu;
                w[k] = l | (r << 16);
            }
        }
        else
        {
            unsigned q[8];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                q[k] = (unsigned)pcm_quant(y[k], 8388608.0f, -8388608.0f, 8388607.0f) & 0xffffffu;
#pragma unroll
            for (int h = 0; h < 2; ++h) // four 24-bit samples are three dwords
            {
                w[3 * h] = q[4 * h] | (q[4 * h + 1] << 24);
                w[3 * h + 1] = (q[4 * h + 1] >> 8) | (q[4 * h + 2] << 16);
                w[3 * h + 2] = (q[4 * h + 2] >> 16) | (q[4 * h + 3] << 8);
            }
        }
        unsigned char *dst = outBase + i * frameBytes; // 16-byte aligned for F32 and S16, 8-byte aligned for S24
        if (cnt == 4)
        {
            if (ENC == DMX_PCM_F32)
            {
                reinterpret_cast<uint4 *>(dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
                reinterpret_cast<uint4 *>(dst)[1] = make_uint4(w[4], w[5], w[6], w[7]);
            }
            else if (ENC == DMX_PCM_S16)
                reinterpret_cast<uint4 *>(dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
            else
            {
                reinterpret_cast<uint2 *>(dst)[0] = make_uint2(w[0], w[1]);
                reinterpret_cast<uint2 *>(dst)[1] = make_uint2(w[2], w[3]);
                reinterpret_cast<uint2 *>(dst)[2] = make_uint2(w[4], w[5]);
            }
        }
        else
        {
            // edge: the dwords that hold the cnt valid frames (the samples past them were formed from zeros: they encode as 0)
            const int nd = (cnt * frameBytes + 3) >> 2;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < nd)
                    reinterpret_cast<unsigned *>(dst)[k] = w[k];
        }
    }
}

} // namespace

// grid (blocks, nOut, pieces), block 256
__global__ __launch_bounds__(256) void pcm_peak_kernel(PcmTable t, int S, int stem) { pcm_peak_body(t, GatherStems{S, stem}); }
template <int ENC>
__global__ __launch_bounds__(256) void pcm_encode_kernel(PcmTable t, int S, int stem, int clip)
{
    pcm_encode_body<ENC>(t, clip, GatherStems{S, stem});
}
// the same under a gain table: grid (blocks, G.nOut, pieces)
__global__ __launch_bounds__(256) void remix_peak_kernel(RemixTable t, PcmGains G) { pcm_peak_body(t, GatherRemix{G}); }
template <int ENC>
__global__ __launch_bounds__(256) void remix_encode_kernel(RemixTable t, PcmGains G, int clip)
{
    pcm_encode_body<ENC>(t, clip, GatherRemix{G});
}
// the remix encode behind a per-output gain read from device memory: grid (blocks, G.nOut, pieces)
template <int ENC>
__global__ __launch_bounds__(256) void loud_encode_kernel(LoudTable t, PcmGains G, int clip)
{
    pcm_encode_body<ENC, 1>(t, clip, GatherRemix{G});
}
// and behind the limiter's gain plane: grid (blocks, G.nOut, pieces)
template <int ENC>
__global__ __launch_bounds__(256) void limit_encode_kernel(LimitTable t, PcmGains G, int clip)
{
    pcm_encode_body<ENC, 2>(t, clip, GatherRemix{G});
}

namespace
{
template <class Table, class Piece, class F>
void pcm_for_tables(const Piece *pieces, int P, F launch)
{
    for (int p0 = 0; p0 < P; p0 += Table::kMax)
    {
        Table t{};
        int nt = 0;
        i64 span = 0;
        for (int k = p0; k < P && k < p0 + Table::kMax; ++k)
        {
            if (pieces[k].i1 <= pieces[k].i0)
                continue;
            t.p[nt++] = pieces[k];
            span = std::max(span, pieces[k].i1 - pieces[k].i0);
        }
        if (!nt)
            continue;
        const i64 groups = (span + 3) / 4;
        launch(t, nt, (int)std::min<i64>(2048, (groups + 255) / 256));
    }
}
} // namespace

void launch_pcm_peak(const PcmPiece *pieces, int P, int S, int stem, hipStream_t s)
{
    const int nOut = stem < 0 ? S : 2;
    pcm_for_tables<PcmTable>(pieces, P, [&](const PcmTable &t, int nt, int gx) {
        hipLaunchKernelGGL(pcm_peak_kernel, dim3(gx, nOut, nt), dim3(256), 0, s, t, S, stem);
    });
}
void launch_pcm_encode(const PcmPiece *pieces, int P, int S, int stem, int encoding, int clip, hipStream_t s)
{
    const int nOut = stem < 0 ? S : 2;
    pcm_for_tables<PcmTable>(pieces, P, [&](const PcmTable &t, int nt, int gx) {
        if (encoding == DMX_PCM_F32)
            hipLaunchKernelGGL(pcm_encode_kernel<DMX_PCM_F32>, dim3(gx, nOut, nt), dim3(256), 0, s, t, S, stem, clip);
        else if (encoding == DMX_PCM_S16)
            hipLaunchKernelGGL(pcm_encode_kernel<DMX_PCM_S16>, dim3(gx, nOut, nt), dim3(256), 0, s, t, S, stem, clip);
        else
            hipLaunchKernelGGL(pcm_encode_kernel<DMX_PCM_S24>, dim3(gx, nOut, nt), dim3(256), 0, s, t, S, stem, clip);
    });
}

void launch_remix_peak(const RemixPiece *pieces, int P, const PcmGains &G, hipStream_t s)
{
    pcm_for_tables<RemixTable>(pieces, P, [&](const RemixTable &t, int nt, int gx) {
        hipLaunchKernelGGL(remix_peak_kernel, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G);
    });
}
void launch_remix_encode(const RemixPiece *pieces, int P, const PcmGains &G, int encoding, int clip, hipStream_t s)
{
    pcm_for_tables<RemixTable>(pieces, P, [&](const RemixTable &t, int nt, int gx) {
        if (encoding == DMX_PCM_F32)
            hipLaunchKernelGGL(remix_encode_kernel<DMX_PCM_F32>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
        else if (encoding == DMX_PCM_S16)
            hipLaunchKernelGGL(remix_encode_kernel<DMX_PCM_S16>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
        else
            hipLaunchKernelGGL(remix_encode_kernel<DMX_PCM_S24>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
    });
}
void launch_loud_encode(const LoudPiece *pieces, int P, const PcmGains &G, int encoding, int clip, hipStream_t s)
{
    pcm_for_tables<LoudTable>(pieces, P, [&](const LoudTable &t, int nt, int gx) {
        if (encoding == DMX_PCM_F32)
            hipLaunchKernelGGL(loud_encode_kernel<DMX_PCM_F32>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
        else if (encoding == DMX_PCM_S16)
            hipLaunchKernelGGL(loud_encode_kernel<DMX_PCM_S16>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
        else
            hipLaunchKernelGGL(loud_encode_kernel<DMX_PCM_S24>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
    });
}
void launch_limit_encode(const LimitPiece *pieces, int P, const PcmGains &G, int encoding, int clip, hipStream_t s)
{
    pcm_for_tables<LimitTable>(pieces, P, [&](const LimitTable &t, int nt, int gx) {
        if (encoding == DMX_PCM_F32)
            hipLaunchKernelGGL(limit_encode_kernel<DMX_PCM_F32>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
        else if (encoding == DMX_PCM_S16)
            hipLaunchKernelGGL(limit_encode_kernel<DMX_PCM_S16>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
        else
            hipLaunchKernelGGL(limit_encode_kernel<DMX_PCM_S24>, dim3(gx, G.nOut, nt), dim3(256), 0, s, t, G, clip);
    });
}

} // namespace dmx
