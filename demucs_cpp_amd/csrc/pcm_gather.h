// pcm_gather.h — how the output stages read one output's samples: 4 consecutive frames of both channels, from the stems'
// planes (dmx_output_spec) or under a row of gains over the stems and the mixture (dmx_remix_spec). Shared by pcm.hip (peak,
// clip, encode) and loudness.hip (the K-weighted energies); device code only. The arithmetic is specified in pcm.hip's head.
#pragma once
#include "kernels.h"

#include <cstdint>

namespace dmx
{
namespace
{
// 4 frames (cnt of them valid) of plane p starting at frame i
__device__ __forceinline__ void pcm_load4(const float *plane, i64 i, int cnt, float v[4])
{
    const float *q = plane + i;
    if (cnt == 4 && ((uintptr_t)q & 15) == 0)
    {
        const float4 t = *reinterpret_cast<const float4 *>(q);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = k < cnt ? q[k] : 0.0f;
    }
}
// the two channels of output o for frames [i, i + cnt)
__device__ __forceinline__ void pcm_gather(const PcmPiece &pc, int S, int stem, int o, i64 i, int cnt, float L[4], float R[4])
{
    if (stem < 0 || o == 0)
    {
        const int s = stem < 0 ? o : stem;
        pcm_load4(pc.planes + (i64)(2 * s) * pc.planeStride, i, cnt, L);
        pcm_load4(pc.planes + (i64)(2 * s + 1) * pc.planeStride, i, cnt, R);
        return;
    }
    bool first = true;
    for (int s = 0; s < S; ++s)
    {
        if (s == stem)
            continue;
        float a[4], b[4];
        pcm_load4(pc.planes + (i64)(2 * s) * pc.planeStride, i, cnt, a);
        pcm_load4(pc.planes + (i64)(2 * s + 1) * pc.planeStride, i, cnt, b);
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            L[k] = first ? a[k] : L[k] + a[k];
            R[k] = first ? b[k] : R[k] + b[k];
        }
        first = false;
    }
}
// frames [i, i + cnt) of the interleaved mixture: L0 R0 L1 R1 ...
__device__ __forceinline__ void pcm_load_mix4(const float *mix, i64 i, int cnt, float L[4], float R[4])
{
    const float *q = mix + 2 * i;
    if (cnt == 4 && ((uintptr_t)q & 15) == 0)
    {
        const float4 t = reinterpret_cast<const float4 *>(q)[0], u = reinterpret_cast<const float4 *>(q)[1];
        L[0] = t.x, R[0] = t.y, L[1] = t.z, R[1] = t.w;
        L[2] = u.x, R[2] = u.y, L[3] = u.z, R[3] = u.w;
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            L[k] = k < cnt ? q[2 * k] : 0.0f;
            R[k] = k < cnt ? q[2 * k + 1] : 0.0f;
        }
    }
}
// a = g x for the first visited source, then p = g x, a = a + p: two roundings, never one
__device__ __forceinline__ void remix_acc(float g, const float x[4], bool first, float a[4])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const float p = g * x[k];
        a[k] = first ? p : a[k] + p;
    }
}
// the two channels of output o for frames [i, i + cnt) under a gain table
__device__ __forceinline__ void remix_gather(const RemixPiece &pc, const PcmGains &G, int o, i64 i, int cnt, float L[4], float R[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
        L[k] = R[k] = 0.0f; // a checked spec has a non-zero gain in every row: never what is used
    bool first = true;
    for (int s = 0; s < G.S; ++s)
    {
        const float g = G.g[o][s];
        if (g == 0.0f) // uniform: the plane is not loaded
            continue;
        float a[4], b[4];
        pcm_load4(pc.planes + (i64)(2 * s) * pc.planeStride, i, cnt, a);
        pcm_load4(pc.planes + (i64)(2 * s + 1) * pc.planeStride, i, cnt, b);
        remix_acc(g, a, first, L);
        remix_acc(g, b, first, R);
        first = false;
    }
    const float gm = G.g[o][G.S];
    if (gm != 0.0f)
    {
        float a[4], b[4];
        pcm_load_mix4(pc.mix, i, cnt, a, b);
        remix_acc(gm, a, first, L);
        remix_acc(gm, b, first, R);
    }
}
struct GatherStems // dmx_output_spec: a stem, or the sum of the others
{
    int S, stem;
    __device__ __forceinline__ void operator()(const PcmPiece &pc, int o, i64 i, int cnt, float L[4], float R[4]) const
    {
        pcm_gather(pc, S, stem, o, i, cnt, L, R);
    }
};
struct GatherRemix // dmx_remix_spec: a row of gains
{
    const PcmGains &G;
    __device__ __forceinline__ void operator()(const RemixPiece &pc, int o, i64 i, int cnt, float L[4], float R[4]) const
    {
        remix_gather(pc, G, o, i, cnt, L, R);
    }
};
} // namespace
} // namespace dmx
