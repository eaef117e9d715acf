// hpss_plan.h — the geometry of the median-filter harmonic/percussive split (hpss.hip), computed on
// the host: the limits of the arguments, the tile of the filter kernel, the fold of an index at a plane's edge and the layout
// of the workspace. The STFT and its inverse are the Wiener stage's (wiener_plan.h). No HIP here.
#pragma once
#include "wiener_plan.h"

namespace dmx
{
constexpr int kHpssMaxSources = 8;
constexpr int kHpssMaxKernel = 31;                  // the windows are odd, 3 .. 31: one selection network of 31 inputs
constexpr int kHpssHalo = kHpssMaxKernel / 2;       // 15 cells on every side of a tile
constexpr int kHpssMaxPower = 8;
constexpr double kHpssMaxMargin = 100.0;
constexpr int kHpssTileBins = 64, kHpssTileFrames = 32; // one workgroup of 256 threads: a lane per bin, 8 frames a thread
constexpr int kHpssLdsRows = kHpssTileFrames + 2 * kHpssHalo;      // 62
constexpr int kHpssLdsCols = kHpssTileBins + 2 * kHpssHalo;        // 94
constexpr int kHpssLdsStride = kHpssLdsCols + 1;                   // 95 floats: 62 x 95 x 4 = 23 560 bytes of LDS
// what dmx_hpss_filter_device takes: the planes sit in the grid's z, the tiles of bins in its y (both stop at 65535)
constexpr int kHpssMaxPlanes = 65535, kHpssMaxRow = 1 << 20, kHpssMaxFrames = 1 << 24;
enum { kHpssMasks = 0, kHpssMedians = 1 };

struct HpssSpec
{
    int kh, kp, power, residual;
    double mh, mp;
};
inline bool hpss_kernel_ok(int k) { return k >= 3 && k <= kHpssMaxKernel && (k & 1) == 1; }
inline bool hpss_margin_ok(double m) { return m >= 1.0 && m <= kHpssMaxMargin; } // false for a NaN
inline bool hpss_spec_ok(const HpssSpec &s)
{
    return hpss_kernel_ok(s.kh) && hpss_kernel_ok(s.kp) && s.power >= 1 && s.power <= kHpssMaxPower && hpss_margin_ok(s.mh) &&
           hpss_margin_ok(s.mp) && (s.residual == 0 || s.residual == 1);
}
inline bool hpss_shape_ok(int J, int C, int64_t n) { return J >= 1 && J <= kHpssMaxSources && wiener_shape_ok(1, C, n); }
inline bool hpss_filter_shape_ok(int64_t planes, int64_t frames, int64_t bins, int64_t row)
{
    return planes >= 1 && planes <= kHpssMaxPlanes && frames >= 1 && frames <= kHpssMaxFrames && bins >= 1 && bins <= row && row <= kHpssMaxRow;
}
// Half-sample symmetric reflection of an index into [0, n): d c b a | a b c d | d c b a, with period 2 n, so an extent below
// the half window folds as often as it takes (SciPy's `reflect`, NumPy's `symmetric`). i > -2^30, n >= 1.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int hpss_fold(int i, int n)
{
    if ((unsigned)i < (unsigned)n) // inside: no division
        return i;
    int m = i % (2 * n);
    if (m < 0)
        m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// byte offsets into the workspace, each a multiple of 256
struct HpssLayout
{
    int64_t T, plane, chunks; // frames, complex64 elements of a plane of D (fp32 elements of a mask plane), chunks of the inverse
    int64_t tw, win, fmax, D, mh, mp, bytes;
};
// tw, win: the transform's tables; fmax: [T] doubles, the forward kernel's by-product; D: [J][C][T][kWienerRow] complex64;
// mh, mp: [J C][T][kWienerRow] fp32, the harmonic and the percussive mask
inline HpssLayout hpss_layout(int J, int C, int64_t n)
{
    HpssLayout l{};
    l.T = 1 + n / kWienerHop;
    l.plane = l.T * kWienerRow;
    l.chunks = (l.T + kWienerChunk - 1) / kWienerChunk;
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t o = at;
        at += (bytes + 255) & ~(int64_t)255;
        return o;
    };
    l.tw = take(2048 * 8);
    l.win = take(4096 * 4);
    l.fmax = take(l.T * 8);
    l.D = take((int64_t)J * C * l.plane * 8);
    l.mh = take((int64_t)J * C * l.plane * 4);
    l.mp = take((int64_t)J * C * l.plane * 4);
    l.bytes = at;
    return l;
}
inline int64_t hpss_workspace_bytes(int J, int C, int64_t n) { return hpss_shape_ok(J, C, n) ? hpss_layout(J, C, n).bytes : -1; }
} // namespace dmx
