// stretch_plan.h — the geometry of the phase-vocoder time stretch and pitch shift (stretch.hip),
// computed on the host: the limits of the arguments, the lengths, the cut of the phasor products and the layout of the
// workspace. The STFT and its inverse are the Wiener stage's (wiener_plan.h). No HIP here.
#pragma once
#include "wiener_plan.h"

namespace dmx
{
constexpr int kStretchMaxSources = 8;
constexpr int kStretchMaxTerm = 1 << 20; // num, den, pitch_num, pitch_den are in [1, 2^20]
constexpr int kStretchMaxRate = 4;       // 1/4 <= num / den <= 4
constexpr int kStretchHalo = 3;          // frames a chunk of the inverse recomputes before its own (wiener_stft.h)

struct StretchSpec
{
    int num, den, pnum, pden; // the rate num / den (above 1: faster, shorter), the converter pnum -> pden behind the inverse
};
inline bool stretch_spec_ok(const StretchSpec &s)
{
    auto term = [](int v) { return v >= 1 && v <= kStretchMaxTerm; };
    return term(s.num) && term(s.den) && term(s.pnum) && term(s.pden) && (int64_t)s.num <= (int64_t)kStretchMaxRate * s.den &&
           (int64_t)s.den <= (int64_t)kStretchMaxRate * s.num;
}
inline bool stretch_converts(const StretchSpec &s) { return s.pnum != s.pden; }
// the samples behind the inverse: n' = ceil(n den / num); n < 2^31 and den <= 2^20, so the product is below 2^51
inline int64_t stretch_mid_length(int64_t n, const StretchSpec &s) { return (n * s.den + s.num - 1) / s.num; }
inline bool stretch_shape_ok(int J, int C, int64_t n, const StretchSpec &s)
{
    return J >= 1 && J <= kStretchMaxSources && wiener_shape_ok(1, C, n) && wiener_shape_ok(1, C, stretch_mid_length(n, s));
}
// the first output frame of product range c: range c covers the frames [first(c), first(c + 1)) and is what takes the phasor
// from the first frame chunk c of the inverse forms (its start less the halo, clipped at 0) to the first of chunk c + 1
constexpr int64_t stretch_first(int64_t c) { return c == 0 ? 0 : c * kWienerChunk - kStretchHalo; }

// byte offsets into the workspace, each a multiple of 256
struct StretchLayout
{
    int64_t T, plane;          // frames and complex64 elements of an input plane
    int64_t n2, T2, chunks;    // samples, frames and chunks of the inverse behind the vocoder
    int64_t mid;               // floats between two planes of `tmp`
    int64_t tw, win, fmax, live, D, carry, tmp, bytes;
};
// tw, win: the transform's tables; fmax: [T] doubles, the forward kernel's by-product; live: [J C][T] ints, 0 where a frame's
// samples are all zero; D: [J][C][T][kWienerRow] complex64;
// carry: [J C][chunks][kWienerRow] complex128, first the products of the ranges (range c at chunk c + 1), then in place the
// phasor at stretch_first(chunk); tmp (with a converter only): [J C][mid] floats, the stretched planes ahead of it
inline StretchLayout stretch_layout(int J, int C, int64_t n, const StretchSpec &s)
{
    StretchLayout l{};
    l.T = 1 + n / kWienerHop;
    l.plane = l.T * kWienerRow;
    l.n2 = stretch_mid_length(n, s);
    l.T2 = 1 + l.n2 / kWienerHop;
    l.chunks = (l.T2 + kWienerChunk - 1) / kWienerChunk;
    l.mid = (l.n2 + 63) & ~(int64_t)63;
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t o = at;
        at += (bytes + 255) & ~(int64_t)255;
        return o;
    };
    l.tw = take(2048 * 8);
    l.win = take(4096 * 4);
    l.fmax = take(l.T * 8);
    l.live = take((int64_t)J * C * l.T * 4);
    l.D = take((int64_t)J * C * l.plane * 8);
    l.carry = take((int64_t)J * C * l.chunks * kWienerRow * 16);
    l.tmp = take(stretch_converts(s) ? (int64_t)J * C * l.mid * 4 : 0);
    l.bytes = at;
    return l;
}
inline int64_t stretch_workspace_bytes(int J, int C, int64_t n, const StretchSpec &s)
{
    return stretch_spec_ok(s) && stretch_shape_ok(J, C, n, s) ? stretch_layout(J, C, n, s).bytes : -1;
}
} // namespace dmx
