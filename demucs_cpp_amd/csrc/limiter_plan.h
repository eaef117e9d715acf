// limiter_plan.h — what the launches of the look-ahead peak limiter need (limiter.hip), computed on the
// host. No HIP here: the header is shared by the library (kernels.h) and by the kernel text compiled as host code
// (tests/limiter_host_main.cpp).
#pragma once
#include "meters_plan.h"

#include <cstdint>

namespace dmx
{
constexpr int kLimUnit = 65536;               // units of an octave
constexpr int kLimCap = 24 * kLimUnit;        // the largest reduction: 24 octaves
constexpr int kLimLut = 4096;                 // LUT: the mantissa's upper 12 bits -> units, rounded up
constexpr int kLimHi = 16 * 24 + 1;           // THI: 2^(-a / 16), a = D >> 12
constexpr int kLimLo = 4096;                  // TLO: 2^(-b / 65536), b = D & 4095
constexpr int kLimHiPad = (kLimHi + 3) & ~3;  // THI's words in the device's copy of the tables
constexpr int kLimTableWords = kLimLut + kLimHiPad + kLimLo; // LUT, THI, TLO: 4-byte words
constexpr int kLimRun = kTpRun;               // consecutive frames of one lane: 8
constexpr int kLimTile = kTpTile;             // frames of a workgroup of 256: the true-peak launch's tile
constexpr int kLimMaxSlope = 1 << 20;         // units per frame
constexpr double kLimAttackMs = 5.0, kLimReleaseMs = 100.0, kLimMinMs = 0.1, kLimMaxMs = 10000.0;

// LUT[k] = ceil(U log2(1 + (k + 1) / 4096)) + 2; THI and TLO rounded towards zero: binary64 with libm's log2 and pow
void lim_tables(int32_t *lut, float *thi, float *tlo);
// the slopes in units per frame: clamp(rint(U log2(10^0.5) 1000 / (ms rate)), 1, 2^20). 0, or -1 (rate < 1, a time that is
// not finite or outside [0.1, 10000])
int lim_slopes(int rate, double attackMs, double releaseMs, int *qa, int *qr);
// the workspace of ONE envelope over n frames: M as int32 [n4] at byte 0, the gain plane as fp32 [n4] at byte 4 n4 (n4 = n
// rounded up to a multiple of 4), then 64 bytes per tile of 2048 frames. A multiple of 16; -1 for n < 1
int64_t lim_workspace_bytes(int64_t n);
#ifdef __HIP__
#define DMX_LIM_HD __host__ __device__ inline
#else
#define DMX_LIM_HD inline
#endif
DMX_LIM_HD int64_t lim_ws_gain_offset(int64_t n) { return 4 * ((n + 3) & ~(int64_t)3); }
DMX_LIM_HD int64_t lim_ws_tiles_offset(int64_t n) { return 8 * ((n + 3) & ~(int64_t)3); }
DMX_LIM_HD int64_t lim_tiles(int64_t n) { return (n + kLimTile - 1) / kLimTile; }
DMX_LIM_HD int64_t lim_ws_bytes(int64_t n) { return lim_ws_tiles_offset(n) + 64 * lim_tiles(n); } // n >= 1
} // namespace dmx
