// loudness_plan.h — what the launches of one loudness measurement need, computed on the host for (rate, n). No HIP here: the
// header is shared by the library (kernels.h) and by the kernel text compiled as host code (tests/loudness_host_main.cpp).
#pragma once
#include <cstdint>

namespace dmx
{
constexpr int kLoudChunk = 64;              // frames a lane filters serially
constexpr int kLoudTile = 64 * kLoudChunk;  // frames of a wave: one workgroup takes one tile, a wave per channel
constexpr int kLoudMinRate = 4000;          // tan(pi f0 / fs) of the shelf needs fs > 2 * 1682
constexpr int kLoudMaxHops = kLoudTile / ((kLoudMinRate + 5) / 10) + 2; // hops a tile can touch at the smallest hop (400): 12
constexpr int kLoudGainSteps = 12001;       // the gain table: -60 dB .. +60 dB in hundredths of a dB

struct LoudPlan
{
    double k[7];        // shelf b0 b1 b2 a1 a2, high-pass a1 a2 (its b is 1 -2 1)
    double lane[6][16]; // A^(64 * 2^j): the scan over a wave's 64 chunks
    double tile[16];    // A^4096: one tile
    double unit[6][16]; // A^(4096 * U * 2^j): the scan over 64 units of U tiles
    double absThr;      // the absolute gate as an energy: 10^((-70 + 0.691) / 10)
    int64_t n;
    int hop, H, nTiles, kHops, U; // hop frames, whole hops, tiles, hops a tile can touch (kLoudTile / hop + 2), tiles per unit
};
// the two stages' b0 b1 b2 a1 a2: libm's tan and pow in binary64
void loud_coefficients(int rate, double coef[10]);
// 0, or -1 (rate < kLoudMinRate, n < 1)
int loud_plan(int rate, int64_t n, LoudPlan *p);
// bytes of workspace per measured signal of n frames, whatever the rate: a multiple of 16: 64 + 256 per tile + 16 per 400 frames, about n / 10
int64_t loud_workspace_bytes(int64_t n);
inline int64_t loud_ws_bytes(int64_t n) // n >= 1
{
    return 64 + (n + kLoudTile - 1) / kLoudTile * (64 + 16 * kLoudMaxHops) + 16 * (n / ((kLoudMinRate + 5) / 10));
}
// where a signal's hop energies e[2][H] start in its workspace slot, in bytes: behind the result (64), the tiles' states
// [2][nTiles][4] and the tiles' hop partials [2][nTiles][kHops], all binary64 (the meters launch reads them: meters.hip)
#ifdef __HIP__
__host__ __device__
#endif
    inline int64_t
    loud_ws_e_offset(const LoudPlan &p) { return 64 + 8 * ((int64_t)8 * p.nTiles + (int64_t)2 * p.nTiles * p.kHops); }
// T[i] = (float)pow(10, (i - 6000) / 2000.0), kLoudGainSteps entries
void loud_gain_table(float *T);
} // namespace dmx
