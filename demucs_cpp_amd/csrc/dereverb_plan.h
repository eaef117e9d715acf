// dereverb_plan.h — the geometry of the WPE de-reverberation (dereverb.hip), computed on the host:
// the limits of the arguments, the tiles of the three kernels and the layout of the workspace. The STFT is the Wiener
// stage's (wiener_plan.h). No HIP here.
#pragma once
#include "wiener_plan.h"

namespace dmx
{
constexpr int kDrvMaxSources = 8, kDrvMaxTaps = 16, kDrvMaxDelay = 8, kDrvMaxIter = 8;
constexpr int kDrvBinTile = 8;    // adjacent bins of one correlation / filter workgroup: 64 contiguous bytes of a [t][f] row
constexpr int kDrvBinTiles = (kWienerBins + kDrvBinTile - 1) / kDrvBinTile; // 257; the last holds the Nyquist bin alone
constexpr int kDrvSlab = 64;      // frames staged into LDS at a time (with D + K - 1 frames of history before them)
constexpr int kDrvMaxRanges = 4;  // frame ranges a bin's correlation is cut into; their partial sums meet in range order
constexpr int kDrvMinRange = 32;  // no range is cut shorter than this unless the track is
constexpr int kDrvMaxTiles = 5;   // 16-row tiles of the embedded vectors: 2 M + 2 C <= 68 rows
constexpr int kDrvFilterFrames = 64; // frames of one filter workgroup

struct DrvSpec
{
    int taps, delay, iterations;
    double eps, reg;
};
inline bool dereverb_shape_ok(int J, int C, int64_t n) { return J >= 1 && J <= kDrvMaxSources && wiener_shape_ok(1, C, n); }

// the embedded real vector S(t) = [Re Yt; Im Yt; Re Y; Im Y] of a bin: rows, 16-row tiles, tiles on and below the diagonal
inline int dereverb_rows(int C, int K) { return 2 * C * K + 2 * C; }
inline int dereverb_tiles(int C, int K) { return (dereverb_rows(C, K) + 15) / 16; }
inline int dereverb_lower(int nt) { return nt * (nt + 1) / 2; }
// floats between two frames of the LDS slab [frame][bin][channel][re | im] (8 bins x 2 channels x 2 = 32 at most). A
// fragment read's addresses are 35 (t - k) + 2 c + part: with 35 = 3 mod 32 the frames that the 32 lanes of a half wave span
// (2 along t, 8 along the taps at C = 2) and the two channels land on 18 different banks
constexpr int kDrvPitch = 35;
constexpr int kDrvSlabRows = kDrvSlab + kDrvMaxDelay + kDrvMaxTaps - 1;

// byte offsets into the workspace, each a multiple of 256
struct DrvLayout
{
    int64_t T, chunks, plane; // frames, chunks of the inverse, complex64 elements of one plane
    int64_t range, ranges;    // frames of a correlation range (a multiple of 4), their number
    int M, nt, lower;         // C K, row tiles, tiles computed
    int64_t tw, win, fmax, peak, Y, Z, lam, part, G, bytes;
};
// tw, win: the transform's tables; fmax: [J][T] doubles, the largest |Y|^2 of a frame; peak: [J] doubles, of a stem;
// Y, Z: [J][C][T][kWienerRow] complex64; lam: [J][T][kWienerRow] doubles; part: [J][bins][ranges][lower][4][64] doubles,
// element r of lane l of a tile's accumulator at [r][l]; G: [J][bins][M][C] complex128
inline DrvLayout dereverb_layout(int J, int C, int64_t n, int K)
{
    DrvLayout l{};
    l.T = 1 + n / kWienerHop;
    l.chunks = (l.T + kWienerChunk - 1) / kWienerChunk;
    l.plane = l.T * kWienerRow;
    int64_t nr = (l.T + kDrvMinRange - 1) / kDrvMinRange;
    nr = nr > kDrvMaxRanges ? kDrvMaxRanges : nr;
    l.range = ((l.T + nr - 1) / nr + 3) & ~(int64_t)3;
    l.ranges = (l.T + l.range - 1) / l.range;
    l.M = C * K, l.nt = dereverb_tiles(C, K), l.lower = dereverb_lower(l.nt);
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t o = at;
        at += (bytes + 255) & ~(int64_t)255;
        return o;
    };
    l.tw = take(2048 * 8);
    l.win = take(4096 * 4);
    l.fmax = take(J * l.T * 8);
    l.peak = take(J * 8);
    l.Y = take((int64_t)J * C * l.plane * 8);
    l.Z = take((int64_t)J * C * l.plane * 8);
    l.lam = take((int64_t)J * l.plane * 8);
    l.part = take((int64_t)J * kWienerBins * l.ranges * l.lower * 256 * 8);
    l.G = take((int64_t)J * kWienerBins * l.M * C * 16);
    l.bytes = at;
    return l;
}
inline int64_t dereverb_workspace_bytes(int J, int C, int64_t n, int K)
{
    return dereverb_shape_ok(J, C, n) && K >= 1 && K <= kDrvMaxTaps ? dereverb_layout(J, C, n, K).bytes : -1;
}
} // namespace dmx
