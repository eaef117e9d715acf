// wiener_plan.h — the geometry of the multichannel Wiener post-filter (wiener.hip), computed on the
// host: the frames, the blocks, the limits of the arguments and the layout of the workspace. No HIP here.
#pragma once
#include <cstdint>

namespace dmx
{
constexpr int kWienerMaxSources = 8;   // J; with the residual the EM kernel carries J + 1 = 9
constexpr int kWienerMaxIter = 8;
constexpr int kWienerNfft = 4096, kWienerHop = 1024, kWienerPad = 2048;
constexpr int kWienerBins = 2049;      // F
constexpr int kWienerRow = 2064;       // complex64 elements between two frames of a plane: F rounded up to 128 bytes, so
                                       // the 64 lanes of a wave (512 bytes) read and write whole lines
constexpr int kWienerTile = 64;        // bins of one EM workgroup: one per lane
constexpr int kWienerTiles = (kWienerBins + kWienerTile - 1) / kWienerTile; // 33; the last holds the Nyquist bin alone
constexpr int kWienerChunk = 12;       // frames one workgroup of the inverse emits (it recomputes a halo of 3 before them)

inline bool wiener_shape_ok(int J, int C, int64_t n)
{
    return J >= 1 && J <= kWienerMaxSources && (C == 1 || C == 2) && n > kWienerPad && n < ((int64_t)1 << 31);
}
inline bool wiener_spec_ok(int iterations, int residual, int win_len)
{
    return iterations >= 1 && iterations <= kWienerMaxIter && (residual == 0 || residual == 1) && win_len >= 1;
}

// byte offsets into the workspace, each a multiple of 256
struct WienerLayout
{
    int64_t T, blocks, chunks; // frames 1 + n / 1024, EM blocks of win_len frames, chunks of the inverse
    int sets;                  // plane sets of C planes: the mixture, J estimates, the residual source
    int64_t plane;             // complex64 elements of one plane: T rows of kWienerRow
    int64_t tw, win, fmax, spec, bytes;
};
// tw: 2048 complex64 exp(-2 pi i k / 4096), win: 4096 floats, the periodic Hann window, fmax: [T] doubles, the largest |X|^2
// of frame t over bins and channels, spec: [sets][C][T][kWienerRow] complex64. Set 0 is X, set 1 + j first E_j and from the
// first EM launch on y_j (the launch overwrites each element it has read: a (block, tile) belongs to one workgroup), set
// 1 + J the residual source.
inline WienerLayout wiener_layout(int J, int C, int64_t n, int residual, int win_len)
{
    WienerLayout l{};
    l.T = 1 + n / kWienerHop;
    l.blocks = (l.T + win_len - 1) / win_len;
    l.chunks = (l.T + kWienerChunk - 1) / kWienerChunk;
    l.sets = 1 + J + (residual ? 1 : 0);
    l.plane = l.T * kWienerRow;
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t o = at;
        at += (bytes + 255) & ~(int64_t)255;
        return o;
    };
    l.tw = take(2048 * 8);
    l.win = take(4096 * 4);
    l.fmax = take(l.T * 8);
    l.spec = take((int64_t)l.sets * C * l.plane * 8);
    l.bytes = at;
    return l;
}
inline int64_t wiener_workspace_bytes(int J, int C, int64_t n, int residual)
{
    return wiener_shape_ok(J, C, n) && (residual == 0 || residual == 1) ? wiener_layout(J, C, n, residual, 1).bytes : -1;
}
} // namespace dmx
