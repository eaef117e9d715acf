// bss_plan.h — the geometry of the BSS Eval v4 decomposition (bss.hip), computed on the host: the
// windows, the limits of the arguments and the layout of the workspace. No HIP here.
#pragma once
#include <cstdint>

namespace dmx
{
constexpr int kBssMaxSources = 8;      // J
constexpr int kBssMaxFilter = 512;     // L
constexpr int kBssMaxOrder = 6144;     // J C L: G is at most 6144^2 doubles = 302 MB
constexpr int kBssCols = 16;           // right-hand sides and output planes of one MFMA tile: J C <= 16
constexpr int kBssGramChunk = 65536;   // samples whose lagged products one workgroup of the Gram kernel keeps in registers; the
                                       // partial sums of the chunks are added in chunk order by a second launch
constexpr int kBssGramSub = 256;       // samples of a chunk staged in LDS at a time
constexpr int kBssPanel = 64;          // the block size of the Cholesky factorisation and of the substitutions
constexpr int kBssProjTile = 256;      // output samples of one workgroup of the projection kernel

// the windows of n samples: floor((n - window + hop) / hop), one window [0, n) for n < window; -1 for a bad argument
inline int64_t bss_windows(int64_t n, int64_t window, int64_t hop)
{
    if (n < 1 || window < 1 || hop < 1)
        return -1;
    return n < window ? 1 : (n - window + hop) / hop;
}
inline bool bss_shape_ok(int J, int C, int64_t n, int L)
{
    return J >= 1 && J <= kBssMaxSources && (C == 1 || C == 2) && n >= 1 && n < ((int64_t)1 << 31) && L >= 1 && L <= kBssMaxFilter &&
           J * C * L <= kBssMaxOrder;
}

// byte offsets into the workspace, each a multiple of 256
struct BssLayout
{
    int M, Lp, nG, nOwn;   // planes J C; L rounded up to 16 lags; the orders J C L and C L
    int64_t chunks;        // Gram chunks
    int64_t part, rho, G, Gown, X, Y, proj, flags, bytes;
};
// part: [chunks][2 M][16][Lp] partial correlations, rho: [2 M][16][Lp] their sums (rho[b][a][k] = sum_m a[m] b[m + k]; b < M a
// reference, else an estimate), G: [nG][nG] row-major, lower triangle, Gown: [J][nOwn][nOwn] the diagonal blocks, X and Y:
// [nG][16] the right-hand sides and then the filters (Y block-diagonal: column (i, c'') is zero outside source i's rows),
// proj: [2][M][n] p_all and p_own, flags: [J][windows] ints, the windows' silence flags, sized [J][n]: the workspace is a
// function of the shape alone, not of window and hop, and there are at most n windows (hop 1)
inline BssLayout bss_layout(int J, int C, int64_t n, int L)
{
    BssLayout l{};
    l.M = J * C, l.Lp = (L + 15) & ~15, l.nG = J * C * L, l.nOwn = C * L;
    l.chunks = (n + kBssGramChunk - 1) / kBssGramChunk;
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t o = at;
        at += (bytes + 255) & ~(int64_t)255;
        return o;
    };
    const int64_t corr = (int64_t)2 * l.M * 16 * l.Lp * 8;
    l.part = take(l.chunks * corr);
    l.rho = take(corr);
    l.G = take((int64_t)l.nG * l.nG * 8);
    l.Gown = take((int64_t)J * l.nOwn * l.nOwn * 8);
    l.X = take((int64_t)l.nG * kBssCols * 8);
    l.Y = take((int64_t)l.nG * kBssCols * 8);
    l.proj = take((int64_t)2 * l.M * n * 8);
    l.flags = take((int64_t)J * n * 4);
    l.bytes = at;
    return l;
}
inline int64_t bss_workspace_bytes(int J, int C, int64_t n, int L) { return bss_shape_ok(J, C, n, L) ? bss_layout(J, C, n, L).bytes : -1; }
} // namespace dmx
