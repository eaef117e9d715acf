// gemm_tiles.h — the tiles of the GEMM kernels and the (tile, prologue, epilogue) combinations that are compiled: written here
// once. gemm_select.cpp decides from these tables (which tile an op gets, whether its kernel exists); igemm.hip, igemm_split.hip
// and dgemm.hip expand the same lists into their launch switches and look a tile's geometry up from its number at compile time.
// No HIP here: plain C++.
#pragma once
#include "plan.h"

namespace dmx
{

enum TileKind
{
    TK_NONE = 0, // no kernel, never chosen: the slot keeps the numbering
    TK_TILE,     // igemm.hip igemm_kernel (and, where DMX_SPLIT_COMBOS lists the tile, igemm_split.hip)
    TK_DIRECT,   // dgemm.hip: register-resident weights, one wave owns 16 rows x all columns (NB = 1)
    TK_LIN256,   // igemm_lin256.hip: four waves of 128x64 with their own pipelined loop, linear layers only
};

// One row per tile cfg. The NUMBERING is fixed: tests, profiles and bench.py's roofline classes use it.
//   X(cfg, BM, BN, waves along M, waves along N, row fragments, column fragments, K sub-steps of 16 per K-tile (0: not igemm_kernel),
//     fp32 label, exact-split label or nullptr, half-height sibling of an op without row statistics, with them (-1: none), kind)
// A tile is (waves M x row fragments x 16) x (waves N x column fragments x 16). The labels are the ops' kernels in dmx_debug_profile =
// bench.py's roofline classes. Siblings keep the column decomposition (waves x fragments along N) of the tile they replace, so the
// row statistics - and every other output bit - are identical; 64x64 (cfg 9: 2 waves x 2 fragments along N) only replaces ops
// without row statistics. Half-height siblings serve launches that would leave CUs idle (few segments in flight), quarter-height
// ones (15, 16) one or two segments per call (gemm_select.cpp refine_cfg).
#define DMX_TILES(X)                                                                                         \
    X(0, 128, 128, 2, 2, 4, 4, 2, "igemm_128x128", "igemm_split_128x128", 7, 7, TK_TILE)                     \
    X(1, 64, 64, 2, 2, 2, 2, 0, "igemm_64x64", nullptr, -1, -1, TK_NONE)                                     \
    X(2, 128, 96, 4, 1, 2, 6, 2, "igemm_128x96", "igemm_split_128x96", 10, 10, TK_TILE)                      \
    X(3, 128, 48, 4, 1, 2, 3, 2, "igemm_128x48", "igemm_split_128x48", 11, 11, TK_TILE)                      \
    X(4, 256, 16, 4, 1, 4, 1, 2, "igemm_256x16", nullptr, 14, 14, TK_TILE)                                   \
    X(5, 128, 32, 4, 1, 2, 2, 2, "igemm_128x32", "igemm_split_128x32d", 12, 12, TK_TILE)                     \
    X(6, 128, 64, 4, 1, 2, 4, 2, "igemm_128x64", "igemm_split_128x64d", 13, 13, TK_TILE)                     \
    X(7, 64, 128, 2, 2, 2, 4, 2, "igemm_64x128", "igemm_split_64x128", 9, 15, TK_TILE)                       \
    X(8, 16, 256, 1, 1, 1, 16, 0, "dgemm_direct", nullptr, -1, -1, TK_DIRECT)                                \
    X(9, 64, 64, 2, 2, 2, 2, 2, "igemm_64x64", "igemm_split_64x64", 16, 16, TK_TILE)                         \
    X(10, 64, 96, 4, 1, 1, 6, 2, "igemm_64x96", "igemm_split_64x96", -1, -1, TK_TILE)                        \
    X(11, 64, 48, 4, 1, 1, 3, 2, "igemm_64x48", "igemm_split_64x48", -1, -1, TK_TILE)                        \
    X(12, 64, 32, 4, 1, 1, 2, 2, "igemm_64x32", "igemm_split_128x32d", -1, -1, TK_TILE)                      \
    X(13, 64, 64, 4, 1, 1, 4, 2, "igemm_64x64", "igemm_split_128x64d", -1, -1, TK_TILE)                      \
    X(14, 128, 16, 4, 1, 2, 1, 2, "igemm_128x16", nullptr, -1, -1, TK_TILE)                                  \
    X(15, 32, 128, 2, 2, 1, 4, 2, "igemm_32x128", "igemm_split_32x128", -1, -1, TK_TILE)                     \
    X(16, 32, 64, 2, 2, 1, 2, 2, "igemm_32x64", "igemm_split_32x64", -1, -1, TK_TILE)                        \
    X(17, 256, 128, 2, 2, 8, 4, 0, "igemm_256x128", nullptr, -1, -1, TK_NONE)                                \
    X(18, 256, 128, 2, 2, 8, 4, 0, "igemm_256x128w4", nullptr, -1, -1, TK_NONE)                              \
    X(19, 256, 128, 2, 2, 8, 4, 0, "igemm_lin256x128", nullptr, -1, -1, TK_LIN256)                           \
    /* 20: four waves of 64x96, 16-deep K-tiles, plain loop: the short-K ops of the 128x96 family (same column decomposition and */ \
    /* k order as 2: identical bits) */                                                                      \
    X(20, 256, 96, 4, 1, 4, 6, 1, "igemm_256x96", nullptr, -1, -1, TK_TILE)

struct TileCfg
{
    int BM, BN;
    int WM, WN, MF, NF, KS;
    const char *label, *splitLabel;
    int half, halfStat;
    int kind;
};
#define DMX_TILE_ROW(cfg, BM, BN, WM, WN, MF, NF, KS, label, splitLabel, half, halfStat, kind) {BM, BN, WM, WN, MF, NF, KS, label, splitLabel, half, halfStat, kind},
inline constexpr TileCfg kTileCfgs[] = {DMX_TILES(DMX_TILE_ROW)};
#undef DMX_TILE_ROW
inline constexpr int kNumTileCfgs = (int)(sizeof(kTileCfgs) / sizeof(kTileCfgs[0]));
inline constexpr int kDirectCfg = 8;
#define DMX_TILE_CHECK(cfg, bm, bn, wm, wn, mf, nf, ...) \
    static_assert(cfg < kNumTileCfgs && kTileCfgs[cfg].BM == bm && bm == wm * mf * 16 && bn == wn * nf * 16, "row cfg of the table is tile cfg; a tile is waves x fragments x 16");
DMX_TILES(DMX_TILE_CHECK)
#undef DMX_TILE_CHECK
static_assert(kNumTileCfgs == 21 && kTileCfgs[kDirectCfg].kind == TK_DIRECT, "the numbering is fixed");

// cfg -> its half-height sibling (-1: none); stat = the op writes row statistics
constexpr int half_cfg(int cfg, bool stat) { return cfg < 0 || cfg >= kNumTileCfgs ? -1 : stat ? kTileCfgs[cfg].halfStat : kTileCfgs[cfg].half; }

// ---- the compiled combinations. Rows are what the plans of the 4- and 6-source models and of Demucs v3 emit at any segment length
// (tests/cpu_interp.cpp interp_combos; tests/test_gemm_select_cpu.py asserts that every chosen kernel is listed).

// igemm.hip igemm_kernel: X(cfg, prologue, epilogue)
#define DMX_TILE_COMBOS(X)                                                                                                           \
    /* cfg 0: 128x128, cfg 7: 64x128 (same column decomposition; STATS_FACT: Demucs v3 level 3, hidden 96 -> 98 factor columns) */   \
    X(0, PRO_NONE, EPI_LINEAR) X(0, PRO_NONE, EPI_SCALE_RES) X(0, PRO_NONE, EPI_GLU) X(0, PRO_NONE, EPI_TRCONV)                      \
    X(0, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES) X(0, PRO_GN_GELU, EPI_STATS_ONLY) X(0, PRO_GN_GELU, EPI_STATS_FACT)                      \
    /* cfg 20: 256x96, the short-K ops of the 128x96 family */                                                                       \
    X(20, PRO_NONE, EPI_LINEAR) X(20, PRO_NONE, EPI_GLU) X(20, PRO_NONE, EPI_TRCONV)                                                 \
    X(7, PRO_NONE, EPI_LINEAR) X(7, PRO_NONE, EPI_SCALE_RES) X(7, PRO_NONE, EPI_GLU) X(7, PRO_NONE, EPI_TRCONV)                      \
    X(7, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES) X(7, PRO_GN_GELU, EPI_STATS_ONLY) X(7, PRO_GN_GELU, EPI_STATS_FACT)                      \
    /* cfg 2: 128x96, cfg 3: 128x48 */                                                                                               \
    X(2, PRO_NONE, EPI_LINEAR) X(2, PRO_NONE, EPI_GLU) X(2, PRO_NONE, EPI_TRCONV)                                                    \
    X(2, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES) X(2, PRO_GN_GELU, EPI_STATS_ONLY)                                                        \
    X(3, PRO_NONE, EPI_LINEAR) X(3, PRO_NONE, EPI_TRCONV) X(3, PRO_AFFINE, EPI_LINEAR)                                               \
    /* cfg 4: 256x16, cfg 5: 128x32, cfg 6: 128x64 */                                                                                \
    X(4, PRO_NONE, EPI_LINEAR) X(4, PRO_GN_GELU, EPI_STATS_FACT) X(5, PRO_GN_GELU, EPI_STATS_FACT) X(6, PRO_GN_GELU, EPI_STATS_FACT) \
    X(5, PRO_NONE, EPI_LINEAR) X(5, PRO_NONE, EPI_TRCONV) X(6, PRO_NONE, EPI_TRCONV) X(6, PRO_NONE, EPI_LINEAR)                      \
    /* half-height siblings: cfg 9: 64x64 of 7; 10: 64x96 of 2; 11: 64x48 of 3; 12: 64x32 of 5; 13: 64x64 (4 x 1 waves) of 6; */     \
    /* 14: 128x16 of 4 */                                                                                                            \
    X(9, PRO_NONE, EPI_LINEAR) X(9, PRO_NONE, EPI_SCALE_RES) X(9, PRO_NONE, EPI_GLU) X(9, PRO_NONE, EPI_TRCONV)                      \
    X(9, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES)                                                                                          \
    X(10, PRO_NONE, EPI_LINEAR) X(10, PRO_NONE, EPI_GLU) X(10, PRO_NONE, EPI_TRCONV)                                                 \
    X(10, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES) X(10, PRO_GN_GELU, EPI_STATS_ONLY)                                                      \
    X(11, PRO_NONE, EPI_LINEAR) X(11, PRO_NONE, EPI_TRCONV) X(11, PRO_AFFINE, EPI_LINEAR)                                            \
    X(12, PRO_GN_GELU, EPI_STATS_FACT) X(12, PRO_NONE, EPI_LINEAR) X(12, PRO_NONE, EPI_TRCONV)                                       \
    X(13, PRO_GN_GELU, EPI_STATS_FACT) X(13, PRO_NONE, EPI_TRCONV) X(13, PRO_NONE, EPI_LINEAR)                                       \
    X(14, PRO_NONE, EPI_LINEAR) X(14, PRO_GN_GELU, EPI_STATS_FACT)                                                                   \
    /* quarter-height siblings: cfg 15: 32x128 of 7 (same column decomposition); 16: 32x64 of 9 */                                   \
    X(15, PRO_NONE, EPI_LINEAR) X(15, PRO_NONE, EPI_SCALE_RES) X(15, PRO_NONE, EPI_GLU) X(15, PRO_NONE, EPI_TRCONV)                  \
    X(15, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES) X(15, PRO_GN_GELU, EPI_STATS_ONLY) X(15, PRO_GN_GELU, EPI_STATS_FACT)                   \
    X(16, PRO_NONE, EPI_LINEAR) X(16, PRO_NONE, EPI_SCALE_RES) X(16, PRO_NONE, EPI_GLU) X(16, PRO_NONE, EPI_TRCONV)                  \
    X(16, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES)

// igemm_split.hip igemm_split_kernel / igemm_split_lin_kernel: X(cfg, prologue, epilogue) - the MFMA-bound tile families only:
// 0 / 7 / 15 (2x2 waves, 4 column fragments), 9 / 16 (2 column fragments), 2 / 10 (4x1 waves, 6 column fragments), 3 / 11 (4x1 waves,
// 3 column fragments, plain convs only). Anything else keeps its fp32 kernel. (The narrow tiles 5 / 12 / 6 / 13 have no staged form:
// gemm_select.cpp narrow_split_ok.)
#define DMX_SPLIT_COMBOS(X)                                                                                                         \
    X(0, PRO_NONE, EPI_LINEAR) X(0, PRO_NONE, EPI_SCALE_RES) X(0, PRO_NONE, EPI_GLU) X(0, PRO_NONE, EPI_TRCONV)                     \
    X(7, PRO_NONE, EPI_LINEAR) X(7, PRO_NONE, EPI_SCALE_RES) X(7, PRO_NONE, EPI_GLU) X(7, PRO_NONE, EPI_TRCONV)                     \
    /* K / V projections that write the attention kernel's operand planes (plan.cpp plane_linear) */                                \
    X(0, PRO_NONE, EPI_KPL) X(0, PRO_NONE, EPI_VT) X(7, PRO_NONE, EPI_KPL) X(7, PRO_NONE, EPI_VT)                                   \
    X(2, PRO_NONE, EPI_LINEAR) X(2, PRO_NONE, EPI_GLU) X(2, PRO_NONE, EPI_TRCONV)                                                   \
    /* half / quarter-height siblings (few segments in flight): same column decomposition, same bits as their parents */            \
    X(15, PRO_NONE, EPI_LINEAR) X(15, PRO_NONE, EPI_SCALE_RES) X(15, PRO_NONE, EPI_GLU) X(15, PRO_NONE, EPI_TRCONV)                 \
    X(9, PRO_NONE, EPI_LINEAR) X(9, PRO_NONE, EPI_SCALE_RES) X(9, PRO_NONE, EPI_GLU) X(9, PRO_NONE, EPI_TRCONV)                     \
    X(16, PRO_NONE, EPI_LINEAR) X(16, PRO_NONE, EPI_SCALE_RES) X(16, PRO_NONE, EPI_GLU) X(16, PRO_NONE, EPI_TRCONV)                 \
    X(10, PRO_NONE, EPI_LINEAR) X(10, PRO_NONE, EPI_GLU) X(10, PRO_NONE, EPI_TRCONV)                                                \
    /* 48-wide tiles (4 x 1 waves, 3 column fragments): the deepest DConv K1 convs (K = 3 C = 1152, N = C / 8 = 48: 72 flops per */ \
    /* byte, above what the fp32 MFMA feeds at HBM speed): 96-102 -> 118-143 TFLOP/s. The 32-wide tiles of the level below */       \
    /* (N = 24) were measured on the staged kernel too: no change (88 split operations per 20 MFMAs) */                             \
    X(3, PRO_NONE, EPI_LINEAR) X(11, PRO_NONE, EPI_LINEAR)

// Which kernel families of igemm_split.hip exist for a row of DMX_SPLIT_COMBOS: linear-layer staging for the epilogues linear layers
// have; igemm_split_lin_kernel for the 128-wide tiles of at least 64 rows (cfg 0 / 7), the only kernel of the K / V plane
// projections besides the 128 x 256 linear tile of cfg 0
constexpr bool split_family_exists(int family, int cfg, int pro, int epi)
{
    const TileCfg t = kTileCfgs[cfg];
    const bool planes = epi == EPI_KPL || epi == EPI_VT;
    const bool linEpi = pro == PRO_NONE && (epi == EPI_LINEAR || epi == EPI_SCALE_RES || epi == EPI_GLU);
    const bool linTile = pro == PRO_NONE && (linEpi || planes) && t.WM == 2 && t.WN == 2 && t.NF == 4 && t.MF >= 2;
    return family == GF_SPLIT_STAGED       ? !planes
           : family == GF_SPLIT_STAGED_LIN ? linEpi
           : family == GF_SPLIT_LIN        ? linTile
           : family == GF_SPLIT_LINH       ? linTile
           : family == GF_SPLIT_LINW       ? linTile && t.MF == 4 && epi != EPI_GLU
                                           : false;
}

// igemm_split.hip igemm_split_linw_kernel<WNF, EPI, true>: X(column fragments per wave, epilogue) - the conv-addressed wide tiles
// (16 / 12 / 6: 128 x 256 / 192 / 96) and the narrow ones (4 / 2: 128 x 64 / 32), 128-row tiles whatever the op's tile cfg
#define DMX_LINW_COMBOS(X)                                            \
    X(16, EPI_LINEAR) X(16, EPI_GLU) X(16, EPI_TRCONV)                \
    X(12, EPI_LINEAR) X(12, EPI_GLU) X(12, EPI_TRCONV)                \
    X(6, EPI_LINEAR) X(6, EPI_GLU) X(6, EPI_TRCONV)                   \
    X(4, EPI_LINEAR) X(4, EPI_TRCONV) X(2, EPI_LINEAR)

// dgemm.hip dgemm_kernel: X(column fragments NF = ceil(N / 16), taps S1, seg0, prologue, epilogue, PIPE)
#define DMX_DIRECT_COMBOS(X)                                                                                         \
    /* DConv k1: Conv1d(C -> C/8, k3): C = 48, 96 (time branch; the frequency branch takes the ring kernels) */      \
    X(1, 3, 48, PRO_NONE, EPI_LINEAR, 0)                                                                             \
    X(1, 3, 96, PRO_NONE, EPI_LINEAR, 1)                                                                             \
    /* DConv k2 / k3: hidden 8 (C=48) / 12 (C=96) -> 2C, statistics / final */                                      \
    X(6, 1, 8, PRO_GN_GELU, EPI_STATS_ONLY, 2)                                                                       \
    X(1, 1, 8, PRO_GN_GELU, EPI_STATS_FACT, 0)                                                                       \
    X(1, 1, 12, PRO_GN_GELU, EPI_STATS_FACT, 0)                                                                      \
    X(6, 1, 8, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES, 0)                                                                 \
    X(12, 1, 12, PRO_GN_GELU, EPI_STATS_ONLY, 0)                                                                     \
    X(12, 1, 12, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES, 1)                                                               \
    /* Demucs v3 DConv (hidden C/4): k3 for hidden 12 (C=48) / 24 (C=96), factorised statistics for hidden 24 */     \
    X(6, 1, 12, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES, 0)                                                                \
    X(12, 1, 24, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES, 1)                                                               \
    X(2, 1, 24, PRO_GN_GELU, EPI_STATS_FACT, 0)                                                                      \
    /* first encoder convs (z-norm prologue) k8 s4: Cin = 4 (freq), 2 (time) */                                      \
    X(3, 1, 32, PRO_AFFINE, EPI_LINEAR, 0)                                                                           \
    X(3, 1, 16, PRO_AFFINE, EPI_LINEAR, 0)                                                                           \
    /* level-0 rewrites 48 -> 96 + GLU */                                                                            \
    X(6, 1, 48, PRO_NONE, EPI_GLU, 0)                                                                                \
    /* last transposed convs 48 -> 4*Cout: Cout = 16 / 8 (4 sources), 24 / 12 (6 sources) */                         \
    X(4, 1, 96, PRO_NONE, EPI_TRCONV, 0)                                                                             \
    X(2, 1, 96, PRO_NONE, EPI_TRCONV, 0)                                                                             \
    X(6, 1, 96, PRO_NONE, EPI_TRCONV, 0)                                                                             \
    X(3, 1, 96, PRO_NONE, EPI_TRCONV, 0)
// DConv k3 of the deep levels (C = 192 / 384: hidden 24 / 48 -> 2C = 384 / 768 packed columns): the weight matrix no longer fits one
// wave's registers, so the op runs as column chunks through the direct kernel (dgemm.hip launch_dgemm)
inline bool direct_chunked(int N, int S1, int seg0, int pro, int epi)
{
    return pro == PRO_GN_GELU && epi == EPI_GN_GLU_SCALE_RES && S1 == 1 && (seg0 == 24 || seg0 == 48) && N > 192 && N % 192 == 0;
}

// ---- membership in the lists (host side: gemm_select.cpp)
constexpr int combo_key(int cfg, int pro, int epi) { return cfg * 100 + pro * 10 + epi; }
constexpr int direct_key(int nf, int s1, int seg0, int pro, int epi) { return nf * 1000000 + s1 * 100000 + seg0 * 100 + pro * 10 + epi; }
#define DMX_KEY3(cfg, PRO, EPI) || key == combo_key(cfg, PRO, EPI)
#define DMX_KEY2(WNF, EPI) || (wnf == WNF && epi == EPI)
#define DMX_KEY6(NF, S1, SEG0, PRO, EPI, PIPE) || key == direct_key(NF, S1, SEG0, PRO, EPI)
inline bool tile_combo_exists(int cfg, int pro, int epi) { const int key = combo_key(cfg, pro, epi); return false DMX_TILE_COMBOS(DMX_KEY3); }
inline bool split_combo_exists(int cfg, int pro, int epi) { const int key = combo_key(cfg, pro, epi); return false DMX_SPLIT_COMBOS(DMX_KEY3); }
inline bool linw_combo_exists(int wnf, int epi) { return false DMX_LINW_COMBOS(DMX_KEY2); }
// shapes served by the direct kernels
inline bool direct_combo_exists(int N, int S1, int seg0, int pro, int epi)
{
    const int key = direct_key((N + 15) / 16, S1, seg0, pro, epi);
    return direct_chunked(N, S1, seg0, pro, epi) DMX_DIRECT_COMBOS(DMX_KEY6);
}
#undef DMX_KEY3
#undef DMX_KEY2
#undef DMX_KEY6

} // namespace dmx
