// gemm_select.cpp — the one place that decides which kernel runs an OP_IGEMM (gemm_select.h). Host arithmetic on plan fields.
#include "gemm_select.h"
#include <algorithm>
#include <cstdlib>

namespace dmx
{

// The A/B switch of the exact-split kernels: 1 (default) = every kernel where it applies and pays; 0 = linear layers on the staged
// 2 x 2-wave kernel and no wide tile (the K / V plane projections, which exist on the linear-layer kernels only, behave as under 1);
// 2 = never a wide tile; 3 = the wide tiles wherever they exist; 4 = as 1 with the 96-wide layers on the staged tile (bitwise A/B:
// tools/gpu_lin_ab.py)
int split_lin_mode()
{
    static const int mode = [] { const char *e = getenv("DMX_SPLIT_LIN"); return e ? atoi(e) : 1; }();
    return mode;
}

static const char *const kCfgNames[] = {"igemm_128x128", "igemm_64x64", "igemm_128x96", "igemm_128x48", "igemm_256x16", "igemm_128x32",
                                        "igemm_128x64",  "igemm_64x128", "dgemm_direct", "igemm_64x64", "igemm_64x96", "igemm_64x48",
                                        "igemm_64x32",   "igemm_64x64",  "igemm_128x16", "igemm_32x128", "igemm_32x64", "igemm_256x128", "igemm_256x128w4", "igemm_lin256x128", "igemm_256x96"};
static_assert(sizeof(kCfgNames) / sizeof(kCfgNames[0]) == kNumTileCfgs, "one label per tile configuration");

// the exact-split kernel of a tile cfg: its own roofline class
static const char *const kSplitNames[kNumTileCfgs] = {"igemm_split_128x128", nullptr, "igemm_split_128x96", "igemm_split_128x48", nullptr, "igemm_split_128x32d", "igemm_split_128x64d",
                                                      "igemm_split_64x128", nullptr, "igemm_split_64x64", "igemm_split_64x96", "igemm_split_64x48",
                                                      "igemm_split_128x32d", "igemm_split_128x64d", nullptr, "igemm_split_32x128", "igemm_split_32x64"};

static bool split_combo_exists(int cfg, int pro, int epi)
{
#define DMX_CASE(cfgid, WM_, WN_, MF, NF, PRO, EPI) case (cfgid * 100 + PRO * 10 + EPI):
    switch (cfg * 100 + pro * 10 + epi)
    {
        DMX_SPLIT_COMBOS(DMX_CASE)
        return true;
    default:
        return false;
    }
#undef DMX_CASE
}

// no listed (inexact) element inside the op's weights [w_w, w_w + Np * Kp)
static bool weights_exact(const std::vector<i64> *inexact, const IGemm &g)
{
    if (!inexact)
        return true;
    const i64 lo = g.w_w, hi = g.w_w + (i64)g.Np * g.Kp;
    auto it = std::lower_bound(inexact->begin(), inexact->end(), lo);
    return it == inexact->end() || *it >= hi;
}

// linear-layer staging of the exact-split kernels: a row is (uniform base) + (32-bit byte offset), so every offset - of the
// activations and of the weight planes, planeDelta elements apart - must fit 32 bits
static bool split_lin(const IGemm &g, i64 planeDelta)
{
    return gemm_is_linear(g, g.pro, g.epi, 32) && ((i64)g.B * g.xBatchStride + 64) * 4 < (1ll << 32) &&
           (planeDelta + (i64)g.Np * g.Kp + 64) * 2 < (1ll << 32);
}

// conv addressing of igemm_split_linw_kernel<., ., true>: a lane's 8 consecutive k never leave one tap (Cin a multiple of 8, whole
// taps), one validity bit per tap, 32-bit element offsets inside a batch element, whole float4 stores of the transposed conv
static bool conv_fragments_ok(const IGemm &g)
{
    return g.Kp % 16 == 0 && g.Cin > 0 && g.Cin % 8 == 0 && g.seg0 % g.Cin == 0 && g.seg0 >= 32 && g.S1 * (g.seg0 / g.Cin) <= 32 &&
           (i64)g.S1 * g.dil1 * g.L0 * g.Cin + g.seg0 < (1ll << 31) && (g.epi != EPI_TRCONV || g.Cout % 4 == 0);
}

// The 128 x 256 linear-layer tile (igemm_split_linw_kernel<16, ., false>) is taken per LAUNCH - it produces the bits of the 128-wide
// tiles - where it pays: N a multiple of 256 and enough row tiles that the half as many, twice as large workgroups still fill the
// 64 slots of an XCD at least `kWideMinRounds` times (the tile map deals row tiles to XCDs). mode: split_lin_mode()
static constexpr double kWideMinRounds = 2.5; // (2.62 rounds: linear1 1 - 3 % faster on the wide tile; 1.75: level)
static bool wide_tile_pays(const IGemm &g, i64 M, int mode)
{
    if (g.N % 256 != 0 || g.Np != g.N || g.Kp % 32 != 0 || mode == 2 || mode == 0 || (g.rowstat >= 0 && g.NB != g.N / 128))
        return false;
    if (mode == 3)
        return true;
    const i64 tm = (M + 127) / 128;
    return (double)(((tm + 7) / 8) * (g.N / 256)) / 64.0 >= kWideMinRounds;
}

// The conv-addressed wide tiles (igemm_split_linw_kernel<WNF, EPI, true>): column fragments per wave (16 = 128 x 256, 12 =
// 128 x 192, 6 = 128 x 96) this launch takes, or 0. Ops of the full-height 128 x 128 / 128 x 96 tiles without prologue and row
// statistics whose A rows are runs of whole 8-float pieces and whose width is whole wide tiles; per LAUNCH, by the same occupancy
// rule as wide_tile_pays (the results are the bits of the narrow tiles). mode: split_lin_mode() (0 / 2: never, 3: always)
static int wide_conv_width(const IGemm &g, i64 M, int mode)
{
    if (mode == 0 || mode == 2 || g.pro != PRO_NONE || !(g.epi == EPI_LINEAR || g.epi == EPI_GLU || g.epi == EPI_TRCONV) || g.rowstat >= 0)
        return 0;
    const int wnf = g.N % 256 == 0 ? 16 : g.N % 192 == 0 ? 12 : g.N == 96 ? 6 : 0;
    if (!wnf || g.Np != g.N || !conv_fragments_ok(g))
        return 0;
    if (mode == 3)
        return wnf;
    if (mode == 4 && wnf == 6) // (A/B switch: the 96-wide layers stay on the staged tile)
        return 0;
    // Measured at 1 - 42 segments per call against the narrow tile the plan chose (profiles/r06_experiments/wide_tile_rounds.txt):
    // the 96-wide form has the narrow tile's workgroup count and wins everywhere (13 - 24 %); an N = 192 layer replaces TWO 96-wide
    // tiles and is never slower from 0.66 rounds of an XCD's 64 slots on; the others pay from about one round (N = 768 at 0.98
    // rounds: 5 - 14 % faster; N = 384 / 512 at 0.66 rounds: 10 - 25 % slower)
    if (wnf == 6)
        return wnf;
    const i64 tm = (M + 127) / 128;
    return (double)(((tm + 7) / 8) * (g.N / (16 * wnf))) / 64.0 >= (g.N == 192 ? 0.6 : 0.9) ? wnf : 0;
}

// The narrow layers in exact-split arithmetic on the direct-fragment kernel, taken at EVERY batch size (full-height tile cfg and
// its half-height sibling alike: one arithmetic per op); where the conditions fail the op keeps its fp32 kernel.
//   cfg 5 / 12, N <= 32 (128 x 32, four workgroups per CU): the DConv K1 of the C = 192 levels (Conv1d(192 -> 24, k3): K = 576; row
//     statistics) - its fp32 tile (igemm_128x32) fetched every input row three times through LDS staging at 2.7x the algorithmic
//     HBM traffic; here the 88 split operations per 20 MFMAs that kept the staged split tile level with fp32 (round 4) are spread
//     over four workgroups per CU with nothing else to do (1.10 -> 1.03 ms per 42-segment step: the op is bound by its fragment loads);
//   cfg 6 / 13, N = 64 (128 x 64, three workgroups per CU): the frequency branch's last transposed conv of a 4-source model
//     (48 -> 4 x 16, K = 96), which sat on the fp32 matrix pipe at 60 % of its peak in the direct kernel (plan.cpp finish).
// No residual on the linear epilogue; row statistics on the 32-wide linear form only.
static bool narrow_split_ok(const IGemm &g, int np)
{
    return g.pro == PRO_NONE && (g.epi == EPI_LINEAR || (g.epi == EPI_TRCONV && np == 64)) && !(g.epi == EPI_LINEAR && g.res >= 0) && g.N <= np &&
           g.Np == np && g.NB == 1 && conv_fragments_ok(g) && !(g.rowstat >= 0 && (g.epi == EPI_TRCONV || np == 64));
}

GemmChoice select_gemm(const IGemm &g, int gemm, const GemmModelFacts &m, int linMode)
{
    const i64 M = (i64)g.B * g.P1 * g.P0;
    const int cfg = g.cfg;
    if (cfg < 0 || cfg >= kNumTileCfgs) // no such tile: nothing to launch (launch_op reports it)
        return GemmChoice{GF_NONE, 0, 0, "?"};
    const GemmChoice fp32{cfg == kDirectCfg ? GF_DIRECT : cfg == 19 ? GF_LIN256 : GF_TILE, 0, 0, kCfgNames[cfg]};
    // exact splits: a split context, the bf16 planes, 32-bit row arithmetic in the kernels' prologues, and every weight the op reads
    // the exact sum of its two planes
    if (gemm == GEMM_F32 || !m.bf16Planes || M >= (1ll << 31) - 256 || !weights_exact(m.inexactW, g))
        return fp32;
    if (cfg == 5 || cfg == 12 || cfg == 6 || cfg == 13) // 128x32 / 64x32, 128x64 / 64x64 (4 x 1 waves)
    {
        const int np = (cfg == 5 || cfg == 12) ? 32 : 64;
        if (!narrow_split_ok(g, np))
            return fp32;
        return GemmChoice{GF_SPLIT_NARROW, 1, np / 16, kSplitNames[cfg]};
    }
    if (!split_combo_exists(cfg, g.pro, g.epi))
        return fp32;
    const bool planes = g.epi == EPI_KPL || g.epi == EPI_VT;
    const bool linTile = cfg == 0 || cfg == 7; // the 128-wide tiles of at least 64 rows: the tiles igemm_split_lin_kernel has
    const bool lin = split_lin(g, m.planeDelta);
    // the K / V plane projections exist on the linear-layer kernels only (plan.cpp plane_linear keeps them on 128- / 64-row tiles;
    // the V^T form needs its transposed MFMAs): get_plan rebuilds the plan in the fp32-K/V form where one cannot take them
    if (planes && !(linTile && lin))
        return fp32;
    // fp16 terms (contexts of GEMM_FP16X3, ops the plan marks): the linear-layer kernel on ONE fp16 weight plane, where every weight
    // the op reads is an fp16 number
    if (gemm == GEMM_FP16X3 && m.fp16Plane && g.hterms && linTile && split_lin(g, 0) && weights_exact(m.inexactH, g))
        return GemmChoice{GF_SPLIT_LINH, 2, 0, cfg == 0 ? "igemm_splith_128x128" : "igemm_splith_64x128"};
    const GemmChoice wide256{GF_SPLIT_LINW, 1, 0, "igemm_split_128x256"};
    const GemmChoice linFrag{GF_SPLIT_LIN, 1, 0, kSplitNames[cfg]};
    if (planes)
        return cfg == 0 && wide_tile_pays(g, M, linMode == 0 ? 1 : linMode) ? wide256 : linFrag;
    // plain linear layers of a width the 128 x 256 linear tile takes go there (below); every other full-height op - strided convs,
    // 3x3 / k3 / 1x1 rewrites, transposed convs - to the conv-addressed wide tiles where they exist and pay
    if ((cfg == 0 || cfg == 2) && !(lin && g.epi == EPI_LINEAR && g.N % 256 == 0))
        if (const int wnf = wide_conv_width(g, M, linMode)) // (96: the tile of cfg 2 with the activation fragments loaded straight into registers)
            return GemmChoice{GF_SPLIT_WIDE_CONV, 1, wnf, wnf == 16 ? "igemm_split_128x256" : wnf == 12 ? "igemm_split_128x192" : "igemm_split_128x96d"};
    if (!lin)
        return GemmChoice{GF_SPLIT_STAGED, 1, 0, kSplitNames[cfg]};
    if (linTile)
    {
        // activation fragments straight into registers (igemm_split_lin_kernel): same tile size and map, same bits; mode 0 keeps
        // the staged form (A/B comparison). Measured at 42 segments (profiles/DESIGN_history_r1-r4.md 7.6): the 34 linear-layer
        // launches 24.62 -> 24.44 ms - the loop is bound by the energy of the bytes it moves from L2, which this form does not
        // change; a 256 x 128 tile with one workgroup per CU (one wave per SIMD, 445 registers) was 15 % slower and is not kept.
        if (cfg == 0 && g.epi != EPI_GLU && wide_tile_pays(g, M, linMode))
            return wide256;
        if (linMode != 0)
            return linFrag;
    }
    return GemmChoice{GF_SPLIT_STAGED_LIN, 1, 0, kSplitNames[cfg]};
}

void build_chosen_plan(const PackedModel &pm, i64 seg, int B, int gemm, bool kvPlanes, const GemmModelFacts &m, int linMode, Plan &plan)
{
    PlanOpts opts;
    opts.gemm = gemm, opts.kvPlanes = kvPlanes ? 1 : 0;
    build_plan(pm, seg, B, plan, opts);
    if (kvPlanes)
        for (const Op &op : plan.ops)
            if (op.kind == OP_IGEMM && (op.g.epi == EPI_KPL || op.g.epi == EPI_VT) && select_gemm(op.g, gemm, m, linMode).arith == 0)
            {
                opts.kvPlanes = 0;
                plan = Plan();
                build_plan(pm, seg, B, plan, opts);
                break;
            }
    for (Op &op : plan.ops)
        if (op.kind == OP_IGEMM)
            op.g.choice = select_gemm(op.g, gemm, m, linMode);
}

} // namespace dmx
