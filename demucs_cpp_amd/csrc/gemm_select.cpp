// gemm_select.cpp — the one place that decides which kernel runs an OP_IGEMM (gemm_select.h). Host arithmetic on plan fields.
#include "gemm_select.h"
#include <algorithm>
#include <cstdlib>

namespace dmx
{

// One function reads the switches. DMX_SPLIT_LIN, the A/B switch of the exact-split kernels: 1 (default) = every kernel where it
// applies and pays; 0 = linear layers on the staged 2 x 2-wave kernel and no wide tile (the K / V plane projections, which exist on
// the linear-layer kernels only, behave as under 1); 2 = never a wide tile; 3 = the wide tiles wherever they exist; 4 = as 1 with the
// 96-wide layers on the staged tile (bitwise A/B: tools/gpu_lin_ab.py). The others: 0 switches the tile / the op off (A/B).
PlanOpts plan_opts_from_env(int gemm, bool kvPlanes)
{
    static const int splitLin = [] { const char *e = getenv("DMX_SPLIT_LIN"); return e ? atoi(e) : 1; }();
    auto on = [](const char *e) { return !e || atoi(e) != 0; };
    PlanOpts o;
    o.gemm = gemm, o.kvPlanes = kvPlanes ? 1 : 0;
    o.sw.splitLin = splitLin, o.sw.lin256 = on(getenv("DMX_LIN256")), o.sw.shortK = on(getenv("DMX_SHORTK"));
    o.dconvRow = on(getenv("DMX_DCONV_ROW"));
    return o;
}
int split_lin_mode() { return plan_opts_from_env(GEMM_F32, false).sw.splitLin; }

// ---------------------------------------------------------------------------------------------------------------- the tile of an op
// The tile family of a width: never a function of the batch size, so results are bit-identical for any batching / sharding of
// segments. The 2 x 4 family comes out as cfg 0: refine_cfg walks down its chain 0 -> 7 -> 15 / 9 -> 16 from the ACTUAL
// row count (round 3: a nominal-batch choice between 0 and 7 kept the time-branch linears on 64x128 tiles even at 42 segments)
static int choose_cfg(int N, bool paired)
{
    if (!paired)
    {
        if (N <= 16)
            return 4;
        if (N <= 32)
            return 5;
        if (N <= 48)
            return 3;
    }
    else if (N <= 32)
        return 5;
    if (N <= 64)
        return 6;
    if (N <= 96)
        return 2;
    if (N % 128 != 0 && N % 96 == 0)
        return 2;
    return 0;
}

// Tile for an op at the ACTUAL number of rows M (all segments in flight): the largest tile of the chain cfg -> half_cfg(cfg) -> ...
// that keeps the 256 CUs evenly busy. Work per CU is what counts (co-resident workgroups share one matrix pipe per SIMD). A launch
// of T tiles puts n = ceil(T / 256) workgroups on its busiest CU; two resident workgroups hide each other's ds_read / barrier /
// staging latencies, ONE does not (measured at one segment per call: 252 tiles of 128x128 take 1.8x as long as
// 504 of 64x128 for the same op, decoder.1.rewrite 224 -> 126 us; the 3 qkv linears 71 -> 50 us). So the cost of
// a tile shape is  (n == 1 ? 1.7 : n) x tile area x (1 + small-tile overhead: staging bytes per MFMA grow as the
// tile shrinks: +3 % per halving, from forced-half runs at batch 24),
// minimised over the chain of bit-identical half-height siblings. Large batches keep the big tile; one segment
// (M = 2688 / 1344 rows) gets 64x64 tiles for its transformer linears.
static int refine_cfg(int cfg, i64 M, int N, bool stat)
{
    auto cost = [&](int c, int depth) {
        // the XCD-aware tile map (igemm.hip) deals ROW tiles round-robin to the 8 XCDs and runs all column tiles of a row
        // tile on that XCD: the busiest XCD holds ceil(tilesM / 8) x tilesN workgroups for its 32 CUs. (Counting T / 256
        // instead missed e.g. 84 x 6 tiles = 11 row tiles on four of the XCDs = 66 workgroups for 64 slots: a second
        // round for two stragglers, decoder.0.rewrite at 4 segments 617 us with 128x128 vs 428 us with 64x128.)
        const i64 tm = (M + kTileCfgs[c].BM - 1) / kTileCfgs[c].BM, tn = (N + kTileCfgs[c].BN - 1) / kTileCfgs[c].BN;
        const i64 n = (((tm + 7) / 8) * tn + 31) / 32;
        return (n == 1 ? 1.7 : (double)n) * (double)(kTileCfgs[c].BM * kTileCfgs[c].BN) * (1.0 + 0.03 * depth);
    };
    int best = cfg;
    double bestCost = cost(cfg, 0);
    int depth = 1;
    for (int c = half_cfg(cfg, stat); c >= 0; c = half_cfg(c, stat), ++depth)
        if (cost(c, depth) < bestCost * 0.95) // the model is good to a few per cent: leave the default tile unless it is clear
        {
            best = c;
            bestCost = cost(c, depth);
        }
    return best;
}

// The shapes of the two tiles choose_tile reaches from another tile by the ROW COUNT of a launch: everything but that count (the
// debug entry points of debug_api.cpp run an op on them at small sizes: gemm_tile_chain).
// cfg 19 (igemm_lin256.hip refuses anything else at run time): plain linear layers, residual and scale present where the epilogue
// reads them; N a multiple of 512 only: with three column tiles (N = 384: the channel up / down samplers) half as many, twice as
// large workgroups quantise worse on the 64 slots of an XCD than they gain (measured 126 -> 115, 121 -> 111 TFLOP/s)
static bool lin256_shape(const IGemm &g)
{
    return lin256_addressing(g) && (g.epi != EPI_SCALE_RES || (g.res >= 0 && g.scale_w >= 0)) && g.N % 512 == 0;
}
// cfg 20: the short-K ops of the 128x96 family, no row statistics
static bool shortk_shape(const IGemm &g)
{
    return g.rowstat < 0 && g.pro == PRO_NONE && (g.epi == EPI_LINEAR || g.epi == EPI_GLU || g.epi == EPI_TRCONV) && g.K <= 160;
}

// The HBM-bound layers the direct kernels (dgemm.hip) take from the tiles. They carry no residual operand for the LINEAR / TRCONV
// epilogues.
static bool direct_residual_ok(const IGemm &g) { return !((g.epi == EPI_LINEAR || g.epi == EPI_TRCONV) && g.res >= 0); }
static bool takes_direct(const IGemm &g, int gemm)
{
    // the level-0 1x1 rewrites (48 -> 96 + GLU) of an exact-split context run on the 128 x 96 direct-fragment split tile
    // (igemm_split.hip, round 6): 0.900 -> 0.815 / 0.435 -> 0.386 ms at 42 segments against the fp32 direct kernel, which
    // sits on the fp32 matrix pipe's ridge; an fp32 context keeps the direct kernel (its tiled fp32 form is 20 % slower)
    const bool rewrite0Split = gemm != GEMM_F32 && g.pro == PRO_NONE && g.epi == EPI_GLU && g.S1 == 1 && g.seg0 == 48 && g.N == 96;
    // likewise the frequency branch's last transposed conv (48 -> 4 x Cout, K = 96): N = 64 (4 sources; igemm_split.hip
    // narrow tile, narrow_split_ok: 0.947 -> 0.917 ms) and N = 96 (6 sources: 1.57 -> 1.22 ms). The time branch's (N = 32 / 48) stays on
    // the direct kernel (N = 32 measured: 0.286 -> 0.293 ms)
    const bool lastTrSplit = gemm != GEMM_F32 && g.pro == PRO_NONE && g.epi == EPI_TRCONV && g.S1 == 1 && g.seg0 == 96 && (g.N == 64 || g.N == 96);
    return direct_residual_ok(g) && !rewrite0Split && !lastTrSplit && direct_combo_exists(g.N, g.S1, g.seg0, g.pro, g.epi);
}

TileChoice choose_tile(const IGemm &g, bool paired, bool pin128Wide, int gemm, const GemmSwitches &sw)
{
    const i64 M = (i64)g.B * g.P1 * g.P0;
    int cfg = refine_cfg(choose_cfg(g.N, paired), M, g.N, g.rowstat >= 0);
    // (the operand-split path has no 256x128 / 256x96 form: its ops stay on the tiles igemm_split.hip instantiates)
    if (gemm == GEMM_F32)
    {
        // plain linear layers that keep the 128x128 tile (i.e. enough rows to fill the chip a few times over) run on the 256x128 /
        // four-wave kernel: the shape and at least three rounds of its workgroups on the 64 slots of an XCD (the tile map deals row
        // tiles to XCDs): at 1.75 rounds (time-branch linears with N = 512 at 42 segments) the 128x128 tile is 10 % faster
        const i64 perXcd = (((M + 255) / 256 + 7) / 8) * ((g.N + 127) / 128);
        if (sw.lin256 && lin256_shape(g) && cfg == 0 && perXcd >= 192)
            cfg = 19;
        // short-K ops of the 128x96 family (K <= 160: the level-1 1x1 rewrites, K = 96, and the time branch's last k3
        // rewrite, K = 144) run on the 256x96 tile with 16-deep K-tiles (cfg 20, plain loop): no half-empty last K-tile
        // (144 = 4.5 x 32) and a shorter pipeline fill - measured 88.8 -> 101.9, 84.6 -> 93.9, 90.4 -> 94.8 TFLOP/s at 42
        // segments; longer K stays on the interleaved 32-deep loop (decoder.3.rewrite, K = 432: 121 vs 118.7). Same column
        // decomposition and k order: identical bits.
        if (sw.shortK && cfg == 2 && shortk_shape(g) && M >= 65536)
            cfg = 20;
    }
    if (takes_direct(g, gemm))
        cfg = kDirectCfg;
    if (pin128Wide && cfg != 0 && cfg != 7)
        cfg = 7;
    return TileChoice{cfg, (g.N + kTileCfgs[cfg].BN - 1) / kTileCfgs[cfg].BN};
}

int gemm_tile_chain(const IGemm &g, int gemm, int *cfgs, int cap)
{
    const bool paired = g.epi == EPI_GLU || g.epi == EPI_GN_GLU_SCALE_RES;
    int n = 0;
    for (int cfg = choose_cfg(g.N, paired); cfg >= 0 && n < cap; cfg = half_cfg(cfg, g.rowstat >= 0))
        cfgs[n++] = cfg;
    if (gemm == GEMM_F32 && lin256_shape(g) && n < cap)
        cfgs[n++] = 19;
    if (gemm == GEMM_F32 && shortk_shape(g) && kTileCfgs[g.cfg].BN == 96 && n < cap)
        cfgs[n++] = 20;
    return n;
}

// -------------------------------------------------------------------------------------------------------------- the kernel on it
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
//     (48 -> 4 x 16, K = 96), which sat on the fp32 matrix pipe at 60 % of its peak in the direct kernel (takes_direct).
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
    const TileCfg &t = kTileCfgs[cfg];
    const GemmChoice fp32{t.kind == TK_DIRECT ? GF_DIRECT : t.kind == TK_LIN256 ? GF_LIN256 : GF_TILE, 0, 0, t.label};
    // exact splits: a split context, the bf16 planes, 32-bit row arithmetic in the kernels' prologues, and every weight the op reads
    // the exact sum of its two planes
    if (gemm == GEMM_F32 || !m.bf16Planes || !gemm_rows_ok(M) || !weights_exact(m.inexactW, g))
        return fp32;
    if (cfg == 5 || cfg == 12 || cfg == 6 || cfg == 13) // 128x32 / 64x32, 128x64 / 64x64 (4 x 1 waves)
    {
        const int np = (cfg == 5 || cfg == 12) ? 32 : 64;
        if (!narrow_split_ok(g, np))
            return fp32;
        return GemmChoice{GF_SPLIT_NARROW, 1, np / 16, t.splitLabel};
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
    const GemmChoice linFrag{GF_SPLIT_LIN, 1, 0, t.splitLabel};
    if (planes)
        return cfg == 0 && wide_tile_pays(g, M, linMode == 0 ? 1 : linMode) ? wide256 : linFrag;
    // plain linear layers of a width the 128 x 256 linear tile takes go there (below); every other full-height op - strided convs,
    // 3x3 / k3 / 1x1 rewrites, transposed convs - to the conv-addressed wide tiles where they exist and pay
    if ((cfg == 0 || cfg == 2) && !(lin && g.epi == EPI_LINEAR && g.N % 256 == 0))
        if (const int wnf = wide_conv_width(g, M, linMode)) // (96: the tile of cfg 2 with the activation fragments loaded straight into registers)
            return GemmChoice{GF_SPLIT_WIDE_CONV, 1, wnf, wnf == 16 ? "igemm_split_128x256" : wnf == 12 ? "igemm_split_128x192" : "igemm_split_128x96d"};
    if (!lin)
        return GemmChoice{GF_SPLIT_STAGED, 1, 0, t.splitLabel};
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
    return GemmChoice{GF_SPLIT_STAGED_LIN, 1, 0, t.splitLabel};
}

// ------------------------------------------------------------------------------------------------------------ does it exist
// (the limits are the launchers': dgemm.hip launch_dgemm, igemm.hip launch_igemm, igemm_lin256.hip lin256_ok)
bool gemm_fp32_kernel_exists(const IGemm &g)
{
    if (g.cfg < 0 || g.cfg >= kNumTileCfgs)
        return false;
    const i64 M = (i64)g.B * g.P1 * g.P0;
    switch (kTileCfgs[g.cfg].kind)
    {
    case TK_DIRECT: // 32-bit row and inner-row arithmetic; no residual operand on the LINEAR / TRCONV epilogues
        return M < (1ll << 31) - 16 && (i64)g.L0 * g.Cin < (1ll << 31) && direct_residual_ok(g) && direct_combo_exists(g.N, g.S1, g.seg0, g.pro, g.epi);
    case TK_LIN256:
        return gemm_rows_ok(M) && lin256_addressing(g) && (g.epi != EPI_SCALE_RES || (g.res >= 0 && g.scale_w >= 0));
    case TK_TILE:
        return gemm_rows_ok(M) && tile_combo_exists(g.cfg, g.pro, g.epi);
    default:
        return false;
    }
}

bool gemm_kernel_exists(const IGemm &g)
{
    if (g.cfg < 0 || g.cfg >= kNumTileCfgs)
        return false;
    const int kind = kTileCfgs[g.cfg].kind;
    switch (g.choice.family)
    {
    case GF_NONE:
        return false;
    case GF_DIRECT:
        return kind == TK_DIRECT && gemm_fp32_kernel_exists(g);
    case GF_LIN256:
        return kind == TK_LIN256 && gemm_fp32_kernel_exists(g);
    case GF_TILE:
        return kind == TK_TILE && gemm_fp32_kernel_exists(g);
    case GF_SPLIT_WIDE_CONV:
    case GF_SPLIT_NARROW:
        return gemm_rows_ok((i64)g.B * g.P1 * g.P0) && linw_combo_exists(g.choice.wnf, g.epi);
    default: // the staged and linear-layer families of igemm_split.hip
        return gemm_rows_ok((i64)g.B * g.P1 * g.P0) && split_combo_exists(g.cfg, g.pro, g.epi) &&
               split_family_exists(g.choice.family, g.cfg, g.pro, g.epi);
    }
}

bool dmx_validate_gemm(const Op &op, std::string &why)
{
    const IGemm &g = op.g;
    const bool al = ((i64)g.L0 * g.Cin) % 4 == 0 && (g.stride0 * g.Cin) % 4 == 0 && (g.pad0 * g.Cin) % 4 == 0 &&
                    g.seg0 % 4 == 0 && g.K % 4 == 0 && g.xBatchStride % 4 == 0 && (g.S1 == 1 || g.seg0 % 16 == 0) &&
                    (g.cfg == kDirectCfg || (g.Cin % 4 == 0 && g.seg0 % g.Cin == 0 && g.S1 * (g.seg0 / g.Cin) <= 31)); // one validity bit per tap (igemm.hip)
    const bool planes = g.epi == EPI_KPL || g.epi == EPI_VT; // exist on the exact-split kernels only; build_chosen_plan keeps them only there
    if (planes && g.choice.arith == 0)
    {
        why = "op " + op.name + ": K / V plane projection without its exact-split kernel";
        return false;
    }
    // the fp32 kernel must exist for split ops too: dmx_ctx_set_model may bind a model whose weights turn them to fp32
    const bool exists = (planes || gemm_fp32_kernel_exists(g)) && (g.choice.arith == 0 || gemm_kernel_exists(g));
    if (!al || !exists)
    {
        why = "op " + op.name + (al ? ": no kernel instantiated for its (tile, prologue, epilogue)" : ": staging alignment contract violated");
        return false;
    }
    return true;
}
bool dmx_validate_plan(const Plan &p, std::string &why)
{
    for (const Op &op : p.ops)
        if (op.kind == OP_IGEMM && !dmx_validate_gemm(op, why))
            return false;
    return true;
}

void build_chosen_plan(const PackedModel &pm, i64 seg, int B, int gemm, bool kvPlanes, const GemmModelFacts &m, int linMode, Plan &plan)
{
    PlanOpts opts = plan_opts_from_env(gemm, kvPlanes);
    opts.sw.splitLin = linMode;
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
