// gemm_select.h — which tile and which kernel run an OP_IGEMM: decided once, on the host, when the op's plan is built, from plan
// fields, a few switches and a few facts about the model. The tile (cfg, NB) is chosen when plan.cpp finishes the op (choose_tile),
// the kernel on it when a context's plan is built (select_gemm: exec.cpp dmx_get_plan). The tiles and the compiled combinations are
// the tables of gemm_tiles.h; every rule is in gemm_select.cpp. The launchers (igemm.hip, dgemm.hip, igemm_lin256.hip,
// igemm_split.hip) launch what was chosen; the per-op profile labels (dmx_debug_profile, bench.py's roofline classes) are the
// choice's. No HIP here: plain C++.
#pragma once
#include "gemm_tiles.h"
#include <string>
#include <vector>

namespace dmx
{

// "linear layer" addressing applies (StageWalk LIN): one contiguous run of K floats per row, K a multiple of the K-tile.
// G: IGemm or GemmArgs (the same field names)
template <class G>
inline bool gemm_is_linear(const G &a, int pro, int epi, int ktile)
{
    return pro == PRO_NONE && (epi == EPI_LINEAR || epi == EPI_SCALE_RES || epi == EPI_GLU || epi == EPI_KPL || epi == EPI_VT) && a.S1 == 1 && a.pad0 == 0 &&
           a.seg0 == a.K && a.K == a.Kp && a.K % ktile == 0 && a.Np % 4 == 0 &&
           (i64)(a.P0 - 1) * a.stride0 * a.Cin + a.seg0 <= (i64)a.L0 * a.Cin && a.P1 == a.L1 && a.stride1 == 1 && a.pad1 == 0;
}
// what igemm_lin256.hip (cfg 19) takes, but for the presence of its residual and scale operands and the row bound: a plain linear
// layer (16-deep K-tiles) with one of its two epilogues and whole float4 column groups
template <class G>
inline bool lin256_addressing(const G &a)
{
    return gemm_is_linear(a, a.pro, a.epi, 16) && (a.epi == EPI_LINEAR || a.epi == EPI_SCALE_RES) && a.N % 4 == 0;
}
// 32-bit row arithmetic in the prologues of the LDS-tiled kernels (fp32 and split, lin256 included)
inline bool gemm_rows_ok(i64 M) { return M < (1ll << 31) - 256; }

// what the selection needs to know about the model bound to the context
struct GemmModelFacts
{
    bool bf16Planes = false, fp16Plane = false; // the weight blob exists as two bf16 planes / as one fp16 plane on the device
    i64 planeDelta = 0;                         // elements between the two bf16 planes
    // sorted blob offsets of the weights that are not the exact sum of their two bf16 terms / not fp16 numbers (true for
    // tensors that come straight from the fp16 file; derived ones are listed): an op that reads a listed element keeps fp32 /
    // bf16 terms. Computed when the weights are uploaded: the same for a model and every replica of it, so all devices of an
    // engine take the same decision
    const std::vector<i64> *inexactW = nullptr, *inexactH = nullptr;
};

// The options of a plan build with every A/B switch read from the environment: DMX_SPLIT_LIN once per process, DMX_LIN256,
// DMX_SHORTK and DMX_DCONV_ROW at every call (tests switch them between contexts of one process)
PlanOpts plan_opts_from_env(int gemm, bool kvPlanes);
// The A/B switch of the exact-split kernels (0 - 4, default 1: gemm_select.cpp), as plan_opts_from_env read it
int split_lin_mode();

// The tile of op g (K, Kp, Np and the batch stride set; cfg and NB are the result) in a plan of GEMM mode `gemm`. paired: the columns
// are GLU pairs; pin128Wide: the op must stay on the 128-wide tiles of at least 64 rows (cfg 0 / 7), the tiles the linear-layer
// kernels of the K / V plane projections and of the fp16 terms have: one kernel family, hence one arithmetic, at every batch size.
struct TileChoice
{
    int cfg, NB;
};
TileChoice choose_tile(const IGemm &g, bool paired, bool pin128Wide, int gemm, const GemmSwitches &sw);
// The tiles op g of a plan of GEMM mode `gemm` can be asked to run on (dmx_debug_run_op_as): the chain of its shape's tile and that
// tile's half-height siblings, then cfg 19 / 20 where everything but the row count of a launch admits them. Returns the count.
int gemm_tile_chain(const IGemm &g, int gemm, int *cfgs, int cap);

// The kernel of op g in a context of GEMM mode `gemm` (plan.h GemmMode) bound to a model with facts m. Depends on nothing else:
// the same op gets the same choice whenever it is asked. The ARITHMETIC of an op never depends on the number of rows or on linMode
// (one op, one arithmetic at every batch size: batching and sharding cannot change a bit); the family within an arithmetic may -
// all families of one arithmetic give the same bits.
GemmChoice select_gemm(const IGemm &g, int gemm, const GemmModelFacts &m, int linMode);

// Is the kernel g.choice names compiled, and does its launcher take the op? Family, tile, prologue and epilogue against the lists of
// gemm_tiles.h, and the limits the launchers apply. The launchers answer -1 to anything else (an internal error in dmx_launch_op).
bool gemm_kernel_exists(const IGemm &g);
// the same for the fp32 kernel of the op's tile, whatever was chosen (dmx_ctx_set_model may bind a model whose weights turn a
// split op to fp32)
bool gemm_fp32_kernel_exists(const IGemm &g);
// alignment contract of the igemm staging loads (igemm.hip header) + kernel availability: one OP_IGEMM / every OP_IGEMM of a plan
bool dmx_validate_gemm(const Op &op, std::string &why);
bool dmx_validate_plan(const Plan &p, std::string &why);

// The plan of a context: build_plan, then every OP_IGEMM's choice stored in the op. kvPlanes: the K / V projections may write the
// attention kernel's bf16 operand planes (PlanOpts::kvPlanes). All or nothing: if any such op cannot take its exact-split kernel
// (weights not two-plane exact) the plan is rebuilt in the fp32-K/V form.
void build_chosen_plan(const PackedModel &pm, i64 seg, int B, int gemm, bool kvPlanes, const GemmModelFacts &m, int linMode, Plan &plan);

inline bool operator==(const GemmChoice &a, const GemmChoice &b) { return a.family == b.family && a.arith == b.arith && a.wnf == b.wnf; }
inline bool operator!=(const GemmChoice &a, const GemmChoice &b) { return !(a == b); }

} // namespace dmx
