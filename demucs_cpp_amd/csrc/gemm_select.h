// gemm_select.h — which kernel runs an OP_IGEMM: decided once, on the host, when the op's plan is built (exec.cpp dmx_get_plan), from plan
// fields and a few facts about the model. The launchers (igemm.hip, dgemm.hip, igemm_lin256.hip, igemm_split.hip) launch what was
// chosen; the per-op profile labels (dmx_debug_profile, bench.py's roofline classes) are the choice's. No HIP here: plain C++.
#pragma once
#include "plan.h"
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

// The (tile cfg, waves along M, waves along N, row fragments, column fragments, prologue, epilogue) combinations igemm_split.hip
// instantiates - the MFMA-bound tile families only (plan.h kTileCfgs): 0 / 7 / 15 (2x2 waves, 4 column fragments), 9 / 16 (2 column
// fragments), 2 / 10 (4x1 waves, 6 column fragments), 3 / 11 (4x1 waves, 3 column fragments, plain convs only). Anything else keeps
// its fp32 kernel. (The narrow tiles 5 / 12 / 6 / 13 have no staged form: gemm_select.cpp narrow_split_ok.)
#define DMX_SPLIT_COMBOS(X)                                                                                                   \
    X(0, 2, 2, 4, 4, PRO_NONE, EPI_LINEAR)                                                                                    \
    X(0, 2, 2, 4, 4, PRO_NONE, EPI_SCALE_RES)                                                                                 \
    X(0, 2, 2, 4, 4, PRO_NONE, EPI_GLU)                                                                                       \
    X(0, 2, 2, 4, 4, PRO_NONE, EPI_TRCONV)                                                                                    \
    X(7, 2, 2, 2, 4, PRO_NONE, EPI_LINEAR)                                                                                    \
    X(7, 2, 2, 2, 4, PRO_NONE, EPI_SCALE_RES)                                                                                 \
    X(7, 2, 2, 2, 4, PRO_NONE, EPI_GLU)                                                                                       \
    X(7, 2, 2, 2, 4, PRO_NONE, EPI_TRCONV)                                                                                    \
    /* K / V projections that write the attention kernel's operand planes (plan.cpp plane_linear) */                          \
    X(0, 2, 2, 4, 4, PRO_NONE, EPI_KPL)                                                                                       \
    X(0, 2, 2, 4, 4, PRO_NONE, EPI_VT)                                                                                        \
    X(7, 2, 2, 2, 4, PRO_NONE, EPI_KPL)                                                                                       \
    X(7, 2, 2, 2, 4, PRO_NONE, EPI_VT)                                                                                        \
    X(2, 4, 1, 2, 6, PRO_NONE, EPI_LINEAR)                                                                                    \
    X(2, 4, 1, 2, 6, PRO_NONE, EPI_GLU)                                                                                       \
    X(2, 4, 1, 2, 6, PRO_NONE, EPI_TRCONV)                                                                                    \
    /* half / quarter-height siblings (few segments in flight): same column decomposition, same bits as their parents */     \
    X(15, 2, 2, 1, 4, PRO_NONE, EPI_LINEAR)                                                                                   \
    X(15, 2, 2, 1, 4, PRO_NONE, EPI_SCALE_RES)                                                                                \
    X(15, 2, 2, 1, 4, PRO_NONE, EPI_GLU)                                                                                      \
    X(15, 2, 2, 1, 4, PRO_NONE, EPI_TRCONV)                                                                                   \
    X(9, 2, 2, 2, 2, PRO_NONE, EPI_LINEAR)                                                                                    \
    X(9, 2, 2, 2, 2, PRO_NONE, EPI_SCALE_RES)                                                                                 \
    X(9, 2, 2, 2, 2, PRO_NONE, EPI_GLU)                                                                                       \
    X(9, 2, 2, 2, 2, PRO_NONE, EPI_TRCONV)                                                                                    \
    X(16, 2, 2, 1, 2, PRO_NONE, EPI_LINEAR)                                                                                   \
    X(16, 2, 2, 1, 2, PRO_NONE, EPI_SCALE_RES)                                                                                \
    X(16, 2, 2, 1, 2, PRO_NONE, EPI_GLU)                                                                                      \
    X(16, 2, 2, 1, 2, PRO_NONE, EPI_TRCONV)                                                                                   \
    X(10, 4, 1, 1, 6, PRO_NONE, EPI_LINEAR)                                                                                   \
    X(10, 4, 1, 1, 6, PRO_NONE, EPI_GLU)                                                                                      \
    X(10, 4, 1, 1, 6, PRO_NONE, EPI_TRCONV)                                                                                   \
    /* 48-wide tiles (4 x 1 waves, 3 column fragments): the deepest DConv K1 convs (K = 3 C = 1152, N = C / 8 = 48: 72 flops  \
       per byte, above what the fp32 MFMA feeds at HBM speed): 96-102 -> 118-143 TFLOP/s. The 32-wide tiles of the level      \
       below (N = 24) were measured on the staged kernel too: no change (88 split operations per 20 MFMAs) */                 \
    X(3, 4, 1, 2, 3, PRO_NONE, EPI_LINEAR)                                                                                    \
    X(11, 4, 1, 1, 3, PRO_NONE, EPI_LINEAR)

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

// The A/B switch of the exact-split kernels (0 - 4, default 1: gemm_select.cpp), read from the environment once per process
int split_lin_mode();

// The kernel of op g in a context of GEMM mode `gemm` (plan.h GemmMode) bound to a model with facts m. Depends on nothing else:
// the same op gets the same choice whenever it is asked. The ARITHMETIC of an op never depends on the number of rows or on linMode
// (one op, one arithmetic at every batch size: batching and sharding cannot change a bit); the family within an arithmetic may -
// all families of one arithmetic give the same bits.
GemmChoice select_gemm(const IGemm &g, int gemm, const GemmModelFacts &m, int linMode);

// The plan of a context: build_plan, then every OP_IGEMM's choice stored in the op. kvPlanes: the K / V projections may write the
// attention kernel's bf16 operand planes (PlanOpts::kvPlanes). All or nothing: if any such op cannot take its exact-split kernel
// (weights not two-plane exact) the plan is rebuilt in the fp32-K/V form.
void build_chosen_plan(const PackedModel &pm, i64 seg, int B, int gemm, bool kvPlanes, const GemmModelFacts &m, int linMode, Plan &plan);

inline bool operator==(const GemmChoice &a, const GemmChoice &b) { return a.family == b.family && a.arith == b.arith && a.wnf == b.wnf; }
inline bool operator!=(const GemmChoice &a, const GemmChoice &b) { return !(a == b); }

} // namespace dmx
