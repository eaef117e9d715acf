// attention_select.h — which form of the exact-split attention kernel (attention_split.hip) runs an OP_ATTENTION: decided once, on
// the host, when the op's plan is built (exec.cpp dmx_get_plan -> plan.h Attention::form), as gemm_select.h decides the GEMM ops'.
// Plain C++, no HIP: a pure function of the op's shape. Every form computes the same bits (same key-tile order, same term order
// per query), so the choice is one of speed only. The fp32 kernel (attention.hip) has the two unpaired shapes and takes them by
// the same att_big_shape, decided at the same place.
#pragma once

namespace dmx
{

enum AttentionForm
{
    ATT_FORM_WG64 = 0,  // 256-thread workgroups of 64 queries
    ATT_FORM_WG128 = 1, // 256-thread workgroups of 128 queries
    ATT_FORM_PAIR = 2   // 512-thread workgroups: two 128-query halves one phase apart (planes form only)
};
inline const char *att_form_name(int form) { return form == ATT_FORM_PAIR ? "pair" : form == ATT_FORM_WG128 ? "wg128" : "wg64"; }

// 32 queries per wave (128 per workgroup) when that still leaves >= 2 rounds of workgroups per CU; the key-tile order,
// hence every rounding, is the same for both shapes. (rounds of the 512 resident workgroups) x (relative duration of
// one workgroup): the 64-query shape does ~0.6x the work of the 128-query one per workgroup (K/V LDS reads amortised
// over half the queries); e.g. Tq = 1344 at batch 12 is 1056 big workgroups = 2.06 rounds -> 3, or 2016 small = 3.94 ->
// 4 x 0.6. Below two full rounds of 128-query workgroups the launch is latency-bound, not matrix-bound, and the 64-query
// shape (twice the waves for the same work) wins whatever the round count says: measured at 1 / 2 / 4 segments
// 1.12 / 1.78 / 3.17 ms (64) vs 1.39 / 2.05 / 3.32 ms (128) for the ten attention launches of a plan run.
inline bool att_big_shape(int Tq, int H, int B)
{
    const long wg128 = (long)((Tq + 127) / 128) * H * B, wg64 = (long)((Tq + 63) / 64) * H * B;
    const double costBig = (double)((wg128 + 511) / 512), costSmall = 0.6 * (double)((wg64 + 511) / 512);
    return wg128 >= 1024 && costBig <= costSmall;
}

// The paired kernel exists for the planes form (whole 64-key tiles, operands already split) at head dims 64 and 48.
inline bool att_pair_exists(int Tk, int hs, bool planes) { return planes && Tk > 0 && Tk % 64 == 0 && (hs == 64 || hs == 48); }

// Where the rule takes the paired form: only for shapes at which profiles/attention_pair_ab.txt shows it faster than the 128-query
// workgroups. That is the frequency branch's queries (2688 tokens = 21 query tiles per (batch, head)) from 12 segments up
// (2016 tiles), 4 - 7 % per op; at the time branch's 1344 queries (11 tiles, the last one half empty) the two forms are level at
// 42 segments, and wherever the 64-query shape is chosen today the paired form is slower.
static constexpr int kAttPairMinQTiles = 21;
static constexpr long kAttPairMinTiles = 2016;

// pairMode (DMX_ATT_PAIR): 0 never, 1 by rule (unset), 2 wherever the kernel exists, at any size
inline int att_select_form(int Tq, int Tk, int H, int B, int hs, bool planes, int pairMode)
{
    const bool big = att_big_shape(Tq, H, B);
    if (pairMode == 2 && att_pair_exists(Tk, hs, planes))
        return ATT_FORM_PAIR;
    const int qTiles = (Tq + 127) / 128;
    if (pairMode == 1 && big && att_pair_exists(Tk, hs, planes) && qTiles >= kAttPairMinQTiles && (long)qTiles * H * B >= kAttPairMinTiles)
        return ATT_FORM_PAIR;
    return big ? ATT_FORM_WG128 : ATT_FORM_WG64;
}

// Workgroup barriers that one half (0: waves 0-3, 1: waves 4-7) of a paired workgroup passes on nt key tiles. s_barrier counts
// every wave of the workgroup, so the two halves must agree or the workgroup never ends. The terms follow the kernel's text
// (attention_split_body, PAIR): half B's stagger barrier, two in the prologue (K(0) and V(0) landed; S(0) done), one behind each
// alpha and each beta phase, half A's closing barrier beside half B's last beta.
constexpr int att_pair_barriers(int nt, int half) { return (half ? 1 : 0) + 2 + 2 * nt + (half ? 0 : 1); }
constexpr bool att_pair_barriers_agree(int ntMax)
{
    for (int nt = 1; nt <= ntMax; ++nt)
        if (att_pair_barriers(nt, 0) != att_pair_barriers(nt, 1))
            return false;
    return true;
}
static_assert(att_pair_barriers_agree(8), "the halves of a paired attention workgroup must pass the same number of barriers");

} // namespace dmx
