// tp_phases.h — the phases of the true-peak launch (meters.hip) that the limiter (limiter.hip) shares:
// the staged tile with its halo and the lane's window of 19 staged values. The includer defines MT_DEV and MT_HD (device
// code, or plain C++ where the kernel text is compiled as host code) and includes meters_plan.h.
#pragma once
namespace dmx
{
namespace
{
// ------------------------------------------------------------------------------------------------ true peak: the phases
constexpr int kTpLead = 8;                               // staged frames in front of the tile and behind it
constexpr int kTpStage = kTpTile + 2 * kTpLead;          // staged frames
constexpr int kTpWords = kTpStage + kTpStage / kTpRun;   // with one word of padding per 8
struct TpLds
{
    float x[2][kTpWords];
};
MT_DEV int tp_pos(int s) { return s + (s >> 3); }
// the frames a piece [i0, i1) of a signal of n frames evaluates
MT_HD void tp_range(i64 i0, i64 i1, i64 n, i64 &lo, i64 &hi)
{
    lo = i0 > kTpHalo ? i0 - kTpHalo : 0;
    hi = i1 >= n ? n : (i1 - kTpHalo > lo ? i1 - kTpHalo : lo);
}
// thread tid of 256 stages its groups of 4 frames of the tile at t0 (a multiple of 4) and of its halo
template <class Piece, class Gather>
MT_DEV void tp_stage(const Piece &pc, const Gather &gather, int o, i64 n, i64 t0, int tid, TpLds &sh)
{
    for (int g = tid; g < kTpStage / 4; g += 256)
    {
        const i64 i = t0 - kTpLead + 4 * g;
        const int cnt = i < 0 ? 0 : (n - i >= 4 ? 4 : (n > i ? (int)(n - i) : 0));
        float L[4] = {0.0f, 0.0f, 0.0f, 0.0f}, R[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (cnt > 0)
            gather(pc, o, i, cnt, L, R);
        for (int k = 0; k < 4; ++k)
        {
            const int at = tp_pos(4 * g + k);
            sh.x[0][at] = L[k], sh.x[1][at] = R[k];
        }
    }
}
// the largest |y| over both channels, the thread's 8 frames inside [lo, hi) and all phases
template <int F>
MT_DEV float tp_lane(const TpLds &sh, const TpFilter &f, int tid, i64 t0, i64 lo, i64 hi)
{
#pragma clang fp contract(off)
    float m = 0.0f;
    const i64 f0 = t0 + (i64)tid * kTpRun;
    if (f0 >= hi || f0 + kTpRun <= lo)
        return m;
    for (int c = 0; c < 2; ++c)
    {
        float w[kTpRun + kTpTaps - 1]; // w[k] = x[f0 - 5 + k]
#pragma unroll
        for (int k = 0; k < kTpRun + kTpTaps - 1; ++k)
            w[k] = sh.x[c][tp_pos(kTpRun * tid + (kTpLead - kTpHalo + 1) + k)];
#pragma unroll
        for (int r = 0; r < kTpRun; ++r)
        {
            const float a = fabsf(w[r + kTpHalo - 1]); // phase 0: the sample
            float mf = 0.0f;
            mf = a > mf ? a : mf;
#pragma unroll
            for (int p = 1; p < F; ++p)
            {
                float acc = f.h[p] * w[r + kTpTaps - 1];
#pragma unroll
                for (int j = 1; j < kTpTaps; ++j)
                {
                    const float q = f.h[p + F * j] * w[r + kTpTaps - 1 - j];
                    acc = acc + q;
                }
                const float b = fabsf(acc);
                mf = b > mf ? b : mf;
            }
            if (f0 + r >= lo && f0 + r < hi)
                m = mf > m ? mf : m;
        }
    }
    return m;
}

// tp_lane per frame: m[r] = the largest |y| over both channels and all phases of frame t0 + 8 tid + r, each |y| first
// multiplied by g (one fp32 product; the limiter's level). The same taps in the same order as tp_lane.
template <int F>
MT_DEV void tp_lane_frames(const TpLds &sh, const TpFilter &f, int tid, float g, float m[kTpRun])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < kTpRun; ++r)
        m[r] = 0.0f;
    for (int c = 0; c < 2; ++c)
    {
        float w[kTpRun + kTpTaps - 1]; // w[k] = x[f0 - 5 + k]
#pragma unroll
        for (int k = 0; k < kTpRun + kTpTaps - 1; ++k)
            w[k] = sh.x[c][tp_pos(kTpRun * tid + (kTpLead - kTpHalo + 1) + k)];
#pragma unroll
        for (int r = 0; r < kTpRun; ++r)
        {
            const float a = fabsf(g * w[r + kTpHalo - 1]); // phase 0: the sample
            m[r] = a > m[r] ? a : m[r];
#pragma unroll
            for (int p = 1; p < F; ++p)
            {
                float acc = f.h[p] * w[r + kTpTaps - 1];
#pragma unroll
                for (int j = 1; j < kTpTaps; ++j)
                {
                    const float q = f.h[p + F * j] * w[r + kTpTaps - 1 - j];
                    acc = acc + q;
                }
                const float b = fabsf(g * acc);
                m[r] = b > m[r] ? b : m[r];
            }
        }
    }
}
} // namespace
} // namespace dmx
