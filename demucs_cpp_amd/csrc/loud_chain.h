// loud_chain.h — the workspace of one whole track's output chain: the loudness measurements, the gains, the true peaks, the
// reports and the limiter, computed on the host. No HIP here: the one rule serves the stage alone
// (codec_api.cpp: the reports are the caller's buffers) and a track slot (tracks_exec.cpp: the reports live in the workspace),
// and tests/loud_chain_harness.cpp prints it.
#pragma once
#include "loudness_plan.h"
#include "meters_plan.h"
#include "limiter_plan.h"

namespace dmx
{
constexpr int kChainMaxOut = 8;       // PcmGains::kMaxOut: the gains take 32 bytes, the true peaks of a call without meters the next 32
constexpr int kChainGainBytes = 64;
constexpr int kChainReportBytes = 16; // sizeof(dmx_loudness_result) and sizeof(dmx_meters_result)
constexpr int kChainLimResBytes = 64; // kept per dmx_limit_result (24 bytes)

struct LoudChainMode
{
    bool meters;    // a meters report of n_out + 1 entries
    bool byTp;      // DMX_LOUD_TRUE_PEAK: the ceiling is the true peak
    bool limited;   // DMX_LOUD_LIMIT
    int limEnvs;    // the limiter's envelopes: 1 (the outputs linked) or n_out
    bool inside;    // the loudness and meters reports live in the workspace
};
// byte offsets from the workspace's base; a region the mode does not have is -1
struct LoudChain
{
    int64_t slotBytes;        // n_out + 1 measurement slots at 0, 16-byte aligned: the outputs, then the mixture
    int64_t gains;            // n_out floats
    int64_t truePeaks;        // tpWords bit patterns: n_out with byTp and no limiter, n_out + 1 with meters, else none
    int tpWords;
    int64_t report, meters;   // inside: n_out + 1 entries each, 8- and 4-byte aligned
    int64_t lim, envBytes;    // limEnvs envelope workspaces at a multiple of 64
    int64_t limRes;           // n_out results, 8-byte aligned
    int64_t total;
};

// n_out in [1, kChainMaxOut], n >= 1. The totals with the reports outside are what include/demucs_hip.h documents for
// dmx_loud_encode_device, dmx_loud_encode_meters_device and dmx_loud_encode_limit_device
inline LoudChain loud_chain_layout(int nOut, int64_t n, const LoudChainMode &m)
{
    LoudChain L{};
    L.slotBytes = loud_ws_bytes(n);
    L.gains = (int64_t)(nOut + 1) * L.slotBytes;
    int64_t off = L.gains + kChainGainBytes;
    L.tpWords = m.meters ? nOut + 1 : (m.byTp && !m.limited) ? nOut : 0;
    L.truePeaks = L.tpWords ? L.gains + (int64_t)sizeof(float) * kChainMaxOut : -1;
    if (m.meters)
    {
        // n_out + 1 true peaks do not fit behind the gains: they take one signal's meters part, and the caller of the stage
        // provides such a part per signal
        L.truePeaks = off;
        off += (m.inside ? 1 : nOut + 1) * meters_ws_bytes(n);
    }
    L.report = L.meters = -1;
    if (m.inside)
    {
        L.report = off;
        off += (int64_t)kChainReportBytes * (nOut + 1);
        if (m.meters)
        {
            L.meters = off;
            off += (int64_t)kChainReportBytes * (nOut + 1);
        }
    }
    L.lim = L.limRes = -1;
    if (m.limited)
    {
        L.envBytes = lim_ws_bytes(n);
        L.lim = (off + 63) & ~(int64_t)63;
        L.limRes = L.lim + m.limEnvs * L.envBytes;
        off = L.limRes + (int64_t)kChainLimResBytes * nOut;
    }
    L.total = off;
    return L;
}
} // namespace dmx
