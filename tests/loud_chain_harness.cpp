// The workspace layout of the loudness / limiter output chain (csrc/loud_chain.h) as a stand-alone CPU program: one JSON line
// per case (tests/test_loud_chain_layout_cpu.py). No HIP, no library: the header is host arithmetic.
//   loud_chain_harness N...   every n_out in 1..8 x meters x true peak x limiter x envelopes {1, n_out} x reports inside / outside
#include "../demucs_cpp_amd/csrc/loud_chain.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a)
    {
        const long long n = std::atoll(argv[a]);
        for (int nOut = 1; nOut <= dmx::kChainMaxOut; ++nOut)
            for (int bits = 0; bits < 32; ++bits)
            {
                const dmx::LoudChainMode m{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) ? nOut : 1, (bits & 16) != 0};
                if (nOut == 1 && (bits & 8))
                    continue; // the same case
                const dmx::LoudChain L = dmx::loud_chain_layout(nOut, n, m);
                std::printf("{\"n_out\": %d, \"n\": %lld, \"meters\": %d, \"by_tp\": %d, \"limited\": %d, \"envs\": %d, \"inside\": %d, "
                            "\"W\": %lld, \"Mw\": %lld, \"Lw\": %lld, \"slot_bytes\": %lld, \"gains\": %lld, \"true_peaks\": %lld, \"tp_words\": %d, "
                            "\"report\": %lld, \"meters_out\": %lld, \"lim\": %lld, \"env_bytes\": %lld, \"lim_res\": %lld, \"total\": %lld}\n",
                            nOut, n, (int)m.meters, (int)m.byTp, (int)m.limited, m.limEnvs, (int)m.inside, (long long)dmx::loud_ws_bytes(n),
                            (long long)dmx::meters_ws_bytes(n), (long long)dmx::lim_ws_bytes(n), (long long)L.slotBytes, (long long)L.gains,
                            (long long)L.truePeaks, L.tpWords, (long long)L.report, (long long)L.meters, (long long)L.lim, (long long)L.envBytes,
                            (long long)L.limRes, (long long)L.total);
            }
    }
    return 0;
}
