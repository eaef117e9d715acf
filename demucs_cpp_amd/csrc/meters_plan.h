// meters_plan.h — what the launches of the meters need (true peak, loudness range, momentary and short-term maxima; meters.hip,
// DESIGN.md section 2.15), computed on the host. No HIP here: the header is shared by the library (kernels.h) and by the kernel
// text compiled as host code (tests/meters_host_main.cpp).
#pragma once
#include "loudness_plan.h"

#include <cstdint>

namespace dmx
{
constexpr int kTpTaps = 12;                  // taps of a phase
constexpr int kTpHalo = kTpTaps / 2;         // frames a phase reaches to either side: x[i - 5 .. i + 6]
constexpr int kTpMaxFactor = 4;              // oversampling below 96 kHz
constexpr int kTpRun = 8;                    // consecutive frames of one lane
constexpr int kTpTile = 256 * kTpRun;        // frames of a workgroup: tiles sit at multiples of it, whatever the piece
constexpr int kMetersBins = 9001;            // the loudness-range histogram: bin k holds s_c = k - 7000, k in [1, 9000]
constexpr int kMetersShort = 30;             // hops of a short-term block (3 s)

struct TpFilter
{
    int F;                                   // 4 below 96 kHz, 2 below 192 kHz, else 1 (the sample peak)
    float h[kTpTaps * kTpMaxFactor + 1];     // 12 F + 1 taps, the rest zeros; phase p uses h[p + F j], j = 0 .. 11
};
// the factor for a rate, and the Hann-windowed sinc made in binary64 and rounded once to fp32 (libm's sin and cos)
int tp_factor(int rate);
void tp_filter(int rate, TpFilter *f);
// bytes per measured signal on top of loud_workspace_bytes(n): the true peak's bit pattern, padded to 64. -1 for n < 1
int64_t meters_workspace_bytes(int64_t n);
inline int64_t meters_ws_bytes(int64_t) { return 64; } // n >= 1
} // namespace dmx
