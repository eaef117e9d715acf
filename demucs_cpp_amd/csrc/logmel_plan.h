// logmel_plan.h — the geometry and the host-made tables of the log-mel stage (logmel.hip): the limits
// of the arguments, chunks and frames, the tile of a workgroup, the layout of the workspace, the mel filterbank. No HIP here.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace dmx
{
constexpr int kLogmelMinFft = 64, kLogmelMaxFft = 2048, kLogmelMaxMels = 128;
constexpr int kLogmelMelTiles = kLogmelMaxMels / 16; // accumulator tiles a wave keeps in registers
constexpr int kLogmelLds = 160 * 1024;               // bytes of LDS of a workgroup on gfx950
constexpr int kLogmelLdsStatic = 64;                 // the waves' maxima
constexpr int kLogmelSlabRow = 32 * 8;               // bytes of one table row of a bin tile: 16 x (w cos, -w sin) in binary64
enum { kMelSlaney = 0, kMelHtk = 1, kMelNormSlaney = 0, kMelNormNone = 1, kLogNone = 0, kLogDb = 1, kLogWhisper = 2 };

// the fields of dmx_logmel_spec (include/demucs_hip.h), in its order
struct LogmelSpec
{
    int sr, n_fft, hop, n_mels;
    double fmin, fmax;
    int mel_scale, mel_norm, log_mode, chunk_frames;
    double amin, top_db;
};

// NULL, or the name of the first bad field and why
inline const char *logmel_spec_error(const LogmelSpec &s)
{
    if (s.sr < 1)
        return "sr is below 1";
    if (s.n_fft < kLogmelMinFft || s.n_fft > kLogmelMaxFft || s.n_fft % 16)
        return "n_fft is not a multiple of 16 in [64, 2048]";
    if (s.hop < 1 || s.hop > s.n_fft)
        return "hop is not in [1, n_fft]";
    if (s.n_mels < 1 || s.n_mels > kLogmelMaxMels)
        return "n_mels is not in [1, 128]";
    if (!(s.fmin >= 0.0 && s.fmin < s.fmax && s.fmax <= 0.5 * s.sr))
        return "fmin, fmax do not satisfy 0 <= fmin < fmax <= sr / 2";
    if (s.mel_scale != kMelSlaney && s.mel_scale != kMelHtk)
        return "mel_scale is not DMX_MEL_SLANEY or DMX_MEL_HTK";
    if (s.mel_norm != kMelNormSlaney && s.mel_norm != kMelNormNone)
        return "mel_norm is not DMX_MEL_NORM_SLANEY or DMX_MEL_NORM_NONE";
    if (s.log_mode != kLogNone && s.log_mode != kLogDb && s.log_mode != kLogWhisper)
        return "log_mode is not DMX_LOG_NONE, DMX_LOG_DB or DMX_LOG_WHISPER";
    if (s.chunk_frames < 0)
        return "chunk_frames is negative";
    if (s.chunk_frames > 0 && (int64_t)s.chunk_frames * s.hop <= s.n_fft / 2)
        return "chunk_frames * hop is not above n_fft / 2";
    if (s.log_mode == kLogDb && !(s.amin > 0.0))
        return "amin is not above 0";
    return nullptr;
}
inline bool logmel_length_ok(const LogmelSpec &s, int64_t n)
{
    return n < ((int64_t)1 << 31) && (s.chunk_frames > 0 ? n >= 1 : n > s.n_fft / 2);
}

// the modes whose clamp needs the maximum of a (plane, chunk): they take the finish launch
inline bool logmel_needs_max(const LogmelSpec &s) { return s.log_mode == kLogWhisper || (s.log_mode == kLogDb && s.top_db > 0.0); }

// chunk c holds the samples [c len, (c + 1) len) of the plane (zeros behind its end) and gives `frames` frames
struct LogmelFrames
{
    int64_t chunks, frames, len;
};
inline LogmelFrames logmel_frames(const LogmelSpec &s, int64_t n)
{
    if (s.chunk_frames == 0)
        return LogmelFrames{1, 1 + n / s.hop, n};
    const int64_t len = (int64_t)s.chunk_frames * s.hop;
    return LogmelFrames{(n + len - 1) / len, s.chunk_frames, len};
}

// The tile of one workgroup: `ft` frames (16 per wave, so ft / 16 waves), their samples in LDS as fp32 and two table slabs
// of K rows. A frame starts hop + skew floats behind the one before it, skew = (4 - hop) mod 64: the 16 frames x 4 samples of
// one MFMA operand then fall into 64 different banks. Sample i of the tile sits at i + skew (i div hop).
struct LogmelTile
{
    int ft, K, skew, nft; // frames, slab rows, see above, bin tiles ceil((n_fft / 2 + 1) / 16)
    int64_t span, sampleFloats, ldsBytes;
};
inline LogmelTile logmel_tile_for(int n_fft, int hop, int ft, int K)
{
    LogmelTile t{};
    t.ft = ft, t.K = K, t.skew = ((4 - hop) % 64 + 64) % 64, t.nft = (n_fft / 2 + 1 + 15) / 16;
    t.span = (int64_t)(ft - 1) * hop + n_fft;
    t.sampleFloats = (t.span + t.skew * ((t.span - 1) / hop + 1) + 3) & ~(int64_t)3;
    t.ldsBytes = kLogmelLdsStatic + 4 * t.sampleFloats + 2 * (int64_t)K * kLogmelSlabRow;
    return t;
}
// the most frames, then the deepest slab (a divisor of n_fft, a multiple of 4, 16 .. 64), with which two workgroups share a CU's
// LDS; where none does, with which one fits
inline LogmelTile logmel_tile(int n_fft, int hop)
{
    for (int budget : {kLogmelLds / 2, kLogmelLds})
        for (int ft : {64, 32, 16})
            for (int K = 64; K >= 16; K -= 4)
                if (n_fft % K == 0 && logmel_tile_for(n_fft, hop, ft, K).ldsBytes <= budget)
                    return logmel_tile_for(n_fft, hop, ft, K);
    return LogmelTile{}; // (not reached for a spec the check accepts: 16 frames and 16 rows take at most 140 KB)
}

// byte offsets into the workspace, each a multiple of 256. [host, table) is made on the host and copied in one piece:
// tw: n_fft x (cos, sin)(2 pi k / n_fft); win: n_fft, the periodic Hann window; wt: [nft][8][4][64] doubles, the filterbank in
// operand order: element ((f * 8 + m) * 4 + s) * 64 + hi * 16 + lo is W[16 m + lo][16 f + 4 s + hi]; mask: [nft] ints, bit m
// set where that block of W is not all zero. table: [nft][n_fft / K][2][K][16] doubles, the windowed DFT matrix in slabs.
// tmax: [planes][chunks][tiles] doubles.
struct LogmelLayout
{
    LogmelFrames fr;
    LogmelTile tile;
    int64_t tiles; // of one chunk
    int64_t tw, win, wt, mask, table, tmax, hostBytes, bytes;
};
inline LogmelLayout logmel_layout(const LogmelSpec &s, int planes, int64_t n)
{
    LogmelLayout l{};
    l.fr = logmel_frames(s, n);
    l.tile = logmel_tile(s.n_fft, s.hop);
    l.tiles = (l.fr.frames + l.tile.ft - 1) / l.tile.ft;
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t o = at;
        at += (bytes + 255) & ~(int64_t)255;
        return o;
    };
    l.tw = take((int64_t)s.n_fft * 16);
    l.win = take((int64_t)s.n_fft * 8);
    l.wt = take((int64_t)l.tile.nft * kLogmelMelTiles * 256 * 8);
    l.mask = take((int64_t)l.tile.nft * 4);
    l.hostBytes = at;
    l.table = take((int64_t)l.tile.nft * s.n_fft * kLogmelSlabRow);
    l.tmax = take((int64_t)planes * l.fr.chunks * l.tiles * 8);
    l.bytes = at;
    return l;
}

// ---- the filterbank of librosa.filters.mel, in binary64
inline double logmel_hz_to_mel(double f, int scale)
{
    if (scale == kMelHtk)
        return 2595.0 * std::log10(1.0 + f / 700.0);
    const double f_sp = 200.0 / 3.0;
    return f >= 1000.0 ? 1000.0 / f_sp + std::log(f / 1000.0) / (std::log(6.4) / 27.0) : f / f_sp;
}
inline double logmel_mel_to_hz(double m, int scale)
{
    if (scale == kMelHtk)
        return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    const double f_sp = 200.0 / 3.0, min_log_mel = 1000.0 / f_sp;
    return m >= min_log_mel ? 1000.0 * std::exp(std::log(6.4) / 27.0 * (m - min_log_mel)) : f_sp * m;
}
// W [n_mels][n_fft / 2 + 1]
inline void logmel_filters(const LogmelSpec &s, double *W)
{
    const int F = s.n_fft / 2 + 1;
    std::vector<double> hz((size_t)s.n_mels + 2);
    const double lo = logmel_hz_to_mel(s.fmin, s.mel_scale), hi = logmel_hz_to_mel(s.fmax, s.mel_scale);
    for (int i = 0; i < s.n_mels + 2; ++i) // np.linspace: lo + i step, the last point hi itself
        hz[(size_t)i] = logmel_mel_to_hz(i == s.n_mels + 1 ? hi : lo + i * ((hi - lo) / (s.n_mels + 1)), s.mel_scale);
    for (int m = 0; m < s.n_mels; ++m)
    {
        const double d0 = hz[(size_t)m + 1] - hz[(size_t)m], d1 = hz[(size_t)m + 2] - hz[(size_t)m + 1];
        const double norm = s.mel_norm == kMelNormSlaney ? 2.0 / (hz[(size_t)m + 2] - hz[(size_t)m]) : 1.0;
        for (int f = 0; f < F; ++f)
        {
            const double bin = (double)f * s.sr / s.n_fft; // (np.fft.rfftfreq: f / (n_fft / sr))
            const double lower = (bin - hz[(size_t)m]) / d0, upper = (hz[(size_t)m + 2] - bin) / d1;
            const double w = lower < upper ? lower : upper;
            W[(size_t)m * F + f] = (w > 0.0 ? w : 0.0) * norm;
        }
    }
}

// the host-made part of the workspace, [0, hostBytes)
inline void logmel_host_tables(const LogmelSpec &s, const LogmelLayout &l, unsigned char *h)
{
    std::memset(h, 0, (size_t)l.hostBytes);
    double *tw = (double *)(h + l.tw), *win = (double *)(h + l.win), *wt = (double *)(h + l.wt);
    int *mask = (int *)(h + l.mask);
    const double pi = 3.141592653589793238462643383279502884;
    for (int k = 0; k < s.n_fft; ++k)
    {
        const double a = 2.0 * pi * k / s.n_fft;
        tw[2 * k] = std::cos(a), tw[2 * k + 1] = std::sin(a);
        win[k] = 0.5 - 0.5 * std::cos(a);
    }
    const int F = s.n_fft / 2 + 1;
    std::vector<double> W((size_t)s.n_mels * F);
    logmel_filters(s, W.data());
    for (int m = 0; m < s.n_mels; ++m)
        for (int f = 0; f < F; ++f)
        {
            const double w = W[(size_t)m * F + f];
            if (w == 0.0)
                continue;
            const int ft = f / 16, mt = m / 16, st = (f % 16) / 4, hi = f % 4, lo = m % 16;
            wt[((size_t)(ft * kLogmelMelTiles + mt) * 4 + st) * 64 + hi * 16 + lo] = w;
            mask[ft] |= 1 << mt;
        }
}
} // namespace dmx
