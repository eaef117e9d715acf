// The host-only plan of a multi-track call (dmx_track_infer, dmx_tracks_infer*): everything the scheduler decides before
// any GPU work, from plain numbers. No HIP: this header and tracks_plan.cpp use the standard library and
// include/demucs_hip.h only, so the arithmetic can be built and checked without a GPU (tests/tracks_plan_harness.cpp).
// The executor that enqueues a plan is csrc/tracks_exec.cpp (tracks_run_impl).
#pragma once
#include "../../include/demucs_hip.h"

#include <cstdint>
#include <string>
#include <vector>

// stride = (int)((1 - overlap) * segment), evaluated in fp32 (model_apply.cpp:162)
int64_t overlap_stride(int64_t seg, float overlap);
// shifted_audio length = length + max_shift - offset (model_apply.cpp:119-120)
inline int64_t track_shifted_len(int64_t n, int shift) { return n + DMX_MAX_SHIFT - shift; }
// segments of the loop `offset += stride` over the shifted track (model_apply.cpp:189)
inline int track_n_segments(int64_t len, int64_t stride) { return (int)((len + stride - 1) / stride); }

struct TrackJob
{
    int64_t n;
    int kFirst, kLast; // the first / last batch (of any model) holding an item of the track
    int slot;          // the track slot it holds during batches [kFirst, kLast + 1]
    bool takeover;     // the slot had a holder (finished in batch kFirst - 2 or earlier): wait on that track's copy-out first
    // a track at another rate (dmx_tracks_infer_rates): n is its length at 44.1 kHz, m the caller's frames at `rate`;
    // rate 44100 (every track of the other entry points): m == n and nothing is converted
    int64_t m = 0;
    int rate = 44100;
    bool converted() const { return rate != 44100; }
    int64_t outFrames() const { return converted() ? m : n; } // the frames of its outputs
};
struct TrackModel // one model's items of one track
{
    int64_t g0, m; // g0: index of the track's first item in the model's sequence; m: its items (the sum of its copies' segment counts)
    int c0, nMin, nMax; // c0: its first copy; nMin / nMax: the fewest / most segments of a copy
};
struct TrackCopy
{
    int64_t len;
    int shift, nseg;
};
struct TrackPiece
{
    int t;
    int64_t lo, hi;
    size_t item0; // pieceItems[item0 + q]: the first item (within the track, of model q) the piece's overlap-add reads
};
struct TrackItem
{
    int t, k, g;
};
struct TrackBatch
{
    int q;  // the model
    int64_t g0; // its first item, in the model's sequence
    int nb;
};
struct PcmRange // frames [lo, hi) of track t encoded (or, in TracksPlan::native, converted) behind one batch
{
    int t;
    int64_t lo, hi;
};

struct TracksPlan
{
    int T = 0, Q = 0, N = 0, B = 0;
    int64_t seg = 0, stride = 0;
    std::vector<TrackJob> jobs;                // [T]
    std::vector<TrackModel> tm;                // [T][Q]
    std::vector<TrackCopy> copies;             // [T][Q][N]
    std::vector<std::vector<TrackItem>> items; // [Q]: model q's sequence, (track, row g, copy k) order
    std::vector<TrackBatch> batches;
    std::vector<int64_t> cum;                        // items done after batch k, over all models
    std::vector<std::vector<TrackPiece>> pieces; // [batch]: the output samples [lo, hi) that are final once batch k is done
    std::vector<int64_t> pieceItems;
    std::vector<int64_t> M, R, ringOff; // [Q]: items, ring blocks and first ring block of model q
    int64_t ringBlocks = 0, nmax = 0, Mtot = 0;
    int nSlots = 0;
    std::vector<std::vector<PcmRange>> pcm; // [batch] with a PCM stage, else empty; a converted track's are in native frames
    // [batch], tracks at another rate only: the frames [lo, hi) at the track's own rate that are final once the batch's
    // pieces are (dmx_resample_ready of the piece's end), in piece order; empty ranges are not listed
    std::vector<std::vector<PcmRange>> native;
    int64_t mmax = 0; // the most native frames of a converted track; 0: the call converts nothing

    int nBatches() const { return (int)batches.size(); }
    const TrackCopy &copy(int t, int q, int k) const { return copies[(size_t)(tm[(size_t)t * Q + q].c0 + k)]; }
};

// shifts: T x Q x N, row-major. ensTailCap: the most tail rows x copies of a track the ensemble overlap-add takes
// (TrackEnsTable::kMaxTail), < 0: no such cap (a bag checks its own, on the plan's nMin / nMax).
// rates (NULL: all 44100) and native (the caller's frames per track, read where rates[t] != 44100): n[t] is then the length
// at 44.1 kHz, ceil(native[t] * 44100 / rates[t]), on which everything but `native` and `pcm` is planned.
// DMX_OK, else an error code and its message in `err` (without the entry point's name)
int tracks_plan_build(TracksPlan &p, int T, const int64_t *n, int Q, int N, const int *shifts, int64_t seg, int64_t stride, int B, bool pcm,
                      int ensTailCap, std::string &err, const int *rates = nullptr, const int64_t *native = nullptr);
