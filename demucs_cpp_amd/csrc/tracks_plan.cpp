// The plan of a multi-track call: host arithmetic only (tracks_plan.h). The executor is csrc/tracks_exec.cpp.
//
// Several tracks: their segments are laid end to end in track order (global item index) and dealt in batches of
// max_batch, so a batch may hold the tail of one track and the head of the next. Every kernel serves each of its tracks
// exactly as it serves a track of its own (tracks.hip), so every result is the bits of a call per track.
// The shifts ensemble (N copies of each track, dmx_tracks_infer_opts): the items of a track are its copies' segments in
// (row g, copy k) order, a copy absent from the rows past its last segment (the copies' segment counts differ when their
// shifted lengths straddle a multiple of the stride), so the copies of one stretch of the track are adjacent.
//   * Segment outputs live in a ring of R blocks: global item G is block G mod R. R is planned on the host before any GPU
//     work: the largest distance from the first item an overlap-add reads to the end of its batch, rounded up to a multiple
//     of max_batch, at least 2 max_batch, at most the total number of items. Batch k writes blocks [k B mod R, + nb)
//     (contiguous: B divides R, or nothing wraps), which the overlap-adds behind batch k-1 and earlier no longer read; all
//     of it is ordered on the context's stream. One copy at overlap 0.25 reads back one item at most: R = 2 max_batch.
//   * A piece of a track is final when, for every copy, every segment covering it is done: its end is the minimum over the
//     copies of "shifted positions below (segments done) * stride".
//   * A track holds a slot (upload, statistics, result) from the batch of its first item until its last copy-out has
//     completed. Batch k needs the slots of the tracks with first batch <= k and last batch >= k-1 (the copy-out of batch
//     k-1 is issued after batch k has been enqueued); the call sizes that many slots for its longest track up front.
//     A slot whose track finished in batch k-2 or earlier is taken over after a host wait on that track's copy-out event
//     (its batch is long done). Every call starts with all slots free and the pick is deterministic, so the plan fixes
//     each track's slot, and whether taking it means that wait, ahead of the GPU work.
//   * A track is uploaded (and its statistics computed) when the first batch that needs it is enqueued.
// The PCM output stage: pieces are encoded in whole groups of 4 frames (the up to 3 frames left over go with the next
// piece; the last piece ends at n); the plan holds these ranges per batch.
// A bag of Q models (dmx_tracks_infer_bag): the call has a model dimension. A track is uploaded once
// and its statistics are computed once; model q's items are the (track, row, copy) sequence above for its own shifts, in a
// sequence and a ring of its own (each ring sized by the rule above from the reach of the overlap-adds into THAT model's
// items); a batch holds items of one model, and the context is rebound (dmx_ctx_set_model) between batches. The next batch
// is always dealt from the model that lags furthest behind - the one whose next item has the lowest (track, row), the lowest
// q on a tie - so the models advance through the tracks abreast (round-robin when their shifts agree) and no ring has to
// span more than the other models' batch in flight: the memory bound stays independent of the number and length of tracks.
// A piece is final when every copy of every model has covered it.
// Tracks at another rate (dmx_tracks_infer_rates): everything above is planned on the track's length
// at 44.1 kHz. Behind a piece that ends at `hi` the converter (resample.hip) can finish the native-rate outputs below
// K(hi) = dmx_resample_ready(hi, ...): output k's newest tap is input (c + k M) div L, so K is the first k with
// c + k M >= hi L. The plan lists these native ranges per batch, and the PCM ranges of such a track are cut from them.
#include "tracks_plan.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <numeric>

typedef int64_t i64;

extern "C" int64_t dmx_resample_ready(int64_t n_in_final, int64_t n_in, int rate_in, int rate_out, int64_t n_out)
{
    if (n_in_final < 0 || n_in_final > n_in || rate_in < 1 || rate_out < 1 || n_out < 0)
        return -1;
    if (n_in_final == n_in)
        return n_out;
    const int g = std::gcd(rate_in, rate_out);
    const i64 L = rate_out / g, M = rate_in / g, c = 16 * std::max(L, M);
    if (n_in_final > (INT64_MAX - M) / L)
        return -1;
    const i64 num = n_in_final * L - c; // the first k with c + k M >= n_in_final L
    return std::min<i64>(n_out, num <= 0 ? 0 : (num + M - 1) / M);
}

i64 overlap_stride(i64 seg, float overlap) { return (i64)((1.0f - overlap) * (float)seg); }

namespace
{
int plan_fail(std::string &err, const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0)
{
    char msg[160];
    snprintf(msg, sizeof(msg), fmt, a, b, c, d);
    err = msg;
    return DMX_ERR_ARG;
}

// item index of (row g, copy k) within a track (tracks.hip ens_item)
i64 track_item(const TrackCopy *cp, int N, int nMin, i64 g, int k)
{
    if (g < nMin)
        return g * N + k;
    i64 it = 0;
    for (int q = 0; q < N; ++q)
    {
        const i64 nq = cp[q].nseg;
        it += std::min<i64>(g, nq);
        if (q < k && nq > g)
            ++it;
    }
    return it;
}

// copy geometry, and each model's item sequence
int plan_items(TracksPlan &p, const int64_t *n, const int *shifts, int ensTailCap, const int *rates, const int64_t *native, std::string &err)
{
    const int T = p.T, Q = p.Q, N = p.N;
    p.jobs.resize((size_t)T);
    p.tm.resize((size_t)T * Q);
    p.copies.resize((size_t)T * Q * N);
    p.M.assign((size_t)Q, 0);
    for (int t = 0; t < T; ++t)
    {
        p.jobs[(size_t)t] = TrackJob{n[t], INT_MAX, -1, -1, false};
        p.jobs[(size_t)t].m = n[t];
        if (rates && rates[t] != 44100)
        {
            TrackJob &j = p.jobs[(size_t)t];
            j.rate = rates[t], j.m = native[t];
            const i64 g = j.rate < 1 ? 1 : std::gcd(j.rate, 44100), up = 44100 / g, down = j.rate / g; // to 44.1 kHz
            if (j.rate < 1 || j.m < 1 || n[t] != (j.m * up + down - 1) / down)
                return plan_fail(err, "internal error (track %lld: %lld frames at %lld Hz are not %lld at 44100 Hz)", t, j.m, j.rate, n[t]);
            p.mmax = std::max<i64>(p.mmax, j.m);
        }
        for (int q = 0; q < Q; ++q)
        {
            TrackModel &x = p.tm[(size_t)t * Q + q];
            x.c0 = (t * Q + q) * N, x.m = 0, x.nMin = INT_MAX, x.nMax = 0;
            for (int k = 0; k < N; ++k)
            {
                TrackCopy &cp = p.copies[(size_t)(x.c0 + k)];
                cp.shift = shifts[x.c0 + k];
                cp.len = track_shifted_len(n[t], cp.shift);
                cp.nseg = track_n_segments(cp.len, p.stride);
                x.nMin = std::min(x.nMin, cp.nseg), x.nMax = std::max(x.nMax, cp.nseg);
                x.m += cp.nseg;
            }
            if (ensTailCap >= 0 && (x.nMax - x.nMin) * N > ensTailCap) // cannot happen for a context's segment (>= 4096) and overlap <= 0.9
                return plan_fail(err, "internal error (track %lld: %lld tail rows x %lld shifts)", t, x.nMax - x.nMin, N);
            if (x.m > INT_MAX / 2)
                return plan_fail(err, "track %lld: too many segments (%lld)", t, x.m);
            x.g0 = p.M[(size_t)q];
            p.M[(size_t)q] += x.m;
        }
        p.nmax = std::max<i64>(p.nmax, n[t]);
    }
    p.items.resize((size_t)Q);
    for (int q = 0; q < Q; ++q)
    {
        p.items[(size_t)q].reserve((size_t)p.M[(size_t)q]);
        for (int t = 0; t < T; ++t)
        {
            const TrackModel &x = p.tm[(size_t)t * Q + q];
            for (int g = 0; g < x.nMax; ++g)
                for (int k = 0; k < N; ++k)
                    if (g < p.copies[(size_t)(x.c0 + k)].nseg)
                        p.items[(size_t)q].push_back(TrackItem{t, k, g});
        }
        p.Mtot += p.M[(size_t)q];
    }
    return DMX_OK;
}

// the batches: each of one model, dealt from the model whose next item is the earliest (track, row)
void plan_batches(TracksPlan &p)
{
    std::vector<i64> pos((size_t)p.Q, 0);
    i64 all = 0;
    for (;;)
    {
        int pick = -1;
        for (int q = 0; q < p.Q; ++q)
        {
            if (pos[(size_t)q] >= p.M[(size_t)q])
                continue;
            if (pick < 0)
            {
                pick = q;
                continue;
            }
            const TrackItem &a = p.items[(size_t)q][(size_t)pos[(size_t)q]], &b = p.items[(size_t)pick][(size_t)pos[(size_t)pick]];
            if (a.t < b.t || (a.t == b.t && a.g < b.g))
                pick = q;
        }
        if (pick < 0)
            break;
        const i64 g0 = pos[(size_t)pick];
        const int nb = (int)std::min<i64>(p.B, p.M[(size_t)pick] - g0);
        const int k = (int)p.batches.size();
        for (i64 g = g0; g < g0 + nb; ++g)
        {
            TrackJob &j = p.jobs[(size_t)p.items[(size_t)pick][(size_t)g].t];
            j.kFirst = std::min(j.kFirst, k), j.kLast = std::max(j.kLast, k);
        }
        p.batches.push_back(TrackBatch{pick, g0, nb});
        p.cum.push_back(all += nb);
        pos[(size_t)pick] += nb;
    }
}

// the pieces each batch makes final and the items their overlap-adds read; reach[q]: the rings they need
int plan_pieces(TracksPlan &p, std::vector<i64> &reach, std::string &err)
{
    const int T = p.T, Q = p.Q, N = p.N;
    const i64 seg = p.seg, stride = p.stride;
    p.pieces.resize(p.batches.size());
    std::vector<int> segDone(p.copies.size(), 0);
    std::vector<i64> done((size_t)T, 0), dealt((size_t)Q, 0);
    int tLo = 0;
    for (int k = 0; k < p.nBatches(); ++k)
    {
        const TrackBatch &bt = p.batches[(size_t)k];
        while (p.jobs[(size_t)tLo].kLast < k)
            ++tLo;
        for (i64 g = bt.g0; g < bt.g0 + bt.nb; ++g)
        {
            const TrackItem &it = p.items[(size_t)bt.q][(size_t)g];
            ++segDone[(size_t)(p.tm[(size_t)it.t * Q + bt.q].c0 + it.k)];
        }
        dealt[(size_t)bt.q] = bt.g0 + bt.nb;
        for (int t = tLo; t < T && p.jobs[(size_t)t].kFirst <= k; ++t)
        {
            const i64 n = p.jobs[(size_t)t].n, lo = done[(size_t)t];
            const size_t all = (size_t)t * Q * N;
            // shifted-track positions below (segments done)*stride are covered only by segments done
            i64 fin = n;
            for (size_t x = all; x < all + (size_t)(Q * N); ++x)
                if (segDone[x] < p.copies[x].nseg)
                    fin = std::min<i64>(fin, (i64)segDone[x] * stride - (DMX_MAX_SHIFT - p.copies[x].shift));
            fin = std::max<i64>(lo, fin);
            TrackPiece pc{t, lo, fin, p.pieceItems.size()};
            p.pieceItems.resize(p.pieceItems.size() + (size_t)Q, 0);
            for (int q = 0; q < Q && fin > lo; ++q)
            {
                const TrackModel &x = p.tm[(size_t)t * Q + q];
                const TrackCopy *cp = &p.copies[(size_t)x.c0];
                i64 itemLo = INT64_MAX, itemHi = -1;
                for (int r = 0; r < N; ++r)
                {
                    const i64 j0 = lo + DMX_MAX_SHIFT - cp[r].shift; // first shifted position of the piece: its first segment
                    const i64 gLo = j0 - seg + 1 <= 0 ? 0 : (j0 - seg + stride) / stride;
                    const i64 gHi = std::min<i64>(cp[r].nseg - 1, (fin - 1 + DMX_MAX_SHIFT - cp[r].shift) / stride); // its last
                    itemLo = std::min(itemLo, track_item(cp, N, x.nMin, gLo, r));
                    itemHi = std::max(itemHi, track_item(cp, N, x.nMin, gHi, r));
                }
                if (itemLo < 0 || itemHi >= dealt[(size_t)q] - x.g0) // every segment the piece reads must be done
                    return plan_fail(err, "internal error (track %lld reads item %lld of model %lld after batch %lld)", t, itemHi, q, k);
                p.pieceItems[pc.item0 + (size_t)q] = itemLo;
                reach[(size_t)q] = std::max(reach[(size_t)q], dealt[(size_t)q] - (x.g0 + itemLo));
            }
            p.pieces[(size_t)k].push_back(pc);
            done[(size_t)t] = fin;
        }
    }
    return DMX_OK;
}

// slots: track t is held during batches [kFirst, kLast + 1]
int plan_slots(TracksPlan &p, std::string &err)
{
    const int nBatches = p.nBatches();
    std::vector<int> diff((size_t)nBatches + 2, 0);
    for (const TrackJob &j : p.jobs)
        ++diff[(size_t)j.kFirst], --diff[(size_t)j.kLast + 2];
    int live = 0;
    for (int k = 0; k <= nBatches; ++k)
        p.nSlots = std::max(p.nSlots, live += diff[(size_t)k]);
    // the tracks take their slots in the order of their first batches, which is track order
    std::vector<int> holder((size_t)p.nSlots, -1);
    for (int t = 0; t < p.T; ++t)
    {
        TrackJob &j = p.jobs[(size_t)t];
        const int k = j.kFirst;
        // a free slot, else the one whose track finished first (in batch k-2 or earlier: its copy-out has been issued)
        int pick = -1;
        for (int i = 0; i < p.nSlots; ++i)
        {
            const int h = holder[(size_t)i];
            if (h < 0)
            {
                pick = i;
                break;
            }
            if (p.jobs[(size_t)h].kLast <= k - 2 && (pick < 0 || p.jobs[(size_t)h].kLast < p.jobs[(size_t)holder[(size_t)pick]].kLast))
                pick = i;
        }
        if (pick < 0)
            return plan_fail(err, "internal error (no free track slot in batch %lld)", k);
        j.takeover = holder[(size_t)pick] >= 0;
        holder[(size_t)pick] = t, j.slot = pick;
    }
    return DMX_OK;
}

// the output frames that are final behind a piece: its end, or for a track at another rate the native frames ready then
i64 piece_out_hi(const TracksPlan &p, const TrackPiece &pc)
{
    const TrackJob &j = p.jobs[(size_t)pc.t];
    return j.converted() ? dmx_resample_ready(pc.hi, j.n, 44100, j.rate, j.m) : pc.hi;
}

// the native-rate frames each batch's converter finishes, for the tracks at another rate
void plan_native(TracksPlan &p)
{
    p.native.resize(p.batches.size());
    std::vector<i64> done((size_t)p.T, 0);
    for (int k = 0; k < p.nBatches(); ++k)
        for (const TrackPiece &pc : p.pieces[(size_t)k])
        {
            if (!p.jobs[(size_t)pc.t].converted())
                continue;
            const i64 hi = piece_out_hi(p, pc);
            if (hi <= done[(size_t)pc.t])
                continue;
            p.native[(size_t)k].push_back(PcmRange{pc.t, done[(size_t)pc.t], hi});
            done[(size_t)pc.t] = hi;
        }
}

// the frames each batch's PCM stage encodes: whole groups of 4, except at the end of the track
void plan_pcm(TracksPlan &p)
{
    p.pcm.resize(p.batches.size());
    std::vector<i64> done((size_t)p.T, 0);
    for (int k = 0; k < p.nBatches(); ++k)
        for (const TrackPiece &pc : p.pieces[(size_t)k])
        {
            const i64 n = p.jobs[(size_t)pc.t].outFrames(), end = piece_out_hi(p, pc);
            const i64 hi = end == n ? n : end & ~(i64)3;
            if (hi <= done[(size_t)pc.t])
                continue;
            p.pcm[(size_t)k].push_back(PcmRange{pc.t, done[(size_t)pc.t], hi});
            done[(size_t)pc.t] = hi;
        }
}
} // namespace

int tracks_plan_build(TracksPlan &p, int T, const int64_t *n, int Q, int N, const int *shifts, i64 seg, i64 stride, int B, bool pcm,
                      int ensTailCap, std::string &err, const int *rates, const int64_t *native)
{
    p = TracksPlan();
    p.T = T, p.Q = Q, p.N = N, p.B = B, p.seg = seg, p.stride = stride;
    if (int rc = plan_items(p, n, shifts, ensTailCap, rates, native, err))
        return rc;
    plan_batches(p);
    std::vector<i64> reach((size_t)Q, 0);
    if (int rc = plan_pieces(p, reach, err))
        return rc;
    p.R.resize((size_t)Q), p.ringOff.resize((size_t)Q);
    for (int q = 0; q < Q; ++q)
    {
        p.R[(size_t)q] = std::min<i64>(p.M[(size_t)q], std::max<i64>(2 * (i64)B, (reach[(size_t)q] + B - 1) / B * B));
        p.ringOff[(size_t)q] = p.ringBlocks;
        p.ringBlocks += p.R[(size_t)q];
    }
    if (int rc = plan_slots(p, err))
        return rc;
    if (p.mmax > 0)
        plan_native(p);
    if (pcm)
        plan_pcm(p);
    return DMX_OK;
}
