// tracks_exec.cpp — the track path of the C ABI: demucs_inference (src/model_apply.cpp:60-288) for one track or many, with
// the shifts ensemble, bags of models and PCM / remix / FLAC outputs. Enqueues the plan that tracks_plan.cpp makes.
#include "api_internal.h"
#include "tracks_plan.h"

#include <algorithm>
#include <cmath>
#include <climits>

using namespace dmx;

// --------------------------------------------------------------------------- track level
extern "C" int dmx_track_geometry(const dmx_ctx *c, int64_t n, int shift_offset, int64_t *shifted_len, int *n_segments,
                                  int64_t *stride)
{
    if (!c || n <= 0 || shift_offset < 0 || shift_offset >= DMX_MAX_SHIFT)
        return fail(DMX_ERR_ARG, "dmx_track_geometry: invalid argument");
    // OVERLAP = 0.25 (model_apply.cpp:162); the formulas: tracks_plan.h
    const i64 len = track_shifted_len(n, shift_offset);
    const i64 st = overlap_stride(c->seg, 0.25f);
    if (shifted_len)
        *shifted_len = len;
    if (stride)
        *stride = st;
    if (n_segments)
        *n_segments = track_n_segments(len, st);
    return DMX_OK;
}

extern "C" int dmx_track_stats_device(dmx_ctx *c, const float *d_audio, int64_t n, float *d_stats)
{
    if (!c || !d_audio || !d_stats || n < 2)
        return fail(DMX_ERR_ARG, "dmx_track_stats_device: invalid argument");
    HIPCHK(hipSetDevice(c->m->device));
    launch_track_stats(d_audio, n, c->dPartials, dmx_ctx::kStatBlocks, c->stream);
    launch_track_stats_final(c->dPartials, dmx_ctx::kStatBlocks, n, d_stats, c->stream);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_track_gather_device(dmx_ctx *c, const float *d_audio, int64_t n, const float *d_stats, int shift_offset,
                                       const int *seg_idx, int n_idx, float *d_mix)
{
    if (!c || !d_audio || !d_stats || !seg_idx || !d_mix || n_idx < 1 || n_idx > 4096)
        return fail(DMX_ERR_ARG, "dmx_track_gather_device: invalid argument");
    HIPCHK(hipSetDevice(c->m->device));
    i64 len, stride;
    int nseg;
    DMXCHK(dmx_track_geometry(c, n, shift_offset, &len, &nseg, &stride));
    for (int i = 0; i < n_idx; ++i)
        if (seg_idx[i] < 0 || seg_idx[i] >= nseg)
            return fail(DMX_ERR_ARG, "dmx_track_gather_device: segment index %d out of range", seg_idx[i]);
    // the indices are kernel arguments (copied at launch): seg_idx may be reused as soon as this returns
    launch_track_gather(d_audio, n, d_stats, shift_offset, c->seg, stride, len, seg_idx, n_idx, d_mix, c->stream);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

int dmx_track_overlap_add_planes(dmx_ctx *c, const float *d_seg_out, int n_segments, int64_t n, int shift_offset,
                                 const float *d_stats, float *d_out, int layout, int planeBase, int nPlanes)
{
    if (!c || !d_seg_out || !d_stats || !d_out)
        return fail(DMX_ERR_ARG, "dmx_track_overlap_add_device: null argument");
    if (layout != DMX_LAYOUT_EIGEN && layout != DMX_LAYOUT_PLANAR)
        return fail(DMX_ERR_ARG, "dmx_track_overlap_add_device: unknown layout %d", layout);
    HIPCHK(hipSetDevice(c->m->device));
    i64 len, stride;
    int nseg;
    DMXCHK(dmx_track_geometry(c, n, shift_offset, &len, &nseg, &stride));
    if (n_segments != nseg)
        return fail(DMX_ERR_ARG, "dmx_track_overlap_add_device: expected %d segments, got %d", nseg, n_segments);
    launch_track_ola(d_seg_out, nseg, c->m->pm.n_sources, c->seg, stride, len, n, shift_offset, d_stats, d_out,
                     layout == DMX_LAYOUT_EIGEN ? 1 : 0, planeBase, nPlanes, 0, n, c->stream);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_track_overlap_add_device(dmx_ctx *c, const float *d_seg_out, int n_segments, int64_t n, int shift_offset,
                                            const float *d_stats, float *d_out, int layout)
{
    if (!c)
        return fail(DMX_ERR_ARG, "dmx_track_overlap_add_device: null argument");
    return dmx_track_overlap_add_planes(c, d_seg_out, n_segments, n, shift_offset, d_stats, d_out, layout, 0,
                                        2 * c->m->pm.n_sources);
}

// demucs_inference on one device, for one track or several. All device buffers belong to the context (grown on first use,
// then reused: no allocation on the per-batch path); every batch is enqueued without waiting for the one before; progress
// is reported from per-batch events, i.e. the stream is never synchronised before the end; and each track is FINISHED IN
// PIECES: as soon as the batch ending with segment g of a track is enqueued, the track's output samples below
// g*stride + (first sample of segment g+1) can no longer change, so their overlap-add is launched right behind that batch
// and their device-to-host copy runs on a second stream underneath the kernels of the following batch (the 339 MB result
// of a 4-minute track otherwise costs as much wall time after the last kernel as a dozen segments).
//
// What is dealt into which batch, the pieces, the rings, the track slots and the PCM ranges are planned on the host before
// any GPU work: tracks_plan.cpp (TracksPlan), which also explains them. The functions below enqueue a plan.
// The PCM output stage (dmx_tracks_infer_pcm, pcm.hip): with an output spec the overlap-add writes the slot in the planar
// layout whatever the caller's layout, the peak kernel runs on every finished piece right behind its overlap-add, and the
// encode kernel turns the planes into interleaved PCM in the slot's staging buffer: per piece when the clip mode needs no
// peak, for the whole track behind its last piece with DMX_CLIP_RESCALE. Pieces are encoded in whole groups of 4 frames (the
// up to 3 frames left over go with the next piece; the last piece ends at n), and each (output, piece) leaves in ONE copy.
// A slot then also holds n_out encoded outputs of n_max frames (each rounded up to 16 bytes; at most the size of its fp32
// result) and n_out peaks. Without a spec nothing of this exists: the same launches and copies as before.
// A bag of Q models (dmx_tracks_infer_bag): a batch holds items of one model, and the context is
// rebound (dmx_ctx_set_model) between batches; one launch of track_ola_bag_kernel combines the rings, and the peak / encode
// stage and the copy-out follow unchanged. One model through the old entry points (no bag) is the sequence of launches it was.
// Tracks at another rate (dmx_tracks_infer_rates): the caller's track goes up into sl.native and the
// whole-signal resampler leaves it at 44.1 kHz in sl.audio, on the upload stream ahead of the statistics; the overlap-add of
// such a track always writes planes; behind it the piece-table resampler (resample.hip) converts the native-rate frames the
// batch's pieces make final (plan.native) into sl.nativeOut, in the caller's layout or, for the PCM stage, as planes; and the
// PCM stage, the FLAC stage and the copy-out work on those frames, with the caller's track (sl.native) as the remix mixture.
// A slot then also holds 2 m_max + S x 2 x m_max floats (m_max: the most frames of a converted track), allocated only in a call
// that converts a track. A call whose rates are all 44100 enqueues exactly what the other entry points enqueue.
namespace
{
struct BagRun // the models of a call and their effective weights [Q][S] (dmx_bag_weights)
{
    const dmx_model *const *models;
    int Q;
    const float *w;
};
struct PcmOut // the output spec of a call, checked (dmx_pcm_check_spec)
{
    dmx_output_spec spec;
    void *const *out;
    float *peaks;
    int nOut, frameBytes;
    const PcmGains *remix; // dmx_tracks_infer_remix: the outputs are rows of gains over the stems and the mixture, else NULL
    // dmx_tracks_infer_flac (flacBits 16 | 24, else 0): out[t] takes n_out files at a stride of dmx_flac_bound, sizes their byte counts
    int flacBits, flacRate;
    int64_t *sizes;
    const int *rates; // dmx_tracks_infer_rates: the tracks' own rates, which their files carry; NULL: flacRate
    int flac_rate(int t) const { return rates ? rates[t] : flacRate; }
    // dmx_tracks_infer_loud (remix specs only): the checked spec, the report (n_out + 1 entries per track) and
    // the device's gain table; else NULL
    const dmx_loudness_spec *loud;
    dmx_loudness_result *report;
    const float *loudTable;
    // dmx_tracks_infer_meters: the meters report, n_out + 1 entries per track; else NULL
    dmx_meters_result *meters;
    // dmx_tracks_infer_limit: the limiter's times (NULL: the defaults), its report of n_out entries per
    // track (or NULL) and the device's tables; read only with DMX_LOUD_LIMIT in the mode
    const dmx_limiter_spec *lim;
    dmx_limit_result *limit;
    const int32_t *limTables;
    int loudMode() const { return loud->mode & ~(DMX_LOUD_TRUE_PEAK | DMX_LOUD_LIMIT); }
    bool byTruePeak() const { return loud && (loud->mode & DMX_LOUD_TRUE_PEAK) != 0; }
    bool limited() const { return loud && (loud->mode & DMX_LOUD_LIMIT) != 0; }
    // the track's true peaks are measured; the limiter's level needs none of the track
    bool truePeaks() const { return (byTruePeak() && !limited()) || meters; }
    bool gained() const { return loud && loudMode() != DMX_LOUD_MEASURE; } // DMX_LOUD_UNITY too: a whole-track, limited
    // a slot's loudness buffer for a track of n frames (loud_chain.h): the reports live in it, and the limiter takes one envelope
    // under DMX_LOUD_MIXTURE, else n_out
    LoudChain chain(i64 n) const
    {
        return loud_chain_layout(nOut, n, LoudChainMode{meters != nullptr, byTruePeak(), limited(), loudMode() == DMX_LOUD_MIXTURE ? 1 : nOut, true});
    }
};
// One call of the track path. shifts: T x Q x N, row-major (Q = 1 without a bag). Without a bag, N == 1 launches
// track_ola_kernel and N >= 2 track_ola_ens_kernel; a bag launches track_ola_bag_kernel.
// pcm: NULL (fp32 results into out[t]), else the results leave as PCM (pcm->out[t]) and `out` is not used
struct TracksRun
{
    dmx_ctx *c = nullptr;
    const char *fn = nullptr;
    int T = 0;
    const float *const *audio = nullptr;
    const int64_t *n = nullptr;
    // dmx_tracks_infer_rates: track t has n[t] frames at rates[t]; a track whose rate is not 44100 is converted in its slot
    // (sl.native -> sl.audio in front of the model, sl.out -> sl.nativeOut behind the overlap-add); NULL: all 44100
    const int *rates = nullptr;
    int N = 1;
    i64 stride = 0;
    const int *shifts = nullptr;
    float *const *out = nullptr;
    int layout = DMX_LAYOUT_EIGEN;
    dmx_progress_fn progress = nullptr;
    void *user = nullptr;
    const PcmOut *pcm = nullptr;
    const BagRun *bag = nullptr;
    // dmx_tracks_infer_from_flac: audio[t] is the image of a .flac file of fileBytes[t] bytes that the probe has described
    // (n[t] = its total samples); the slot's interleaved track is decoded on the upload stream; trackStatus: 2 per track
    const dmx_flac_info *flacIn = nullptr;
    const int64_t *fileBytes = nullptr;
    int64_t *trackStatus = nullptr;
    // set by tracks_run_impl
    TracksPlan plan;
    int S = 0, eigen = 0, olaEigen = 0;
    i64 blk = 0;
    bool wholeTrack = false; // encode when the track's peak is complete
    std::vector<const float *> rings;
    // the tables of the batch being enqueued
    std::vector<TrackSegItem> batchItems;
    std::vector<TrackOlaEntry> ola;
    std::vector<TrackEnsPiece> ens;
    std::vector<TrackEnsCopy> ensCopies;
    std::vector<TrackBagPiece> bagPieces;
    std::vector<TrackBagModel> bagModels;
    std::vector<RemixPiece> pieces, whole; // the PCM stage's; under a remix spec the mixture is the slot's upload
    std::vector<PcmPiece> pcmPeak, pcmEnc;  // the same without the mixture, for the kernels of an output spec
    std::vector<ResamplePiece> conv;        // the converter's, of one ratio
    std::vector<LoudPlan> loudPlans;        // per track, made before the first batch (host arithmetic)
    std::vector<LoudPiece> loudEnc;         // the whole tracks of a batch, each with its gains
    std::vector<LimitPiece> limitEnc;       // the same behind the limiter, each with its gain planes

    const dmx_ctx::TrackSlot &slot(int t) const { return c->slots[(size_t)plan.jobs[(size_t)t].slot]; }
};
} // namespace

// the context's buffers, streams and events for the plan
static int tracks_prepare(TracksRun &r)
{
    dmx_ctx *c = r.c;
    const TracksPlan &p = r.plan;
    const PcmOut *pcm = r.pcm;
    const i64 nmax = p.nmax, mmax = p.mmax;
    i64 omax = 0; // the most frames of a track's outputs
    for (const TrackJob &j : p.jobs)
        omax = std::max<i64>(omax, j.outFrames());
    DMXCHK(dmx_ensure_buf(c->bMix, 2 * p.seg * p.B));
    DMXCHK(dmx_ensure_buf(c->bSegOut, p.ringBlocks * r.blk));
    if ((int)c->slots.size() < p.nSlots)
        c->slots.resize((size_t)p.nSlots);
    for (int i = 0; i < p.nSlots; ++i)
    {
        dmx_ctx::TrackSlot &sl = c->slots[(size_t)i];
        DMXCHK(dmx_ensure_buf(sl.audio, 2 * nmax));
        if (r.layout == DMX_LAYOUT_PLANAR)
            DMXCHK(dmx_ensure_buf(sl.tmp, 2 * std::max(nmax, mmax)));
        if (mmax > 0)
        {
            DMXCHK(dmx_ensure_buf(sl.native, 2 * mmax));
            DMXCHK(dmx_ensure_buf(sl.nativeOut, (i64)r.S * 2 * mmax));
        }
        DMXCHK(dmx_ensure_buf(sl.out, (i64)r.S * 2 * nmax));
        DMXCHK(dmx_ensure_buf(sl.stats, 4));
        if (pcm)
        {
            DMXCHK(dmx_ensure_buf(sl.pcm, (i64)pcm->nOut * (DMX_OUTPUT_STRIDE(omax * pcm->frameBytes) / 4)));
            DMXCHK(dmx_ensure_buf(sl.peaks, 8));
            if (pcm->loud)
                DMXCHK(dmx_ensure_buf(sl.loud, (pcm->chain(omax).total + 3) / 4));
            if (pcm->flacBits)
            {
                DMXCHK(dmx_ensure_buf(sl.flac, (i64)pcm->nOut * (flac_bound(pcm->flacBits, omax) / 4)));
                DMXCHK(dmx_ensure_buf(sl.flacWork, (i64)pcm->nOut * (flac_workspace_bytes(pcm->flacBits, omax) / 4)));
                DMXCHK(dmx_ensure_buf(sl.flacSizes, 2 * DMX_MAX_OUTPUTS));
            }
        }
        if (r.flacIn)
        {
            i64 fileMax = 0, workMax = 0;
            for (int t = 0; t < r.T; ++t)
            {
                fileMax = std::max<i64>(fileMax, r.fileBytes[t]);
                workMax = std::max<i64>(workMax, flac_in_workspace_bytes(&r.flacIn[t], r.fileBytes[t]));
            }
            DMXCHK(dmx_ensure_buf(sl.flacIn, (fileMax + 15) / 16 * 4));
            DMXCHK(dmx_ensure_buf(sl.flacInWork, workMax / 4));
            DMXCHK(dmx_ensure_buf(sl.flacInStatus, 4));
        }
        if (!sl.copied)
            HIPCHK(hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
    }
    for (const TrackJob &j : p.jobs) // the filters go up now (once per process and ratio), not between the batches
        if (j.converted())
        {
            DMXCHK(resample_prepare(c->m->device, j.rate, 44100));
            DMXCHK(resample_prepare(c->m->device, 44100, j.rate));
        }
    if (!c->uploadStream)
        HIPCHK(hipStreamCreateWithFlags(&c->uploadStream, hipStreamNonBlocking));
    if (!c->evUpload)
        HIPCHK(hipEventCreateWithFlags(&c->evUpload, hipEventDisableTiming));
    r.rings.resize((size_t)p.Q);
    for (int q = 0; q < p.Q; ++q)
        r.rings[(size_t)q] = c->bSegOut.p + p.ringOff[(size_t)q] * r.blk;
    r.batchItems.resize((size_t)p.B);
    return DMX_OK;
}

// upload the tracks [tLo, tHi) that start in batch k into their slots, and their statistics
static int tracks_upload(TracksRun &r, int k, int tLo, int tHi)
{
    dmx_ctx *c = r.c;
    TrackStatsTable st{};
    int nSt = 0;
    for (int t = tLo; t < tHi; ++t)
    {
        const TrackJob &j = r.plan.jobs[(size_t)t];
        if (j.kFirst != k)
            continue;
        const dmx_ctx::TrackSlot &sl = r.slot(t);
        if (j.takeover) // the previous holder's copy-out (and every kernel that read the slot) is done
            HIPCHK(hipEventSynchronize(sl.copied));
        if (r.pcm)
            HIPCHK(hipMemsetAsync(sl.peaks.p, 0, sizeof(float) * (size_t)r.pcm->nOut, c->stream));
        float *up = j.converted() ? sl.native.p : sl.audio.p; // the caller's track, interleaved, j.m frames
        if (r.flacIn) // the file's bytes go up; the five launches of flac_in.hip leave the interleaved track in the slot
        {
            HIPCHK(hipMemcpyAsync(sl.flacIn.p, r.audio[t], (size_t)r.fileBytes[t], hipMemcpyHostToDevice, c->uploadStream));
            if (launch_flac_decode((const unsigned char *)sl.flacIn.p, r.fileBytes[t], &r.flacIn[t], DMX_PCM_F32, up,
                                   (long long *)sl.flacInStatus.p, sl.flacInWork.p, c->uploadStream) != 0)
                return fail(DMX_ERR_ARG, "%s: track %d: internal error (the probe's description was refused)", r.fn, t);
        }
        else if (r.eigen)
            HIPCHK(hipMemcpyAsync(up, r.audio[t], sizeof(float) * 2 * (size_t)j.m, hipMemcpyHostToDevice, c->uploadStream));
        else
        {
            HIPCHK(hipMemcpyAsync(sl.tmp.p, r.audio[t], sizeof(float) * 2 * (size_t)j.m, hipMemcpyHostToDevice, c->uploadStream));
            launch_planar_to_interleaved(sl.tmp.p, up, j.m, c->uploadStream);
        }
        if (j.converted()) // the whole track to 44.1 kHz, ahead of its statistics
            DMXCHK(dmx_resample_device(c->m->device, sl.native.p, j.m, 2, 1, 2, j.rate, 44100, sl.audio.p, 1, 2, c->uploadStream));
        st.audio[nSt] = sl.audio.p, st.n[nSt] = j.n, st.stats[nSt] = sl.stats.p;
        if (++nSt == TrackStatsTable::kMax || t == tHi - 1)
        {
            HIPCHK(hipEventRecord(c->evUpload, c->uploadStream));
            HIPCHK(hipStreamWaitEvent(c->stream, c->evUpload, 0));
            launch_track_stats(st, nSt, c->dPartials, dmx_ctx::kStatBlocks, c->stream);
            launch_track_stats_final(st, nSt, c->dPartials, dmx_ctx::kStatBlocks, c->stream);
            nSt = 0;
        }
    }
    return DMX_OK;
}

// gather batch k (its model's items [g0, g0 + nb)) and run the model on it, into the model's ring
static int tracks_infer(TracksRun &r, int k)
{
    dmx_ctx *c = r.c;
    const TracksPlan &p = r.plan;
    const TrackBatch &bt = p.batches[(size_t)k];
    for (i64 g = bt.g0; g < bt.g0 + bt.nb; ++g)
    {
        const TrackItem &it = p.items[(size_t)bt.q][(size_t)g];
        const dmx_ctx::TrackSlot &sl = r.slot(it.t);
        r.batchItems[(size_t)(g - bt.g0)] = TrackSegItem{sl.audio.p, sl.stats.p, p.jobs[(size_t)it.t].n, p.copy(it.t, bt.q, it.k).shift, it.g};
    }
    launch_track_gather(r.batchItems.data(), bt.nb, p.seg, p.stride, c->bMix.p, c->stream);
    HIPCHK(hipGetLastError());
    return dmx_segment_infer_device(c, c->bMix.p, const_cast<float *>(r.rings[(size_t)bt.q]) + (bt.g0 % p.R[(size_t)bt.q]) * r.blk, bt.nb);
}

// the overlap-add of what batch k makes final: one of three kernels (N == 1, the shifts ensemble, a bag).
// which < 0: every piece, in the call's layout. A call that converts a track launches twice instead: which 0, the pieces of
// the tracks at 44.1 kHz in the call's layout; which 1, those of the converted tracks as planes, which the converter reads
static int tracks_ola(TracksRun &r, int k, int which = -1)
{
    const TracksPlan &p = r.plan;
    const int Q = p.Q, N = p.N, S = r.S;
    const i64 Rq = p.R[(size_t)p.batches[(size_t)k].q];
    const int olaEigen = which == 1 ? 0 : r.olaEigen;
    hipStream_t s = r.c->stream;
    r.ola.clear(), r.ens.clear(), r.ensCopies.clear(), r.bagPieces.clear(), r.bagModels.clear();
    for (const TrackPiece &pc : p.pieces[(size_t)k])
    {
        if (pc.hi <= pc.lo || (which >= 0 && (int)p.jobs[(size_t)pc.t].converted() != which))
            continue;
        const i64 n = p.jobs[(size_t)pc.t].n;
        const dmx_ctx::TrackSlot &sl = r.slot(pc.t);
        if (r.bag)
        {
            r.bagPieces.push_back(TrackBagPiece{sl.stats.p, sl.out.p, n, pc.lo, pc.hi});
            for (int q = 0; q < Q; ++q)
            {
                const TrackModel &x = p.tm[(size_t)pc.t * Q + q];
                const i64 itemLo = p.pieceItems[pc.item0 + (size_t)q];
                r.bagModels.push_back(TrackBagModel{(int)itemLo, (int)((x.g0 + itemLo) % p.R[(size_t)q]), x.nMin, x.nMax - x.nMin});
                for (int k2 = 0; k2 < N; ++k2)
                    r.ensCopies.push_back(TrackEnsCopy{p.copy(pc.t, q, k2).shift, p.copy(pc.t, q, k2).nseg});
            }
            continue;
        }
        const TrackModel &x = p.tm[(size_t)pc.t];
        const i64 itemLo = p.pieceItems[pc.item0], slotLo = (x.g0 + itemLo) % Rq;
        if (N == 1)
        {
            const TrackCopy &cp = p.copy(pc.t, 0, 0);
            r.ola.push_back(TrackOlaEntry{r.rings[0], sl.stats.p, sl.out.p, n, cp.len, pc.lo, pc.hi, itemLo, slotLo, cp.nseg, cp.shift});
        }
        else
        {
            r.ens.push_back(TrackEnsPiece{sl.stats.p, sl.out.p, n, pc.lo, pc.hi, itemLo, slotLo, x.nMin, x.nMax - x.nMin});
            for (int k2 = 0; k2 < N; ++k2)
                r.ensCopies.push_back(TrackEnsCopy{p.copy(pc.t, 0, k2).shift, p.copy(pc.t, 0, k2).nseg});
        }
    }
    if (which >= 0 && r.ola.empty() && r.ens.empty() && r.bagPieces.empty())
        return DMX_OK;
    if (r.bag)
    {
        if (!launch_track_ola_bag(r.bagPieces.data(), r.bagModels.data(), r.ensCopies.data(), (int)r.bagPieces.size(), Q, N, r.bag->w,
                                  r.rings.data(), p.R.data(), S, p.seg, p.stride, olaEigen, 0, 2 * S, s))
            return fail(DMX_ERR_ARG, "%s: internal error (the bag's overlap-add was refused in batch %d)", r.fn, k);
    }
    else if (N == 1)
        launch_track_ola(r.ola.data(), (int)r.ola.size(), S, p.seg, p.stride, Rq, olaEigen, 0, 2 * S, s);
    else
        launch_track_ola_ens(r.ens.data(), r.ensCopies.data(), (int)r.ens.size(), N, r.rings[0], S, p.seg, p.stride, Rq, olaEigen, 0,
                             2 * S, s);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

// the converter behind batch k's overlap-add: the native-rate frames that the batch's pieces make final (plan.native), one
// launch per ratio, from the planes of sl.out to sl.nativeOut - planes for the PCM stage, else the caller's layout
static int tracks_convert(TracksRun &r, int k)
{
    const TracksPlan &p = r.plan;
    const std::vector<PcmRange> &ranges = p.native[(size_t)k];
    const i64 S = r.S;
    const bool eigen = !r.pcm && r.eigen;
    for (size_t a = 0; a < ranges.size(); ++a)
    {
        const int rate = p.jobs[(size_t)ranges[a].t].rate;
        bool seen = false; // a ratio is launched where it first occurs
        for (size_t b = 0; b < a; ++b)
            seen = seen || p.jobs[(size_t)ranges[b].t].rate == rate;
        if (seen)
            continue;
        r.conv.clear();
        for (size_t b = a; b < ranges.size(); ++b)
        {
            const TrackJob &j = p.jobs[(size_t)ranges[b].t];
            if (j.rate != rate)
                continue;
            const dmx_ctx::TrackSlot &sl = r.slot(ranges[b].t);
            r.conv.push_back(ResamplePiece{sl.out.p, sl.nativeOut.p, j.n, eigen ? 1 : 2 * j.m, eigen ? S : j.m, eigen ? 2 * S : 1,
                                           ranges[b].lo, ranges[b].hi});
        }
        DMXCHK(launch_resample_pieces(r.c->m->device, r.conv.data(), (int)r.conv.size(), 2 * r.S, 44100, rate, r.c->stream));
    }
    return DMX_OK;
}

// the PCM stage behind batch k's overlap-add: the peaks of its ranges, their encoding (the whole track behind its last
// range when the clip mode needs the peak), and the files of a track whose PCM is complete
static int tracks_output_stage(TracksRun &r, int k)
{
    const TracksPlan &p = r.plan;
    const PcmOut *pcm = r.pcm;
    hipStream_t s = r.c->stream;
    r.pieces.clear(), r.whole.clear();
    for (const PcmRange &g : p.pcm[(size_t)k])
    {
        const TrackJob &j = p.jobs[(size_t)g.t];
        const i64 n = j.outFrames();
        const dmx_ctx::TrackSlot &sl = r.slot(g.t);
        // a converted track: its stems and the caller's track at its own rate
        RemixPiece pp{PcmPiece{j.converted() ? sl.nativeOut.p : sl.out.p, (unsigned char *)sl.pcm.p, (unsigned *)sl.peaks.p, n, n,
                               DMX_OUTPUT_STRIDE(n * pcm->frameBytes), g.lo, g.hi},
                      !pcm->remix ? nullptr : j.converted() ? sl.native.p : sl.audio.p};
        r.pieces.push_back(pp);
        if (g.hi == n)
        {
            pp.i0 = 0;
            r.whole.push_back(pp);
        }
    }
    const std::vector<RemixPiece> &enc = r.wholeTrack ? r.whole : r.pieces;
    if (pcm->loud)
    {
        // behind a track's last piece: its outputs and its mixture are measured, and one launch turns lufs_c and the peaks into
        // the gains, the gained peaks and the report; the gained tracks are whole-track ones, encoded here with their gains
        if (!pcm->limited()) // (the limiter measures the peaks of what it leaves: the peak kernel is not needed)
            launch_remix_peak(r.pieces.data(), (int)r.pieces.size(), *pcm->remix, s);
        r.loudEnc.clear(), r.limitEnc.clear();
        for (size_t x = 0, w = 0; x < p.pcm[(size_t)k].size(); ++x)
        {
            const PcmRange &g = p.pcm[(size_t)k][x];
            if (g.hi != p.jobs[(size_t)g.t].outFrames())
                continue;
            LoudChainJob job{};
            job.pp = r.whole[w++];
            job.G = pcm->remix, job.lp = &r.loudPlans[(size_t)g.t], job.rate = r.rates ? r.rates[g.t] : 44100;
            job.loud = pcm->loud, job.lim = pcm->lim, job.loudTable = pcm->loudTable, job.limTables = pcm->limTables;
            job.work = (unsigned char *)r.slot(g.t).loud.p, job.L = pcm->chain(job.lp->n);
            job.report = job.work + job.L.report, job.meters = pcm->meters ? job.work + job.L.meters : nullptr;
            LimitPiece piece;
            DMXCHK(dmx_loud_chain_enqueue(job, s, &piece));
            if (pcm->limited())
                r.limitEnc.push_back(piece);
            else
                r.loudEnc.push_back(piece);
        }
        if (pcm->limited())
            launch_limit_encode(r.limitEnc.data(), (int)r.limitEnc.size(), *pcm->remix, pcm->spec.encoding, pcm->spec.clip, s);
        else if (pcm->gained())
            launch_loud_encode(r.loudEnc.data(), (int)r.loudEnc.size(), *pcm->remix, pcm->spec.encoding, pcm->spec.clip, s);
        else
            launch_remix_encode(enc.data(), (int)enc.size(), *pcm->remix, pcm->spec.encoding, pcm->spec.clip, s);
    }
    else if (pcm->remix)
    {
        launch_remix_peak(r.pieces.data(), (int)r.pieces.size(), *pcm->remix, s);
        launch_remix_encode(enc.data(), (int)enc.size(), *pcm->remix, pcm->spec.encoding, pcm->spec.clip, s);
    }
    else
    {
        r.pcmPeak.assign(r.pieces.begin(), r.pieces.end());
        r.pcmEnc.assign(enc.begin(), enc.end());
        launch_pcm_peak(r.pcmPeak.data(), (int)r.pcmPeak.size(), r.S, pcm->spec.stem, s);
        launch_pcm_encode(r.pcmEnc.data(), (int)r.pcmEnc.size(), r.S, pcm->spec.stem, pcm->spec.encoding, pcm->spec.clip, s);
    }
    if (pcm->flacBits)
        for (const PcmRange &g : p.pcm[(size_t)k])
        {
            const i64 n = p.jobs[(size_t)g.t].outFrames();
            if (g.hi != n)
                continue;
            const dmx_ctx::TrackSlot &sl = r.slot(g.t);
            launch_flac_encode((const unsigned char *)sl.pcm.p, DMX_OUTPUT_STRIDE(n * pcm->frameBytes), pcm->flacBits, n, pcm->flac_rate(g.t),
                               pcm->nOut, (unsigned char *)sl.flac.p, flac_bound(pcm->flacBits, n), (long long *)sl.flacSizes.p,
                               (unsigned char *)sl.flacWork.p, s, r.c->flacLevel);
        }
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

// the encoded outputs of range g of batch k leave: PCM per range (the whole track behind its last range with
// DMX_CLIP_RESCALE), FLAC files and the peaks behind the track's last range
static int tracks_copy_pcm(TracksRun &r, int k, const PcmRange &g)
{
    dmx_ctx *c = r.c;
    const PcmOut *pcm = r.pcm;
    const i64 n = r.plan.jobs[(size_t)g.t].outFrames();
    const dmx_ctx::TrackSlot &sl = r.slot(g.t);
    const bool last = g.hi == n;
    const i64 lo = r.wholeTrack ? 0 : g.lo, fb = pcm->frameBytes;
    const i64 outBytes = n * fb, devStride = DMX_OUTPUT_STRIDE(outBytes);
    if (pcm->flacBits)
    {
        if (!last)
            return DMX_OK;
        // the files' byte counts first (the batch that made them is done once its event is; the next batch is
        // already enqueued), then one copy per output of exactly its length
        int64_t *sz = pcm->sizes + (size_t)g.t * pcm->nOut;
        HIPCHK(hipEventSynchronize(c->batchEvents[(size_t)k]));
        HIPCHK(hipMemcpyAsync(sz, sl.flacSizes.p, sizeof(int64_t) * (size_t)pcm->nOut, hipMemcpyDeviceToHost, c->copyStream));
        HIPCHK(hipStreamSynchronize(c->copyStream));
        const i64 bound = flac_bound(pcm->flacBits, n);
        for (int o = 0; o < pcm->nOut; ++o)
        {
            if (sz[o] < 42 || sz[o] > bound)
                return fail(DMX_ERR_HIP, "%s: internal error (track %d, output %d: %lld encoded bytes, bound %lld)", r.fn, g.t, o,
                            (long long)sz[o], (long long)bound);
            HIPCHK(hipMemcpyAsync((unsigned char *)pcm->out[g.t] + (size_t)(o * bound), (const unsigned char *)sl.flac.p + (size_t)(o * bound),
                                  (size_t)sz[o], hipMemcpyDeviceToHost, c->copyStream));
        }
    }
    else if (!r.wholeTrack || last)
        for (int o = 0; o < pcm->nOut; ++o)
            HIPCHK(hipMemcpyAsync((unsigned char *)pcm->out[g.t] + (size_t)(o * outBytes + lo * fb),
                                  (const unsigned char *)sl.pcm.p + (size_t)(o * devStride + lo * fb), (size_t)((g.hi - lo) * fb),
                                  hipMemcpyDeviceToHost, c->copyStream));
    if (last && pcm->peaks)
        HIPCHK(hipMemcpyAsync(pcm->peaks + (size_t)g.t * pcm->nOut, sl.peaks.p, sizeof(float) * (size_t)pcm->nOut, hipMemcpyDeviceToHost,
                              c->copyStream));
    if (!last || !pcm->loud)
        return DMX_OK;
    const LoudChain L = pcm->chain(n);
    const unsigned char *work = (const unsigned char *)sl.loud.p;
    if (pcm->report) // the report leaves with the peaks
        HIPCHK(hipMemcpyAsync(pcm->report + (size_t)g.t * (pcm->nOut + 1), work + L.report, sizeof(dmx_loudness_result) * (size_t)(pcm->nOut + 1),
                              hipMemcpyDeviceToHost, c->copyStream));
    if (pcm->limit && pcm->limited()) // the limiter's results
        HIPCHK(hipMemcpyAsync(pcm->limit + (size_t)g.t * pcm->nOut, work + L.limRes, sizeof(dmx_limit_result) * (size_t)pcm->nOut,
                              hipMemcpyDeviceToHost, c->copyStream));
    if (pcm->meters) // and the meters report
        HIPCHK(hipMemcpyAsync(pcm->meters + (size_t)g.t * (pcm->nOut + 1), work + L.meters, sizeof(dmx_meters_result) * (size_t)(pcm->nOut + 1),
                              hipMemcpyDeviceToHost, c->copyStream));
    return DMX_OK;
}

// What batch k made final leaves on the copy stream. It is issued AFTER batch k+1 has been enqueued: a device-to-host copy
// into pageable memory blocks the calling thread until the data has left the GPU, and the GPU must have its next batch
// queued by then.
static int tracks_copy_out(TracksRun &r, int k)
{
    dmx_ctx *c = r.c;
    const TracksPlan &p = r.plan;
    const int S = r.S;
    HIPCHK(hipStreamWaitEvent(c->copyStream, c->batchEvents[(size_t)k], 0));
    if (r.pcm)
        for (const PcmRange &g : p.pcm[(size_t)k])
            DMXCHK(tracks_copy_pcm(r, k, g));
    for (size_t x = 0; !r.pcm && p.mmax > 0 && x < p.native[(size_t)k].size(); ++x) // fp32 stems of the converted tracks
    {
        const PcmRange &g = p.native[(size_t)k][x];
        const i64 m = p.jobs[(size_t)g.t].m;
        const float *dOut = r.slot(g.t).nativeOut.p;
        float *out = r.out[g.t];
        if (r.eigen)
            HIPCHK(hipMemcpyAsync(out + (size_t)g.lo * 2 * S, dOut + (size_t)g.lo * 2 * S, sizeof(float) * (size_t)(g.hi - g.lo) * 2 * S,
                                  hipMemcpyDeviceToHost, c->copyStream));
        else
            for (int pl = 0; pl < 2 * S; ++pl)
                HIPCHK(hipMemcpyAsync(out + (size_t)pl * m + g.lo, dOut + (size_t)pl * m + g.lo, sizeof(float) * (size_t)(g.hi - g.lo),
                                      hipMemcpyDeviceToHost, c->copyStream));
    }
    for (const TrackPiece &pc : p.pieces[(size_t)k])
    {
        const TrackJob &j = p.jobs[(size_t)pc.t];
        const dmx_ctx::TrackSlot &sl = r.slot(pc.t);
        const float *dOut = sl.out.p;
        float *out = r.out ? r.out[pc.t] : nullptr;
        const i64 i0 = pc.lo, i1 = pc.hi;
        if (i1 > i0 && !r.pcm && !j.converted())
        {
            if (r.eigen)
                HIPCHK(hipMemcpyAsync(out + (size_t)i0 * 2 * S, dOut + (size_t)i0 * 2 * S, sizeof(float) * (size_t)(i1 - i0) * 2 * S,
                                      hipMemcpyDeviceToHost, c->copyStream));
            else
                for (int pl = 0; pl < 2 * S; ++pl)
                    HIPCHK(hipMemcpyAsync(out + (size_t)pl * j.n + i0, dOut + (size_t)pl * j.n + i0, sizeof(float) * (size_t)(i1 - i0),
                                          hipMemcpyDeviceToHost, c->copyStream));
        }
        if (j.kLast == k && r.flacIn) // behind batch k, so behind the decode; before the slot's next holder may start
            HIPCHK(hipMemcpyAsync(r.trackStatus + 2 * (size_t)pc.t, sl.flacInStatus.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->copyStream));
        if (j.kLast == k)
            HIPCHK(hipEventRecord(sl.copied, c->copyStream));
    }
    if (r.progress)
    {
        const i64 hi = p.cum[(size_t)k], lo = hi - p.batches[(size_t)k].nb;
        HIPCHK(hipEventSynchronize(c->batchEvents[(size_t)k]));
        char msg[128];
        snprintf(msg, sizeof(msg), "2., apply model w/ split, segments %lld..%lld of %lld", (long long)lo, (long long)(hi - 1),
                 (long long)p.Mtot);
        r.progress((float)hi / (float)p.Mtot, msg, r.user);
    }
    return DMX_OK;
}

// every cap of track_ola_bag_kernel (copies per piece, tail entries, LDS), on the tracks' whole tails
static int tracks_check_bag_caps(const TracksRun &r)
{
    const TracksPlan &p = r.plan;
    std::vector<TrackBagModel> whole(p.tm.size());
    for (size_t i = 0; i < whole.size(); ++i)
        whole[i] = TrackBagModel{0, 0, p.tm[i].nMin, p.tm[i].nMax - p.tm[i].nMin};
    if (track_ola_bag_tail_entries(whole.data(), p.T, p.Q, p.N, r.S, r.bag->w) < 0)
        return fail(DMX_ERR_ARG,
                    "%s: the bag does not fit the overlap-add kernel (%d models x %d shifts of at most %d, %d stems of at most %d, or "
                    "more than %d uneven tail rows x copies of one track and stem)",
                    r.fn, p.Q, p.N, TrackBagTable::kMaxCopies, r.S, TrackBagTable::kMaxStems, TrackBagTable::kMaxTail);
    return DMX_OK;
}

static int tracks_run_impl(TracksRun &r)
{
    dmx_ctx *c = r.c;
    HIPCHK(hipSetDevice(c->m->device));
    r.S = c->m->pm.n_sources;
    r.blk = (i64)r.S * 2 * c->seg;
    r.eigen = r.layout == DMX_LAYOUT_EIGEN ? 1 : 0;
    r.olaEigen = r.pcm ? 0 : r.eigen; // the PCM stage reads planes
    r.wholeTrack = r.pcm && (r.pcm->spec.clip == DMX_CLIP_RESCALE || r.pcm->gained());
    std::string why;
    std::vector<int64_t> n44; // the plan is made on the tracks' lengths at 44.1 kHz
    if (r.rates)
    {
        n44.assign(r.n, r.n + r.T);
        for (int t = 0; t < r.T; ++t)
            if (r.rates[t] != 44100)
                n44[(size_t)t] = dmx_resample_length(r.n[t], r.rates[t], 44100);
    }
    const int rcPlan = tracks_plan_build(r.plan, r.T, r.rates ? n44.data() : r.n, r.bag ? r.bag->Q : 1, r.N, r.shifts, c->seg, r.stride, c->maxBatch,
                                         r.pcm != nullptr, r.bag ? -1 : TrackEnsTable::kMaxTail, why, r.rates, r.n);
    if (rcPlan != DMX_OK)
        return fail(rcPlan, "%s: %s", r.fn, why.c_str());
    if (r.bag)
        DMXCHK(tracks_check_bag_caps(r));
    DMXCHK(tracks_prepare(r));
    const TracksPlan &p = r.plan;
    if (r.pcm && r.pcm->loud)
    {
        r.loudPlans.resize((size_t)p.T);
        for (int t = 0; t < p.T; ++t)
            if (loud_plan(r.rates ? r.rates[t] : 44100, p.jobs[(size_t)t].outFrames(), &r.loudPlans[(size_t)t]) != 0)
                return fail(DMX_ERR_ARG, "%s: track %d: no loudness plan for %lld frames", r.fn, t, (long long)p.jobs[(size_t)t].outFrames());
    }
    if (r.progress)
        r.progress(0.0f, "1., apply model w/ shift", r.user);
    int tLo = 0; // first track of the current batch
    for (int k = 0; k < p.nBatches(); ++k)
    {
        if (r.bag)
            DMXCHK(dmx_ctx_set_model(c, r.bag->models[p.batches[(size_t)k].q]));
        while (p.jobs[(size_t)tLo].kLast < k)
            ++tLo;
        int tHi = tLo; // one past the last track of the batch
        while (tHi < p.T && p.jobs[(size_t)tHi].kFirst <= k)
            ++tHi;
        DMXCHK(tracks_upload(r, k, tLo, tHi));
        DMXCHK(tracks_infer(r, k));
        if (p.mmax == 0)
            DMXCHK(tracks_ola(r, k));
        else
        {
            DMXCHK(tracks_ola(r, k, 0));
            DMXCHK(tracks_ola(r, k, 1));
            DMXCHK(tracks_convert(r, k));
        }
        if (r.pcm)
            DMXCHK(tracks_output_stage(r, k));
        hipEvent_t ev = dmx_batch_event(c, (size_t)k);
        if (!ev)
            return fail(DMX_ERR_HIP, "%s: hipEventCreate failed", r.fn);
        HIPCHK(hipEventRecord(ev, c->stream));
        if (k > 0)
            DMXCHK(tracks_copy_out(r, k - 1));
    }
    DMXCHK(tracks_copy_out(r, p.nBatches() - 1));
    const int rcSync = dmx_ctx_sync_checked(c);
    HIPCHK(hipStreamSynchronize(c->copyStream));
    return rcSync;
}

// a bag leaves the context bound to the model it entered with, on success and on error
static int tracks_run(TracksRun &r)
{
    dmx_ctx *c = r.c;
    const dmx_model *entry = c->m;
    const int rc = tracks_run_impl(r);
    if (c->m == entry)
        return rc;
    const std::string err = rc != DMX_OK ? dmx_err_string() : std::string();
    const int rcBind = dmx_ctx_set_model(c, entry);
    if (rc != DMX_OK)
        dmx_set_err_string(err);
    return rc != DMX_OK ? rc : rcBind;
}

extern "C" int dmx_track_infer(dmx_ctx *c, const float *audio, int64_t n, int shift_offset, float *out, int layout,
                               dmx_progress_fn progress, void *user)
{
    if (!c || !audio || !out || n < 2)
        return fail(DMX_ERR_ARG, "dmx_track_infer: invalid argument");
    if (layout != DMX_LAYOUT_EIGEN && layout != DMX_LAYOUT_PLANAR)
        return fail(DMX_ERR_ARG, "dmx_track_infer: unknown layout %d", layout);
    if (shift_offset < 0)
        shift_offset = rand() % DMX_MAX_SHIFT; // model_apply.cpp:114
    if (shift_offset >= DMX_MAX_SHIFT)
        return fail(DMX_ERR_ARG, "dmx_track_infer: shift_offset must be < %d", DMX_MAX_SHIFT);
    TracksRun r;
    r.c = c, r.fn = "dmx_track_infer", r.T = 1, r.audio = &audio, r.n = &n, r.N = 1, r.stride = overlap_stride(c->seg, 0.25f);
    r.shifts = &shift_offset, r.out = &out, r.layout = layout, r.progress = progress, r.user = user;
    return tracks_run(r);
}

extern "C" int dmx_tracks_infer(dmx_ctx *c, int n_tracks, const float *const *audio, const int64_t *n, const int *shift_offsets,
                                float *const *out, int layout, dmx_progress_fn progress, void *user)
{
    if (!c)
        return fail(DMX_ERR_ARG, "dmx_tracks_infer: null context");
    if (n_tracks < 1)
        return fail(DMX_ERR_ARG, "dmx_tracks_infer: n_tracks must be >= 1, got %d", n_tracks);
    if (!audio || !n || !out)
        return fail(DMX_ERR_ARG, "dmx_tracks_infer: null %s array", !audio ? "audio" : !n ? "n" : "out");
    if (layout != DMX_LAYOUT_EIGEN && layout != DMX_LAYOUT_PLANAR)
        return fail(DMX_ERR_ARG, "dmx_tracks_infer: unknown layout %d", layout);
    for (int t = 0; t < n_tracks; ++t)
    {
        if (!audio[t])
            return fail(DMX_ERR_ARG, "dmx_tracks_infer: track %d: null audio pointer", t);
        if (!out[t])
            return fail(DMX_ERR_ARG, "dmx_tracks_infer: track %d: null out pointer", t);
        if (n[t] < 2)
            return fail(DMX_ERR_ARG, "dmx_tracks_infer: track %d: n = %lld, must be >= 2", t, (long long)n[t]);
        if (shift_offsets && (shift_offsets[t] < -1 || shift_offsets[t] >= DMX_MAX_SHIFT))
            return fail(DMX_ERR_ARG, "dmx_tracks_infer: track %d: shift_offset %d not in [-1, %d)", t, shift_offsets[t], DMX_MAX_SHIFT);
    }
    std::vector<int> shifts((size_t)n_tracks);
    for (int t = 0; t < n_tracks; ++t) // drawn in track order, like successive dmx_track_infer calls (model_apply.cpp:114)
        shifts[(size_t)t] = !shift_offsets || shift_offsets[t] < 0 ? rand() % DMX_MAX_SHIFT : shift_offsets[t];
    TracksRun r;
    r.c = c, r.fn = "dmx_tracks_infer", r.T = n_tracks, r.audio = audio, r.n = n, r.N = 1, r.stride = overlap_stride(c->seg, 0.25f);
    r.shifts = shifts.data(), r.out = out, r.layout = layout, r.progress = progress, r.user = user;
    return tracks_run(r);
}

extern "C" int dmx_track_geometry_overlap(int64_t segment_samples, int64_t n, int shift_offset, float overlap, int64_t *shifted_len,
                                          int *n_segments, int64_t *stride)
{
    if (segment_samples < 1 || n <= 0)
        return fail(DMX_ERR_ARG, "dmx_track_geometry_overlap: invalid argument (segment_samples %lld, n %lld)",
                    (long long)segment_samples, (long long)n);
    if (shift_offset < 0 || shift_offset >= DMX_MAX_SHIFT)
        return fail(DMX_ERR_ARG, "dmx_track_geometry_overlap: shift_offset %d not in [0, %d)", shift_offset, DMX_MAX_SHIFT);
    if (!(overlap >= 0.0f && overlap <= DMX_MAX_OVERLAP)) // also NaN
        return fail(DMX_ERR_ARG, "dmx_track_geometry_overlap: overlap %g not in [0, %g]", (double)overlap, (double)DMX_MAX_OVERLAP);
    const i64 st = overlap_stride(segment_samples, overlap);
    if (st < 1)
        return fail(DMX_ERR_ARG, "dmx_track_geometry_overlap: stride %lld < 1", (long long)st);
    const i64 len = track_shifted_len(n, shift_offset);
    if (shifted_len)
        *shifted_len = len;
    if (stride)
        *stride = st;
    if (n_segments)
        *n_segments = track_n_segments(len, st);
    return DMX_OK;
}

// One request of dmx_tracks_infer_{opts,pcm,bag,remix,flac}: the entry points fill it, tracks_call checks and runs it
enum // TracksCall::kind
{
    TRACKS_OUT_F32,   // fp32 stems into out[t]
    TRACKS_OUT_PCM,   // an output spec
    TRACKS_OUT_REMIX, // a remix spec
    TRACKS_OUT_FLAC   // a remix spec, and the outputs leave as .flac files
};
struct TracksCall
{
    const char *fn;
    dmx_ctx *c;
    int n_tracks;
    const float *const *audio;
    const int64_t *n;
    int n_shifts;
    float overlap;
    const int *shift_offsets; // tracks x shifts; with models: tracks x models x shifts
    bool bag;                 // the call has a model dimension: models, n_models, weights
    const dmx_model *const *models;
    int n_models;
    const float *weights;
    int kind; // TRACKS_OUT_*: which of spec, remix, flacRate and flacSizes are read
    const dmx_output_spec *spec;
    const dmx_remix_spec *remix;
    int flacRate;
    int64_t *flacSizes;
    const int *rates;            // dmx_tracks_infer_rates: n[t] frames at rates[t] (checked: check_tracks_rates); else NULL, all 44100
    const dmx_loudness_spec *loud; // dmx_tracks_infer_loud: the loudness stage behind a remix spec, and its report; else NULL
    dmx_loudness_result *report;
    dmx_meters_result *meters;   // dmx_tracks_infer_meters: the meters report, or NULL
    const dmx_limiter_spec *lim; // dmx_tracks_infer_limit: the limiter's times (NULL: the defaults) and its report, or NULL
    dmx_limit_result *limit;
    const dmx_flac_info *flacIn; // dmx_tracks_infer_from_flac: audio[t] is a file image, described here; else NULL
    const int64_t *fileBytes;
    int64_t *trackStatus;
    void *const *out;
    float *peaks;
    int layout;
    dmx_progress_fn progress;
    void *user;
};
static int tracks_call(const TracksCall &a);

// the argument checks every such request shares (before any GPU work); gives the stride
static int check_tracks_opts(const TracksCall &a, i64 &stride)
{
    const char *fn = a.fn;
    const int n_models = a.bag ? a.n_models : 0, N = a.n_shifts;
    if (!a.c)
        return fail(DMX_ERR_ARG, "%s: null context", fn);
    if (a.n_tracks < 1)
        return fail(DMX_ERR_ARG, "%s: n_tracks must be >= 1, got %d", fn, a.n_tracks);
    if (!a.audio || !a.n || !a.out)
        return fail(DMX_ERR_ARG, "%s: null %s array", fn, !a.audio ? "audio" : !a.n ? "n" : "out");
    if (a.layout != DMX_LAYOUT_EIGEN && a.layout != DMX_LAYOUT_PLANAR)
        return fail(DMX_ERR_ARG, "%s: unknown layout %d", fn, a.layout);
    if (N < 1 || N > DMX_MAX_SHIFTS)
        return fail(DMX_ERR_ARG, "%s: n_shifts must be in [1, %d], got %d", fn, DMX_MAX_SHIFTS, N);
    if (!(a.overlap >= 0.0f && a.overlap <= DMX_MAX_OVERLAP))
        return fail(DMX_ERR_ARG, "%s: overlap %g not in [0, %g]", fn, (double)a.overlap, (double)DMX_MAX_OVERLAP);
    stride = overlap_stride(a.c->seg, a.overlap);
    if (stride < 1)
        return fail(DMX_ERR_ARG, "%s: stride %lld < 1 (segment %lld, overlap %g)", fn, (long long)stride, (long long)a.c->seg,
                    (double)a.overlap);
    for (int t = 0; t < a.n_tracks; ++t)
    {
        if (!a.audio[t])
            return fail(DMX_ERR_ARG, "%s: track %d: null audio pointer", fn, t);
        if (!a.out[t])
            return fail(DMX_ERR_ARG, "%s: track %d: null out pointer", fn, t);
        if (a.n[t] < 2)
            return fail(DMX_ERR_ARG, "%s: track %d: n = %lld, must be >= 2", fn, t, (long long)a.n[t]);
        for (int k = 0; a.shift_offsets && !n_models && k < N; ++k)
        {
            const int s = a.shift_offsets[(size_t)t * N + k];
            if (s < -1 || s >= DMX_MAX_SHIFT)
                return fail(DMX_ERR_ARG, "%s: track %d, shift %d: shift_offset %d not in [-1, %d)", fn, t, k, s, DMX_MAX_SHIFT);
        }
        for (int x = 0; a.shift_offsets && x < n_models * N; ++x)
        {
            const int s = a.shift_offsets[(size_t)t * n_models * N + x];
            if (s < -1 || s >= DMX_MAX_SHIFT)
                return fail(DMX_ERR_ARG, "%s: track %d, model %d, shift %d: shift_offset %d not in [-1, %d)", fn, t, x / N, x % N, s,
                            DMX_MAX_SHIFT);
        }
    }
    return DMX_OK;
}
// drawn in (track, copy) order; N = 1: dmx_tracks_infer's order
static std::vector<int> draw_shifts(int n_tracks, int N, const int *shift_offsets)
{
    std::vector<int> shifts((size_t)n_tracks * N);
    for (size_t i = 0; i < shifts.size(); ++i)
        shifts[i] = !shift_offsets || shift_offsets[i] < 0 ? rand() % DMX_MAX_SHIFT : shift_offsets[i];
    return shifts;
}

extern "C" int dmx_tracks_infer_opts(dmx_ctx *c, int n_tracks, const float *const *audio, const int64_t *n, int n_shifts,
                                     float overlap, const int *shift_offsets, float *const *out, int layout, dmx_progress_fn progress,
                                     void *user)
{
    TracksCall a{};
    a.fn = "dmx_tracks_infer_opts", a.c = c, a.n_tracks = n_tracks, a.audio = audio, a.n = n;
    a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.kind = TRACKS_OUT_F32, a.out = reinterpret_cast<void *const *>(out), a.layout = layout, a.progress = progress, a.user = user;
    return tracks_call(a);
}

// --------------------------------------------------------------------------- PCM output (pcm.hip)
// the spec's own fields; S < 0: the model is not known yet (the stem's upper bound is checked once it is)
int dmx_pcm_check_spec(const char *fn, const dmx_output_spec *spec, int S)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: output spec: null", fn);
    if (spec->encoding != DMX_PCM_F32 && spec->encoding != DMX_PCM_S16 && spec->encoding != DMX_PCM_S24)
        return fail(DMX_ERR_ARG, "%s: output spec: encoding %d (DMX_PCM_F32 0, DMX_PCM_S16 1, DMX_PCM_S24 2)", fn, spec->encoding);
    if (spec->clip != DMX_CLIP_NONE && spec->clip != DMX_CLIP_RESCALE && spec->clip != DMX_CLIP_CLAMP)
        return fail(DMX_ERR_ARG, "%s: output spec: clip %d (DMX_CLIP_NONE 0, DMX_CLIP_RESCALE 1, DMX_CLIP_CLAMP 2)", fn, spec->clip);
    if (spec->stem < -1)
        return fail(DMX_ERR_ARG, "%s: output spec: stem %d (-1: all stems)", fn, spec->stem);
    if (S >= 0 && spec->stem >= S)
        return fail(DMX_ERR_ARG, "%s: output spec: stem %d of a %d-source model", fn, spec->stem, S);
    return DMX_OK;
}
int dmx_pcm_frame_bytes(int encoding) { return encoding == DMX_PCM_F32 ? 8 : encoding == DMX_PCM_S16 ? 4 : 6; }

extern "C" int dmx_output_count(const dmx_model *m, const dmx_output_spec *spec)
{
    if (!m || dmx_pcm_check_spec("dmx_output_count", spec, m->pm.n_sources) != DMX_OK)
        return -1;
    return spec->stem < 0 ? m->pm.n_sources : 2;
}
extern "C" int64_t dmx_output_bytes(const dmx_output_spec *spec, int64_t n)
{
    if (n < 0 || dmx_pcm_check_spec("dmx_output_bytes", spec, -1) != DMX_OK)
        return -1;
    return n * dmx_pcm_frame_bytes(spec->encoding);
}

extern "C" int dmx_tracks_infer_pcm(dmx_ctx *c, int n_tracks, const float *const *audio, const int64_t *n, int n_shifts, float overlap,
                                    const int *shift_offsets, const dmx_output_spec *spec, void *const *out, float *peaks, int layout,
                                    dmx_progress_fn progress, void *user)
{
    TracksCall a{};
    a.fn = "dmx_tracks_infer_pcm", a.c = c, a.n_tracks = n_tracks, a.audio = audio, a.n = n;
    a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.kind = TRACKS_OUT_PCM, a.spec = spec, a.out = out, a.peaks = peaks, a.layout = layout, a.progress = progress, a.user = user;
    return tracks_call(a);
}

// --------------------------------------------------------------------------- remix outputs (pcm.hip)
// the checks of dmx_remix_check; G (may be NULL): the kernels' table. noModel (S and G unused): the model is not known (no
// context): the checks that do not need the width of the matrix
int dmx_remix_check_spec(const char *fn, int S, const dmx_remix_spec *spec, PcmGains *G, bool noModel)
{
    if (!noModel && (S < 1 || S > PcmGains::kMaxSrc - 1))
        return fail(DMX_ERR_ARG, "%s: remix spec: n_sources must be in [1, %d], got %d", fn, PcmGains::kMaxSrc - 1, S);
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: remix spec: null", fn);
    if (spec->n_out < 1 || spec->n_out > DMX_MAX_OUTPUTS)
        return fail(DMX_ERR_ARG, "%s: remix spec: n_out must be in [1, %d], got %d", fn, DMX_MAX_OUTPUTS, spec->n_out);
    if (!spec->gains)
        return fail(DMX_ERR_ARG, "%s: remix spec: null gain matrix", fn);
    for (int o = 0; !noModel && o < spec->n_out; ++o)
    {
        bool any = false;
        for (int s = 0; s <= S; ++s)
        {
            const float g = spec->gains[o * (S + 1) + s];
            if (!std::isfinite(g))
            {
                if (s < S)
                    return fail(DMX_ERR_ARG, "%s: remix spec: output %d, source %d: gain %g is not finite", fn, o, s, (double)g);
                return fail(DMX_ERR_ARG, "%s: remix spec: output %d, source %d (the mixture): gain %g is not finite", fn, o, s, (double)g);
            }
            any = any || g != 0.0f;
        }
        if (!any)
            return fail(DMX_ERR_ARG, "%s: remix spec: output %d has no non-zero gain", fn, o);
    }
    if (spec->encoding != DMX_PCM_F32 && spec->encoding != DMX_PCM_S16 && spec->encoding != DMX_PCM_S24)
        return fail(DMX_ERR_ARG, "%s: remix spec: encoding %d (DMX_PCM_F32 0, DMX_PCM_S16 1, DMX_PCM_S24 2)", fn, spec->encoding);
    if (spec->clip != DMX_CLIP_NONE && spec->clip != DMX_CLIP_RESCALE && spec->clip != DMX_CLIP_CLAMP)
        return fail(DMX_ERR_ARG, "%s: remix spec: clip %d (DMX_CLIP_NONE 0, DMX_CLIP_RESCALE 1, DMX_CLIP_CLAMP 2)", fn, spec->clip);
    if (G && !noModel)
    {
        std::memset(G, 0, sizeof(*G));
        G->nOut = spec->n_out, G->S = S;
        for (int o = 0; o < spec->n_out; ++o)
            for (int s = 0; s <= S; ++s)
                G->g[o][s] = spec->gains[o * (S + 1) + s];
    }
    return DMX_OK;
}

extern "C" int dmx_remix_check(int n_sources, const dmx_remix_spec *spec)
{
    return dmx_remix_check_spec("dmx_remix_check", n_sources, spec, nullptr, false);
}

extern "C" int dmx_remix_two_stems(int n_sources, int stem, int method, float *gains_out, int *n_out)
{
    const char *fn = "dmx_remix_two_stems";
    const int S = n_sources;
    if (S < 1 || S > PcmGains::kMaxSrc - 1)
        return fail(DMX_ERR_ARG, "%s: n_sources must be in [1, %d], got %d", fn, PcmGains::kMaxSrc - 1, S);
    if (stem < 0 || stem >= S)
        return fail(DMX_ERR_ARG, "%s: stem %d of a %d-source model", fn, stem, S);
    if (method != DMX_OTHER_ADD && method != DMX_OTHER_MINUS && method != DMX_OTHER_NONE)
        return fail(DMX_ERR_ARG, "%s: method %d (DMX_OTHER_ADD 0, DMX_OTHER_MINUS 1, DMX_OTHER_NONE 2)", fn, method);
    if (method == DMX_OTHER_ADD && S < 2)
        return fail(DMX_ERR_ARG, "%s: DMX_OTHER_ADD needs at least 2 sources", fn);
    if (!gains_out || !n_out)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !gains_out ? "gains_out" : "n_out");
    const int rows = method == DMX_OTHER_NONE ? 1 : 2;
    for (int i = 0; i < rows * (S + 1); ++i)
        gains_out[i] = 0.0f;
    gains_out[stem] = 1.0f;
    if (method == DMX_OTHER_ADD)
        for (int s = 0; s < S; ++s)
            gains_out[(S + 1) + s] = s == stem ? 0.0f : 1.0f;
    else if (method == DMX_OTHER_MINUS)
        gains_out[(S + 1) + stem] = -1.0f, gains_out[(S + 1) + S] = 1.0f;
    *n_out = rows;
    return DMX_OK;
}

// --------------------------------------------------------------------------- bags of models
// the checks of dmx_bag_weights; eff (Q x S) and sums (S) may be NULL
static int bag_weights_check(const char *fn, int Q, int S, const float *weights, float *eff, float *sums)
{
    if (Q < 1 || Q > DMX_MAX_BAG)
        return fail(DMX_ERR_ARG, "%s: n_models must be in [1, %d], got %d", fn, DMX_MAX_BAG, Q);
    if (S < 1 || S > TrackBagTable::kMaxStems)
        return fail(DMX_ERR_ARG, "%s: n_sources must be in [1, %d], got %d", fn, TrackBagTable::kMaxStems, S);
    if (!weights && Q != S)
        return fail(DMX_ERR_ARG, "%s: weights: NULL (the diagonal bag) needs n_models == n_sources, got %d models of %d sources", fn, Q, S);
    float w[DMX_MAX_BAG * TrackBagTable::kMaxStems];
    for (int q = 0; q < Q; ++q)
        for (int s = 0; s < S; ++s)
        {
            const float v = weights ? weights[q * S + s] : (q == s ? 1.0f : 0.0f);
            if (!(v >= 0.0f) || std::isinf(v)) // also NaN
                return fail(DMX_ERR_ARG, "%s: weights: model %d, stem %d: weight %g is negative or not finite", fn, q, s, (double)v);
            w[q * S + s] = v;
        }
    float W[TrackBagTable::kMaxStems];
    for (int s = 0; s < S; ++s)
    {
        bool have = false;
        W[s] = 0.0f;
        for (int q = 0; q < Q; ++q) // the kernel's order: the first contributing weight initialises the sum
            if (w[q * S + s] != 0.0f)
                W[s] = have ? W[s] + w[q * S + s] : w[q * S + s], have = true;
        if (!have)
            return fail(DMX_ERR_ARG, "%s: weights: stem %d has no model", fn, s);
        if (std::isinf(W[s]))
            return fail(DMX_ERR_ARG, "%s: weights: stem %d: the sum of the weights is not finite", fn, s);
    }
    for (int q = 0; q < Q; ++q)
    {
        bool any = false;
        for (int s = 0; s < S; ++s)
            any = any || w[q * S + s] != 0.0f;
        if (!any)
            return fail(DMX_ERR_ARG, "%s: weights: model %d has no non-zero weight", fn, q);
    }
    if (eff)
        std::memcpy(eff, w, sizeof(float) * (size_t)(Q * S));
    if (sums)
        std::memcpy(sums, W, sizeof(float) * (size_t)S);
    return DMX_OK;
}

extern "C" int dmx_bag_weights(int n_models, int n_sources, const float *weights, float *weights_out, float *sums_out)
{
    return bag_weights_check("dmx_bag_weights", n_models, n_sources, weights, weights_out, sums_out);
}

// the model dimension of a request: the models against the context's, and the weights -> w (Q x S)
static int check_tracks_bag(const TracksCall &a, float *w)
{
    const char *fn = a.fn;
    if (!a.c)
        return fail(DMX_ERR_ARG, "%s: null context", fn);
    if (a.n_models < 1 || a.n_models > DMX_MAX_BAG)
        return fail(DMX_ERR_ARG, "%s: n_models must be in [1, %d], got %d", fn, DMX_MAX_BAG, a.n_models);
    if (!a.models)
        return fail(DMX_ERR_ARG, "%s: null models array", fn);
    const dmx_model *cm = a.c->m;
    for (int q = 0; q < a.n_models; ++q)
    {
        const dmx_model *m = a.models[q];
        if (!m)
            return fail(DMX_ERR_ARG, "%s: model %d: null", fn, q);
        if (m->device != cm->device || m->pm.arch != cm->pm.arch || m->pm.n_sources != cm->pm.n_sources || m->pm.dim != cm->pm.dim ||
            m->blobFloats != cm->blobFloats || m->pm.index != cm->pm.index) // dmx_ctx_set_model's test
            return fail(DMX_ERR_ARG, "%s: model %d: differs in architecture or device from the context's", fn, q);
    }
    return bag_weights_check(fn, a.n_models, cm->pm.n_sources, a.weights, w, nullptr);
}

// what dmx_tracks_infer_flac asks of its own arguments
static int check_tracks_flac(const TracksCall &a)
{
    const char *fn = a.fn;
    DMXCHK(dmx_remix_check_spec(fn, 0, a.remix, nullptr, true)); // what of the spec can be checked without a model
    if (a.remix->encoding == DMX_PCM_F32)
        return fail(DMX_ERR_ARG, "%s: remix spec: encoding DMX_PCM_F32 has no FLAC form (DMX_PCM_S16 1 or DMX_PCM_S24 2)", fn);
    if (!a.flacSizes)
        return fail(DMX_ERR_ARG, "%s: null sizes array", fn);
    if (a.flacRate < 1 || a.flacRate > 655350)
        return fail(DMX_ERR_ARG, "%s: sample_rate %d not in [1, 655350]", fn, a.flacRate);
    for (int t = 0; a.n && t < a.n_tracks; ++t)
        if (a.n[t] >= (int64_t)1 << 36)
            return fail(DMX_ERR_ARG, "%s: track %d: n = %lld, must be < 2^36", fn, t, (long long)a.n[t]);
    return DMX_OK;
}

// The checks of a request, in the order that decides which error a doubly-wrong call reports, then the run.
// With a remix spec the spec comes before the context's other uses; with models, the models, the weights and the output
// spec come before the arguments every request shares; without models an output spec is checked before them (the stem's
// upper bound after them, once the model is known).
static int tracks_call(const TracksCall &a)
{
    const char *fn = a.fn;
    const bool remix = a.kind == TRACKS_OUT_REMIX || a.kind == TRACKS_OUT_FLAC;
    if (a.kind == TRACKS_OUT_FLAC)
        DMXCHK(check_tracks_flac(a));
    PcmGains G;
    if (remix)
    {
        if (!a.c)
        {
            DMXCHK(dmx_remix_check_spec(fn, 0, a.remix, nullptr, true)); // what of the spec can be checked without a model
            return fail(DMX_ERR_ARG, "%s: null context", fn);
        }
        DMXCHK(dmx_remix_check_spec(fn, a.c->m->pm.n_sources, a.remix, &G, false));
        if (!a.bag && a.weights)
            return fail(DMX_ERR_ARG, "%s: weights given without models", fn);
    }
    float w[DMX_MAX_BAG * TrackBagTable::kMaxStems];
    if (a.bag)
    {
        DMXCHK(check_tracks_bag(a, w));
        if (a.kind == TRACKS_OUT_PCM)
            DMXCHK(dmx_pcm_check_spec(fn, a.spec, a.c->m->pm.n_sources));
        if (a.n_shifts >= 1 && (i64)a.n_models * a.n_shifts > TrackBagTable::kMaxCopies)
            return fail(DMX_ERR_ARG, "%s: n_models * n_shifts must be <= %d, got %d x %d", fn, TrackBagTable::kMaxCopies, a.n_models,
                        a.n_shifts);
    }
    else if (a.kind == TRACKS_OUT_PCM)
        DMXCHK(dmx_pcm_check_spec(fn, a.spec, -1));
    i64 stride = 0;
    DMXCHK(check_tracks_opts(a, stride));
    const int S = a.c->m->pm.n_sources;
    if (!a.bag && a.kind == TRACKS_OUT_PCM)
        DMXCHK(dmx_pcm_check_spec(fn, a.spec, S));
    const BagRun bag{a.models, a.n_models, w};
    PcmOut pcm{};
    if (remix)
        pcm = PcmOut{dmx_output_spec{a.remix->encoding, a.remix->clip, -1}, a.out, a.peaks, a.remix->n_out, dmx_pcm_frame_bytes(a.remix->encoding),
                     &G, 0, 0, nullptr};
    else if (a.kind == TRACKS_OUT_PCM)
        pcm = PcmOut{*a.spec, a.out, a.peaks, a.spec->stem < 0 ? S : 2, dmx_pcm_frame_bytes(a.spec->encoding), nullptr, 0, 0, nullptr};
    if (a.kind == TRACKS_OUT_FLAC)
        pcm.flacBits = pcm.spec.encoding == DMX_PCM_S16 ? 16 : 24, pcm.flacRate = a.flacRate, pcm.sizes = a.flacSizes, pcm.rates = a.rates;
    if (remix && a.loud)
    {
        pcm.loud = a.loud, pcm.report = a.report, pcm.meters = a.meters;
        if (!a.c->dLoudTable) // once per context: built on the host, uploaded, freed with the context
        {
            std::vector<float> h((size_t)kLoudGainSteps);
            loud_gain_table(h.data());
            HIPCHK(hipSetDevice(a.c->m->device));
            HIPCHK(hipMalloc(&a.c->dLoudTable, sizeof(float) * h.size()));
            HIPCHK(hipMemcpy(a.c->dLoudTable, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
        }
        pcm.loudTable = a.c->dLoudTable;
        pcm.lim = a.lim, pcm.limit = a.limit;
        if (pcm.limited())
            DMXCHK(dmx_limiter_device_tables(a.c->m->device, &pcm.limTables));
        else if (a.limit) // nothing is limited: the report says so
            std::memset(a.limit, 0, sizeof(dmx_limit_result) * (size_t)a.n_tracks * (size_t)pcm.nOut);
    }
    // (track, copy) order; with models (track, model, copy) order
    const std::vector<int> shifts = draw_shifts(a.bag ? a.n_tracks * a.n_models : a.n_tracks, a.n_shifts, a.shift_offsets);
    TracksRun r;
    r.c = a.c, r.fn = fn, r.T = a.n_tracks, r.audio = a.audio, r.n = a.n, r.N = a.n_shifts, r.stride = stride, r.shifts = shifts.data();
    r.layout = a.layout, r.progress = a.progress, r.user = a.user;
    r.flacIn = a.flacIn, r.fileBytes = a.fileBytes, r.trackStatus = a.trackStatus, r.rates = a.rates;
    if (a.kind == TRACKS_OUT_F32)
        r.out = reinterpret_cast<float *const *>(a.out);
    else
        r.pcm = &pcm;
    if (a.bag)
        r.bag = &bag;
    for (int t = 0; a.trackStatus && t < 2 * a.n_tracks; ++t) // every argument has passed
        a.trackStatus[t] = -1;
    return tracks_run(r);
}

extern "C" int dmx_tracks_infer_bag(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                    const float *const *audio, const int64_t *n, int n_shifts, float overlap, const int *shift_offsets,
                                    const dmx_output_spec *spec, void *const *out, float *peaks, int layout, dmx_progress_fn progress,
                                    void *user)
{
    TracksCall a{};
    a.fn = "dmx_tracks_infer_bag", a.c = c, a.n_tracks = n_tracks, a.audio = audio, a.n = n;
    a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.bag = true, a.models = models, a.n_models = n_models, a.weights = weights;
    a.kind = spec ? TRACKS_OUT_PCM : TRACKS_OUT_F32, a.spec = spec;
    a.out = out, a.peaks = peaks, a.layout = layout, a.progress = progress, a.user = user;
    return tracks_call(a);
}

// dmx_tracks_infer_remix and dmx_tracks_infer_flac: the request has a model dimension when models are given
static TracksCall remix_call(const char *fn, dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights,
                             const dmx_remix_spec *spec)
{
    TracksCall a{};
    a.fn = fn, a.c = c, a.bag = models || n_models != 0, a.models = models, a.n_models = n_models, a.weights = weights;
    a.kind = TRACKS_OUT_REMIX, a.remix = spec;
    return a;
}

extern "C" int dmx_tracks_infer_remix(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                      const float *const *audio, const int64_t *n, int n_shifts, float overlap, const int *shift_offsets,
                                      const dmx_remix_spec *spec, void *const *out, float *peaks, int layout, dmx_progress_fn progress,
                                      void *user)
{
    TracksCall a = remix_call("dmx_tracks_infer_remix", c, models, n_models, weights, spec);
    a.n_tracks = n_tracks, a.audio = audio, a.n = n, a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.out = out, a.peaks = peaks, a.layout = layout, a.progress = progress, a.user = user;
    return tracks_call(a);
}

extern "C" int dmx_tracks_infer_flac(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                     const float *const *audio, const int64_t *n, int n_shifts, float overlap, const int *shift_offsets,
                                     const dmx_remix_spec *spec, int sample_rate, void *const *out, int64_t *sizes, float *peaks, int layout,
                                     dmx_progress_fn progress, void *user)
{
    TracksCall a = remix_call("dmx_tracks_infer_flac", c, models, n_models, weights, spec);
    a.kind = TRACKS_OUT_FLAC, a.flacRate = sample_rate, a.flacSizes = sizes;
    a.n_tracks = n_tracks, a.audio = audio, a.n = n, a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.out = out, a.peaks = peaks, a.layout = layout, a.progress = progress, a.user = user;
    return tracks_call(a);
}

// what a call with rates asks of them, from numbers alone (no context, no device): n may be NULL (reported later)
static int check_tracks_rates(const char *fn, int n_tracks, const int64_t *n, const int *rates, bool flac)
{
    for (int t = 0; t < n_tracks; ++t)
    {
        const int rate = rates[t];
        if (rate == 44100)
            continue;
        if (rate >= 1 && n && n[t] >= 0 && dmx_resample_length(n[t], rate, 44100) < 2)
            return fail(DMX_ERR_ARG, "%s: track %d: %lld frames at %d Hz leave %lld at 44100 Hz", fn, t, (long long)n[t], rate,
                        (long long)dmx_resample_length(n[t], rate, 44100));
        if (resample_check(rate, 44100, 2) != DMX_OK || resample_check(44100, rate, 2) != DMX_OK)
        {
            const std::string why = dmx_err_string();
            return fail(DMX_ERR_ARG, "%s: track %d: sample rate %d: %s", fn, t, rate, why.c_str());
        }
        if (flac && rate > 655350)
            return fail(DMX_ERR_ARG, "%s: track %d: sample rate %d has no FLAC form (at most 655350)", fn, t, rate);
    }
    return DMX_OK;
}

// tracks given as .flac files: every file is probed before any GPU work, then the request is dmx_tracks_infer_remix's or
// dmx_tracks_infer_flac's with the tracks decoded in their slots (tracks_upload)
// anyRate (dmx_tracks_infer_from_flac_rates): every track runs at its file's rate, as dmx_tracks_infer_rates runs it
static int tracks_from_flac(const char *fn, bool anyRate, dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights,
                            int n_tracks, const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                            const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes, float *peaks,
                            int64_t *track_status, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud = nullptr,
                            dmx_loudness_result *report = nullptr, dmx_meters_result *meters = nullptr, const dmx_limiter_spec *lim = nullptr,
                            dmx_limit_result *limit = nullptr)
{
    if (n_tracks < 1)
        return fail(DMX_ERR_ARG, "%s: n_tracks must be >= 1, got %d", fn, n_tracks);
    if (!files || !file_bytes || !track_status)
        return fail(DMX_ERR_ARG, "%s: null %s array", fn, !files ? "files" : !file_bytes ? "file_bytes" : "track_status");
    std::vector<dmx_flac_info> infos((size_t)n_tracks);
    std::vector<int64_t> ns((size_t)n_tracks);
    std::vector<int> rates((size_t)n_tracks);
    for (int t = 0; t < n_tracks; ++t)
    {
        if (!files[t])
            return fail(DMX_ERR_ARG, "%s: track %d: null file pointer", fn, t);
        char msg[160];
        if (flac_in_probe(files[t], file_bytes[t], &infos[(size_t)t], msg, sizeof msg) != 0)
            return fail(DMX_ERR_FORMAT, "%s: track %d: %s", fn, t, msg);
        if (!anyRate && infos[(size_t)t].sample_rate != 44100)
            return fail(DMX_ERR_ARG, "%s: track %d: sample rate %d (the track path takes 44100; decode with dmx_flac_decode and resample)", fn,
                        t, infos[(size_t)t].sample_rate);
        if (flac_in_workspace_bytes(&infos[(size_t)t], file_bytes[t]) < 0)
            return fail(DMX_ERR_FORMAT, "%s: track %d: block size range %d..%d is not supported", fn, t, infos[(size_t)t].min_block,
                        infos[(size_t)t].max_block);
        ns[(size_t)t] = infos[(size_t)t].total_samples;
        rates[(size_t)t] = infos[(size_t)t].sample_rate;
    }
    for (int t = 0; loud && t < n_tracks; ++t) // the loudness stage's own floor on a rate, with the track's number
        DMXCHK(dmx_limit_check_spec(fn, loud, lim, rates[(size_t)t], t));
    if (anyRate)
        DMXCHK(check_tracks_rates(fn, n_tracks, ns.data(), rates.data(), flac_out != 0));
    TracksCall a = remix_call(fn, c, models, n_models, weights, spec);
    a.rates = anyRate ? rates.data() : nullptr;
    if (flac_out)
        a.kind = TRACKS_OUT_FLAC, a.flacRate = 44100, a.flacSizes = sizes;
    a.n_tracks = n_tracks, a.audio = reinterpret_cast<const float *const *>(files), a.n = ns.data();
    a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.flacIn = infos.data(), a.fileBytes = file_bytes, a.trackStatus = track_status;
    a.loud = loud, a.report = report, a.meters = meters, a.lim = lim, a.limit = limit;
    a.out = out, a.peaks = peaks, a.layout = DMX_LAYOUT_EIGEN, a.progress = progress, a.user = user;
    DMXCHK(tracks_call(a)); // (track_status: -1 until the track's own arrives)
    for (int t = 0; t < n_tracks; ++t)
        if (track_status[2 * t] != DMX_FLAC_OK)
            return fail(DMX_ERR_FORMAT, "%s: track %d: %s at sample %lld of %lld (the samples from there on were taken as silence)", fn, t,
                        track_status[2 * t] == DMX_FLAC_BROKEN ? "the stream breaks" : "too many frame header look-alikes, nothing decoded",
                        (long long)track_status[2 * t + 1], (long long)ns[(size_t)t]);
    return DMX_OK;
}

extern "C" int dmx_tracks_infer_from_flac(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                          const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                          const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                          float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user)
{
    return tracks_from_flac("dmx_tracks_infer_from_flac", false, c, models, n_models, weights, n_tracks, files, file_bytes, n_shifts, overlap,
                            shift_offsets, spec, flac_out, out, sizes, peaks, track_status, progress, user);
}

extern "C" int dmx_tracks_infer_from_flac_rates(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                                const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                                const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out,
                                                int64_t *sizes, float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user)
{
    return tracks_from_flac("dmx_tracks_infer_from_flac_rates", true, c, models, n_models, weights, n_tracks, files, file_bytes, n_shifts,
                            overlap, shift_offsets, spec, flac_out, out, sizes, peaks, track_status, progress, user);
}

extern "C" int dmx_tracks_infer_rates(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                      const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                                      const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                      float *peaks, int layout, dmx_progress_fn progress, void *user)
{
    const char *fn = "dmx_tracks_infer_rates";
    if (n_tracks < 1)
        return fail(DMX_ERR_ARG, "%s: n_tracks must be >= 1, got %d", fn, n_tracks);
    if (!rates)
        return fail(DMX_ERR_ARG, "%s: null rates array", fn);
    if (!spec && flac_out)
        return fail(DMX_ERR_ARG, "%s: FLAC files need a remix spec", fn);
    DMXCHK(check_tracks_rates(fn, n_tracks, n, rates, flac_out != 0));
    TracksCall a = remix_call(fn, c, models, n_models, weights, spec);
    a.kind = !spec ? TRACKS_OUT_F32 : flac_out ? TRACKS_OUT_FLAC : TRACKS_OUT_REMIX;
    a.flacRate = 44100, a.flacSizes = sizes, a.rates = rates; // (flacRate: not used, every track's file carries its own)
    a.n_tracks = n_tracks, a.audio = audio, a.n = n, a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.out = out, a.peaks = peaks, a.layout = layout, a.progress = progress, a.user = user;
    return tracks_call(a);
}

// dmx_tracks_infer_rates / dmx_tracks_infer_from_flac_rates behind the loudness stage
static int tracks_infer_loud(const char *fn, dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                             const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                             const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes, float *peaks,
                             int layout, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud, dmx_loudness_result *report,
                             dmx_meters_result *meters, const dmx_limiter_spec *lim = nullptr, dmx_limit_result *limit = nullptr)
{
    if (n_tracks < 1)
        return fail(DMX_ERR_ARG, "%s: n_tracks must be >= 1, got %d", fn, n_tracks);
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: the loudness stage needs a remix spec", fn);
    DMXCHK(dmx_limit_check_spec(fn, loud, lim, 44100, -1));
    for (int t = 0; rates && t < n_tracks; ++t) // the loudness stage's own floor on a rate, with the track's number
        DMXCHK(dmx_limit_check_spec(fn, loud, lim, rates[t], t));
    if (rates)
        DMXCHK(check_tracks_rates(fn, n_tracks, n, rates, flac_out != 0));
    TracksCall a = remix_call(fn, c, models, n_models, weights, spec);
    a.kind = flac_out ? TRACKS_OUT_FLAC : TRACKS_OUT_REMIX;
    a.flacRate = 44100, a.flacSizes = sizes, a.rates = rates;
    a.n_tracks = n_tracks, a.audio = audio, a.n = n, a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.out = out, a.peaks = peaks, a.layout = layout, a.progress = progress, a.user = user;
    a.loud = loud, a.report = report, a.meters = meters, a.lim = lim, a.limit = limit;
    return tracks_call(a);
}

extern "C" int dmx_tracks_infer_loud(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                     const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                                     const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                     float *peaks, int layout, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud,
                                     dmx_loudness_result *report)
{
    return tracks_infer_loud("dmx_tracks_infer_loud", c, models, n_models, weights, n_tracks, audio, n, rates, n_shifts, overlap, shift_offsets,
                             spec, flac_out, out, sizes, peaks, layout, progress, user, loud, report, nullptr);
}

// the two calls behind the loudness stage with a meters report
extern "C" int dmx_tracks_infer_meters(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                       const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                                       const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                       float *peaks, int layout, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud,
                                       dmx_loudness_result *report, dmx_meters_result *meters)
{
    return tracks_infer_loud("dmx_tracks_infer_meters", c, models, n_models, weights, n_tracks, audio, n, rates, n_shifts, overlap,
                             shift_offsets, spec, flac_out, out, sizes, peaks, layout, progress, user, loud, report, meters);
}

extern "C" int dmx_tracks_infer_from_flac_meters(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                                 const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                                 const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out,
                                                 int64_t *sizes, float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user,
                                                 const dmx_loudness_spec *loud, dmx_loudness_result *report, dmx_meters_result *meters)
{
    const char *fn = "dmx_tracks_infer_from_flac_meters";
    DMXCHK(dmx_limit_check_spec(fn, loud, nullptr, 44100, -1));
    return tracks_from_flac(fn, true, c, models, n_models, weights, n_tracks, files, file_bytes, n_shifts, overlap, shift_offsets, spec,
                            flac_out, out, sizes, peaks, track_status, progress, user, loud, report, meters);
}

extern "C" int dmx_tracks_infer_from_flac_loud(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                               const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                               const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out,
                                               int64_t *sizes, float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user,
                                               const dmx_loudness_spec *loud, dmx_loudness_result *report)
{
    const char *fn = "dmx_tracks_infer_from_flac_loud";
    DMXCHK(dmx_limit_check_spec(fn, loud, nullptr, 44100, -1));
    return tracks_from_flac(fn, true, c, models, n_models, weights, n_tracks, files, file_bytes, n_shifts, overlap, shift_offsets, spec,
                            flac_out, out, sizes, peaks, track_status, progress, user, loud, report);
}

// the two calls above with the limiter: its times and its report
extern "C" int dmx_tracks_infer_limit(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                      const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                                      const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                      float *peaks, int layout, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud,
                                      dmx_loudness_result *report, dmx_meters_result *meters, const dmx_limiter_spec *lim,
                                      dmx_limit_result *limit)
{
    return tracks_infer_loud("dmx_tracks_infer_limit", c, models, n_models, weights, n_tracks, audio, n, rates, n_shifts, overlap,
                             shift_offsets, spec, flac_out, out, sizes, peaks, layout, progress, user, loud, report, meters, lim, limit);
}

extern "C" int dmx_tracks_infer_from_flac_limit(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                                const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                                const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out,
                                                int64_t *sizes, float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user,
                                                const dmx_loudness_spec *loud, dmx_loudness_result *report, dmx_meters_result *meters,
                                                const dmx_limiter_spec *lim, dmx_limit_result *limit)
{
    const char *fn = "dmx_tracks_infer_from_flac_limit";
    DMXCHK(dmx_limit_check_spec(fn, loud, lim, 44100, -1));
    return tracks_from_flac(fn, true, c, models, n_models, weights, n_tracks, files, file_bytes, n_shifts, overlap, shift_offsets, spec,
                            flac_out, out, sizes, peaks, track_status, progress, user, loud, report, meters, lim, limit);
}
