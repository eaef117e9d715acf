// api_internal.h — host-side state shared by the units of the single-context C ABI (api.cpp: models and contexts; exec.cpp:
// the plan executor; tracks_exec.cpp: the track path; codec_api.cpp: the codecs; debug_api.cpp) and engine.cpp
// (multi-device / multi-model scheduler). Nothing here crosses the C ABI.
#pragma once
#include "../../include/demucs_hip.h"
#include "kernels.h"
#include "loud_chain.h"

#include <cstring>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

int dmx_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const std::string &dmx_err_string();         // last error of the calling thread
void dmx_set_err_string(const std::string &); // adopt an error produced on another thread
#define fail dmx_fail

#define HIPCHK(expr)                                                                                              \
    do                                                                                                            \
    {                                                                                                             \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return dmx_fail(DMX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define DMXCHK(expr)        \
    do                      \
    {                       \
        int rc_ = (expr);   \
        if (rc_ != DMX_OK)  \
            return rc_;     \
    } while (0)

struct dmx_model
{
    dmx::PackedModel pm;    // index / dimensions stay; the packed weights (pm.blob) are kept on the host so that the model
                            // can be replicated onto further devices (dmx_model_clone) without re-reading the file
    size_t blobFloats = 0;  // size of the packed weights (also when pm.blob has been released)
    float *dW = nullptr;
    unsigned short *dWb = nullptr; // two bf16 planes of the blob (GEMM_BF16X3 contexts): w = w1 + w2 by round-to-nearest splits,
                                   // plane 2 starts at element blobFloats + 512
    std::vector<dmx::i64> inexactW; // blob elements that are NOT the exact sum of their two planes (derived tensors), ascending;
                                    // filled at upload, so replicas on other devices (dmx_model_clone) agree with the original
    // one fp16 plane of the blob (GEMM_FP16X3 contexts: the linear layers' weights as ONE exact term). The mode is opt-in: the
    // plane is built on the device from dW when the first such context binds the model (dmx_model_fp16_plane), not at upload
    mutable unsigned short *dWh = nullptr;
    mutable std::mutex hMutex;
    std::vector<dmx::i64> inexactH; // blob elements that are not fp16 numbers, ascending (same role as inexactW; listed at upload)
    int device = 0;
};
// makes m->dWh exist (idempotent, thread-safe); DMX_OK or an error
int dmx_model_fp16_plane(const dmx_model *m);
// uploads `blob` (blobFloats floats) as the weights of `m` on m->device
int dmx_model_upload(dmx_model *m, const float *blob);

// grow-only device buffer owned by a context (track-level scratch: allocated on first use, reused by
// every later call, freed with the context — no hipMalloc/hipFree on the per-track path)
struct DevBuf
{
    float *p = nullptr;
    dmx::i64 cap = 0; // floats
};

struct dmx_ctx
{
    const dmx_model *m = nullptr;
    dmx::i64 seg = 0;
    int maxBatch = 1;
    std::map<int, std::unique_ptr<dmx::Plan>> plans;
    float *dA = nullptr;
    dmx::i64 arenaFloats = 0;
    hipStream_t stream = nullptr;    // main / freq branch; every API call is ordered on this stream
    hipStream_t ownStream = nullptr; // the stream created with the context (`stream` may be a caller's)
    hipStream_t stream2 = nullptr;   // time branch (forked from and joined back into `stream` inside run_plan)
    hipStream_t copyStream = nullptr; // D2H of finished parts of a track behind the kernels of later segments
    int streamMode = 0;              // 0 auto (two streams for batches < kTwoStreamMaxBatch), 1 one stream, 2 always two (env DMX_STREAMS)
    static const int kTwoStreamMaxBatch = 8;
    std::vector<hipEvent_t> events; // one per op index (created on first use), + fork / join
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    int lastBatch = 0;
    // caller buffers the plan reads its input from / writes its output to directly (device entry point):
    // the arena regions [mixOff, +mixLen) and [outOff, +outLen) are redirected while they are set
    const float *extMix = nullptr;
    float *extOut = nullptr;
    dmx::i64 redirMixOff = 0, redirMixLen = 0, redirOutOff = 0, redirOutLen = 0;
    // track-level scratch
    double *dPartials = nullptr;
    static const int kStatBlocks = 256;
    DevBuf bAudio, bTmp, bMix, bSegOut, bOut; // bSegOut: the ring of segment outputs of dmx_track(s)_infer
    // dmx_track(s)_infer: one slot per track in flight (its upload, statistics and result), reused once the track's last
    // copy-out has completed; uploads run on their own stream so that a pageable source never waits for queued kernels
    struct TrackSlot
    {
        DevBuf audio, tmp, out, stats;
        DevBuf pcm, peaks; // dmx_tracks_infer_pcm: the encoded outputs (each at a 16-byte-rounded stride) and their peaks
        DevBuf flac, flacWork, flacSizes; // dmx_tracks_infer_flac: the files (stride dmx_flac_bound), the workspace, n_out int64 counts
        DevBuf flacIn, flacInWork, flacInStatus; // dmx_tracks_infer_from_flac: the file's bytes, the decoder's workspace, {status, good}
        DevBuf loud; // dmx_tracks_infer_loud: the chain's workspace with the reports inside (loud_chain.h)
        DevBuf native, nativeOut; // dmx_tracks_infer_rates, a call with a converted track: the track [m][2] and its stems at its own rate
        hipEvent_t copied = nullptr; // on copyStream behind the last copy-out of the track that holds the slot (TracksPlan)
    };
    std::vector<TrackSlot> slots;
    float *dLoudTable = nullptr; // dmx_tracks_infer_loud: the gain table (loud_gain_table), built and uploaded on the context's first such call
    int flacLevel = 0; // dmx_ctx_set_flac_level: 0 FIXED predictors alone, 1 + LPC order 8, 2 + LPC orders 8 and 12
    hipStream_t uploadStream = nullptr;
    hipEvent_t evUpload = nullptr;
    float *dStats = nullptr;            // 4 floats
    float *dRowScale[2] = {nullptr, nullptr}; // GEMM_FP16X3: per-row scales of the linear layer in flight, one buffer per stream of the plan
    unsigned *dStatus = nullptr;        // device status word: raised by a kernel whose bounded spin timed out (v3.hip LSTM)
    unsigned *hStatus = nullptr;        // pinned host copy (dmx_ctx_sync_checked)
    std::vector<hipEvent_t> batchEvents; // progress reporting without host synchronisation of the stream
    // HIP graphs of the batch-1 plan (launch-bound latency path), keyed by the redirected I/O pointers
    struct GraphKey
    {
        const float *mix;
        float *out;
        const float *dW; // device weights the captured kernels read (NOT the host dmx_model*: a freed model's address
                         // can be reused by another model with different weights)
        bool operator<(const GraphKey &o) const
        {
            if (mix != o.mix)
                return mix < o.mix;
            if (out != o.out)
                return out < o.out;
            return dW < o.dW;
        }
    };
    std::map<GraphKey, hipGraphExec_t> graphs;
    int gemm = 0;      // dmx::GemmMode of every plan of this context (DMX_GEMM_* of the C ABI), fixed at creation
    int graphMode = 1; // env DMX_GRAPH: 0 off, 1 (default) capture the two-stream plans of small batches into HIP graphs
    int fuseIstft = 1; // env DMX_FUSE_ISTFT=0: ISTFT and overlap-add as two kernels through the `frames` tensor (A/B)
    int graphBatch = 0; // batch size the cached graphs were captured for
    bool capturing = false; // enqueue_plan runs inside hipStreamBeginCapture (no cross-context event waits may be recorded)
    GraphKey lastKey{nullptr, nullptr, nullptr};
    bool haveLastKey = false;
    ~dmx_ctx();
};

// the device scratch of a host convenience wrapper: freed when the wrapper returns, whichever way it does
struct DevScratch
{
    void *held[4];
    int n = 0;
    bool ok = true; // no hipMalloc has failed; after a failure nothing more is attempted
    void *get(size_t bytes)
    {
        void *p = nullptr;
        ok = ok && n < 4 && hipMalloc(&p, bytes) == hipSuccess;
        return ok ? held[n++] = p : nullptr;
    }
    ~DevScratch()
    {
        while (n > 0)
            (void)hipFree(held[--n]);
    }
};

// bf16 <-> fp32 on the host (round to nearest even; the weight planes of the exact-split GEMM path)
static inline unsigned short dmx_bf16_rn(float f)
{
    unsigned u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) // inf / NaN: truncate, keep a NaN a NaN
        return (unsigned short)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
static inline float dmx_bf16_f32(unsigned short h)
{
    const unsigned u = (unsigned)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// w = w1 + w2 + (remainder): the two-term round-to-nearest split of the weight planes; returns true when it is exact
static inline bool dmx_split_weight(float w, unsigned short &w1, unsigned short &w2)
{
    w1 = dmx_bf16_rn(w);
    const float r = w - dmx_bf16_f32(w1); // exact (Sterbenz-like: w1 is w rounded to 8 significant bits)
    w2 = dmx_bf16_rn(r);
    return dmx_bf16_f32(w1) + dmx_bf16_f32(w2) == w;
}
// D2H of the context's status word behind the work already enqueued + stream synchronisation + test-and-clear:
// every host-side wait on a context's results goes through this (a cooperative kernel whose bounded spin timed
// out must never produce silently corrupt stems)
int dmx_ctx_sync_checked(dmx_ctx *c);

// ---- exec.cpp, used by api.cpp and debug_api.cpp
dmx::GemmModelFacts dmx_model_facts(const dmx_model *m);       // what the kernel selection reads of a model (gemm_select.h)
dmx::Plan *dmx_get_plan(dmx_ctx *c, int batch);               // the context's plan for `batch`, built and chosen on first use
int dmx_launch_op(const dmx_ctx *c, const dmx::Op &op, hipStream_t s, dmx::i64 zeroOff); // one op of a plan on stream s
namespace dmx { extern std::mutex g_graphMutex; }             // every HIP graph API call of the process holds it
// ---- tracks_exec.cpp, used by codec_api.cpp
int dmx_pcm_check_spec(const char *fn, const dmx_output_spec *spec, int S); // S < 0: the model is not known yet
int dmx_pcm_frame_bytes(int encoding);                                      // bytes of one stereo frame
int dmx_remix_check_spec(const char *fn, int S, const dmx_remix_spec *spec, dmx::PcmGains *G, bool noModel);
// ---- codec_api.cpp, used by tracks_exec.cpp (the loudness stage)
int dmx_loud_check_spec(const char *fn, const dmx_loudness_spec *spec, int rate, int track); // track < 0: no track to name
// the same validator for the entry points that take the limiter: DMX_LOUD_LIMIT, DMX_LOUD_UNITY and the times
int dmx_limit_check_spec(const char *fn, const dmx_loudness_spec *spec, const dmx_limiter_spec *lim, int rate, int track);
// the limiter's tables on `device` (kLimTableWords words): one copy per device, uploaded on first use, kept for the process
int dmx_limiter_device_tables(int device, const int32_t **T);
// The output chain of one whole track behind its remix, enqueued on s: the measurements of the outputs
// and of the mixture, the true peaks and the meters the layout L has, and the gain launch or, with DMX_LOUD_LIMIT, the gain
// without a ceiling and the limiter, whose peaks replace pp.peaks. pp: the whole track, peaks the n_out sample peaks (behind
// the peak kernel unless limited); work: L.total bytes laid out by loud_chain_layout; report and meters (NULL: none) are n_out
// + 1 entries on the device, in the workspace or the caller's. The caller encodes *piece: launch_limit_encode when limited,
// else launch_loud_encode or, ungained, launch_remix_encode (gplaneStride 0 when the envelopes are linked).
struct LoudChainJob
{
    dmx::RemixPiece pp;
    const dmx::PcmGains *G;
    const dmx::LoudPlan *lp;
    int rate;
    const dmx_loudness_spec *loud; // checked
    const dmx_limiter_spec *lim;   // NULL: the default times
    const float *loudTable;
    const int32_t *limTables;      // read only with DMX_LOUD_LIMIT
    unsigned char *work;
    dmx::LoudChain L;
    void *report, *meters;
};
int dmx_loud_chain_enqueue(const LoudChainJob &job, hipStream_t s, dmx::LimitPiece *piece);

// ---- internal entry points used by engine.cpp
int dmx_ensure_buf(DevBuf &b, dmx::i64 floats);
// OLA of a plane range: planes [planeBase, planeBase + nPlanes) of the (S, 2, n) result
int dmx_track_overlap_add_planes(dmx_ctx *c, const float *d_seg_out, int n_segments, int64_t n, int shift_offset,
                                 const float *d_stats, float *d_out, int layout, int planeBase, int nPlanes);
hipEvent_t dmx_batch_event(dmx_ctx *c, size_t i);
