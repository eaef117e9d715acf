// api.cpp — C ABI (include/demucs_hip.h): the error state, models and contexts of the MI355X HTDemucs path.
//
// Host-side restatement of the reference's entry points (citations in demucs_hip.h):
//   load_demucs_model  -> dmx_model_load        (src/model_load.cpp:50)
//   model_inference    -> dmx_segment_infer*    (src/model_inference.cpp:48; exec.cpp)
//   demucs_inference   -> dmx_track_infer       (src/model_apply.cpp:60-288; tracks_exec.cpp)
// The codecs' own entry points are in codec_api.cpp, dmx_debug_* in debug_api.cpp.
// No CPU fallback exists: without a usable HIP device every compute entry point fails.
#include "api_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

using namespace dmx;

static thread_local std::string g_err;
int dmx_fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
const std::string &dmx_err_string() { return g_err; }
void dmx_set_err_string(const std::string &s) { g_err = s; }

extern "C" const char *dmx_last_error(void) { return g_err.c_str(); }

extern "C" int dmx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

extern "C" int dmx_model_load(const char *model_file, int device, dmx_model **out)
{
    if (!model_file || !out)
        return fail(DMX_ERR_ARG, "dmx_model_load: null argument");
    *out = nullptr;
    auto m = std::make_unique<dmx_model>();
    std::string err;
    if (!load_and_pack(model_file, m->pm, err))
    {
        bool io = err.find("failed to open") != std::string::npos || err.find("truncated") != std::string::npos;
        fprintf(stderr, "%s\n", err.c_str()); // the reference loader also reports on stderr
        return fail(io ? DMX_ERR_IO : DMX_ERR_FORMAT, "%s", err.c_str());
    }
    int ndev = dmx_device_count();
    if (ndev <= 0)
        return fail(DMX_ERR_NO_DEVICE, "dmx_model_load: no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev)
        return fail(DMX_ERR_ARG, "dmx_model_load: device %d out of range (have %d)", device, ndev);
    m->device = device;
    m->blobFloats = m->pm.blob.size();
    DMXCHK(dmx_model_upload(m.get(), m->pm.blob.data()));
    *out = m.release();
    return DMX_OK;
}

// ---- GEMM arithmetic of a context (include/demucs_hip.h DMX_GEMM_*). The process default comes from the environment
// (DMX_GEMM=f32|bf16x3) the first time it is needed and can be changed with dmx_set_default_gemm; a context keeps the
// mode it was created with.
static std::atomic<int> g_defaultGemm{-1};
extern "C" int dmx_default_gemm(void)
{
    int g = g_defaultGemm.load();
    if (g < 0)
    {
        // default since round 4: the exact operand-split path (every -m gpu parity test runs in both modes; DESIGN.md
        // section 2.5); DMX_GEMM=f32 selects the fp32 MFMA kernels
        const char *e = getenv("DMX_GEMM");
        g = e && !strcmp(e, "f32") ? DMX_GEMM_F32 : e && !strcmp(e, "fp16x3") ? DMX_GEMM_FP16X3 : DMX_GEMM_BF16X3;
        if (e && *e && strcmp(e, "f32") && strcmp(e, "bf16x3") && strcmp(e, "fp16x3")) // a typo must not silently select the other arithmetic
            fprintf(stderr, "demucs_hip: DMX_GEMM=%s is not one of {f32, bf16x3, fp16x3}; using bf16x3 (the default)\n", e);
        g_defaultGemm.store(g);
    }
    return g;
}
extern "C" int dmx_set_default_gemm(int gemm)
{
    if (gemm != DMX_GEMM_F32 && gemm != DMX_GEMM_BF16X3 && gemm != DMX_GEMM_FP16X3)
        return fail(DMX_ERR_ARG, "dmx_set_default_gemm: unknown mode %d", gemm);
    g_defaultGemm.store(gemm);
    return DMX_OK;
}

// a failed upload leaves nothing on the device (the caller drops the half-built model without calling dmx_model_free)
static int upload_failed(dmx_model *m, hipError_t e)
{
    for (void *p : {(void *)m->dW, (void *)m->dWb, (void *)m->dWh})
        if (p)
            (void)hipFree(p);
    m->dW = nullptr, m->dWb = nullptr, m->dWh = nullptr;
    return fail(DMX_ERR_HIP, "dmx_model_load: weight upload failed: %s", hipGetErrorString(e));
}

int dmx_model_upload(dmx_model *m, const float *blob)
{
    HIPCHK(hipSetDevice(m->device));
    // + 1 KB: the igemm staging prefetches two K-tiles (2 x 128 B per row) beyond the last one (never used, must be readable)
    HIPCHK(hipMalloc((void **)&m->dW, m->blobFloats * sizeof(float) + 1024));
    // the tail must read as finite numbers (it meets zero activations: 0 x NaN would poison an accumulator)
    hipError_t e = hipMemset(reinterpret_cast<char *>(m->dW) + m->blobFloats * sizeof(float), 0, 1024);
    if (e == hipSuccess)
        e = hipMemcpy(m->dW, blob, m->blobFloats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return upload_failed(m, e);
    {
        // igemm_split.hip: every blob element as two bf16 terms by round-to-nearest splits, w1 = bf16(w), w2 = bf16(w - w1).
        // Exact for fp16-representable values (11 significand bits <= 8 + 8, fp16 subnormals included: bf16 has the fp32
        // exponent range); whether an op's weights ARE exact is checked per op when the plan is built (gemm_select.h).
        std::vector<unsigned short> planes(2 * m->blobFloats + 1024, 0);
        m->inexactW.clear();
        for (size_t i = 0; i < m->blobFloats; ++i)
            if (!dmx_split_weight(blob[i], planes[i], planes[m->blobFloats + 512 + i]))
                m->inexactW.push_back((i64)i);
        e = hipMalloc((void **)&m->dWb, planes.size() * sizeof(unsigned short));
        if (e == hipSuccess)
            e = hipMemcpy(m->dWb, planes.data(), planes.size() * sizeof(unsigned short), hipMemcpyHostToDevice);
        if (e != hipSuccess)
            return upload_failed(m, e);
    }
    // DMX_GEMM_FP16X3 (opt-in): every blob element as ONE fp16 number (round to nearest). Exact for everything that comes
    // straight from the fp16 weight file; the rest is listed here, and an op that touches a listed element keeps bf16 terms
    // (gemm_select.h). The plane itself is only built when a context of that mode binds the model (dmx_model_fp16_plane).
    m->inexactH.clear();
    for (size_t i = 0; i < m->blobFloats; ++i)
        if (!((float)(_Float16)blob[i] == blob[i]))
            m->inexactH.push_back((i64)i);
    return DMX_OK;
}

int dmx_model_fp16_plane(const dmx_model *m)
{
    std::lock_guard<std::mutex> lock(m->hMutex);
    if (m->dWh)
        return DMX_OK;
    HIPCHK(hipSetDevice(m->device));
    unsigned short *pl = nullptr;
    const size_t n = m->blobFloats + 1024; // (the same readable, finite tail as the other planes)
    HIPCHK(hipMalloc((void **)&pl, n * sizeof(unsigned short)));
    hipError_t e = hipMemset(pl, 0, n * sizeof(unsigned short));
    if (e == hipSuccess)
    {
        launch_f32_to_f16(m->dW, pl, (i64)m->blobFloats, nullptr); // round to nearest even: the conversion inexactH was listed with
        e = hipDeviceSynchronize();
    }
    if (e != hipSuccess)
    {
        (void)hipFree(pl);
        return fail(DMX_ERR_HIP, "fp16 weight plane: %s", hipGetErrorString(e));
    }
    m->dWh = pl;
    return DMX_OK;
}

// Replicates a loaded model onto another device (the weights are packed once per file, not once per GPU).
extern "C" int dmx_model_clone(const dmx_model *src, int device, dmx_model **out)
{
    if (!src || !out)
        return fail(DMX_ERR_ARG, "dmx_model_clone: null argument");
    *out = nullptr;
    if (src->pm.blob.size() != src->blobFloats)
        return fail(DMX_ERR_ARG, "dmx_model_clone: the source model no longer holds its packed weights on the host");
    const int ndev = dmx_device_count();
    if (device < 0 || device >= ndev)
        return fail(DMX_ERR_ARG, "dmx_model_clone: device %d out of range (have %d)", device, ndev);
    auto m = std::make_unique<dmx_model>();
    m->pm.arch = src->pm.arch, m->pm.n_sources = src->pm.n_sources, m->pm.dim = src->pm.dim, m->pm.n_tensors = src->pm.n_tensors;
    m->pm.index = src->pm.index; // offsets only: the plan never reads the host blob
    m->blobFloats = src->blobFloats;
    m->device = device;
    DMXCHK(dmx_model_upload(m.get(), src->pm.blob.data()));
    *out = m.release();
    return DMX_OK;
}

extern "C" void dmx_model_free(dmx_model *m)
{
    if (!m)
        return;
    if (m->dW)
    {
        (void)hipSetDevice(m->device);
        (void)hipFree(m->dW);
        if (m->dWb)
            (void)hipFree(m->dWb);
        if (m->dWh)
            (void)hipFree(m->dWh);
    }
    delete m;
}
extern "C" int dmx_model_n_sources(const dmx_model *m) { return m ? m->pm.n_sources : 0; }
extern "C" int dmx_model_n_tensors(const dmx_model *m) { return m ? m->pm.n_tensors : 0; }
extern "C" int dmx_model_device(const dmx_model *m) { return m ? m->device : -1; }
extern "C" int dmx_model_arch(const dmx_model *m) { return m ? m->pm.arch : 0; }

static int ctx_init(dmx_ctx *c, const dmx_model *m, int64_t segment_samples, int max_batch, int gemm)
{
    c->m = m;
    c->gemm = gemm;
    c->seg = segment_samples;
    c->maxBatch = max_batch;
    HIPCHK(hipSetDevice(m->device));
    if (gemm == DMX_GEMM_FP16X3)
        DMXCHK(dmx_model_fp16_plane(m));
    Plan *p = dmx_get_plan(c, max_batch);
    std::string why;
    if (!dmx_validate_plan(*p, why))
        return fail(DMX_ERR_ARG, "dmx_ctx_create: unsupported geometry (%s)", why.c_str());
    c->arenaFloats = p->arenaFloats;
    if (gemm != DMX_GEMM_F32 && m->pm.arch != 3)
    {
        // dmx_ctx_set_model may bind a model whose K / V projections take the operand-plane form when this one's do not (the
        // decision follows the model's weights, dmx_get_plan): the arena is sized for the larger layout, planes on
        Plan q;
        build_plan(m->pm, c->seg, max_batch, q, plan_opts_from_env(gemm, true));
        c->arenaFloats = std::max(c->arenaFloats, q.arenaFloats);
    }
    // + 1 KB of slack behind the last activation for the same prefetch
    HIPCHK(hipMalloc((void **)&c->dA, (size_t)c->arenaFloats * sizeof(float) + 1024));
    HIPCHK(hipMemset(c->dA, 0, (size_t)c->arenaFloats * sizeof(float) + 1024));
    HIPCHK(hipMemcpy(c->dA, p->constants.data(), p->constants.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking));
    c->stream = c->ownStream;
    HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming));
    {
        const char *e = getenv("DMX_STREAMS");
        c->streamMode = e ? atoi(e) : 0;
        const char *g = getenv("DMX_GRAPH");
        c->graphMode = g ? atoi(g) : 1;
        const char *f = getenv("DMX_FUSE_ISTFT");
        c->fuseIstft = f ? atoi(f) : 1;
    }
    HIPCHK(hipMalloc((void **)&c->dPartials, sizeof(double) * 2 * dmx_ctx::kStatBlocks * TrackStatsTable::kMax));
    HIPCHK(hipMalloc((void **)&c->dStats, sizeof(float) * 4));
    if (gemm == DMX_GEMM_FP16X3)
    {
        // per-row scales of the linear layer in flight (launch_rowscale): two floats per A row, one buffer per stream of the plan
        i64 maxM = 0;
        for (const Op &op : p->ops)
            if (op.kind == OP_IGEMM && op.g.hterms) // (every op the plan marks, whatever THIS model's weights allow: dmx_ctx_set_model)
                maxM = std::max(maxM, (i64)op.g.B * op.g.P1 * op.g.P0);
        if (maxM > 0)
            for (int k = 0; k < 2; ++k)
                HIPCHK(hipMalloc((void **)&c->dRowScale[k], sizeof(float) * 2 * (size_t)maxM));
    }
    HIPCHK(hipMalloc((void **)&c->dStatus, sizeof(unsigned)));
    HIPCHK(hipMemset(c->dStatus, 0, sizeof(unsigned)));
    HIPCHK(hipHostMalloc((void **)&c->hStatus, sizeof(unsigned), hipHostMallocDefault));
    *c->hStatus = 0;
    return DMX_OK;
}

extern "C" int dmx_ctx_create(const dmx_model *m, int64_t segment_samples, int max_batch, dmx_ctx **out)
{
    return dmx_ctx_create_gemm(m, segment_samples, max_batch, dmx_default_gemm(), out);
}

extern "C" int dmx_ctx_gemm(const dmx_ctx *c) { return c ? c->gemm : -1; }

extern "C" int dmx_ctx_create_gemm(const dmx_model *m, int64_t segment_samples, int max_batch, int gemm, dmx_ctx **out)
{
    if (!m || !out || max_batch < 1 || max_batch > 64 || (gemm != DMX_GEMM_F32 && gemm != DMX_GEMM_BF16X3 && gemm != DMX_GEMM_FP16X3))
        return fail(DMX_ERR_ARG, "dmx_ctx_create: invalid argument");
    *out = nullptr;
    if (segment_samples == 0)
        segment_samples = DMX_SEGMENT_SAMPLES;
    if (segment_samples < 4096 || segment_samples % 2 != 0)
        return fail(DMX_ERR_ARG, "dmx_ctx_create: segment_samples must be even and >= 4096");
    auto c = std::make_unique<dmx_ctx>(); // ~dmx_ctx releases whatever an early return leaves behind
    DMXCHK(ctx_init(c.get(), m, segment_samples, max_batch, gemm));
    *out = c.release();
    return DMX_OK;
}

dmx_ctx::~dmx_ctx()
{
    if (!m)
        return;
    (void)hipSetDevice(m->device);
    if (stream)
        (void)hipStreamSynchronize(stream);
    {
        std::lock_guard<std::mutex> graphLock(g_graphMutex);
        for (auto &kv : graphs)
            (void)hipGraphExecDestroy(kv.second);
    }
    for (hipStream_t s : {ownStream, stream2, copyStream, uploadStream})
        if (s)
        {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    for (hipEvent_t e : events)
        if (e)
            (void)hipEventDestroy(e);
    for (hipEvent_t e : batchEvents)
        if (e)
            (void)hipEventDestroy(e);
    if (evFork)
        (void)hipEventDestroy(evFork);
    if (evJoin)
        (void)hipEventDestroy(evJoin);
    if (evUpload)
        (void)hipEventDestroy(evUpload);
    for (TrackSlot &sl : slots)
    {
        if (sl.copied)
            (void)hipEventDestroy(sl.copied);
        for (DevBuf *b : {&sl.audio, &sl.tmp, &sl.out, &sl.stats, &sl.pcm, &sl.peaks, &sl.flac, &sl.flacWork, &sl.flacSizes, &sl.flacIn, &sl.flacInWork, &sl.flacInStatus, &sl.native, &sl.nativeOut, &sl.loud})
            if (b->p)
                (void)hipFree(b->p);
    }
    for (void *p : {(void *)dA, (void *)dPartials, (void *)dStats, (void *)dStatus, (void *)dRowScale[0], (void *)dRowScale[1], (void *)dLoudTable, (void *)bAudio.p, (void *)bTmp.p, (void *)bMix.p,
                    (void *)bSegOut.p, (void *)bOut.p})
        if (p)
            (void)hipFree(p);
    if (hStatus)
        (void)hipHostFree(hStatus);
}

extern "C" void dmx_ctx_free(dmx_ctx *c) { delete c; }

// Rebinds the context to another model of the SAME architecture on the same device (identical packed
// layout => identical plan): the fine-tuned bag runs its four models through one arena.
extern "C" int dmx_ctx_set_model(dmx_ctx *c, const dmx_model *m)
{
    if (!c || !m)
        return fail(DMX_ERR_ARG, "dmx_ctx_set_model: null argument");
    if (m == c->m)
        return DMX_OK;
    if (m->device != c->m->device || m->pm.arch != c->m->pm.arch || m->pm.n_sources != c->m->pm.n_sources || m->pm.dim != c->m->pm.dim ||
        m->blobFloats != c->m->blobFloats || m->pm.index != c->m->pm.index)
        return fail(DMX_ERR_ARG, "dmx_ctx_set_model: the model differs in architecture or device from the context's");
    if (c->gemm == DMX_GEMM_FP16X3)
    {
        HIPCHK(hipSetDevice(m->device));
        DMXCHK(dmx_model_fp16_plane(m));
    }
    bool sameDecisions = true; // (the lists differ between the models of a bag - derived tensors - without changing any decision)
    const GemmModelFacts facts = dmx_model_facts(m);
    if (m->inexactW != c->m->inexactW || m->inexactH != c->m->inexactH)
        for (const auto &kv : c->plans)
            for (const Op &op : kv.second->ops)
                if (op.kind == OP_IGEMM && select_gemm(op.g, c->gemm, facts, split_lin_mode()) != op.g.choice)
                    sameDecisions = false;
    if (!sameDecisions)
    {
        // the cached plans (and captured graphs) decided per op between the exact-split and the fp32 kernel from the OLD
        // model's list of weights that are not two-plane representable: decide again for this model
        std::lock_guard<std::mutex> graphLock(g_graphMutex);
        for (auto &kv : c->graphs)
            (void)hipGraphExecDestroy(kv.second);
        c->graphs.clear();
        c->haveLastKey = false;
        c->plans.clear();
    }
    c->m = m; // kernels of earlier calls hold the old weight pointer by value: no synchronisation needed
    return DMX_OK;
}

int dmx_ensure_buf(DevBuf &b, i64 floats)
{
    if (b.cap >= floats)
        return DMX_OK;
    if (b.p)
        HIPCHK(hipFree(b.p)); // hipFree synchronises the device: nothing still reads the old buffer
    b.p = nullptr, b.cap = 0;
    HIPCHK(hipMalloc((void **)&b.p, sizeof(float) * (size_t)floats));
    b.cap = floats;
    return DMX_OK;
}

hipEvent_t dmx_batch_event(dmx_ctx *c, size_t i)
{
    if (c->batchEvents.size() <= i)
        c->batchEvents.resize(i + 1, nullptr);
    if (!c->batchEvents[i] && hipEventCreateWithFlags(&c->batchEvents[i], hipEventDisableTiming) != hipSuccess)
        return nullptr;
    return c->batchEvents[i];
}

extern "C" int64_t dmx_ctx_segment_samples(const dmx_ctx *c) { return c ? c->seg : 0; }
extern "C" int dmx_ctx_max_batch(const dmx_ctx *c) { return c ? c->maxBatch : 0; }
extern "C" int64_t dmx_ctx_arena_bytes(const dmx_ctx *c) { return c ? c->arenaFloats * 4 : 0; }
int dmx_ctx_sync_checked(dmx_ctx *c)
{
    // the cooperative LSTM kernel (Demucs v3) bounds its spins and raises the status word instead of hanging (v3.hip):
    // its copy rides on the stream behind the work it reports on, into pinned memory - no second round trip, no
    // legacy-stream synchronisation with other contexts' streams
    const bool check = c->m->pm.arch == 3;
    if (check)
        HIPCHK(hipMemcpyAsync(c->hStatus, c->dStatus, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (check && *c->hStatus != 0)
    {
        *c->hStatus = 0;
        HIPCHK(hipMemsetAsync(c->dStatus, 0, sizeof(unsigned), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return fail(DMX_ERR_HIP, "a cooperative kernel timed out waiting for its partner workgroups (results invalid)");
    }
    return DMX_OK;
}

extern "C" int dmx_ctx_synchronize(dmx_ctx *c)
{
    if (!c)
        return fail(DMX_ERR_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->m->device));
    return dmx_ctx_sync_checked(c);
}

extern "C" int dmx_ctx_set_stream(dmx_ctx *c, void *hip_stream)
{
    if (!c)
        return fail(DMX_ERR_ARG, "dmx_ctx_set_stream: null context");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->stream2));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->ownStream;
    return DMX_OK;
}
