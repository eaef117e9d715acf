// api.cpp — C ABI (include/demucs_hip.h) + plan executor for the MI355X HTDemucs path.
//
// Host-side restatement of the reference's entry points (citations in demucs_hip.h):
//   load_demucs_model  -> dmx_model_load        (src/model_load.cpp:50)
//   model_inference    -> dmx_segment_infer*    (src/model_inference.cpp:48)
//   demucs_inference   -> dmx_track_infer       (src/model_apply.cpp:60-288)
// No CPU fallback exists: without a usable HIP device every compute entry point fails.
#include "api_internal.h"
#include "tracks_plan.h"
#include "plan_describe.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <cctype>
#include <cerrno>
#include <climits>
#include <fcntl.h>
#include <pthread.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

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
#define fail dmx_fail

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
// pure host function (tests): the two-term weight split of the exact-split GEMM path; returns the number of inexact elements
extern "C" int64_t dmx_debug_split_weights(const float *w, int64_t n, unsigned short *w1, unsigned short *w2)
{
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i)
        bad += dmx_split_weight(w[i], w1[i], w2[i]) ? 0 : 1;
    return bad;
}

extern "C" int dmx_debug_split_activations(int device, const float *x, int64_t n, unsigned short *planes)
{
    if (!x || !planes || n < 1)
        return fail(DMX_ERR_ARG, "dmx_debug_split_activations: invalid argument");
    if (device < 0 || device >= dmx_device_count())
        return fail(DMX_ERR_NO_DEVICE, "dmx_debug_split_activations: no such HIP device (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    float *dx = nullptr;
    unsigned short *dp = nullptr;
    HIPCHK(hipMalloc((void **)&dx, sizeof(float) * (size_t)n));
    hipError_t e = hipMalloc((void **)&dp, sizeof(unsigned short) * 3 * (size_t)n);
    if (e == hipSuccess)
        e = hipMemcpy(dx, x, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        launch_split3_debug(dx, n, dp, nullptr);
        e = hipMemcpy(planes, dp, sizeof(unsigned short) * 3 * (size_t)n, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dx);
    if (dp)
        (void)hipFree(dp);
    if (e != hipSuccess)
        return fail(DMX_ERR_HIP, "dmx_debug_split_activations: %s", hipGetErrorString(e));
    return DMX_OK;
}

extern "C" int dmx_debug_split_activations_fp16(int device, const float *x, int64_t n, int scale_exp, unsigned short *planes)
{
    if (!x || !planes || n < 1 || scale_exp < -126 || scale_exp > 126)
        return fail(DMX_ERR_ARG, "dmx_debug_split_activations_fp16: invalid argument");
    if (device < 0 || device >= dmx_device_count())
        return fail(DMX_ERR_NO_DEVICE, "dmx_debug_split_activations_fp16: no such HIP device (this library has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    float *dx = nullptr;
    unsigned short *dp = nullptr;
    HIPCHK(hipMalloc((void **)&dx, sizeof(float) * (size_t)n));
    hipError_t e = hipMalloc((void **)&dp, sizeof(unsigned short) * 3 * (size_t)n);
    if (e == hipSuccess)
        e = hipMemcpy(dx, x, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        launch_split3h_debug(dx, n, scale_exp, dp, nullptr);
        e = hipMemcpy(planes, dp, sizeof(unsigned short) * 3 * (size_t)n, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dx);
    if (dp)
        (void)hipFree(dp);
    if (e != hipSuccess)
        return fail(DMX_ERR_HIP, "dmx_debug_split_activations_fp16: %s", hipGetErrorString(e));
    return DMX_OK;
}

// the geometry of an op as the kernels see it (no pointers): launch_op adds the pointers; the launchers' existence queries
// (validate_plan) read only this
static void fill_gemm_geometry(GemmArgs &k, const IGemm &g)
{
    k.xBS = g.xBatchStride;
    k.B = g.B, k.P1 = g.P1, k.P0 = g.P0, k.L1 = g.L1, k.L0 = g.L0, k.Cin = g.Cin;
    k.S1 = g.S1, k.stride1 = g.stride1, k.dil1 = g.dil1, k.pad1 = g.pad1;
    k.seg0 = g.seg0, k.stride0 = g.stride0, k.pad0 = g.pad0, k.K = g.K, k.Kp = g.Kp;
    k.pro = g.pro, k.G0 = g.G0;
    k.N = g.N, k.Np = g.Np;
    k.epi = g.epi, k.act = g.act, k.yBS = g.yBatchStride, k.ldy = g.ldy;
    k.NB = g.NB, k.tableScale = g.tableScale;
    k.Lout = g.Lout, k.Cout = g.Cout, k.trS = g.trS, k.trOff = g.trOff;
    k.kvPlane = (i64)g.B * g.kvT * g.kvH * g.kvHs, k.kvCol0 = g.kvCol0, k.kvT = g.kvT, k.kvH = g.kvH, k.kvHs = g.kvHs;
    k.M = (i64)g.B * g.P1 * g.P0;
}

// what the kernel selection reads of a model (gemm_select.h)
static GemmModelFacts model_facts(const dmx_model *m)
{
    GemmModelFacts f;
    f.bf16Planes = m->dWb != nullptr, f.fp16Plane = m->dWh != nullptr;
    f.planeDelta = (i64)m->blobFloats + 512; // (dmx_model_upload)
    f.inexactW = &m->inexactW, f.inexactH = &m->inexactH;
    return f;
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

// alignment contract of the igemm staging loads (igemm.hip header) + kernel availability, one OP_IGEMM
static bool validate_gemm(const Op &op, std::string &why)
{
    const IGemm &g = op.g;
    const bool al = ((i64)g.L0 * g.Cin) % 4 == 0 && (g.stride0 * g.Cin) % 4 == 0 && (g.pad0 * g.Cin) % 4 == 0 &&
                    g.seg0 % 4 == 0 && g.K % 4 == 0 && g.xBatchStride % 4 == 0 && (g.S1 == 1 || g.seg0 % 16 == 0) &&
                    (g.cfg == kDirectCfg || (g.Cin % 4 == 0 && g.seg0 % g.Cin == 0 && g.S1 * (g.seg0 / g.Cin) <= 31)); // one validity bit per tap (igemm.hip)
    if (g.epi == EPI_KPL || g.epi == EPI_VT) // exist on the exact-split kernels only; build_chosen_plan keeps them only there
    {
        if (g.choice.arith == 0)
        {
            why = "op " + op.name + ": K / V plane projection without its exact-split kernel";
            return false;
        }
        return true;
    }
    // the fp32 kernel must exist for split ops too: dmx_ctx_set_model may bind a model whose weights turn them to fp32
    GemmArgs k{};
    fill_gemm_geometry(k, g);
    const bool exists = (g.cfg == kDirectCfg ? launch_dgemm(k, nullptr, true) : launch_igemm(g.cfg, k, nullptr, true)) == 0;
    if (!al || !exists)
    {
        why = "op " + op.name + (al ? ": no kernel instantiated for its (tile, prologue, epilogue)" : ": staging alignment contract violated");
        return false;
    }
    return true;
}
static bool validate_plan(const Plan &p, std::string &why)
{
    for (const Op &op : p.ops)
        if (op.kind == OP_IGEMM && !validate_gemm(op, why))
            return false;
    return true;
}

static Plan *get_plan(dmx_ctx *c, int batch)
{
    auto it = c->plans.find(batch);
    if (it != c->plans.end())
        return it->second.get();
    auto p = std::make_unique<Plan>();
    // K / V projections write the attention kernel's bf16 operand planes (plan.cpp plane_linear; DMX_KV_PLANES=0: A/B) where the
    // attention kernel that reads them exists and every such op can take its exact-split kernel (build_chosen_plan)
    const bool planesOff = getenv("DMX_KV_PLANES") && atoi(getenv("DMX_KV_PLANES")) == 0; // (read per plan: tests switch it)
    AttnArgs kv{};
    kv.hs = c->m->pm.dim / 8;
    const bool kvPlanes = c->gemm != DMX_GEMM_F32 && !planesOff && c->m->pm.arch != 3 && launch_attention_split(kv, nullptr, true) == 0;
    build_chosen_plan(c->m->pm, c->seg, batch, c->gemm, kvPlanes, model_facts(c->m), split_lin_mode(), *p);
    // DMX_ATT_PAIR (read per plan, like DMX_KV_PLANES): 0 never the paired kernel, 2 wherever it exists, unset: attention_select.h's rule
    const char *pairEnv = getenv("DMX_ATT_PAIR");
    const int pairMode = !pairEnv ? 1 : atoi(pairEnv) == 0 ? 0 : atoi(pairEnv) == 2 ? 2 : 1;
    for (Op &op : p->ops)
        if (op.kind == OP_ATTENTION)
        {
            Attention &t = op.at;
            AttnArgs k{};
            k.hs = t.hs;
            t.split = c->gemm != DMX_GEMM_F32 && launch_attention_split(k, nullptr, true) == 0 ? 1 : 0;
            if (t.split)
                t.form = att_select_form(t.Tq, t.Tk, t.H, t.B, t.hs, t.kpl >= 0 && t.vt >= 0, pairMode);
        }
    Plan *raw = p.get();
    c->plans[batch] = std::move(p);
    return raw;
}

// --------------------------------------------------------------------------- device lanes
// The cooperative LSTM kernel (v3.hip) spins on partner workgroups. Within ONE launch in-order dispatch makes that safe; a
// launch is dealt to the XCDs in blocks of 8 recurrences (8 x 12 / 24 workgroups), so the unit that must be resident
// together is 96 / 192 workgroups and three concurrent launches at H = 384 can exceed the 512 resident workgroups of the
// device (the bounded spin then raises the status word: an error, never a hang). Launches on one device therefore form a
// lane: each waits for the previous one's completion event, whatever stream or context of this process issued it. Graph
// captures (batches below 8: at most 48 spinning workgroups per launch, i.e. ten concurrently replaying contexts fit)
// stay outside, a capture cannot wait on a foreign event. Lanes are created on demand, one per visible device, and live
// until the process ends (their events are not destroyed from a static destructor: the HIP runtime may be gone by then).
// Several PROCESSES on one GPU (bench.py --backend gloo) take turns through a robust process-shared mutex in POSIX shared
// memory keyed by the GPU's PCI bus id; who is "registered on this GPU" is a table of process ids whose liveness is checked
// with kill(pid, 0), so a process that dies without running its exit handlers leaves nothing behind.
//
// (Round 4 also had a PLAN lane here that serialised whole plan runs of different contexts of a device while a bf16x3
// context existed. It contained a corruption of FFT frames whose cause round 5 found: packed fp32 VALU instructions with
// half routing miscompute next to 16-bit MFMAs of another wave - profiles/DESIGN_history_r5.md section 7.1, tools/micro/pk_f32_erratum.hip. The
// library is now built without packed fp32 arithmetic (Makefile NOPK, tests/test_isa_rules.py), and the lane is gone:
// contexts that share a GPU overlap again.)
struct SharedLane // one per GPU in POSIX shared memory, keyed by the PCI bus id
{
    static const int kSlots = 64;
    std::atomic<int> ready;
    std::atomic<int> pid[kSlots]; // processes registered on this GPU (0 = free); dead ones are reclaimed
    pthread_mutex_t mu;
};
struct LstmLane
{
    std::mutex mu;
    hipEvent_t ev = nullptr;
    bool recorded = false;
    SharedLane *shared = nullptr;
};
static std::mutex g_lanesMu;
static std::vector<std::unique_ptr<LstmLane>> g_lanes;
static std::vector<SharedLane *> g_sharedRegistered;

static bool pid_alive(int pid) { return pid > 0 && (kill((pid_t)pid, 0) == 0 || errno != ESRCH); }

// other live processes registered on the lane's GPU (dead entries are cleared on the way)
static int shared_lane_peers(SharedLane *sl)
{
    const int self = (int)getpid();
    int n = 0;
    for (int i = 0; i < SharedLane::kSlots; ++i)
    {
        int p = sl->pid[i].load(std::memory_order_acquire);
        if (p == 0 || p == self)
            continue;
        if (pid_alive(p))
            ++n;
        else
            sl->pid[i].compare_exchange_strong(p, 0);
    }
    return n;
}

static SharedLane *open_shared_lane(int device)
{
    if (const char *e = getenv("DMX_LSTM_SHARED_LANE"))
        if (atoi(e) == 0)
            return nullptr;
    auto give_up = [](const char *what) -> SharedLane * {
        // not fatal (one process per GPU never needs it), but not silent either: concurrent v3 PROCESSES on this GPU would
        // then issue the cooperative LSTM kernel unordered (a starved launch raises the status word, it cannot hang)
        fprintf(stderr, "demucs_hip: the process-shared LSTM lane is unavailable (%s: %s); several Demucs v3 processes on one GPU are not ordered\n", what,
                strerror(errno));
        return nullptr;
    };
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess)
        return nullptr;
    std::string name = "/dmx_lane2_"; // (layout 2: pid table; round 4's counters lived in /dmx_lstm_lane_*)
    for (const char *q = bus; *q; ++q)
        name += (isalnum((unsigned char)*q) ? *q : '_');
    bool creator = true;
    int fd = shm_open(name.c_str(), O_RDWR | O_CREAT | O_EXCL, 0666);
    if (fd < 0)
    {
        creator = false;
        fd = shm_open(name.c_str(), O_RDWR, 0666);
    }
    if (fd < 0)
        return give_up("shm_open");
    if (creator && ftruncate(fd, sizeof(SharedLane)) != 0)
    {
        close(fd);
        shm_unlink(name.c_str());
        return give_up("ftruncate");
    }
    void *mem = MAP_FAILED;
    for (int tries = 0; tries < 200 && mem == MAP_FAILED; ++tries) // a second opener may arrive before the creator's ftruncate
    {
        struct stat st;
        if (fstat(fd, &st) == 0 && (size_t)st.st_size >= sizeof(SharedLane))
            mem = mmap(nullptr, sizeof(SharedLane), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        else
            usleep(1000);
    }
    close(fd);
    if (mem == MAP_FAILED)
        return give_up("mmap");
    SharedLane *sl = static_cast<SharedLane *>(mem);
    if (creator)
    {
        pthread_mutexattr_t at;
        pthread_mutexattr_init(&at);
        pthread_mutexattr_setpshared(&at, PTHREAD_PROCESS_SHARED);
        pthread_mutexattr_setrobust(&at, PTHREAD_MUTEX_ROBUST);
        pthread_mutex_init(&sl->mu, &at);
        pthread_mutexattr_destroy(&at);
        for (int i = 0; i < SharedLane::kSlots; ++i)
            sl->pid[i].store(0);
        sl->ready.store(1, std::memory_order_release);
    }
    else
        for (int tries = 0; tries < 2000 && sl->ready.load(std::memory_order_acquire) != 1; ++tries)
            usleep(1000);
    if (sl->ready.load(std::memory_order_acquire) != 1)
    {
        errno = ETIMEDOUT;
        return give_up("creator never finished");
    }
    // register: a free slot, or one whose owner is dead
    const int self = (int)getpid();
    bool registered = false;
    for (int i = 0; i < SharedLane::kSlots && !registered; ++i)
    {
        int p = sl->pid[i].load();
        if (p == self)
            registered = true;
        else if (p == 0 || !pid_alive(p))
            registered = sl->pid[i].compare_exchange_strong(p, self);
    }
    if (!registered)
    {
        errno = ENOSPC;
        return give_up("pid table full");
    }
    g_sharedRegistered.push_back(sl);
    static bool hooked = false;
    if (!hooked)
    {
        hooked = true;
        atexit([] {
            const int me = (int)getpid();
            for (SharedLane *l : g_sharedRegistered)
                for (int i = 0; i < SharedLane::kSlots; ++i)
                {
                    int p = me;
                    l->pid[i].compare_exchange_strong(p, 0);
                }
        });
    }
    return sl;
}

static LstmLane *lstm_lane(int device)
{
    std::lock_guard<std::mutex> lk(g_lanesMu);
    if (g_lanes.empty())
    {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
            return nullptr;
        g_lanes.resize((size_t)n);
    }
    if (device < 0 || device >= (int)g_lanes.size())
        return nullptr;
    if (!g_lanes[(size_t)device])
    {
        g_lanes[(size_t)device] = std::make_unique<LstmLane>();
        g_lanes[(size_t)device]->shared = open_shared_lane(device);
    }
    return g_lanes[(size_t)device].get();
}

// holds the process-shared mutex of a lane while another live process is registered on the same GPU
struct SharedLaneGuard
{
    SharedLane *sl = nullptr;
    explicit SharedLaneGuard(SharedLane *l)
    {
        if (l && shared_lane_peers(l) > 0)
        {
            const int rc = pthread_mutex_lock(&l->mu);
            if (rc == EOWNERDEAD)
                pthread_mutex_consistent(&l->mu);
            if (rc == 0 || rc == EOWNERDEAD)
                sl = l;
        }
    }
    bool held() const { return sl != nullptr; }
    ~SharedLaneGuard()
    {
        if (sl)
            pthread_mutex_unlock(&sl->mu);
    }
};

static int ctx_init(dmx_ctx *c, const dmx_model *m, int64_t segment_samples, int max_batch, int gemm)
{
    c->m = m;
    c->gemm = gemm;
    c->seg = segment_samples;
    c->maxBatch = max_batch;
    HIPCHK(hipSetDevice(m->device));
    if (gemm == DMX_GEMM_FP16X3)
        DMXCHK(dmx_model_fp16_plane(m));
    Plan *p = get_plan(c, max_batch);
    std::string why;
    if (!validate_plan(*p, why))
        return fail(DMX_ERR_ARG, "dmx_ctx_create: unsupported geometry (%s)", why.c_str());
    c->arenaFloats = p->arenaFloats;
    if (gemm != DMX_GEMM_F32 && m->pm.arch != 3)
    {
        // dmx_ctx_set_model may bind a model whose K / V projections take the operand-plane form when this one's do not (the
        // decision follows the model's weights, get_plan): the arena is sized for the larger layout, planes on
        Plan q;
        PlanOpts o;
        o.gemm = gemm, o.kvPlanes = 1;
        build_plan(m->pm, c->seg, max_batch, q, o);
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

// hipGraphLaunch / capture / instantiate are not safe to call from several host threads at once in this runtime
// (observed: SIGSEGV in hip::Graph::UpdateStreams under hipGraphLaunch when the engine's device threads replay their
// graphs concurrently - different graphs, different streams). All graph API calls of the process go through this
// mutex; a launch only enqueues (tens of microseconds), so the device threads lose no overlap.
static std::mutex g_graphMutex;

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
        for (DevBuf *b : {&sl.audio, &sl.tmp, &sl.out, &sl.stats, &sl.pcm, &sl.peaks, &sl.flac, &sl.flacWork, &sl.flacSizes, &sl.flacIn, &sl.flacInWork, &sl.flacInStatus})
            if (b->p)
                (void)hipFree(b->p);
    }
    for (void *p : {(void *)dA, (void *)dPartials, (void *)dStats, (void *)dStatus, (void *)dRowScale[0], (void *)dRowScale[1], (void *)bAudio.p, (void *)bTmp.p, (void *)bMix.p,
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
    const GemmModelFacts facts = model_facts(m);
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

// --------------------------------------------------------------------------- executor
static int launch_op(const dmx_ctx *c, const Op &op, hipStream_t s, i64 zeroOff)
{
    float *A = c->dA;
    const float *W = c->m->dW;
    auto a = [&](i64 off) -> float * {
        if (off < 0)
            return nullptr;
        if (c->extMix && off >= c->redirMixOff && off < c->redirMixOff + c->redirMixLen)
            return const_cast<float *>(c->extMix) + (off - c->redirMixOff); // only ever read
        if (c->extOut && off >= c->redirOutOff && off < c->redirOutOff + c->redirOutLen)
            return c->extOut + (off - c->redirOutOff);
        return A + off;
    };
    auto w = [&](i64 off) -> const float * { return off >= 0 ? W + off : nullptr; };
    switch (op.kind)
    {
    case OP_IGEMM:
    {
        const IGemm &g = op.g;
        GemmArgs k{};
        fill_gemm_geometry(k, g);
        k.X = a(g.x), k.proStats = a(g.proStats), k.proW = w(g.proW_w), k.proB = w(g.proB_w);
        k.Wt = w(g.w_w), k.bias = w(g.bias_w), k.Y = a(g.y);
        k.res = a(g.res), k.scale = w(g.scale_w), k.epiStats = a(g.epiStats), k.epiW = w(g.epiW_w), k.epiB = w(g.epiB_w);
        k.rowstat = a(g.rowstat), k.table = w(g.table_w);
        k.kvPl = g.kv >= 0 ? reinterpret_cast<unsigned short *>(A + g.kv) : nullptr;
        k.zero = A + zeroOff;
        int rc = -1;
        switch (g.choice.family)
        {
        case GF_DIRECT:
            rc = launch_dgemm(k, s);
            break;
        case GF_TILE:
        case GF_LIN256:
            rc = launch_igemm(g.cfg, k, s);
            break;
        case GF_SPLIT_LINH:
        {
            // fp16 terms (opt-in DMX_GEMM_FP16X3): the row scales of this op's A operand first, then the linear-layer kernel on
            // one fp16 weight plane
            float *rs = c->dRowScale[op.stream ? 1 : 0];
            if (!c->m->dWh || !rs)
                break;
            launch_rowscale(k, rs, s);
            k.rowScale = rs;
            k.Wb1 = k.Wb2 = c->m->dWh + g.w_w;
            rc = launch_igemm_split(g.choice, g.cfg, k, s);
            break;
        }
        case GF_NONE:
            break;
        default: // the bf16-term families
            if (!c->m->dWb)
                break;
            k.Wb1 = c->m->dWb + g.w_w;
            k.Wb2 = c->m->dWb + c->m->blobFloats + 512 + g.w_w;
            rc = launch_igemm_split(g.choice, g.cfg, k, s);
            break;
        }
        if (rc != 0) // never another arithmetic than the one the plan chose
            return fail(DMX_ERR_ARG, "internal error: the kernel chosen for op %s does not exist (%s: family %d, cfg %d pro %d epi %d)", op.name.c_str(),
                        g.choice.label ? g.choice.label : "none", g.choice.family, g.cfg, g.pro, g.epi);
        break;
    }
    case OP_DCONV_ROW:
    {
        const DconvRow &r = op.dr;
        DconvRowArgs k{};
        k.x = a(r.x), k.B = r.B, k.T = r.T, k.F = r.F, k.C = r.C, k.hid = r.hid, k.eps = r.eps, k.zero = A + zeroOff;
        k.img[0] = w(r.img_w[0]), k.img[1] = w(r.img_w[1]);
        if (launch_dconv_row(k, s) != 0)
            return fail(DMX_ERR_ARG, "internal error: no row-resident DConv kernel for op %s (C %d hidden %d T %d)", op.name.c_str(), r.C, r.hid, r.T);
        break;
    }
    case OP_STATS_REDUCE:
    {
        const StatsReduce &r = op.sr;
        launch_stats_reduce(ReduceArgs{a(r.rowstat), a(r.out), r.B, r.R, r.NB, r.G0, r.count, r.mode, r.eps,
                                       reinterpret_cast<double *>(a(r.scratch)), r.nchunk},
                            s);
        break;
    }
    case OP_STFT:
    {
        const Stft &t = op.stft;
        launch_stft(StftArgs{a(t.mix), a(t.x), a(t.rowstat), a(t.rowstatT), t.B, t.T, t.seg, t.pad, a(t.window), a(t.twiddle)}, s);
        break;
    }
    case OP_LAYERNORM:
    {
        const LayerNorm &l = op.ln;
        launch_layernorm(LnArgs{a(l.x), a(l.y), l.rows, l.D, l.rowsPerBatch, w(l.w_w), w(l.b_w), a(l.pe), l.eps}, s);
        break;
    }
    case OP_GN_APPLY:
    {
        const GnApply &g = op.gn;
        launch_gn_apply(GnArgs{a(g.x), a(g.y), a(g.res), g.B, g.rows, g.C, a(g.stats), w(g.w_w), w(g.b_w)}, s);
        break;
    }
    case OP_ATTENTION:
    {
        const Attention &t = op.at;
        AttnArgs k{a(t.q), a(t.k), a(t.v), a(t.o), t.ldq, t.ldk, t.ldv, t.ldo, t.qBatch, t.kBatch, t.vBatch,
                   t.oBatch, t.B, t.Tq, t.Tk, t.H, t.hs, t.scale};
        k.kpl = t.kpl >= 0 ? reinterpret_cast<const unsigned short *>(A + t.kpl) : nullptr;
        k.vt = t.vt >= 0 ? reinterpret_cast<const unsigned short *>(A + t.vt) : nullptr;
        k.kvPlane = (i64)t.B * t.Tk * t.H * t.hs;
        k.form = t.form;
        if (!(t.split && launch_attention_split(k, s) == 0))
        {
            if (t.kpl >= 0)
                return fail(DMX_ERR_ARG, "internal error: attention op %s reads operand planes but has no exact-split kernel", op.name.c_str());
            launch_attention(k, s);
        }
        break;
    }
    case OP_ISTFT:
    {
        const Istft &t = op.istft;
        if (!(t.fused && c->fuseIstft)) // fused: runs inside the following OP_OLA
            launch_istft(IstftArgs{a(t.x), a(t.stats), a(t.frames), t.B, t.T, t.S, a(t.window), a(t.twiddle)}, s);
        break;
    }
    case OP_OLA:
    {
        const Ola &o = op.ola;
        if (o.x >= 0 && c->fuseIstft)
            launch_istft_ola(IstftOlaArgs{a(o.x), a(o.stats), a(o.xt), a(o.statsT), a(o.wss), a(o.window), a(o.twiddle), a(o.out), o.B, o.T,
                                          o.S, o.seg, o.pad, 0, 0, a(o.rden)},
                             s);
        else
            launch_ola(OlaArgs{a(o.frames), a(o.xt), a(o.statsT), a(o.wss), a(o.out), o.B, o.T, o.S, o.seg, o.pad}, s);
        break;
    }
    case OP_GROUP_STATS:
    {
        const GroupStats &g = op.gs;
        launch_group_stats(GroupStatsArgs{a(g.x), a(g.out), reinterpret_cast<double *>(a(g.scratch)), g.B, g.rows, g.C, g.G, g.eps}, s);
        break;
    }
    case OP_GN_ACT:
    {
        const GnAct &g = op.ga;
        launch_gn_act(GnActArgs{a(g.x), a(g.y), a(g.stats), a(g.res), w(g.w_w), w(g.b_w), w(g.scale_w), g.B, g.rowsIn, g.C, g.G, g.mode,
                                g.rowOff, g.rowsOut},
                      s);
        break;
    }
    case OP_LSTM:
    {
        const Lstm &l = op.lstm;
        // The cooperative kernel spins on its partner workgroups, which is safe for ONE launch (in-order dispatch: every
        // recurrence's partners are resident before any later recurrence's) but not for launches of SEVERAL contexts that
        // share a device: at 42 segments a launch keeps 144 workgroups spinning, the device holds 512, and the fourth
        // concurrent launch could leave every resident workgroup waiting for a partner that has no slot (the bounded
        // spin would then turn it into an error, not a hang). LSTM launches of one device therefore form a lane: each
        // waits for the previous one's completion event, whatever stream or context it came from. (Graph captures - batches
        // below 8, at most 48 spinning workgroups per launch - stay outside: a capture cannot wait on a foreign event.)
        LstmLane *lane = c->capturing ? nullptr : lstm_lane(c->m->device);
        std::unique_lock<std::mutex> laneLock;
        if (lane)
        {
            laneLock = std::unique_lock<std::mutex>(lane->mu);
            if (!lane->ev)
                HIPCHK(hipEventCreateWithFlags(&lane->ev, hipEventDisableTiming));
            if (lane->recorded)
                HIPCHK(hipStreamWaitEvent(s, lane->ev, 0));
        }
        // several PROCESSES on this GPU (bench.py --backend gloo puts every rank on GPU 0): the in-process lane cannot
        // order their launches, so they take turns through a process-shared mutex, each waiting for its own launch to
        // finish before the next process may issue one (host-blocking, only while another process is registered)
        SharedLaneGuard shared(lane ? lane->shared : nullptr);
        const int lrc = launch_lstm(LstmArgs{a(l.xproj), w(l.whh_w), a(l.out), a(l.sync), c->dStatus, l.B, l.T, l.H}, s);
        if (lrc == -2)
            return fail(DMX_ERR_ARG, "op %s: the %d-segment LSTM launch needs more co-resident workgroups than this device holds", op.name.c_str(), l.B);
        if (lrc != 0)
            return fail(DMX_ERR_ARG, "internal error: no LSTM kernel for op %s (H = %d)", op.name.c_str(), l.H);
        if (lane)
        {
            HIPCHK(hipEventRecord(lane->ev, s));
            lane->recorded = true;
        }
        if (shared.held())
            HIPCHK(hipStreamSynchronize(s));
        break;
    }
    case OP_LOCAL_ATTN:
    {
        const LocalAttn &l = op.la;
        // default: the flash attention kernel with the decay penalty (fp32 MFMA; csrc/attention.hip LOC);
        // shapes it does not cover: the reference-order VALU kernel of csrc/v3.hip
        const int hd = l.H / 4;
        AttnArgs t{};
        t.q = a(l.qkvd), t.k = a(l.qkvd) + l.H, t.v = a(l.qkvd) + 2 * l.H, t.o = a(l.out);
        t.ldq = t.ldk = t.ldv = l.ld, t.ldo = l.H;
        t.qB = t.kB = t.vB = (i64)l.T * l.ld, t.oB = (i64)l.T * l.H;
        t.B = l.B, t.Tq = t.Tk = l.T, t.H = 4, t.hs = hd;
        t.scale = 1.0f / std::sqrt((float)hd);
        t.decay = a(l.qkvd) + 3 * l.H, t.ldd = l.ld, t.dB = (i64)l.T * l.ld;
        const int rc = launch_attention_local(t, s);
        if (rc != 0 && launch_local_attn(LocalAttnArgs{a(l.qkvd), a(l.out), l.B, l.T, l.H, l.ld}, s) != 0)
            return fail(DMX_ERR_ARG, "internal error: no LocalState kernel for op %s (T = %d, H = %d)", op.name.c_str(), l.T, l.H);
        break;
    }
    default:
        break;
    }
    return DMX_OK;
}

// enqueues the ops of the plan (one stream, or freq / time branch on two streams with the derived joins)
static int enqueue_plan(dmx_ctx *c, Plan *p, bool two)
{
    if (!two)
    {
        static const bool dbgSync = getenv("DMX_DEBUG_SYNC") && atoi(getenv("DMX_DEBUG_SYNC")) != 0; // diagnostics: name the op that faults
        for (const Op &op : p->ops)
        {
            if (dbgSync && op.kind != OP_TAP)
                fprintf(stderr, "dmx op %s (kind %d)\n", op.name.c_str(), (int)op.kind);
            DMXCHK(launch_op(c, op, c->stream, p->zeroOff));
            if (dbgSync)
                HIPCHK(hipStreamSynchronize(c->stream));
        }
        return DMX_OK;
    }
    // freq branch on `stream`, time branch on `stream2`, joined by the waits plan.cpp derived from
    // the ops' arena ranges (Op::waitOp / Op::signals); fork and join bracket the whole plan so
    // that callers only ever need to order themselves against `stream`.
    const size_t n = p->ops.size();
    if (c->events.size() < n)
        c->events.resize(n, nullptr);
    HIPCHK(hipEventRecord(c->evFork, c->stream));
    HIPCHK(hipStreamWaitEvent(c->stream2, c->evFork, 0));
    for (size_t i = 0; i < n; ++i)
    {
        const Op &op = p->ops[i];
        if (op.kind == OP_TAP)
            continue;
        hipStream_t s = op.stream ? c->stream2 : c->stream;
        if (op.waitOp >= 0)
            HIPCHK(hipStreamWaitEvent(s, c->events[(size_t)op.waitOp], 0));
        DMXCHK(launch_op(c, op, s, p->zeroOff));
        if (op.signals)
        {
            if (!c->events[i])
                HIPCHK(hipEventCreateWithFlags(&c->events[i], hipEventDisableTiming));
            HIPCHK(hipEventRecord(c->events[i], s));
        }
    }
    HIPCHK(hipEventRecord(c->evJoin, c->stream2));
    HIPCHK(hipStreamWaitEvent(c->stream, c->evJoin, 0));
    return DMX_OK;
}

static int run_plan(dmx_ctx *c, int batch)
{
    Plan *p = get_plan(c, batch);
    if (p->arenaFloats > c->arenaFloats)
        return fail(DMX_ERR_ARG, "internal: plan for batch %d exceeds the arena", batch);
    // Large batches fill all 256 CUs from one branch alone (two streams: +1.7 % at batch 12, while every
    // kernel's own duration stretches by the overlap); small batches gain up to 24 % from running the
    // freq and time branches concurrently.
    const bool two = c->streamMode == 2 || (c->streamMode == 0 && batch < dmx_ctx::kTwoStreamMaxBatch);
    // Small batches are launch-bound (~330 kernels of ~20 us on two streams with 23 event joins): when the
    // same call (same I/O buffers, model and batch) comes a second time in a row, the whole two-stream
    // schedule is captured into a HIP graph and replayed from then on (shapes are static).
    const bool graphable = c->graphMode == 1 && two && c->stream == c->ownStream;
    const dmx_ctx::GraphKey key{c->extMix, c->extOut, c->m->dW}; // the captured kernels hold the weight pointer by value
    hipGraphExec_t exec = nullptr;
    if (graphable)
    {
        if (batch != c->graphBatch)
        {
            {
                std::lock_guard<std::mutex> graphLock(g_graphMutex);
                for (auto &kv : c->graphs)
                    (void)hipGraphExecDestroy(kv.second);
            }
            c->graphs.clear();
            c->graphBatch = batch;
            c->haveLastKey = false;
        }
        auto it = c->graphs.find(key);
        if (it != c->graphs.end())
            exec = it->second;
        else if (c->haveLastKey && !(key < c->lastKey) && !(c->lastKey < key))
        {
            if (c->graphs.size() >= 8)
            {
                std::lock_guard<std::mutex> graphLock(g_graphMutex);
                for (auto &kv : c->graphs)
                    (void)hipGraphExecDestroy(kv.second);
                c->graphs.clear();
            }
            // events recorded during the capture must exist beforehand
            if (c->events.size() < p->ops.size())
                c->events.resize(p->ops.size(), nullptr);
            for (size_t i = 0; i < p->ops.size(); ++i)
                if (p->ops[i].signals && !c->events[i])
                    HIPCHK(hipEventCreateWithFlags(&c->events[i], hipEventDisableTiming));
            hipGraph_t g = nullptr;
            std::lock_guard<std::mutex> graphLock(g_graphMutex);
            HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            c->capturing = true;
            const int rc = enqueue_plan(c, p, true);
            c->capturing = false;
            const hipError_t e = hipStreamEndCapture(c->stream, &g);
            if (rc != DMX_OK || e != hipSuccess)
            {
                if (g)
                    (void)hipGraphDestroy(g);
                return rc != DMX_OK ? rc : fail(DMX_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
            }
            const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ei != hipSuccess)
                return fail(DMX_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ei));
            c->graphs.emplace(key, exec);
        }
        c->lastKey = key, c->haveLastKey = true;
    }
    if (exec)
    {
        std::lock_guard<std::mutex> graphLock(g_graphMutex);
        HIPCHK(hipGraphLaunch(exec, c->stream));
    }
    else
        DMXCHK(enqueue_plan(c, p, two));
    c->lastBatch = batch;
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_segment_infer_device(dmx_ctx *c, const float *d_mix, float *d_out, int batch)
{
    if (!c || !d_mix || !d_out || batch < 1 || batch > c->maxBatch)
        return fail(DMX_ERR_ARG, "dmx_segment_infer_device: invalid argument");
    HIPCHK(hipSetDevice(c->m->device));
    Plan *p = get_plan(c, batch);
    const int S = c->m->pm.n_sources;
    // the kernels read the caller's mix and write the caller's output directly (no staging copies):
    // both buffers have exactly the layout of the arena regions they stand in for
    c->extMix = d_mix, c->extOut = d_out;
    c->redirMixOff = p->mixOff, c->redirMixLen = (i64)batch * c->seg * 2;
    c->redirOutOff = p->outOff, c->redirOutLen = (i64)batch * S * 2 * c->seg;
    int rc = run_plan(c, batch);
    c->extMix = nullptr, c->extOut = nullptr;
    return rc;
}

extern "C" int dmx_segment_infer(dmx_ctx *c, const float *mix, float *out, int layout)
{
    if (!c || !mix || !out)
        return fail(DMX_ERR_ARG, "dmx_segment_infer: null argument");
    HIPCHK(hipSetDevice(c->m->device));
    Plan *p = get_plan(c, 1);
    const int S = c->m->pm.n_sources;
    const i64 seg = c->seg;
    std::vector<float> tmp;
    const float *src = mix;
    if (layout == DMX_LAYOUT_PLANAR)
    {
        tmp.resize((size_t)(2 * seg));
        for (i64 i = 0; i < seg; ++i)
        {
            tmp[(size_t)(2 * i)] = mix[i];
            tmp[(size_t)(2 * i + 1)] = mix[seg + i];
        }
        src = tmp.data();
    }
    else if (layout != DMX_LAYOUT_EIGEN)
        return fail(DMX_ERR_ARG, "dmx_segment_infer: unknown layout %d", layout);
    HIPCHK(hipMemcpyAsync(c->dA + p->mixOff, src, sizeof(float) * (size_t)(2 * seg), hipMemcpyHostToDevice, c->stream));
    int rc = run_plan(c, 1);
    if (rc)
        return rc;
    std::vector<float> planar((size_t)(S * 2 * seg));
    HIPCHK(hipMemcpyAsync(planar.data(), c->dA + p->outOff, sizeof(float) * planar.size(), hipMemcpyDeviceToHost, c->stream));
    DMXCHK(dmx_ctx_sync_checked(c));
    if (layout == DMX_LAYOUT_PLANAR)
        std::memcpy(out, planar.data(), sizeof(float) * planar.size());
    else
        for (int s = 0; s < S; ++s)
            for (int ch = 0; ch < 2; ++ch)
                for (i64 i = 0; i < seg; ++i)
                    out[s + (i64)S * (ch + 2 * i)] = planar[(size_t)((s * 2 + ch) * seg + i)];
    return DMX_OK;
}

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
namespace
{
struct BagRun // the models of a call and their effective weights [Q][S] (dmx_bag_weights)
{
    const dmx_model *const *models;
    int Q;
    const float *w;
};
struct PcmOut // the output spec of a call, checked (pcm_check_spec)
{
    dmx_output_spec spec;
    void *const *out;
    float *peaks;
    int nOut, frameBytes;
    const PcmGains *remix; // dmx_tracks_infer_remix: the outputs are rows of gains over the stems and the mixture, else NULL
    // dmx_tracks_infer_flac (flacBits 16 | 24, else 0): out[t] takes n_out files at a stride of dmx_flac_bound, sizes their byte counts
    int flacBits, flacRate;
    int64_t *sizes;
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

    const dmx_ctx::TrackSlot &slot(int t) const { return c->slots[(size_t)plan.jobs[(size_t)t].slot]; }
};
} // namespace

// the context's buffers, streams and events for the plan
static int tracks_prepare(TracksRun &r)
{
    dmx_ctx *c = r.c;
    const TracksPlan &p = r.plan;
    const PcmOut *pcm = r.pcm;
    const i64 nmax = p.nmax;
    DMXCHK(dmx_ensure_buf(c->bMix, 2 * p.seg * p.B));
    DMXCHK(dmx_ensure_buf(c->bSegOut, p.ringBlocks * r.blk));
    if ((int)c->slots.size() < p.nSlots)
        c->slots.resize((size_t)p.nSlots);
    for (int i = 0; i < p.nSlots; ++i)
    {
        dmx_ctx::TrackSlot &sl = c->slots[(size_t)i];
        DMXCHK(dmx_ensure_buf(sl.audio, 2 * nmax));
        if (r.layout == DMX_LAYOUT_PLANAR)
            DMXCHK(dmx_ensure_buf(sl.tmp, 2 * nmax));
        DMXCHK(dmx_ensure_buf(sl.out, (i64)r.S * 2 * nmax));
        DMXCHK(dmx_ensure_buf(sl.stats, 4));
        if (pcm)
        {
            DMXCHK(dmx_ensure_buf(sl.pcm, (i64)pcm->nOut * (DMX_OUTPUT_STRIDE(nmax * pcm->frameBytes) / 4)));
            DMXCHK(dmx_ensure_buf(sl.peaks, 8));
            if (pcm->flacBits)
            {
                DMXCHK(dmx_ensure_buf(sl.flac, (i64)pcm->nOut * (flac_bound(pcm->flacBits, nmax) / 4)));
                DMXCHK(dmx_ensure_buf(sl.flacWork, (i64)pcm->nOut * (flac_workspace_bytes(pcm->flacBits, nmax) / 4)));
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
        if (r.flacIn) // the file's bytes go up; the five launches of flac_in.hip leave the interleaved track in the slot
        {
            HIPCHK(hipMemcpyAsync(sl.flacIn.p, r.audio[t], (size_t)r.fileBytes[t], hipMemcpyHostToDevice, c->uploadStream));
            if (launch_flac_decode((const unsigned char *)sl.flacIn.p, r.fileBytes[t], &r.flacIn[t], DMX_PCM_F32, sl.audio.p,
                                   (long long *)sl.flacInStatus.p, sl.flacInWork.p, c->uploadStream) != 0)
                return fail(DMX_ERR_ARG, "%s: track %d: internal error (the probe's description was refused)", r.fn, t);
        }
        else if (r.eigen)
            HIPCHK(hipMemcpyAsync(sl.audio.p, r.audio[t], sizeof(float) * 2 * (size_t)j.n, hipMemcpyHostToDevice, c->uploadStream));
        else
        {
            HIPCHK(hipMemcpyAsync(sl.tmp.p, r.audio[t], sizeof(float) * 2 * (size_t)j.n, hipMemcpyHostToDevice, c->uploadStream));
            launch_planar_to_interleaved(sl.tmp.p, sl.audio.p, j.n, c->uploadStream);
        }
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

// the overlap-add of what batch k makes final: one of three kernels (N == 1, the shifts ensemble, a bag)
static int tracks_ola(TracksRun &r, int k)
{
    const TracksPlan &p = r.plan;
    const int Q = p.Q, N = p.N, S = r.S;
    const i64 Rq = p.R[(size_t)p.batches[(size_t)k].q];
    hipStream_t s = r.c->stream;
    r.ola.clear(), r.ens.clear(), r.ensCopies.clear(), r.bagPieces.clear(), r.bagModels.clear();
    for (const TrackPiece &pc : p.pieces[(size_t)k])
    {
        if (pc.hi <= pc.lo)
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
    if (r.bag)
    {
        if (!launch_track_ola_bag(r.bagPieces.data(), r.bagModels.data(), r.ensCopies.data(), (int)r.bagPieces.size(), Q, N, r.bag->w,
                                  r.rings.data(), p.R.data(), S, p.seg, p.stride, r.olaEigen, 0, 2 * S, s))
            return fail(DMX_ERR_ARG, "%s: internal error (the bag's overlap-add was refused in batch %d)", r.fn, k);
    }
    else if (N == 1)
        launch_track_ola(r.ola.data(), (int)r.ola.size(), S, p.seg, p.stride, Rq, r.olaEigen, 0, 2 * S, s);
    else
        launch_track_ola_ens(r.ens.data(), r.ensCopies.data(), (int)r.ens.size(), N, r.rings[0], S, p.seg, p.stride, Rq, r.olaEigen, 0,
                             2 * S, s);
    HIPCHK(hipGetLastError());
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
        const i64 n = p.jobs[(size_t)g.t].n;
        const dmx_ctx::TrackSlot &sl = r.slot(g.t);
        RemixPiece pp{PcmPiece{sl.out.p, (unsigned char *)sl.pcm.p, (unsigned *)sl.peaks.p, n, n, DMX_OUTPUT_STRIDE(n * pcm->frameBytes), g.lo, g.hi},
                      pcm->remix ? sl.audio.p : nullptr};
        r.pieces.push_back(pp);
        if (g.hi == n)
        {
            pp.i0 = 0;
            r.whole.push_back(pp);
        }
    }
    const std::vector<RemixPiece> &enc = r.wholeTrack ? r.whole : r.pieces;
    if (pcm->remix)
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
            const i64 n = p.jobs[(size_t)g.t].n;
            if (g.hi != n)
                continue;
            const dmx_ctx::TrackSlot &sl = r.slot(g.t);
            launch_flac_encode((const unsigned char *)sl.pcm.p, DMX_OUTPUT_STRIDE(n * pcm->frameBytes), pcm->flacBits, n, pcm->flacRate,
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
    const i64 n = r.plan.jobs[(size_t)g.t].n;
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
    for (const TrackPiece &pc : p.pieces[(size_t)k])
    {
        const TrackJob &j = p.jobs[(size_t)pc.t];
        const dmx_ctx::TrackSlot &sl = r.slot(pc.t);
        const float *dOut = sl.out.p;
        float *out = r.out ? r.out[pc.t] : nullptr;
        const i64 i0 = pc.lo, i1 = pc.hi;
        if (i1 > i0 && !r.pcm)
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
    r.wholeTrack = r.pcm && r.pcm->spec.clip == DMX_CLIP_RESCALE;
    std::string why;
    const int rcPlan = tracks_plan_build(r.plan, r.T, r.n, r.bag ? r.bag->Q : 1, r.N, r.shifts, c->seg, r.stride, c->maxBatch, r.pcm != nullptr,
                                         r.bag ? -1 : TrackEnsTable::kMaxTail, why);
    if (rcPlan != DMX_OK)
        return fail(rcPlan, "%s: %s", r.fn, why.c_str());
    if (r.bag)
        DMXCHK(tracks_check_bag_caps(r));
    DMXCHK(tracks_prepare(r));
    const TracksPlan &p = r.plan;
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
        DMXCHK(tracks_ola(r, k));
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
static int pcm_check_spec(const char *fn, const dmx_output_spec *spec, int S)
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
static int pcm_frame_bytes(int encoding) { return encoding == DMX_PCM_F32 ? 8 : encoding == DMX_PCM_S16 ? 4 : 6; }

extern "C" int dmx_output_count(const dmx_model *m, const dmx_output_spec *spec)
{
    if (!m || pcm_check_spec("dmx_output_count", spec, m->pm.n_sources) != DMX_OK)
        return -1;
    return spec->stem < 0 ? m->pm.n_sources : 2;
}
extern "C" int64_t dmx_output_bytes(const dmx_output_spec *spec, int64_t n)
{
    if (n < 0 || pcm_check_spec("dmx_output_bytes", spec, -1) != DMX_OK)
        return -1;
    return n * pcm_frame_bytes(spec->encoding);
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
static int remix_check_spec(const char *fn, int S, const dmx_remix_spec *spec, PcmGains *G, bool noModel)
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
static bool remix_uses_mix(const PcmGains &G)
{
    for (int o = 0; o < G.nOut; ++o)
        if (G.g[o][G.S] != 0.0f)
            return true;
    return false;
}

extern "C" int dmx_remix_check(int n_sources, const dmx_remix_spec *spec)
{
    return remix_check_spec("dmx_remix_check", n_sources, spec, nullptr, false);
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
    DMXCHK(remix_check_spec(fn, 0, a.remix, nullptr, true)); // what of the spec can be checked without a model
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
            DMXCHK(remix_check_spec(fn, 0, a.remix, nullptr, true)); // what of the spec can be checked without a model
            return fail(DMX_ERR_ARG, "%s: null context", fn);
        }
        DMXCHK(remix_check_spec(fn, a.c->m->pm.n_sources, a.remix, &G, false));
        if (!a.bag && a.weights)
            return fail(DMX_ERR_ARG, "%s: weights given without models", fn);
    }
    float w[DMX_MAX_BAG * TrackBagTable::kMaxStems];
    if (a.bag)
    {
        DMXCHK(check_tracks_bag(a, w));
        if (a.kind == TRACKS_OUT_PCM)
            DMXCHK(pcm_check_spec(fn, a.spec, a.c->m->pm.n_sources));
        if (a.n_shifts >= 1 && (i64)a.n_models * a.n_shifts > TrackBagTable::kMaxCopies)
            return fail(DMX_ERR_ARG, "%s: n_models * n_shifts must be <= %d, got %d x %d", fn, TrackBagTable::kMaxCopies, a.n_models,
                        a.n_shifts);
    }
    else if (a.kind == TRACKS_OUT_PCM)
        DMXCHK(pcm_check_spec(fn, a.spec, -1));
    i64 stride = 0;
    DMXCHK(check_tracks_opts(a, stride));
    const int S = a.c->m->pm.n_sources;
    if (!a.bag && a.kind == TRACKS_OUT_PCM)
        DMXCHK(pcm_check_spec(fn, a.spec, S));
    const BagRun bag{a.models, a.n_models, w};
    PcmOut pcm{};
    if (remix)
        pcm = PcmOut{dmx_output_spec{a.remix->encoding, a.remix->clip, -1}, a.out, a.peaks, a.remix->n_out, pcm_frame_bytes(a.remix->encoding),
                     &G, 0, 0, nullptr};
    else if (a.kind == TRACKS_OUT_PCM)
        pcm = PcmOut{*a.spec, a.out, a.peaks, a.spec->stem < 0 ? S : 2, pcm_frame_bytes(a.spec->encoding), nullptr, 0, 0, nullptr};
    if (a.kind == TRACKS_OUT_FLAC)
        pcm.flacBits = pcm.spec.encoding == DMX_PCM_S16 ? 16 : 24, pcm.flacRate = a.flacRate, pcm.sizes = a.flacSizes;
    // (track, copy) order; with models (track, model, copy) order
    const std::vector<int> shifts = draw_shifts(a.bag ? a.n_tracks * a.n_models : a.n_tracks, a.n_shifts, a.shift_offsets);
    TracksRun r;
    r.c = a.c, r.fn = fn, r.T = a.n_tracks, r.audio = a.audio, r.n = a.n, r.N = a.n_shifts, r.stride = stride, r.shifts = shifts.data();
    r.layout = a.layout, r.progress = a.progress, r.user = a.user;
    r.flacIn = a.flacIn, r.fileBytes = a.fileBytes, r.trackStatus = a.trackStatus;
    if (a.kind == TRACKS_OUT_F32)
        r.out = reinterpret_cast<float *const *>(a.out);
    else
        r.pcm = &pcm;
    if (a.bag)
        r.bag = &bag;
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

extern "C" int dmx_pcm_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                     const dmx_output_spec *spec, void *d_out, float *d_peaks, void *stream)
{
    const char *fn = "dmx_pcm_encode_device";
    if (n_sources < 1 || n_sources > 64)
        return fail(DMX_ERR_ARG, "%s: n_sources %d", fn, n_sources);
    DMXCHK(pcm_check_spec(fn, spec, n_sources));
    if (!d_planes || !d_out || !d_peaks)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_planes ? "d_planes" : !d_out ? "d_out" : "d_peaks");
    if (n < 1 || plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (1 <= n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    if (((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_planes & 3) != 0 || ((uintptr_t)d_peaks & 3) != 0)
        return fail(DMX_ERR_ARG, "%s: d_out must be 16-byte aligned, d_planes and d_peaks 4-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const int nOut = spec->stem < 0 ? n_sources : 2;
    HIPCHK(hipMemsetAsync(d_peaks, 0, sizeof(float) * (size_t)nOut, s));
    const PcmPiece pp{d_planes, (unsigned char *)d_out, (unsigned *)d_peaks, n, plane_stride,
                      DMX_OUTPUT_STRIDE(n * pcm_frame_bytes(spec->encoding)), 0, n};
    launch_pcm_peak(&pp, 1, n_sources, spec->stem, s);
    launch_pcm_encode(&pp, 1, n_sources, spec->stem, spec->encoding, spec->clip, s);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_pcm_encode(int device, const float *planes, int n_sources, int64_t n, const dmx_output_spec *spec, void *out,
                              float *peaks)
{
    const char *fn = "dmx_pcm_encode";
    if (n_sources < 1 || n_sources > 64)
        return fail(DMX_ERR_ARG, "%s: n_sources %d", fn, n_sources);
    DMXCHK(pcm_check_spec(fn, spec, n_sources));
    if (!planes || !out || n < 1)
        return fail(DMX_ERR_ARG, "%s: invalid argument (null pointer or n < 1)", fn);
    HIPCHK(hipSetDevice(device));
    const int nOut = spec->stem < 0 ? n_sources : 2;
    const i64 bytes = n * pcm_frame_bytes(spec->encoding), devStride = DMX_OUTPUT_STRIDE(bytes);
    const size_t inBytes = sizeof(float) * (size_t)n_sources * 2 * (size_t)n;
    float *dIn = nullptr, *dPeaks = nullptr;
    unsigned char *dOut = nullptr;
    int rc = DMX_OK;
    if (hipMalloc((void **)&dIn, inBytes) != hipSuccess || hipMalloc((void **)&dOut, (size_t)(nOut * devStride)) != hipSuccess ||
        hipMalloc((void **)&dPeaks, sizeof(float) * (size_t)nOut) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (rc == DMX_OK && hipMemcpy(dIn, planes, inBytes, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: upload failed", fn);
    if (rc == DMX_OK)
        rc = dmx_pcm_encode_device(device, dIn, n_sources, n, n, spec, dOut, dPeaks, nullptr);
    if (rc == DMX_OK && hipDeviceSynchronize() != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    for (int o = 0; rc == DMX_OK && o < nOut; ++o)
        if (hipMemcpy((unsigned char *)out + (size_t)(o * bytes), dOut + (size_t)(o * devStride), (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(DMX_ERR_HIP, "%s: download failed", fn);
    if (rc == DMX_OK && peaks && hipMemcpy(peaks, dPeaks, sizeof(float) * (size_t)nOut, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: download failed", fn);
    for (void *p : {(void *)dIn, (void *)dOut, (void *)dPeaks})
        if (p)
            (void)hipFree(p);
    return rc;
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

extern "C" int dmx_remix_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                       const float *d_mix, const dmx_remix_spec *spec, void *d_out, float *d_peaks, void *stream)
{
    const char *fn = "dmx_remix_encode_device";
    PcmGains G;
    DMXCHK(remix_check_spec(fn, n_sources, spec, &G, false));
    if (!d_planes || !d_out || !d_peaks)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_planes ? "d_planes" : !d_out ? "d_out" : "d_peaks");
    if (!d_mix && remix_uses_mix(G))
        return fail(DMX_ERR_ARG, "%s: null d_mix pointer, and the mixture column of the gains is not all zero", fn);
    if (n < 1 || plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (1 <= n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    if (((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_planes & 3) != 0 || ((uintptr_t)d_peaks & 3) != 0 || ((uintptr_t)d_mix & 3) != 0)
        return fail(DMX_ERR_ARG, "%s: d_out must be 16-byte aligned, d_planes, d_mix and d_peaks 4-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_peaks, 0, sizeof(float) * (size_t)G.nOut, s));
    RemixPiece pp{PcmPiece{d_planes, (unsigned char *)d_out, (unsigned *)d_peaks, n, plane_stride,
                           DMX_OUTPUT_STRIDE(n * pcm_frame_bytes(spec->encoding)), 0, n},
                  d_mix};
    launch_remix_peak(&pp, 1, G, s);
    launch_remix_encode(&pp, 1, G, spec->encoding, spec->clip, s);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_remix_encode(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                                void *out, float *peaks)
{
    const char *fn = "dmx_remix_encode";
    PcmGains G;
    DMXCHK(remix_check_spec(fn, n_sources, spec, &G, false));
    if (!planes || !out || n < 1)
        return fail(DMX_ERR_ARG, "%s: invalid argument (null pointer or n < 1)", fn);
    if (!mix && remix_uses_mix(G))
        return fail(DMX_ERR_ARG, "%s: null mix pointer, and the mixture column of the gains is not all zero", fn);
    HIPCHK(hipSetDevice(device));
    const int nOut = G.nOut;
    const i64 bytes = n * pcm_frame_bytes(spec->encoding), devStride = DMX_OUTPUT_STRIDE(bytes);
    const size_t inBytes = sizeof(float) * (size_t)n_sources * 2 * (size_t)n, mixBytes = sizeof(float) * 2 * (size_t)n;
    float *dIn = nullptr, *dPeaks = nullptr, *dMix = nullptr;
    unsigned char *dOut = nullptr;
    int rc = DMX_OK;
    if (hipMalloc((void **)&dIn, inBytes) != hipSuccess || hipMalloc((void **)&dOut, (size_t)(nOut * devStride)) != hipSuccess ||
        hipMalloc((void **)&dPeaks, sizeof(float) * (size_t)nOut) != hipSuccess || (mix && hipMalloc((void **)&dMix, mixBytes) != hipSuccess))
        rc = fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (rc == DMX_OK && (hipMemcpy(dIn, planes, inBytes, hipMemcpyHostToDevice) != hipSuccess ||
                         (mix && hipMemcpy(dMix, mix, mixBytes, hipMemcpyHostToDevice) != hipSuccess)))
        rc = fail(DMX_ERR_HIP, "%s: upload failed", fn);
    if (rc == DMX_OK)
        rc = dmx_remix_encode_device(device, dIn, n_sources, n, n, dMix, spec, dOut, dPeaks, nullptr);
    if (rc == DMX_OK && hipDeviceSynchronize() != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    for (int o = 0; rc == DMX_OK && o < nOut; ++o)
        if (hipMemcpy((unsigned char *)out + (size_t)(o * bytes), dOut + (size_t)(o * devStride), (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(DMX_ERR_HIP, "%s: download failed", fn);
    if (rc == DMX_OK && peaks && hipMemcpy(peaks, dPeaks, sizeof(float) * (size_t)nOut, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: download failed", fn);
    for (void *p : {(void *)dIn, (void *)dOut, (void *)dPeaks, (void *)dMix})
        if (p)
            (void)hipFree(p);
    return rc;
}

// --------------------------------------------------------------------------- FLAC output (flac.hip)
extern "C" int64_t dmx_flac_bound(int bits, int64_t n) { return flac_bound(bits, n); }
extern "C" int64_t dmx_flac_workspace_bytes(int bits, int64_t n) { return flac_workspace_bytes(bits, n); }

static int flac_check(const char *fn, int bits, int64_t n, int sample_rate)
{
    if (bits != 16 && bits != 24)
        return fail(DMX_ERR_ARG, "%s: bits %d (16 or 24)", fn, bits);
    if (n < 1 || n >= (int64_t)1 << 36)
        return fail(DMX_ERR_ARG, "%s: n = %lld, must be in [1, 2^36)", fn, (long long)n);
    if (sample_rate < 1 || sample_rate > 655350)
        return fail(DMX_ERR_ARG, "%s: sample_rate %d not in [1, 655350]", fn, sample_rate);
    return DMX_OK;
}

static int flac_level_check(const char *fn, int level)
{
    if (level < 0 || level > 2)
        return fail(DMX_ERR_ARG, "%s: level %d (0, 1 or 2)", fn, level);
    return DMX_OK;
}

// marks: null, or four events recorded around the three launches (dmx_flac_encode_device_timed)
static int flac_encode_device(const char *fn, int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                              int64_t *d_size, void *d_work, void *stream, hipEvent_t *marks)
{
    DMXCHK(flac_check(fn, bits, n, sample_rate));
    DMXCHK(flac_level_check(fn, level));
    if (!d_pcm || !d_out || !d_size || !d_work)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_pcm ? "d_pcm" : !d_out ? "d_out" : !d_size ? "d_size" : "d_work");
    if (((uintptr_t)d_pcm & 15) != 0 || ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_size & 7) != 0)
        return fail(DMX_ERR_ARG, "%s: d_pcm and d_work must be 16-byte aligned, d_size 8-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    launch_flac_encode((const unsigned char *)d_pcm, 0, bits, n, sample_rate, 1, (unsigned char *)d_out, 0, (long long *)d_size,
                       (unsigned char *)d_work, (hipStream_t)stream, level, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_flac_encode_device(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, void *d_out, int64_t *d_size,
                                      void *d_work, void *stream)
{
    return flac_encode_device("dmx_flac_encode_device", device, d_pcm, bits, n, sample_rate, 0, d_out, d_size, d_work, stream, nullptr);
}
extern "C" int dmx_flac_encode_device_level(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                                            int64_t *d_size, void *d_work, void *stream)
{
    return flac_encode_device("dmx_flac_encode_device_level", device, d_pcm, bits, n, sample_rate, level, d_out, d_size, d_work, stream,
                              nullptr);
}
// measurement (tools/flac_bench.py): the call above, synchronised, with the three kernels' times between HIP events in ms[0..3)
extern "C" int dmx_flac_encode_device_timed(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                                            int64_t *d_size, void *d_work, void *stream, float *ms)
{
    const char *fn = "dmx_flac_encode_device_timed";
    if (!ms)
        return fail(DMX_ERR_ARG, "%s: null ms pointer", fn);
    HIPCHK(hipSetDevice(device));
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = DMX_OK;
    for (int i = 0; i < 4 && rc == DMX_OK; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess)
            rc = fail(DMX_ERR_HIP, "%s: hipEventCreate failed", fn);
    if (rc == DMX_OK)
        rc = flac_encode_device(fn, device, d_pcm, bits, n, sample_rate, level, d_out, d_size, d_work, stream, ev);
    if (rc == DMX_OK && hipEventSynchronize(ev[3]) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    for (int i = 0; i < 3 && rc == DMX_OK; ++i)
        if (hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess)
            rc = fail(DMX_ERR_HIP, "%s: hipEventElapsedTime failed", fn);
    for (hipEvent_t e : ev)
        if (e)
            (void)hipEventDestroy(e);
    return rc;
}

static int flac_encode_host(const char *fn, int device, const void *pcm, int bits, int64_t n, int sample_rate, int level, void *out,
                            int64_t *size)
{
    DMXCHK(flac_check(fn, bits, n, sample_rate));
    DMXCHK(flac_level_check(fn, level));
    if (!pcm || !out || !size)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !pcm ? "pcm" : !out ? "out" : "size");
    HIPCHK(hipSetDevice(device));
    const size_t inBytes = (size_t)n * 2 * (size_t)(bits / 8);
    const i64 bound = flac_bound(bits, n), workBytes = flac_workspace_bytes(bits, n);
    unsigned char *dIn = nullptr, *dOut = nullptr, *dWork = nullptr;
    int64_t *dSize = nullptr;
    int64_t got = 0;
    int rc = DMX_OK;
    if (hipMalloc((void **)&dIn, DMX_OUTPUT_STRIDE(inBytes)) != hipSuccess || hipMalloc((void **)&dOut, (size_t)bound) != hipSuccess ||
        hipMalloc((void **)&dWork, (size_t)workBytes) != hipSuccess || hipMalloc((void **)&dSize, sizeof(int64_t)) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (rc == DMX_OK && hipMemcpy(dIn, pcm, inBytes, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: upload failed", fn);
    if (rc == DMX_OK)
        rc = flac_encode_device(fn, device, dIn, bits, n, sample_rate, level, dOut, dSize, dWork, nullptr, nullptr);
    if (rc == DMX_OK && hipDeviceSynchronize() != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    if (rc == DMX_OK && hipMemcpy(&got, dSize, sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: download failed", fn);
    if (rc == DMX_OK && (got < 42 || got > bound))
        rc = fail(DMX_ERR_HIP, "%s: internal error (%lld encoded bytes, bound %lld)", fn, (long long)got, (long long)bound);
    if (rc == DMX_OK && hipMemcpy(out, dOut, (size_t)got, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: download failed", fn);
    for (void *p : {(void *)dIn, (void *)dOut, (void *)dWork, (void *)dSize})
        if (p)
            (void)hipFree(p);
    if (rc == DMX_OK)
        *size = got;
    return rc;
}
extern "C" int dmx_flac_encode(int device, const void *pcm, int bits, int64_t n, int sample_rate, void *out, int64_t *size)
{
    return flac_encode_host("dmx_flac_encode", device, pcm, bits, n, sample_rate, 0, out, size);
}
extern "C" int dmx_flac_encode_level(int device, const void *pcm, int bits, int64_t n, int sample_rate, int level, void *out, int64_t *size)
{
    return flac_encode_host("dmx_flac_encode_level", device, pcm, bits, n, sample_rate, level, out, size);
}

extern "C" int dmx_ctx_set_flac_level(dmx_ctx *c, int level)
{
    if (!c)
        return fail(DMX_ERR_ARG, "dmx_ctx_set_flac_level: null context");
    DMXCHK(flac_level_check("dmx_ctx_set_flac_level", level));
    c->flacLevel = level;
    return DMX_OK;
}
extern "C" int dmx_ctx_flac_level(const dmx_ctx *c) { return c ? c->flacLevel : -1; }

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

// --------------------------------------------------------------------------- FLAC input (flac_in.hip)
extern "C" int dmx_flac_probe(const void *file, int64_t bytes, dmx_flac_info *info)
{
    if (!file || !info)
        return fail(DMX_ERR_ARG, "dmx_flac_probe: null %s pointer", !file ? "file" : "info");
    char msg[160];
    if (flac_in_probe(file, bytes, info, msg, sizeof msg) != 0)
        return fail(DMX_ERR_FORMAT, "dmx_flac_probe: %s", msg);
    return DMX_OK;
}
extern "C" int64_t dmx_flac_decode_workspace_bytes(const dmx_flac_info *info, int64_t bytes) { return flac_in_workspace_bytes(info, bytes); }

static int flac_in_check(const char *fn, int64_t bytes, const dmx_flac_info *info, int encoding)
{
    if (!info)
        return fail(DMX_ERR_ARG, "%s: null info pointer", fn);
    if (flac_in_workspace_bytes(info, bytes) < 0)
        return fail(DMX_ERR_ARG, "%s: info is not what dmx_flac_probe returns for a file of %lld bytes", fn, (long long)bytes);
    if (info->bits != 8 && info->bits != 12 && info->bits != 16 && info->bits != 20 && info->bits != 24)
        return fail(DMX_ERR_ARG, "%s: %d bits per sample (8, 12, 16, 20 or 24)", fn, info->bits);
    if (encoding != DMX_PCM_F32 && encoding != DMX_PCM_S16 && encoding != DMX_PCM_S24)
        return fail(DMX_ERR_ARG, "%s: encoding %d (DMX_PCM_F32 0, DMX_PCM_S16 1, DMX_PCM_S24 2)", fn, encoding);
    if (encoding != DMX_PCM_F32 && (info->channels != 2 || info->bits != (encoding == DMX_PCM_S16 ? 16 : 24)))
        return fail(DMX_ERR_ARG, "%s: encoding %s needs a stereo stream of exactly that depth (this one: %d channel(s), %d bits)", fn,
                    encoding == DMX_PCM_S16 ? "DMX_PCM_S16" : "DMX_PCM_S24", info->channels, info->bits);
    return DMX_OK;
}

extern "C" int dmx_flac_decode_device(int device, const void *d_file, int64_t bytes, const dmx_flac_info *info, int encoding, void *d_out,
                                      int64_t *d_status, void *d_work, void *stream)
{
    const char *fn = "dmx_flac_decode_device";
    DMXCHK(flac_in_check(fn, bytes, info, encoding));
    if (!d_file || !d_out || !d_status || !d_work)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_file ? "d_file" : !d_out ? "d_out" : !d_status ? "d_status" : "d_work");
    if (((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_status & 7) != 0)
        return fail(DMX_ERR_ARG, "%s: d_out and d_work must be 16-byte aligned, d_status 8-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    if (launch_flac_decode((const unsigned char *)d_file, bytes, info, encoding, d_out, (long long *)d_status, d_work, (hipStream_t)stream) != 0)
        return fail(DMX_ERR_ARG, "%s: info rejected", fn);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_flac_decode(int device, const void *file, int64_t bytes, const dmx_flac_info *info, int encoding, void *out, int64_t *status)
{
    const char *fn = "dmx_flac_decode";
    DMXCHK(flac_in_check(fn, bytes, info, encoding));
    if (!file || !out || !status)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !file ? "file" : !out ? "out" : "status");
    HIPCHK(hipSetDevice(device));
    const size_t outBytes = (size_t)info->total_samples * (encoding == DMX_PCM_F32 ? 8 : encoding == DMX_PCM_S16 ? 4 : 6);
    const i64 workBytes = flac_in_workspace_bytes(info, bytes);
    unsigned char *dIn = nullptr, *dOut = nullptr, *dWork = nullptr;
    int64_t *dStatus = nullptr;
    int rc = DMX_OK;
    if (hipMalloc((void **)&dIn, (size_t)bytes) != hipSuccess || hipMalloc((void **)&dOut, DMX_OUTPUT_STRIDE(outBytes)) != hipSuccess ||
        hipMalloc((void **)&dWork, (size_t)workBytes) != hipSuccess || hipMalloc((void **)&dStatus, 2 * sizeof(int64_t)) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (rc == DMX_OK && hipMemcpy(dIn, file, (size_t)bytes, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: upload failed", fn);
    if (rc == DMX_OK)
        rc = dmx_flac_decode_device(device, dIn, bytes, info, encoding, dOut, dStatus, dWork, nullptr);
    if (rc == DMX_OK && hipDeviceSynchronize() != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    if (rc == DMX_OK && (hipMemcpy(status, dStatus, 2 * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(DMX_ERR_HIP, "%s: download failed", fn);
    for (void *p : {(void *)dIn, (void *)dOut, (void *)dWork, (void *)dStatus})
        if (p)
            (void)hipFree(p);
    return rc;
}

// measurement aid (tools/flac_in_bench.py): dmx_flac_decode_device with HIP events around each of the five launches;
// ms[0..5): candidates, scan, chain, decode, finish. Synchronises the stream.
extern "C" int dmx_flac_decode_profile(int device, const void *d_file, int64_t bytes, const dmx_flac_info *info, int encoding, void *d_out,
                                       int64_t *d_status, void *d_work, void *stream, float *ms)
{
    const char *fn = "dmx_flac_decode_profile";
    DMXCHK(flac_in_check(fn, bytes, info, encoding));
    if (!d_file || !d_out || !d_status || !d_work || !ms)
        return fail(DMX_ERR_ARG, "%s: null pointer", fn);
    HIPCHK(hipSetDevice(device));
    hipEvent_t ev[6] = {};
    int rc = DMX_OK;
    for (hipEvent_t &e : ev)
        if (hipEventCreate(&e) != hipSuccess)
            rc = fail(DMX_ERR_HIP, "%s: hipEventCreate failed", fn);
    if (rc == DMX_OK && launch_flac_decode((const unsigned char *)d_file, bytes, info, encoding, d_out, (long long *)d_status, d_work,
                                           (hipStream_t)stream, ev) != 0)
        rc = fail(DMX_ERR_ARG, "%s: info rejected", fn);
    if (rc == DMX_OK && hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        rc = fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    for (int k = 0; rc == DMX_OK && k < 5; ++k)
        if (hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess)
            rc = fail(DMX_ERR_HIP, "%s: hipEventElapsedTime failed", fn);
    for (hipEvent_t e : ev)
        if (e)
            (void)hipEventDestroy(e);
    return rc;
}

// tracks given as .flac files: every file is probed before any GPU work, then the request is dmx_tracks_infer_remix's or
// dmx_tracks_infer_flac's with the tracks decoded in their slots (tracks_upload)
extern "C" int dmx_tracks_infer_from_flac(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                          const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                          const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                          float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user)
{
    const char *fn = "dmx_tracks_infer_from_flac";
    if (n_tracks < 1)
        return fail(DMX_ERR_ARG, "%s: n_tracks must be >= 1, got %d", fn, n_tracks);
    if (!files || !file_bytes || !track_status)
        return fail(DMX_ERR_ARG, "%s: null %s array", fn, !files ? "files" : !file_bytes ? "file_bytes" : "track_status");
    std::vector<dmx_flac_info> infos((size_t)n_tracks);
    std::vector<int64_t> ns((size_t)n_tracks);
    for (int t = 0; t < n_tracks; ++t)
    {
        if (!files[t])
            return fail(DMX_ERR_ARG, "%s: track %d: null file pointer", fn, t);
        char msg[160];
        if (flac_in_probe(files[t], file_bytes[t], &infos[(size_t)t], msg, sizeof msg) != 0)
            return fail(DMX_ERR_FORMAT, "%s: track %d: %s", fn, t, msg);
        if (infos[(size_t)t].sample_rate != 44100)
            return fail(DMX_ERR_ARG, "%s: track %d: sample rate %d (the track path takes 44100; decode with dmx_flac_decode and resample)", fn,
                        t, infos[(size_t)t].sample_rate);
        if (flac_in_workspace_bytes(&infos[(size_t)t], file_bytes[t]) < 0)
            return fail(DMX_ERR_FORMAT, "%s: track %d: block size range %d..%d is not supported", fn, t, infos[(size_t)t].min_block,
                        infos[(size_t)t].max_block);
        ns[(size_t)t] = infos[(size_t)t].total_samples;
    }
    TracksCall a = remix_call(fn, c, models, n_models, weights, spec);
    if (flac_out)
        a.kind = TRACKS_OUT_FLAC, a.flacRate = 44100, a.flacSizes = sizes;
    a.n_tracks = n_tracks, a.audio = reinterpret_cast<const float *const *>(files), a.n = ns.data();
    a.n_shifts = n_shifts, a.overlap = overlap, a.shift_offsets = shift_offsets;
    a.flacIn = infos.data(), a.fileBytes = file_bytes, a.trackStatus = track_status;
    a.out = out, a.peaks = peaks, a.layout = DMX_LAYOUT_EIGEN, a.progress = progress, a.user = user;
    for (int t = 0; t < 2 * n_tracks; ++t)
        track_status[t] = -1;
    DMXCHK(tracks_call(a));
    for (int t = 0; t < n_tracks; ++t)
        if (track_status[2 * t] != DMX_FLAC_OK)
            return fail(DMX_ERR_FORMAT, "%s: track %d: %s at sample %lld of %lld (the samples from there on were taken as silence)", fn, t,
                        track_status[2 * t] == DMX_FLAC_BROKEN ? "the stream breaks" : "too many frame header look-alikes, nothing decoded",
                        (long long)track_status[2 * t + 1], (long long)ns[(size_t)t]);
    return DMX_OK;
}

// --------------------------------------------------------------------------- debug
extern "C" int dmx_debug_tap(dmx_ctx *c, const char *name, int64_t *shape, float *host_dst)
{
    if (!c || !name || !shape || c->lastBatch < 1)
        return -1;
    (void)hipSetDevice(c->m->device);
    Plan *p = get_plan(c, c->lastBatch);
    for (const Op &op : p->ops)
        if (op.kind == OP_TAP && op.name == name)
        {
            int nd = 0;
            i64 per = 1;
            shape[nd++] = p->B;
            for (int j = 0; j < 4 && op.tap.shape[j] > 0; ++j)
            {
                shape[nd++] = op.tap.shape[j];
                per *= op.tap.shape[j];
            }
            if (host_dst)
            {
                (void)hipStreamSynchronize(c->stream);
                for (int b = 0; b < p->B; ++b)
                    if (hipMemcpy(host_dst + b * per, c->dA + op.tap.off + b * op.tap.batchStride, sizeof(float) * (size_t)per,
                                  hipMemcpyDeviceToHost) != hipSuccess)
                        return -1;
            }
            return nd;
        }
    return -1;
}

extern "C" int dmx_debug_n_ops(const dmx_ctx *c)
{
    if (!c)
        return 0;
    auto it = c->plans.find(c->maxBatch);
    return it == c->plans.end() ? 0 : (int)it->second->ops.size();
}

// algorithmic work of one op: 2*MAC flops, and bytes with every operand read / result written once
static void op_work(const Op &op, const char *&kernel, double &flops, double &bytes)
{
    flops = bytes = 0;
    kernel = "?";
    switch (op.kind)
    {
    case OP_IGEMM:
    {
        const IGemm &g = op.g;
        const double M = (double)g.B * g.P1 * g.P0;
        kernel = g.choice.label; // (each exact-split tile is its own roofline class; fp16 terms + the row-scale pre-pass: 2516.6 / 3)
        flops = 2.0 * M * g.N * g.K;
        double in = (double)g.B * g.L1 * g.L0 * g.Cin, w = (double)g.N * g.K, out = 0;
        if (g.epi == EPI_LINEAR || g.epi == EPI_SCALE_RES)
            out = M * g.N;
        else if (g.epi == EPI_KPL || g.epi == EPI_VT) // (algorithmic bytes stay those of the fp32 result: SURVEY 8d prices the unfused form)
            out = M * g.N;
        else if (g.epi == EPI_GLU || g.epi == EPI_GN_GLU_SCALE_RES)
            out = M * g.N / 2;
        else if (g.epi == EPI_TRCONV)
            out = (double)g.B * g.P1 * g.Lout * g.Cout;
        double res = g.res >= 0 ? out : 0;
        bytes = 4.0 * (in + w + out + res);
        break;
    }
    case OP_ATTENTION:
    {
        const Attention &t = op.at;
        kernel = t.split ? "attention_split" : "attention";
        flops = 4.0 * t.B * t.H * (double)t.Tq * t.Tk * t.hs;
        bytes = 4.0 * t.B * t.H * t.hs * (2.0 * t.Tq + 2.0 * t.Tk);
        break;
    }
    case OP_DCONV_ROW:
    {
        // the ten ops it replaces, priced as SURVEY 8d prices them (hidden width as packed: rup(hid, 4)); bytes: the row in and out
        const DconvRow &r = op.dr;
        const double M = (double)r.B * r.T * r.F, hp = (r.hid + 3) / 4 * 4;
        kernel = "dconv_row";
        flops = 2.0 * (2.0 * M * hp * 3.0 * r.C + 2.0 * M * (hp + 2) * hp + 2.0 * M * 2.0 * r.C * hp);
        bytes = 4.0 * 2.0 * M * r.C;
        break;
    }
    case OP_STATS_REDUCE:
        kernel = "stats_reduce";
        bytes = 8.0 * op.sr.B * op.sr.R * op.sr.NB;
        break;
    case OP_STFT:
        kernel = "stft";
        flops = (double)op.stft.B * op.stft.T * 5.0 * 4096 * 12;
        bytes = 4.0 * op.stft.B * ((double)op.stft.seg * 2 + (double)op.stft.T * 2048 * 4);
        break;
    case OP_LAYERNORM:
        kernel = "layernorm";
        bytes = 8.0 * op.ln.rows * op.ln.D;
        break;
    case OP_GN_APPLY:
        kernel = "gn_apply";
        bytes = 8.0 * op.gn.B * op.gn.rows * op.gn.C;
        break;
    case OP_ISTFT:
        kernel = "istft";
        if (op.istft.fused)
            break; // accounted with the fused kernel (OP_OLA)
        flops = (double)op.istft.B * op.istft.T * op.istft.S * 5.0 * 4096 * 12;
        bytes = 4.0 * op.istft.B * op.istft.T * op.istft.S * (2048.0 * 4 + 2 * 4096.0);
        break;
    case OP_OLA:
        kernel = "ola";
        bytes = 4.0 * op.ola.B * op.ola.S * 2 * ((double)op.ola.T * 4096 + 2.0 * op.ola.seg);
        if (op.ola.x >= 0) // fused execution (the default): spectrum in, time branch in, stems out; the ISTFT's flops
        {
            kernel = "istft_ola";
            flops = (double)op.ola.B * op.ola.T * op.ola.S * 5.0 * 4096 * 12;
            bytes = 4.0 * op.ola.B * ((double)op.ola.T * 2048 * 4 * op.ola.S + 4.0 * op.ola.seg * op.ola.S);
        }
        break;
    case OP_GROUP_STATS:
        kernel = "group_stats";
        bytes = 4.0 * op.gs.B * op.gs.rows * op.gs.C; // the second pass re-reads from L2
        break;
    case OP_GN_ACT:
    {
        const GnAct &g = op.ga;
        const double Co = g.mode == 2 ? g.C / 2 : g.C;
        kernel = "gn_act";
        bytes = 4.0 * g.B * ((double)g.rowsOut * g.C + (double)g.rowsOut * Co * (g.res >= 0 ? 2 : 1));
        break;
    }
    case OP_LSTM:
    {
        const Lstm &l = op.lstm;
        kernel = "lstm";
        flops = 2.0 * l.B * l.T * 2.0 * 4.0 * l.H * l.H; // recurrent matmul of both directions
        bytes = 4.0 * (l.B * (double)l.T * 10.0 * l.H + 8.0 * l.H * l.H);
        break;
    }
    case OP_LOCAL_ATTN:
    {
        const LocalAttn &l = op.la;
        kernel = "local_attn";
        flops = 4.0 * l.B * (double)l.T * l.T * l.H; // scores + weighted content over 4 heads of H/4
        bytes = 4.0 * l.B * l.T * ((double)l.ld + l.H);
        break;
    }
    default:
        break;
    }
}

// Times every op of the plan with HIP events on the context's stream: `reps` back-to-back
// launches per op between one event pair. Report: one line per op
//   name \t kernel \t ms_per_launch \t algorithmic_flops \t algorithmic_bytes
// Leaves the arena in an undefined state (in-place ops are repeated).
extern "C" int dmx_debug_profile(dmx_ctx *c, int batch, int reps, char *report, int report_cap)
{
    if (!c || batch < 1 || batch > c->maxBatch || reps < 1)
        return -1;
    (void)hipSetDevice(c->m->device);
    Plan *p = get_plan(c, batch);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
        return -1;
    int n = 0;
    std::string all;
    char line[512];
    for (const Op &op : p->ops)
    {
        if (op.kind == OP_TAP)
            continue;
        launch_op(c, op, c->stream, p->zeroOff); // warm
        (void)hipEventRecord(e0, c->stream);
        for (int r = 0; r < reps; ++r)
            launch_op(c, op, c->stream, p->zeroOff);
        (void)hipEventRecord(e1, c->stream);
        (void)hipEventSynchronize(e1);
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e0, e1);
        const char *kernel;
        double fl, by;
        op_work(op, kernel, fl, by);
        char geom[160] = "";
        if (op.kind == OP_IGEMM)
        {
            const IGemm &g = op.g;
            const i64 M = (i64)g.B * g.P1 * g.P0;
            const i64 tiles = ((M + kTileCfgs[g.cfg].BM - 1) / kTileCfgs[g.cfg].BM) * g.NB;
            snprintf(geom, sizeof(geom), "M=%lld N=%d K=%d tiles=%lld pro=%d epi=%d lin=%d stat=%d s%d", (long long)M, g.N, g.K, (long long)tiles,
                     g.pro, g.epi, (int)(g.S1 == 1 && g.pad0 == 0 && g.seg0 == g.K), (int)(g.rowstat >= 0), op.stream);
        }
        else
            snprintf(geom, sizeof(geom), "s%d", op.stream);
        snprintf(line, sizeof(line), "%s\t%s\t%.6f\t%.6e\t%.6e\t%s\n", op.name.c_str(), kernel, t / reps, fl, by, geom);
        all += line;
        ++n;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (report && report_cap > 0)
    {
        size_t k = std::min((size_t)report_cap - 1, all.size());
        std::memcpy(report, all.data(), k);
        report[k] = 0;
    }
    return n;
}

// --------------------------------------------------------------------------- one op at a time (tests/test_gpu_op_parity.py)
// The entry points below act on the context's own plan for `batch` and launch through launch_op on the context's stream, one op
// per call, each followed by a checked synchronisation: a kernel can be put next to its specification (tests/cpu_interp.cpp
// interp_step) on inputs the caller wrote into the arena.
static const Op *debug_op(dmx_ctx *c, int batch, int i, Plan **plan)
{
    if (!c || batch < 1 || batch > c->maxBatch)
        return nullptr;
    (void)hipSetDevice(c->m->device);
    Plan *p = get_plan(c, batch);
    if (i < 0 || i >= (int)p->ops.size())
        return nullptr;
    *plan = p;
    return &p->ops[(size_t)i];
}
static bool debug_launches(const dmx_ctx *c, const Op &op)
{
    return op.kind != OP_TAP && !(op.kind == OP_ISTFT && op.istft.fused && c->fuseIstft);
}
static int debug_copy_out(const std::string &all, char *buf, int cap)
{
    if (!buf || (int)all.size() + 1 > cap)
        return -1;
    std::memcpy(buf, all.c_str(), all.size() + 1);
    return (int)all.size();
}

extern "C" int dmx_debug_plan_info(dmx_ctx *c, int batch, int *n_ops, int64_t *arena_floats, int64_t *plan_floats, int64_t *const_floats)
{
    if (!c || batch < 1 || batch > c->maxBatch)
        return fail(DMX_ERR_ARG, "dmx_debug_plan_info: bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    Plan *p = get_plan(c, batch);
    if (n_ops)
        *n_ops = (int)p->ops.size();
    if (arena_floats)
        *arena_floats = c->arenaFloats;
    if (plan_floats)
        *plan_floats = p->arenaFloats;
    if (const_floats)
        *const_floats = (int64_t)p->constants.size();
    return DMX_OK;
}

extern "C" int dmx_debug_op_info(dmx_ctx *c, int batch, int i, char *buf, int cap)
{
    Plan *p = nullptr;
    const Op *opp = debug_op(c, batch, i, &p);
    if (!opp)
        return -1;
    const Op &op = *opp;
    const std::string all = describe_op(op) + " launches=" + std::to_string(debug_launches(c, op) ? 1 : 0);
    return debug_copy_out(all, buf, cap);
}

extern "C" int dmx_debug_arena_fill(dmx_ctx *c, int batch, unsigned pattern)
{
    if (!c || batch < 1 || batch > c->maxBatch)
        return fail(DMX_ERR_ARG, "dmx_debug_arena_fill: bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    Plan *p = get_plan(c, batch);
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->dA, (int)pattern, (size_t)c->arenaFloats, c->stream));
    HIPCHK(hipMemcpyAsync(c->dA, p->constants.data(), p->constants.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return dmx_ctx_sync_checked(c);
}

extern "C" int dmx_debug_arena_io(dmx_ctx *c, int64_t off, int64_t n, float *host, int write)
{
    if (!c || !host || off < 0 || n < 0 || off + n > c->arenaFloats)
        return fail(DMX_ERR_ARG, "dmx_debug_arena_io: range outside the arena");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (write)
        HIPCHK(hipMemcpy(c->dA + off, host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    else
        HIPCHK(hipMemcpy(host, c->dA + off, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return DMX_OK;
}

extern "C" int dmx_debug_run_op(dmx_ctx *c, int batch, int i)
{
    Plan *p = nullptr;
    const Op *op = debug_op(c, batch, i, &p);
    if (!op)
        return fail(DMX_ERR_ARG, "dmx_debug_run_op: no such op");
    DMXCHK(launch_op(c, *op, c->stream, p->zeroOff));
    return dmx_ctx_sync_checked(c);
}

// the tile cfgs op i can be asked to run on: the chain choose_cfg -> half_cfg -> ... of its shape, and cfg 19 / 20 where their
// shape conditions hold (fp32 contexts: plan.cpp finish); returns the count, -1 if op i is no OP_IGEMM of the plan
extern "C" int dmx_debug_op_cfgs(dmx_ctx *c, int batch, int i, int *cfgs, int cap)
{
    Plan *p = nullptr;
    const Op *op = debug_op(c, batch, i, &p);
    if (!op || op->kind != OP_IGEMM || !cfgs)
        return -1;
    const IGemm &g = op->g;
    const bool paired = g.epi == EPI_GLU || g.epi == EPI_GN_GLU_SCALE_RES;
    int n = 0;
    for (int cfg = choose_cfg((i64)g.P1 * g.P0, g.N, paired); cfg >= 0 && n < cap; cfg = half_cfg(cfg, g.rowstat >= 0))
        cfgs[n++] = cfg;
    if (c->gemm == DMX_GEMM_F32 && lin256_shape(g) && n < cap)
        cfgs[n++] = 19;
    if (c->gemm == DMX_GEMM_F32 && shortk_shape(g) && kTileCfgs[g.cfg].BN == 96 && n < cap)
        cfgs[n++] = 20;
    return n;
}

// Runs a COPY of OP_IGEMM i on tile cfg `cfg`: NB from the tile, the kernel select_gemm gives for the context's GEMM mode, the
// model's facts and lin_mode (gemm_select.h). The copy passes the per-op checks of validate_plan; DMX_DEBUG_NO_KERNEL (nothing
// launched) where they fail, where the tile is not one of the op's (dmx_debug_op_cfgs), where an op with row statistics would
// change the layout of its partials (another column block width, unless one block covers the row in both), or where a K / V plane
// projection would lose its exact-split kernel. `choice` receives the copy's
// "cfg= family= arith= wnf= label= BM= BN= NB=".
extern "C" int dmx_debug_run_op_as(dmx_ctx *c, int batch, int i, int cfg, int lin_mode, char *choice, int cap)
{
    Plan *p = nullptr;
    const Op *src = debug_op(c, batch, i, &p);
    if (!src || src->kind != OP_IGEMM)
        return fail(DMX_ERR_ARG, "dmx_debug_run_op_as: op %d is no OP_IGEMM of the plan", i);
    int cfgs[16];
    const int nc = dmx_debug_op_cfgs(c, batch, i, cfgs, 16);
    if (cfg != src->g.cfg && std::find(cfgs, cfgs + nc, cfg) == cfgs + nc)
        return fail(DMX_DEBUG_NO_KERNEL, "op %s: tile cfg %d is not one of its shape's", src->name.c_str(), cfg);
    Op op = *src;
    IGemm &g = op.g;
    // row statistics are [M][NB][2] partials per column block: a tile of another block width keeps the layout (and the op's write
    // range) only where both cover the row with ONE block
    const int nbNew = (g.N + kTileCfgs[cfg].BN - 1) / kTileCfgs[cfg].BN;
    if (g.rowstat >= 0 && kTileCfgs[cfg].BN != kTileCfgs[g.cfg].BN && !(nbNew == 1 && g.NB == 1))
        return fail(DMX_DEBUG_NO_KERNEL, "op %s: row statistics in column blocks of %d, tile cfg %d has %d", op.name.c_str(), kTileCfgs[g.cfg].BN, cfg,
                    kTileCfgs[cfg].BN);
    g.cfg = cfg;
    g.NB = (g.N + kTileCfgs[cfg].BN - 1) / kTileCfgs[cfg].BN;
    g.choice = select_gemm(g, c->gemm, model_facts(c->m), lin_mode);
    std::string why;
    if (g.choice.family == GF_NONE || !validate_gemm(op, why))
        return fail(DMX_DEBUG_NO_KERNEL, "%s", why.c_str());
    if (choice && debug_copy_out(describe_choice(g), choice, cap) < 0)
        return fail(DMX_ERR_ARG, "dmx_debug_run_op_as: choice buffer too small");
    DMXCHK(launch_op(c, op, c->stream, p->zeroOff));
    return dmx_ctx_sync_checked(c);
}
