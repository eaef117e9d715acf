// exec.cpp — the plan executor: a context's plans (dmx_get_plan), the device lanes of the cooperative LSTM kernel, one op
// (dmx_launch_op), a plan on one or two streams or as a HIP graph (run_plan), and dmx_segment_infer*.
#include "api_internal.h"
#include "attention_select.h"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <fcntl.h>
#include <pthread.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace dmx;

// the geometry of an op as the kernels see it (no pointers): dmx_launch_op adds the pointers
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
GemmModelFacts dmx_model_facts(const dmx_model *m)
{
    GemmModelFacts f;
    f.bf16Planes = m->dWb != nullptr, f.fp16Plane = m->dWh != nullptr;
    f.planeDelta = (i64)m->blobFloats + 512; // (dmx_model_upload)
    f.inexactW = &m->inexactW, f.inexactH = &m->inexactH;
    return f;
}

Plan *dmx_get_plan(dmx_ctx *c, int batch)
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
    build_chosen_plan(c->m->pm, c->seg, batch, c->gemm, kvPlanes, dmx_model_facts(c->m), split_lin_mode(), *p);
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
            // the fp32 kernel (attention.hip) has the two unpaired shapes only, by the same rule
            t.form = t.split                           ? att_select_form(t.Tq, t.Tk, t.H, t.B, t.hs, t.kpl >= 0 && t.vt >= 0, pairMode)
                     : att_big_shape(t.Tq, t.H, t.B) ? ATT_FORM_WG128
                                                     : ATT_FORM_WG64;
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

// --------------------------------------------------------------------------- executor
// hipGraphLaunch / capture / instantiate are not safe to call from several host threads at once in this runtime
// (observed: SIGSEGV in hip::Graph::UpdateStreams under hipGraphLaunch when the engine's device threads replay their
// graphs concurrently - different graphs, different streams). All graph API calls of the process go through this
// mutex; a launch only enqueues (tens of microseconds), so the device threads lose no overlap.
std::mutex dmx::g_graphMutex;

int dmx_launch_op(const dmx_ctx *c, const Op &op, hipStream_t s, i64 zeroOff)
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
            DMXCHK(dmx_launch_op(c, op, c->stream, p->zeroOff));
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
        DMXCHK(dmx_launch_op(c, op, s, p->zeroOff));
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
    Plan *p = dmx_get_plan(c, batch);
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
    Plan *p = dmx_get_plan(c, batch);
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
    Plan *p = dmx_get_plan(c, 1);
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
