// debug_api.cpp — the dmx_debug_* entry points: the operand splits, taps, the per-op profile and one op at a time.
#include "api_internal.h"
#include "plan_describe.h"

#include <algorithm>
#include <cstdio>

using namespace dmx;

// pure host function (tests): the two-term weight split of the exact-split GEMM path; returns the number of inexact elements
extern "C" int64_t dmx_debug_split_weights(const float *w, int64_t n, unsigned short *w1, unsigned short *w2)
{
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i)
        bad += dmx_split_weight(w[i], w1[i], w2[i]) ? 0 : 1;
    return bad;
}

// the three planes of x as the exact-split kernels stage them: bf16 terms, or (fp16) fp16 terms at scale 2^scale_exp
static int split_activations(const char *fn, int device, const float *x, int64_t n, bool fp16, int scale_exp, unsigned short *planes)
{
    if (device < 0 || device >= dmx_device_count())
        return fail(DMX_ERR_NO_DEVICE, "%s: no such HIP device (this library has no CPU fallback)", fn);
    HIPCHK(hipSetDevice(device));
    DevScratch d;
    float *dx = (float *)d.get(sizeof(float) * (size_t)n);
    unsigned short *dp = (unsigned short *)d.get(sizeof(unsigned short) * 3 * (size_t)n);
    hipError_t e = d.ok ? hipMemcpy(dx, x, sizeof(float) * (size_t)n, hipMemcpyHostToDevice) : hipErrorOutOfMemory;
    if (e == hipSuccess)
    {
        fp16 ? launch_split3h_debug(dx, n, scale_exp, dp, nullptr) : launch_split3_debug(dx, n, dp, nullptr);
        e = hipMemcpy(planes, dp, sizeof(unsigned short) * 3 * (size_t)n, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return DMX_OK;
}
extern "C" int dmx_debug_split_activations(int device, const float *x, int64_t n, unsigned short *planes)
{
    if (!x || !planes || n < 1)
        return fail(DMX_ERR_ARG, "dmx_debug_split_activations: invalid argument");
    return split_activations("dmx_debug_split_activations", device, x, n, false, 0, planes);
}
extern "C" int dmx_debug_split_activations_fp16(int device, const float *x, int64_t n, int scale_exp, unsigned short *planes)
{
    if (!x || !planes || n < 1 || scale_exp < -126 || scale_exp > 126)
        return fail(DMX_ERR_ARG, "dmx_debug_split_activations_fp16: invalid argument");
    return split_activations("dmx_debug_split_activations_fp16", device, x, n, true, scale_exp, planes);
}

// --------------------------------------------------------------------------- debug
extern "C" int dmx_debug_tap(dmx_ctx *c, const char *name, int64_t *shape, float *host_dst)
{
    if (!c || !name || !shape || c->lastBatch < 1)
        return -1;
    (void)hipSetDevice(c->m->device);
    Plan *p = dmx_get_plan(c, c->lastBatch);
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
    Plan *p = dmx_get_plan(c, batch);
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
        dmx_launch_op(c, op, c->stream, p->zeroOff); // warm
        (void)hipEventRecord(e0, c->stream);
        for (int r = 0; r < reps; ++r)
            dmx_launch_op(c, op, c->stream, p->zeroOff);
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
// The entry points below act on the context's own plan for `batch` and launch through dmx_launch_op on the context's stream, one op
// per call, each followed by a checked synchronisation: a kernel can be put next to its specification (tests/cpu_interp.cpp
// interp_step) on inputs the caller wrote into the arena.
static const Op *debug_op(dmx_ctx *c, int batch, int i, Plan **plan)
{
    if (!c || batch < 1 || batch > c->maxBatch)
        return nullptr;
    (void)hipSetDevice(c->m->device);
    Plan *p = dmx_get_plan(c, batch);
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
    Plan *p = dmx_get_plan(c, batch);
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
    Plan *p = dmx_get_plan(c, batch);
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
    DMXCHK(dmx_launch_op(c, *op, c->stream, p->zeroOff));
    return dmx_ctx_sync_checked(c);
}

// the tile cfgs op i can be asked to run on (gemm_select.h gemm_tile_chain); returns the count, -1 if op i is no OP_IGEMM of the plan
extern "C" int dmx_debug_op_cfgs(dmx_ctx *c, int batch, int i, int *cfgs, int cap)
{
    Plan *p = nullptr;
    const Op *op = debug_op(c, batch, i, &p);
    if (!op || op->kind != OP_IGEMM || !cfgs)
        return -1;
    return gemm_tile_chain(op->g, c->gemm, cfgs, cap);
}

// Runs a COPY of OP_IGEMM i on tile cfg `cfg`: NB from the tile, the kernel select_gemm gives for the context's GEMM mode, the
// model's facts and lin_mode (gemm_select.h). The copy passes the per-op checks of dmx_validate_plan; DMX_DEBUG_NO_KERNEL (nothing
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
    g.choice = select_gemm(g, c->gemm, dmx_model_facts(c->m), lin_mode);
    std::string why;
    if (g.choice.family == GF_NONE || !dmx_validate_gemm(op, why))
        return fail(DMX_DEBUG_NO_KERNEL, "%s", why.c_str());
    if (choice && debug_copy_out(describe_choice(g), choice, cap) < 0)
        return fail(DMX_ERR_ARG, "dmx_debug_run_op_as: choice buffer too small");
    DMXCHK(dmx_launch_op(c, op, c->stream, p->zeroOff));
    return dmx_ctx_sync_checked(c);
}

// Runs a COPY of OP_ATTENTION / OP_LOCAL_ATTN i in AttentionForm `form` (attention_select.h: every form computes the same bits).
// DMX_DEBUG_NO_KERNEL, nothing launched, where the form does not exist: the paired form without operand planes, with keys that
// are no whole 64-key tiles or in an fp32 context; LocalState in anything but 64-query workgroups.
extern "C" int dmx_debug_run_attention_as(dmx_ctx *c, int batch, int i, int form)
{
    Plan *p = nullptr;
    const Op *src = debug_op(c, batch, i, &p);
    if (!src || (src->kind != OP_ATTENTION && src->kind != OP_LOCAL_ATTN))
        return fail(DMX_ERR_ARG, "dmx_debug_run_attention_as: op %d is no attention op of the plan", i);
    if (form != ATT_FORM_WG64 && form != ATT_FORM_WG128 && form != ATT_FORM_PAIR)
        return fail(DMX_ERR_ARG, "dmx_debug_run_attention_as: no such form %d", form);
    Op op = *src;
    if (op.kind == OP_LOCAL_ATTN)
    {
        if (form != ATT_FORM_WG64)
            return fail(DMX_DEBUG_NO_KERNEL, "op %s: LocalState runs on 64-query workgroups only", op.name.c_str());
    }
    else
    {
        const Attention &t = op.at;
        if (form == ATT_FORM_PAIR && !(t.split && att_pair_exists(t.Tk, t.hs, t.kpl >= 0 && t.vt >= 0)))
            return fail(DMX_DEBUG_NO_KERNEL, "op %s: no paired kernel (needs the exact-split kernel, operand planes and whole key tiles)",
                        op.name.c_str());
        op.at.form = form;
    }
    DMXCHK(dmx_launch_op(c, op, c->stream, p->zeroOff));
    return dmx_ctx_sync_checked(c);
}
