// plan.cpp — builds the static op list of one HTDemucs segment batch (see plan.h).
//
// The op order restates the reference graph, src/model_inference.cpp:48-475
// (/root/reference), with its sub-blocks: encoders/decoders src/encdec.cpp:8-361,
// DConv src/layers.cpp:152-375, transformer src/crosstransformer.cpp:205-339 +
// src/layers.cpp:377-531, STFT/ISTFT src/dsp.cpp:51-185. Fusions relative to the
// reference are documented per op in DESIGN.md §4.
#include "gemm_select.h"
#include <string>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

namespace dmx
{

Geo make_geo(i64 seg)
{
    // src/model.hpp:618-625 (le, pad, pad_end), :19-24 (time lengths), conv.hpp:25-29
    Geo g;
    g.seg = seg;
    g.le = (seg + 1023) / 1024;
    g.pad = 1536;
    g.pad_end = g.pad + g.le * 1024 - seg;
    g.padded = seg + g.pad + g.pad_end;
    g.nfr = g.padded / 1024 + 1;
    g.Lt[0] = seg;
    for (int i = 0; i < 4; ++i)
    {
        i64 L = g.Lt[i];
        g.Lt[i + 1] = (L - 4 + 3) / 4 + 1; // ceil((L+4-7-1)/4)+1
    }
    return g;
}

// dconv_row.hip: C = 48 / 96 with hidden C/8 (v4), C = 48 with hidden C/4 (v3)
bool dconv_row_geo(int C, int hid, DconvRowGeo &g)
{
    if (!((C == 48 && (hid == 6 || hid == 12)) || (C == 96 && hid == 12)))
        return false;
    g.HP = (hid + 3) / 4 * 4, g.RPL = g.HP / 4, g.NP = 16 * ((3 * g.RPL + 3) / 4), g.WS = C + 8;
    g.nWp = (g.NP * g.WS + 255) / 256 * 256;
    g.oW3 = 0, g.oLf = g.RPL * 2 * C * 4, g.oCst = g.oLf + g.RPL * 16 * 4;
    g.nWk = (g.oCst + 7 * C + 64 + 255) / 256 * 256;
    g.resident = C == 48;
    return true;
}
i64 dconv_row_image_floats(int C, int hid)
{
    DconvRowGeo g;
    return dconv_row_geo(C, hid, g) ? (i64)g.nWp + g.nWk : 0;
}
// at most 16 waves x 3 fragments of 16 time steps; [K1 sides | K3 sides of both layers | reduction scratch | P0, P2] within the CU's LDS
size_t dconv_row_lds_bytes(int C, int hid, int T)
{
    DconvRowGeo g;
    if (!dconv_row_geo(C, hid, g) || T < 2 || (T + 15) / 16 > 48)
        return 0;
    const size_t floats = (size_t)(g.resident ? 2 : 1) * g.nWp + 2 * (size_t)g.nWk + 128 + (size_t)2 * T * g.HP;
    const size_t bytes = floats * sizeof(float);
    return bytes <= 160 * 1024 ? bytes : 0;
}

namespace
{
struct Builder
{
    const PackedModel &pm;
    Plan &pl;
    i64 top = 0;
    i64 redScratch[2] = {-1, -1};
    PlanOpts opts;
    Builder(const PackedModel &m, Plan &p, const PlanOpts &o) : pm(m), pl(p), opts(o) { pl.gemm = o.gemm; }

    i64 alloc(i64 n)
    {
        i64 off = (top + 63) / 64 * 64;
        top = off + n;
        return off;
    }
    i64 W(const std::string &n) const { return pm.find(n); }

    IGemm base_gemm()
    {
        IGemm g;
        std::memset((void *)&g, 0, sizeof(g));
        g.S1 = 1;
        g.stride1 = 1;
        g.dil1 = 1;
        g.stride0 = 1;
        g.pro = PRO_NONE;
        g.proStats = g.proW_w = g.proB_w = -1;
        g.G0 = 1;
        g.res = g.scale_w = g.epiStats = g.epiW_w = g.epiB_w = g.rowstat = g.table_w = -1;
        g.tableScale = 0.f;
        g.NB = 1;
        g.trS = 4, g.trOff = 2;
        g.kv = -1;
        return g;
    }
    void finish(IGemm &g, bool paired, bool pin128Wide = false)
    {
        g.K = g.S1 * g.seg0;
        g.Kp = rup(g.K, 16);
        g.Np = rup(g.N, 16);
        g.xBatchStride = (i64)g.L1 * g.L0 * g.Cin;
        const TileChoice t = choose_tile(g, paired, pin128Wide, opts.gemm, opts.sw); // all tile policy: gemm_select.cpp
        g.cfg = t.cfg, g.NB = t.NB;
    }
    void push_gemm(const std::string &name, int stream, IGemm g)
    {
        Op op;
        op.kind = OP_IGEMM;
        op.stream = stream;
        op.name = name;
        op.g = g;
        pl.ops.push_back(op);
    }
    void push_reduce(const std::string &name, int stream, i64 rowstat, i64 out, int B, int R, int NB, int G0,
                     double count, int mode)
    {
        Op op;
        op.kind = OP_STATS_REDUCE;
        op.stream = stream;
        op.name = name;
        op.sr = StatsReduce{rowstat, out, B, R, NB, G0, count, mode, 1e-5f, -1, 0};
        if (G0 <= 1)
        {
            // two-stage: nchunk workgroups per batch element, then one finalising workgroup
            i64 entries = (i64)R * NB;
            int nchunk = (int)std::min<i64>(256, (entries + 2047) / 2048);
            op.sr.nchunk = std::max(nchunk, 1);
            op.sr.scratch = stream == 0 ? redScratch[0] : redScratch[1];
        }
        pl.ops.push_back(op);
    }
    void push_tap(const std::string &name, i64 off, std::initializer_list<int> shape, i64 batchStride)
    {
        Op op;
        op.kind = OP_TAP;
        op.stream = 0;
        op.name = name;
        op.tap.off = off;
        int i = 0;
        for (int j = 0; j < 4; ++j)
            op.tap.shape[j] = 0;
        for (int s : shape)
            op.tap.shape[i++] = s;
        op.tap.batchStride = batchStride;
        pl.ops.push_back(op);
    }

    // DConv residual branch, in place on y = [B][P1][P0][C]; src/layers.cpp:152-375.
    // freq branch: taps along axis 1 (T), GroupNorm groups (b, f): G0 = P0 = F.
    // time branch: view [B][L][1][C] (P0 = 1), groups b: G0 = 1.
    void dconv(const std::string &p, int stream, i64 y, int B, int P1, int P0, int C, i64 scratchH, i64 rs,
               i64 st1, i64 st2)
    {
        const int C8 = C / (pm.arch == 3 ? 4 : 8), C8p = rup(C8, 4); // hidden width: compress 8 (v4) / 4 (v3)
        const int G0 = P0 > 1 ? P0 : 1;
        const i64 rows = (i64)P1 * P0;
        // frequency branch, levels 0 / 1: the whole residual branch as ONE op with the (C, T) row of a bin resident on the CU
        // (dconv_row.hip). A function of (C, hidden width, T) alone - never of the batch. PlanOpts::dconvRow off: the op chain (A/B).
        {
            if (P0 > 1 && opts.dconvRow && dconv_row_lds_bytes(C, C8, P1) > 0 && (i64)B * P1 * P0 * C < (1ll << 31) &&
                pm.has(p + ".dconv.0.rowimg"))
            {
                Op op;
                op.kind = OP_DCONV_ROW;
                op.stream = stream;
                op.name = p + ".dconv";
                DconvRow &r = op.dr;
                r.x = y, r.B = B, r.T = P1, r.F = P0, r.C = C, r.hid = C8, r.eps = 1e-5f;
                for (int j = 0; j < 2; ++j)
                {
                    const std::string w = p + ".dconv." + std::to_string(j) + ".";
                    r.k1_w[j] = W(w + "k1.Wt"), r.k1_b[j] = W(w + "k1.b"), r.gn1_w[j] = W(w + "gn1.w"), r.gn1_b[j] = W(w + "gn1.b");
                    r.k2_w[j] = W(w + "k2.Wt"), r.k2_b[j] = W(w + "k2.b"), r.k2f_w[j] = W(w + "k2f.Wt"), r.k2f_b[j] = W(w + "k2f.b");
                    r.gn2_w[j] = W(w + "gn2.w"), r.gn2_b[j] = W(w + "gn2.b"), r.scale_w[j] = W(w + "scale");
                    r.img_w[j] = W(w + "rowimg");
                }
                pl.ops.push_back(op);
                return;
            }
        }
        for (int j = 0; j < 2; ++j)
        {
            const int d = j == 0 ? 1 : 2;
            std::string w = p + ".dconv." + std::to_string(j) + ".";
            std::string nm = p + ".dconv" + std::to_string(j);
            // K1: Conv1d(C -> C/8, k3, dilation d, padding d)  layers.cpp:161-195 / 261-302
            IGemm g = base_gemm();
            g.B = B, g.P1 = P1, g.P0 = P0;
            g.x = y, g.L1 = P1, g.L0 = P0, g.Cin = C;
            g.S1 = 3, g.dil1 = d, g.pad1 = d;
            g.seg0 = C, g.pad0 = 0;
            g.w_w = W(w + "k1.Wt"), g.bias_w = W(w + "k1.b");
            g.N = C8p;
            g.epi = EPI_LINEAR, g.act = 0;
            g.y = scratchH, g.ldy = C8p, g.yBatchStride = rows * C8p;
            g.rowstat = rs;
            finish(g, false);
            push_gemm(nm + ".k1", stream, g);
            // GroupNorm(1, C/8) statistics  layers.cpp:197-202 / 304-309
            push_reduce(nm + ".r1", stream, rs, st1, B, (int)rows, g.NB, G0, (double)C8 * P1 * (G0 > 1 ? 1 : P0), MODE_RSTD);
            // K2: [GN+GELU prologue] Conv1d(C/8 -> 2C, 1x1): statistics only  layers.cpp:204-245
            IGemm h = base_gemm();
            h.B = B, h.P1 = P1, h.P0 = P0;
            h.x = scratchH, h.L1 = P1, h.L0 = P0, h.Cin = C8p;
            h.seg0 = C8p;
            h.pro = PRO_GN_GELU, h.proStats = st1, h.proW_w = W(w + "gn1.w"), h.proB_w = W(w + "gn1.b");
            h.G0 = G0;
            h.w_w = W(w + "k2.Wt"), h.bias_w = W(w + "k2.b");
            h.N = 2 * C;
            h.epi = EPI_STATS_ONLY;
            h.y = -1, h.ldy = 0;
            h.rowstat = rs;
            {
                // statistics through the factorised weights (EPI_STATS_FACT): C/8 + 2 columns instead of 2C
                IGemm f = h;
                f.w_w = W(w + "k2f.Wt"), f.bias_w = W(w + "k2f.b");
                f.N = C8p + 2, f.Cout = C8p;
                f.epi = EPI_STATS_FACT;
                finish(f, false);
                push_gemm(nm + ".k2", stream, f);
            }
            push_reduce(nm + ".r2", stream, rs, st2, B, (int)rows, 1, G0, (double)2 * C * P1 * (G0 > 1 ? 1 : P0), MODE_RSTD);
            // K3: recompute, GroupNorm(1,2C) + GLU + LayerScale + residual  layers.cpp:240-253 / 348-374
            IGemm k = h;
            k.epi = EPI_GN_GLU_SCALE_RES;
            k.epiStats = st2, k.epiW_w = W(w + "gn2.w"), k.epiB_w = W(w + "gn2.b");
            k.scale_w = W(w + "scale");
            k.res = y, k.y = y, k.ldy = C, k.yBatchStride = rows * C;
            finish(k, true); // (the tile of the full product with row statistics, as when K2 computed them unfactorised: the sibling chain)
            k.rowstat = -1;
            push_gemm(nm + ".k3", stream, k);
        }
    }
};
} // namespace

void build_plan(const PackedModel &pm, i64 seg, int B, Plan &pl, const PlanOpts &opts)
{
    if (pm.arch == 3)
    {
        build_plan_v3(pm, seg, B, pl, opts);
        return;
    }
    Builder b(pm, pl, opts);
    pl.B = B;
    pl.geo = make_geo(seg);
    pl.S = pm.n_sources;
    pl.D = pm.dim;
    const Geo &G = pl.geo;
    const int T = (int)G.le, S = pl.S, D = pl.D, FF = 4 * D;
    const int ch[4] = {48, 96, 192, 384};
    const int Fl[5] = {2048, 512, 128, 32, 8};
    const int tokF = T * 8, tokT = (int)G.Lt[4];
    const bool is4 = S == 4;

    // ------------------------------------------------------------------ constants
    // Hann window: periodic, PI literal and float math of src/dsp.hpp:59-75
    pl.zeroOff = b.alloc(64);
    const i64 cWindow = b.alloc(4096);
    const i64 cTwiddle = b.alloc(2 * 2048);
    const int nfr = T + 4;
    const i64 wssLen = 4096 + 1024 * (i64)(nfr - 1);
    const i64 cWss = b.alloc(wssLen);
    const i64 cRden = b.alloc(wssLen);
    const i64 cPe2 = b.alloc((i64)tokF * D);
    const i64 cPe1 = b.alloc((i64)tokT * D);
    pl.constants.assign((size_t)b.top, 0.0f);
    {
        float *win = &pl.constants[(size_t)cWindow];
        static constexpr float PI = 3.14159265359F;
        float floatN = (float)(4096 + 1);
        for (int n = 0; n < 4096; ++n)
            win[n] = 0.5F * (1.0F - cosf(2.0F * PI * (float)n / (floatN - 1)));
        float *tw = &pl.constants[(size_t)cTwiddle];
        for (int k = 0; k < 2048; ++k)
        {
            double a = -2.0 * M_PI * (double)k / 4096.0;
            tw[2 * k] = (float)cos(a);
            tw[2 * k + 1] = (float)sin(a);
        }
        // window sum-square over all T+4 frames, float accumulation in frame order: dsp.hpp:77-100
        float *wss = &pl.constants[(size_t)cWss];
        for (int i = 0; i < nfr; ++i)
            for (int j = 0; j < 4096; ++j)
                wss[(i64)i * 1024 + j] += win[j] * win[j];
        float *rden = &pl.constants[(size_t)cRden];
        for (i64 n = 0; n < wssLen; ++n)
            rden[n] = (1.0f / 4096.0f) / (wss[n] + 1e-8f);
        // 2-D sinusoidal embedding on tokens (t*8+f): crosstransformer.cpp:7-53,227-238
        float *pe2 = &pl.constants[(size_t)cPe2];
        {
            int dm = D / 2;
            std::vector<float> div((size_t)(dm / 2));
            for (int j = 0; j < dm / 2; ++j)
                div[(size_t)j] = std::exp((float)(2 * j) * (-std::log(10000.0f) / (float)dm));
            for (int t = 0; t < T; ++t)
                for (int f = 0; f < 8; ++f)
                {
                    float *row = pe2 + ((i64)t * 8 + f) * D;
                    for (int j = 0; j < dm / 2; ++j)
                    {
                        float vw = (float)t * div[(size_t)j]; // width axis = time
                        float vh = (float)f * div[(size_t)j]; // height axis = freq
                        row[2 * j] = std::sin(vw);
                        row[2 * j + 1] = std::cos(vw);
                        row[dm + 2 * j] = std::sin(vh);
                        row[dm + 2 * j + 1] = std::cos(vh);
                    }
                }
        }
        // 1-D embedding: crosstransformer.cpp:55-77
        float *pe1 = &pl.constants[(size_t)cPe1];
        {
            int half = D / 2;
            for (int t = 0; t < tokT; ++t)
                for (int i = 0; i < half; ++i)
                {
                    float divt = (float)i / (float)(half - 1);
                    float phase = (float)t / std::pow(10000.0f, divt);
                    pe1[(i64)t * D + i] = std::cos(phase);
                    pe1[(i64)t * D + i + half] = std::sin(phase);
                }
        }
    }

    // ------------------------------------------------------------------ activations
    pl.mixOff = b.alloc((i64)B * seg * 2);
    pl.outOff = b.alloc((i64)B * S * 2 * seg);
    const i64 aXcac = b.alloc((i64)B * T * 2048 * 4);
    const i64 aRsX = b.alloc((i64)B * T * 2), aRsT = b.alloc((i64)B * T * 2);
    const i64 aStF = b.alloc((i64)B * 4), aStT = b.alloc((i64)B * 4);
    b.redScratch[0] = b.alloc((i64)B * 256 * 4);
    b.redScratch[1] = b.alloc((i64)B * 256 * 4);
    i64 aY[4], aX[4], aYt[4], aXt[4]; // conv outputs (dconv in place), saved skips
    for (int i = 0; i < 4; ++i)
    {
        aY[i] = b.alloc((i64)B * T * Fl[i + 1] * ch[i]);
        aX[i] = b.alloc((i64)B * T * Fl[i + 1] * ch[i]);
        aYt[i] = b.alloc((i64)B * G.Lt[i + 1] * ch[i]);
        aXt[i] = b.alloc((i64)B * G.Lt[i + 1] * ch[i]);
    }
    // dconv scratch, sized for the largest level of each branch
    i64 maxRowsF = 0, maxHF = 0, maxRowsT = 0, maxHT = 0;
    for (int i = 0; i < 4; ++i)
    {
        i64 rf = (i64)B * T * Fl[i + 1], rt = (i64)B * G.Lt[i + 1];
        maxRowsF = std::max(maxRowsF, rf);
        maxRowsT = std::max(maxRowsT, rt);
        maxHF = std::max(maxHF, rf * rup(ch[i] / 8, 4));
        maxHT = std::max(maxHT, rt * rup(ch[i] / 8, 4));
    }
    const int kMaxNB = 16;
    const i64 aHf = b.alloc(maxHF), aHt = b.alloc(maxHT);
    const i64 aRsF = b.alloc(std::max(maxRowsF, (i64)B * tokF) * kMaxNB * 2);
    const i64 aRsTt = b.alloc(std::max(maxRowsT, (i64)B * tokT) * kMaxNB * 2);
    const i64 aSt1F = b.alloc((i64)B * 512 * 4), aSt2F = b.alloc((i64)B * 512 * 4);
    const i64 aSt1T = b.alloc((i64)B * 4), aSt2T = b.alloc((i64)B * 4);
    // transformer
    const i64 aQf = b.alloc((i64)B * tokF * D), aQt = b.alloc((i64)B * tokT * D); // token streams x, xt
    const i64 aNf = b.alloc((i64)B * tokF * D), aNt = b.alloc((i64)B * tokT * D); // LN outputs
    const i64 aN2f = b.alloc((i64)B * tokT * D), aN2t = b.alloc((i64)B * tokF * D); // LN of the other branch (cross)
    const i64 aQKVf = b.alloc((i64)B * tokF * 3 * D), aQKVt = b.alloc((i64)B * tokT * 3 * D);
    const i64 aKVf = b.alloc((i64)B * tokT * 2 * D), aKVt = b.alloc((i64)B * tokF * 2 * D);
    const i64 aAttF = b.alloc((i64)B * tokF * D), aAttT = b.alloc((i64)B * tokT * D);
    // bf16 operand planes of K and V^T per branch (plane_linear below): three planes of B x tokens x D elements = 1.5 floats each
    const bool planesOn = opts.kvPlanes && opts.gemm != GEMM_F32 && (D / 8 == 64 || D / 8 == 48) && D % 128 == 0;
    const i64 planeFloats = ((i64)B * std::max(tokF, tokT) * D * 3 + 1) / 2;
    const i64 aKplF = planesOn ? b.alloc(planeFloats) : -1, aVtF = planesOn ? b.alloc(planeFloats) : -1;
    const i64 aKplT = planesOn ? b.alloc(planeFloats) : -1, aVtT = planesOn ? b.alloc(planeFloats) : -1;
    const i64 aHidF = b.alloc((i64)B * tokF * FF), aHidT = b.alloc((i64)B * tokT * FF);
    const i64 aStNf = b.alloc((i64)B * 4), aStNt = b.alloc((i64)B * 4);
    // decoders
    i64 aDin[5], aG[4], aTDin[5], aTG[4];
    for (int k = 0; k < 4; ++k)
    {
        int Cd = ch[3 - k];
        aDin[k] = b.alloc((i64)B * T * Fl[4 - k] * Cd);
        aG[k] = b.alloc((i64)B * T * Fl[4 - k] * Cd);
        aTDin[k] = b.alloc((i64)B * G.Lt[4 - k] * Cd);
        aTG[k] = b.alloc((i64)B * G.Lt[4 - k] * Cd);
    }
    aDin[4] = b.alloc((i64)B * T * 2048 * 4 * S);  // x_out
    aTDin[4] = b.alloc((i64)B * seg * 2 * S);      // xt_out
    const i64 aFrames = b.alloc((i64)B * S * 2 * T * 4096);
    pl.arenaFloats = b.top + 64;

    // ------------------------------------------------------------------ ops
    // STFT + CaC + statistics; model_inference.cpp:64-124, dsp.cpp:51-149
    {
        Op op;
        op.kind = OP_STFT;
        op.stream = 0;
        op.name = "stft";
        // the same op also emits per-hop (sum, sumsq) of the raw mix (time-branch z-norm)
        op.stft = Stft{pl.mixOff, aXcac, aRsX, aRsT, B, T, (int)seg, (int)G.pad, cWindow, cTwiddle};
        pl.ops.push_back(op);
    }
    b.push_reduce("znorm.freq", 0, aRsX, aStF, B, T, 1, 1, (double)4 * 2048 * T, MODE_ZNORM);
    b.push_reduce("znorm.time", 1, aRsT, aStT, B, T, 1, 1, (double)2 * seg, MODE_ZNORM);
    b.push_tap("x_cac", aXcac, {T, 2048, 4}, (i64)T * 2048 * 4);

    for (int i = 0; i < 4; ++i)
    {
        const int C = ch[i], Fin = Fl[i], Fo = Fl[i + 1];
        const int cinF = i == 0 ? 4 : ch[i - 1], cinT = i == 0 ? 2 : ch[i - 1];
        const i64 Lin = G.Lt[i], Lo = G.Lt[i + 1];
        std::string pe = "encoder." + std::to_string(i), pt = "tencoder." + std::to_string(i);
        // ---- time encoder (encdec.cpp:82-164)
        {
            IGemm g = b.base_gemm();
            g.B = B, g.P1 = 1, g.P0 = (int)Lo;
            g.x = i == 0 ? pl.mixOff : aXt[i - 1];
            g.L1 = 1, g.L0 = (int)Lin, g.Cin = cinT;
            g.seg0 = 8 * cinT, g.stride0 = 4, g.pad0 = 2;
            if (i == 0)
                g.pro = PRO_AFFINE, g.proStats = aStT;
            g.w_w = b.W(pt + ".conv.Wt"), g.bias_w = b.W(pt + ".conv.b");
            g.N = C;
            g.epi = EPI_LINEAR, g.act = 1;
            g.y = aYt[i], g.ldy = C, g.yBatchStride = Lo * C;
            b.finish(g, false);
            b.push_gemm(pt + ".conv", 1, g);
            b.dconv(pt, 1, aYt[i], B, (int)Lo, 1, C, aHt, aRsTt, aSt1T, aSt2T);
            IGemm r = b.base_gemm();
            r.B = B, r.P1 = (int)Lo, r.P0 = 1;
            r.x = aYt[i], r.L1 = (int)Lo, r.L0 = 1, r.Cin = C;
            r.seg0 = C;
            r.w_w = b.W(pt + ".rewrite.Wt"), r.bias_w = b.W(pt + ".rewrite.b");
            r.N = 2 * C;
            r.epi = EPI_GLU;
            r.y = aXt[i], r.ldy = C, r.yBatchStride = Lo * C;
            b.finish(r, true);
            b.push_gemm(pt + ".rewrite", 1, r);
        }
        // ---- freq encoder (encdec.cpp:8-80)
        {
            IGemm g = b.base_gemm();
            g.B = B, g.P1 = T, g.P0 = Fo;
            g.x = i == 0 ? aXcac : aX[i - 1];
            g.L1 = T, g.L0 = Fin, g.Cin = cinF;
            g.seg0 = 8 * cinF, g.stride0 = 4, g.pad0 = 2;
            if (i == 0)
                g.pro = PRO_AFFINE, g.proStats = aStF;
            g.w_w = b.W(pe + ".conv.Wt"), g.bias_w = b.W(pe + ".conv.b");
            g.N = C;
            g.epi = EPI_LINEAR, g.act = 1;
            g.y = aY[i], g.ldy = C, g.yBatchStride = (i64)T * Fo * C;
            b.finish(g, false);
            b.push_gemm(pe + ".conv", 0, g);
            b.dconv(pe, 0, aY[i], B, T, Fo, C, aHf, aRsF, aSt1F, aSt2F);
            IGemm r = b.base_gemm();
            r.B = B, r.P1 = T, r.P0 = Fo;
            r.x = aY[i], r.L1 = T, r.L0 = Fo, r.Cin = C;
            r.seg0 = C;
            r.w_w = b.W(pe + ".rewrite.Wt"), r.bias_w = b.W(pe + ".rewrite.b");
            r.N = 2 * C;
            r.epi = EPI_GLU;
            if (i == 0)
                r.table_w = b.W("freq_emb.table"), r.tableScale = 10.0f * 0.2f; // model_inference.cpp:163-179
            r.y = aX[i], r.ldy = C, r.yBatchStride = (i64)T * Fo * C;
            b.finish(r, true);
            b.push_gemm(pe + ".rewrite", 0, r);
        }
        b.push_tap("x_" + std::to_string(i), aX[i], {T, Fo, C}, (i64)T * Fo * C);
        b.push_tap("xt_" + std::to_string(i), aXt[i], {(int)Lo, C}, Lo * C);
    }

    // ------------------------------------------------------------------ transformer
    auto linear = [&](const std::string &name, int stream, i64 x, int rows, int K, i64 w, i64 bias, int N, i64 y,
                      int ldy, int epi, int act, i64 res, i64 scale, i64 rowstat) {
        IGemm g = b.base_gemm();
        g.B = B, g.P1 = rows, g.P0 = 1;
        g.x = x, g.L1 = rows, g.L0 = 1, g.Cin = K;
        g.seg0 = K;
        g.w_w = w, g.bias_w = bias, g.N = N;
        g.epi = epi, g.act = act;
        g.y = y, g.ldy = ldy, g.yBatchStride = (i64)rows * ldy;
        g.res = res, g.scale_w = scale, g.rowstat = rowstat;
        // GEMM_FP16X3: the fp16-term arithmetic exists on the linear-layer kernel only (128- / 64-row tiles of the 128-wide
        // family); an op must take ONE arithmetic at every batch size (batch = singles bitwise), so the quarter-height sibling
        // (a staged kernel, bf16 terms) is not offered to it
        g.hterms = opts.gemm == GEMM_FP16X3 && N % 128 == 0 && K % 32 == 0 ? 1 : 0;
        b.finish(g, false, g.hterms != 0);
        b.push_gemm(name, stream, g);
    };
    auto layernorm = [&](const std::string &name, int stream, i64 x, i64 y, int rows, const std::string &w,
                         const std::string &bs, i64 pe) {
        Op op;
        op.kind = OP_LAYERNORM;
        op.stream = stream;
        op.name = name;
        op.ln = LayerNorm{x, y, B * rows, D, rows, b.W(w), b.W(bs), pe, 1e-5f};
        pl.ops.push_back(op);
    };
    auto attention = [&](const std::string &name, int stream, i64 q, int ldq, i64 qB, i64 k, i64 v, int ldkv, i64 kvB,
                         i64 o, int Tq, int Tk, i64 kpl = -1, i64 vt = -1) {
        Op op;
        op.kind = OP_ATTENTION;
        op.stream = stream;
        op.name = name;
        int hs = D / 8;
        op.at = Attention{q, k, v, o, ldq, ldkv, ldkv, D, qB, kvB, kvB, (i64)Tq * D, B, Tq, Tk, 8, hs,
                          1.0f / std::sqrt((float)hs)};
        op.at.kpl = kpl, op.at.vt = vt;
        pl.ops.push_back(op);
    };
    // K / V projections that leave the attention kernel's bf16 operand planes (GEMM_BF16X3 plans, PlanOpts::kvPlanes): the
    // key / value tokens of a layer must be whole 64-key tiles (full-size segments: 2688 and 1344), head dim 64 or 48. Such an op
    // always runs on igemm_split_lin_kernel (128- or 64-row tiles, whatever the batch: the V^T form issues its MFMAs with the
    // operands the other way round, which only that kernel implements - one kernel family per op keeps batch = singles bitwise)
    auto planes_ok = [&](int tokSrc) { return planesOn && tokSrc % 64 == 0; };
    auto plane_linear = [&](const std::string &name, int stream, i64 x, int rows, i64 w, i64 bias, int N, i64 y, int ldy, int epi, i64 kv,
                            int kvCol0) {
        IGemm g = b.base_gemm();
        g.B = B, g.P1 = rows, g.P0 = 1;
        g.x = x, g.L1 = rows, g.L0 = 1, g.Cin = D;
        g.seg0 = D;
        g.w_w = w, g.bias_w = bias, g.N = N;
        g.epi = epi, g.act = 0;
        g.y = y, g.ldy = ldy, g.yBatchStride = (i64)rows * ldy;
        g.kv = kv, g.kvCol0 = kvCol0, g.kvT = rows, g.kvH = 8, g.kvHs = D / 8;
        b.finish(g, false, true);
        g.hterms = opts.gemm == GEMM_FP16X3 ? 1 : 0;
        b.push_gemm(name, stream, g);
    };


    // channel upsamplers (4s) + norm_in + positional embeddings; model_inference.cpp:214-252,
    // crosstransformer.cpp:205-263
    if (is4)
    {
        linear("channel_upsampler", 0, aX[3], tokF, 384, b.W("channel_upsampler.Wt"), b.W("channel_upsampler.b"), 512,
               aNf, 512, EPI_LINEAR, 0, -1, -1, -1);
        linear("channel_upsampler_t", 1, aXt[3], tokT, 384, b.W("channel_upsampler_t.Wt"), b.W("channel_upsampler_t.b"),
               512, aNt, 512, EPI_LINEAR, 0, -1, -1, -1);
        b.push_tap("x_3_up", aNf, {tokF, D}, (i64)tokF * D);
        layernorm("norm_in", 0, aNf, aQf, tokF, "crosstransformer.norm_in.w", "crosstransformer.norm_in.b", cPe2);
        layernorm("norm_in_t", 1, aNt, aQt, tokT, "crosstransformer.norm_in_t.w", "crosstransformer.norm_in_t.b", cPe1);
    }
    else
    {
        layernorm("norm_in", 0, aX[3], aQf, tokF, "crosstransformer.norm_in.w", "crosstransformer.norm_in.b", cPe2);
        layernorm("norm_in_t", 1, aXt[3], aQt, tokT, "crosstransformer.norm_in_t.w", "crosstransformer.norm_in_t.b", cPe1);
    }
    b.push_tap("ct_in_x", aQf, {tokF, D}, (i64)tokF * D);
    b.push_tap("ct_in_xt", aQt, {tokT, D}, (i64)tokT * D);

    for (int layer = 0; layer < 5; ++layer)
    {
        const bool self = layer % 2 == 0;
        std::string pf = "crosstransformer.layers." + std::to_string(layer);
        std::string ptn = "crosstransformer.layers_t." + std::to_string(layer);
        struct Br
        {
            std::string p;
            int stream;
            i64 x, n, n2, qkv, kv, att, hid, stn, rs;
            int tok, tokOther;
            i64 xOther, kpl, vt;
        };
        Br br[2] = {{pf, 0, aQf, aNf, aN2f, aQKVf, aKVf, aAttF, aHidF, aStNf, aRsF, tokF, tokT, aQt, aKplF, aVtF},
                    {ptn, 1, aQt, aNt, aN2t, aQKVt, aKVt, aAttT, aHidT, aStNt, aRsTt, tokT, tokF, aQf, aKplT, aVtT}};
        // phase 1: norms + projections (cross layers read the OTHER branch before it is
        // updated: "old_x" of crosstransformer.cpp:286-295)
        for (auto &r : br)
        {
            layernorm(r.p + ".norm1", r.stream, r.x, r.n, r.tok, r.p + ".norm1.w", r.p + ".norm1.b", -1);
            if (self && planes_ok(r.tok))
            {
                // q (fp32, columns [0, D) of the [tok][3D] buffer) and the K planes in one launch, the V^T planes in a second
                plane_linear(r.p + ".qk", r.stream, r.n, r.tok, b.W(r.p + ".in_proj.Wt"), b.W(r.p + ".in_proj.b"), 2 * D, r.qkv, 3 * D,
                             EPI_KPL, r.kpl, D);
                plane_linear(r.p + ".v", r.stream, r.n, r.tok, b.W(r.p + ".in_proj.Wt") + (i64)2 * D * D, b.W(r.p + ".in_proj.b") + 2 * D, D,
                             r.qkv, 3 * D, EPI_VT, r.vt, 0);
            }
            else if (self)
                linear(r.p + ".qkv", r.stream, r.n, r.tok, D, b.W(r.p + ".in_proj.Wt"), b.W(r.p + ".in_proj.b"), 3 * D,
                       r.qkv, 3 * D, EPI_LINEAR, 0, -1, -1, -1);
            else
            {
                layernorm(r.p + ".norm2", r.stream, r.xOther, r.n2, r.tokOther, r.p + ".norm2.w", r.p + ".norm2.b", -1);
                linear(r.p + ".q", r.stream, r.n, r.tok, D, b.W(r.p + ".in_proj.Wt"), b.W(r.p + ".in_proj.b"), D, r.qkv, D,
                       EPI_LINEAR, 0, -1, -1, -1);
                if (planes_ok(r.tokOther))
                {
                    plane_linear(r.p + ".k", r.stream, r.n2, r.tokOther, b.W(r.p + ".in_proj.Wt") + (i64)D * D, b.W(r.p + ".in_proj.b") + D, D,
                                 r.kv, 2 * D, EPI_KPL, r.kpl, 0);
                    plane_linear(r.p + ".v", r.stream, r.n2, r.tokOther, b.W(r.p + ".in_proj.Wt") + (i64)2 * D * D,
                                 b.W(r.p + ".in_proj.b") + 2 * D, D, r.kv, 2 * D, EPI_VT, r.vt, 0);
                }
                else
                    linear(r.p + ".kv", r.stream, r.n2, r.tokOther, D, b.W(r.p + ".in_proj.Wt") + (i64)D * D,
                           b.W(r.p + ".in_proj.b") + D, 2 * D, r.kv, 2 * D, EPI_LINEAR, 0, -1, -1, -1);
            }
        }
        // phase 2: attention, out_proj, FFN, norm_out; layers.cpp:454-530
        for (auto &r : br)
        {
            if (self)
                attention(r.p + ".attn", r.stream, r.qkv, 3 * D, (i64)r.tok * 3 * D, r.qkv + D, r.qkv + 2 * D, 3 * D,
                          (i64)r.tok * 3 * D, r.att, r.tok, r.tok, planes_ok(r.tok) ? r.kpl : -1, planes_ok(r.tok) ? r.vt : -1);
            else
                attention(r.p + ".attn", r.stream, r.qkv, D, (i64)r.tok * D, r.kv, r.kv + D, 2 * D, (i64)r.tokOther * 2 * D,
                          r.att, r.tok, r.tokOther, planes_ok(r.tokOther) ? r.kpl : -1, planes_ok(r.tokOther) ? r.vt : -1);
            linear(r.p + ".out_proj", r.stream, r.att, r.tok, D, b.W(r.p + ".out_proj.Wt"), b.W(r.p + ".out_proj.b"), D, r.x,
                   D, EPI_SCALE_RES, 0, r.x, b.W(r.p + ".gamma_1"), -1);
            std::string n3 = self ? ".norm2" : ".norm3"; // crosstransformer.cpp:111-113
            layernorm(r.p + n3, r.stream, r.x, r.n, r.tok, r.p + n3 + ".w", r.p + n3 + ".b", -1);
            linear(r.p + ".linear1", r.stream, r.n, r.tok, D, b.W(r.p + ".linear1.Wt"), b.W(r.p + ".linear1.b"), FF, r.hid, FF,
                   EPI_LINEAR, 1, -1, -1, -1);
            linear(r.p + ".linear2", r.stream, r.hid, r.tok, FF, b.W(r.p + ".linear2.Wt"), b.W(r.p + ".linear2.b"), D, r.x, D,
                   EPI_SCALE_RES, 0, r.x, b.W(r.p + ".gamma_2"), r.rs);
            int NBl = pl.ops.back().g.NB;
            b.push_reduce(r.p + ".norm_out.stats", r.stream, r.rs, r.stn, B, r.tok, NBl, 1, (double)r.tok * D, MODE_RSTD);
            Op op;
            op.kind = OP_GN_APPLY;
            op.stream = r.stream;
            op.name = r.p + ".norm_out";
            op.gn = GnApply{r.x, r.x, -1, B, r.tok, D, r.stn, b.W(r.p + ".norm_out.w"), b.W(r.p + ".norm_out.b")};
            pl.ops.push_back(op);
        }
    }
    b.push_tap("ct_x", aQf, {tokF, D}, (i64)tokF * D);
    b.push_tap("ct_xt", aQt, {tokT, D}, (i64)tokT * D);

    // channel downsamplers (4s) with the decoder-0 skip add fused as the epilogue residual;
    // model_inference.cpp:271-286, encdec.cpp:172,291. 6s: a 1x1 "identity" is avoided by
    // letting decoder 0 read x and skip through a residual-only linear (N = K = 384).
    if (is4)
    {
        linear("channel_downsampler", 0, aQf, tokF, 512, b.W("channel_downsampler.Wt"), b.W("channel_downsampler.b"), 384,
               aDin[0], 384, EPI_LINEAR, 0, aX[3], -1, -1);
        linear("channel_downsampler_t", 1, aQt, tokT, 512, b.W("channel_downsampler_t.Wt"), b.W("channel_downsampler_t.b"),
               384, aTDin[0], 384, EPI_LINEAR, 0, aXt[3], -1, -1);
    }
    else
    {
        // 6s: no resampler GEMM to fuse into; decoder-0 input = transformer output + skip
        Op a0;
        a0.kind = OP_GN_APPLY;
        a0.stream = 0;
        a0.name = "dec0.skip_add";
        a0.gn = GnApply{aQf, aDin[0], aX[3], B, tokF, D, -1, -1, -1};
        pl.ops.push_back(a0);
        Op a1;
        a1.kind = OP_GN_APPLY;
        a1.stream = 1;
        a1.name = "tdec0.skip_add";
        a1.gn = GnApply{aQt, aTDin[0], aXt[3], B, tokT, D, -1, -1, -1};
        pl.ops.push_back(a1);
    }
    b.push_tap("dec_in_0", aDin[0], {T, 8, 384}, (i64)T * 8 * 384);
    b.push_tap("tdec_in_0", aTDin[0], {tokT, 384}, (i64)tokT * 384);

    // ------------------------------------------------------------------ decoders
    for (int k = 0; k < 4; ++k)
    {
        const int Cd = ch[3 - k], F = Fl[4 - k];
        const int coutF = k < 3 ? ch[2 - k] : 4 * S, coutT = k < 3 ? ch[2 - k] : 2 * S;
        const i64 L = G.Lt[4 - k], Lout = G.Lt[3 - k];
        std::string pd = "decoder." + std::to_string(k), ptd = "tdecoder." + std::to_string(k);
        // ---- freq decoder (encdec.cpp:166-256)
        {
            IGemm g = b.base_gemm(); // Conv2d 3x3 pad 1 + GLU
            g.B = B, g.P1 = T, g.P0 = F;
            g.x = aDin[k], g.L1 = T, g.L0 = F, g.Cin = Cd;
            g.S1 = 3, g.pad1 = 1;
            g.seg0 = 3 * Cd, g.pad0 = 1;
            g.w_w = b.W(pd + ".rewrite.Wt"), g.bias_w = b.W(pd + ".rewrite.b");
            g.N = 2 * Cd;
            g.epi = EPI_GLU;
            g.y = aG[k], g.ldy = Cd, g.yBatchStride = (i64)T * F * Cd;
            b.finish(g, true);
            b.push_gemm(pd + ".rewrite", 0, g);
            b.dconv(pd, 0, aG[k], B, T, F, Cd, aHf, aRsF, aSt1F, aSt2F);
            IGemm t = b.base_gemm(); // ConvTranspose2d (8,1)/(4,1) (+GELU) + crop + next skip
            t.B = B, t.P1 = T, t.P0 = F + 1;
            t.x = aG[k], t.L1 = T, t.L0 = F, t.Cin = Cd;
            t.seg0 = 2 * Cd, t.pad0 = 1;
            t.w_w = b.W(pd + ".conv_tr.Wt"), t.bias_w = b.W(pd + ".conv_tr.b");
            t.N = 4 * coutF;
            t.epi = EPI_TRCONV, t.act = k < 3 ? 1 : 0;
            t.Lout = 4 * F, t.Cout = coutF;
            t.res = k < 3 ? aX[2 - k] : -1;
            t.y = aDin[k + 1], t.ldy = coutF, t.yBatchStride = (i64)T * 4 * F * coutF;
            b.finish(t, false);
            b.push_gemm(pd + ".conv_tr", 0, t);
            b.push_tap("dec_" + std::to_string(k), aDin[k + 1], {T, 4 * F, coutF}, (i64)T * 4 * F * coutF);
        }
        // ---- time decoder (encdec.cpp:258-361)
        {
            IGemm g = b.base_gemm(); // Conv1d k3 pad 1 + GLU
            g.B = B, g.P1 = (int)L, g.P0 = 1;
            g.x = aTDin[k], g.L1 = (int)L, g.L0 = 1, g.Cin = Cd;
            g.S1 = 3, g.pad1 = 1;
            g.seg0 = Cd;
            g.w_w = b.W(ptd + ".rewrite.Wt"), g.bias_w = b.W(ptd + ".rewrite.b");
            g.N = 2 * Cd;
            g.epi = EPI_GLU;
            g.y = aTG[k], g.ldy = Cd, g.yBatchStride = L * Cd;
            b.finish(g, true);
            b.push_gemm(ptd + ".rewrite", 1, g);
            b.dconv(ptd, 1, aTG[k], B, (int)L, 1, Cd, aHt, aRsTt, aSt1T, aSt2T);
            IGemm t = b.base_gemm();
            t.B = B, t.P1 = 1, t.P0 = (int)L + 1;
            t.x = aTG[k], t.L1 = 1, t.L0 = (int)L, t.Cin = Cd;
            t.seg0 = 2 * Cd, t.pad0 = 1;
            t.w_w = b.W(ptd + ".conv_tr.Wt"), t.bias_w = b.W(ptd + ".conv_tr.b");
            t.N = 4 * coutT;
            t.epi = EPI_TRCONV, t.act = k < 3 ? 1 : 0;
            t.Lout = (int)Lout, t.Cout = coutT;
            t.res = k < 3 ? aXt[2 - k] : -1;
            t.y = aTDin[k + 1], t.ldy = coutT, t.yBatchStride = Lout * coutT;
            b.finish(t, false);
            b.push_gemm(ptd + ".conv_tr", 1, t);
            b.push_tap("tdec_" + std::to_string(k), aTDin[k + 1], {(int)Lout, coutT}, Lout * coutT);
        }
    }

    // ------------------------------------------------------------------ ISTFT + sum
    {
        Op op;
        op.kind = OP_ISTFT;
        op.stream = 0;
        op.name = "istft";
        op.istft = Istft{aDin[4], aStF, aFrames, B, T, S, cWindow, cTwiddle, 1};
        pl.ops.push_back(op);
        Op o2;
        o2.kind = OP_OLA;
        o2.stream = 0;
        o2.name = "ola";
        o2.ola = Ola{aFrames, aTDin[4], aStT, cWss, pl.outOff, B, T, S, (int)seg, (int)G.pad, aDin[4], aStF, cWindow, cTwiddle, cRden};
        pl.ops.push_back(o2);
    }
    compute_deps(pl);
}

// ---------------------------------------------------------------------------------------------
// Cross-stream dependencies. The two branches of the model (/root/reference/src/model_inference.cpp
// runs them one after the other on one thread) only meet at the STFT output, in the cross-attention
// layers and in the final sum, so the engine runs them on two HIP streams. Instead of hand-placing
// the joins, every op declares the arena ranges it touches and the joins are derived: op i must wait
// for the latest earlier op j of the other stream with a RAW, WAR or WAW overlap.
void op_access(const Op &op, std::vector<Range> &rd, std::vector<Range> &wr)
{
    rd.clear();
    wr.clear();
    auto R = [&](i64 lo, i64 n) {
        if (lo >= 0 && n > 0)
            rd.push_back(Range{lo, lo + n});
    };
    auto Wr = [&](i64 lo, i64 n) {
        if (lo >= 0 && n > 0)
            wr.push_back(Range{lo, lo + n});
    };
    switch (op.kind)
    {
    case OP_IGEMM:
    {
        const IGemm &g = op.g;
        const i64 M = (i64)g.B * g.P1 * g.P0;
        R(g.x, (i64)(g.B - 1) * g.xBatchStride + (i64)g.L1 * g.L0 * g.Cin);
        if (g.pro != PRO_NONE)
            R(g.proStats, (i64)g.B * std::max(g.G0, 1) * 4);
        i64 yext;
        if (g.epi == EPI_TRCONV)
            yext = (i64)(g.B - 1) * g.yBatchStride + (i64)g.P1 * g.Lout * g.ldy;
        else
            yext = (M - 1) * g.ldy + g.N;
        if (g.epi != EPI_STATS_ONLY && g.epi != EPI_VT && !(g.epi == EPI_KPL && g.kvCol0 == 0))
            Wr(g.y, yext);
        if (g.kv >= 0) // three bf16 planes of B * kvT * kvH * kvHs elements = 1.5 floats per element
            Wr(g.kv, ((i64)g.B * g.kvT * g.kvH * g.kvHs * 3 + 1) / 2);
        if (g.res >= 0)
            R(g.res, yext);
        if (g.epi == EPI_GN_GLU_SCALE_RES)
            R(g.epiStats, (i64)g.B * std::max(g.G0, 1) * 4);
        if (g.rowstat >= 0)
            Wr(g.rowstat, M * std::max(g.NB, 1) * 2);
        break;
    }
    case OP_DCONV_ROW:
        R(op.dr.x, (i64)op.dr.B * op.dr.T * op.dr.F * op.dr.C);
        Wr(op.dr.x, (i64)op.dr.B * op.dr.T * op.dr.F * op.dr.C);
        break;
    case OP_STATS_REDUCE:
    {
        const StatsReduce &s = op.sr;
        R(s.rowstat, (i64)s.B * s.R * s.NB * 2);
        Wr(s.out, (i64)s.B * std::max(s.G0, 1) * 4);
        if (s.scratch >= 0)
        {
            R(s.scratch, (i64)s.B * s.nchunk * 4);
            Wr(s.scratch, (i64)s.B * s.nchunk * 4);
        }
        break;
    }
    case OP_STFT:
    {
        const Stft &s = op.stft;
        R(s.mix, (i64)s.B * s.seg * 2);
        Wr(s.x, (i64)s.B * s.T * 2048 * 4);
        Wr(s.rowstat, (i64)s.B * s.T * 2);
        Wr(s.rowstatT, (i64)s.B * s.T * 2);
        break;
    }
    case OP_LAYERNORM:
        R(op.ln.x, (i64)op.ln.rows * op.ln.D);
        Wr(op.ln.y, (i64)op.ln.rows * op.ln.D);
        break;
    case OP_GN_APPLY:
    {
        const GnApply &g = op.gn;
        const i64 n = (i64)g.B * g.rows * g.C;
        R(g.x, n);
        R(g.res, n);
        R(g.stats, (i64)g.B * 4);
        Wr(g.y, n);
        break;
    }
    case OP_ATTENTION:
    {
        const Attention &t = op.at;
        R(t.q, (i64)(t.B - 1) * t.qBatch + (i64)(t.Tq - 1) * t.ldq + (i64)t.H * t.hs);
        if (t.kpl >= 0)
        {
            R(t.kpl, ((i64)t.B * t.Tk * t.H * t.hs * 3 + 1) / 2);
            R(t.vt, ((i64)t.B * t.Tk * t.H * t.hs * 3 + 1) / 2);
        }
        else
        {
            R(t.k, (i64)(t.B - 1) * t.kBatch + (i64)(t.Tk - 1) * t.ldk + (i64)t.H * t.hs);
            R(t.v, (i64)(t.B - 1) * t.vBatch + (i64)(t.Tk - 1) * t.ldv + (i64)t.H * t.hs);
        }
        Wr(t.o, (i64)(t.B - 1) * t.oBatch + (i64)(t.Tq - 1) * t.ldo + (i64)t.H * t.hs);
        break;
    }
    case OP_ISTFT:
        R(op.istft.x, (i64)op.istft.B * op.istft.T * 2048 * 4 * op.istft.S);
        R(op.istft.stats, (i64)op.istft.B * 4);
        Wr(op.istft.frames, (i64)op.istft.B * op.istft.S * 2 * op.istft.T * 4096);
        break;
    case OP_OLA:
        if (op.ola.x >= 0) // fused execution reads the ISTFT's operands itself
        {
            R(op.ola.x, (i64)op.ola.B * op.ola.T * 2048 * 4 * op.ola.S);
            R(op.ola.stats, (i64)op.ola.B * 4);
        }
        R(op.ola.frames, (i64)op.ola.B * op.ola.S * 2 * op.ola.T * 4096);
        R(op.ola.xt, (i64)op.ola.B * op.ola.seg * 2 * op.ola.S);
        R(op.ola.statsT, (i64)op.ola.B * 4);
        Wr(op.ola.out, (i64)op.ola.B * op.ola.S * 2 * op.ola.seg);
        break;
    case OP_GROUP_STATS:
        R(op.gs.x, (i64)op.gs.B * op.gs.rows * op.gs.C);
        Wr(op.gs.out, (i64)op.gs.B * op.gs.G * 4);
        Wr(op.gs.scratch, (i64)op.gs.B * op.gs.G * 32 * 4);
        break;
    case OP_GN_ACT:
    {
        const GnAct &g = op.ga;
        const int Co = g.mode == 2 ? g.C / 2 : g.C;
        R(g.x, (i64)g.B * g.rowsIn * g.C);
        R(g.stats, (i64)g.B * g.G * 4);
        R(g.res, (i64)g.B * g.rowsOut * Co);
        Wr(g.y, (i64)g.B * g.rowsOut * Co);
        break;
    }
    case OP_LSTM:
        R(op.lstm.xproj, (i64)op.lstm.B * op.lstm.T * 8 * op.lstm.H);
        Wr(op.lstm.out, (i64)op.lstm.B * op.lstm.T * 2 * op.lstm.H);
        Wr(op.lstm.sync, lstm_xchg_floats(op.lstm.B, op.lstm.T, op.lstm.H));
        break;
    case OP_LOCAL_ATTN:
        R(op.la.qkvd, (i64)op.la.B * op.la.T * op.la.ld);
        Wr(op.la.out, (i64)op.la.B * op.la.T * op.la.H);
        break;
    default:
        break;
    }
}

void compute_deps(Plan &pl)
{
    const int n = (int)pl.ops.size();
    std::vector<std::vector<Range>> rd(n), wr(n);
    for (int i = 0; i < n; ++i)
        op_access(pl.ops[i], rd[i], wr[i]);
    auto overlap = [](const std::vector<Range> &a, const std::vector<Range> &b) {
        for (const Range &x : a)
            for (const Range &y : b)
                if (x.lo < y.hi && y.lo < x.hi)
                    return true;
        return false;
    };
    int waited[2] = {-1, -1}; // per stream: the latest op of the other stream it has already joined
    for (int i = 0; i < n; ++i)
    {
        Op &op = pl.ops[i];
        op.waitOp = -1;
        if (op.kind == OP_TAP)
            continue;
        const int s = op.stream ? 1 : 0;
        for (int j = i - 1; j > waited[s]; --j)
        {
            const Op &o = pl.ops[j];
            if (o.kind == OP_TAP || (o.stream ? 1 : 0) == s)
                continue;
            if (overlap(wr[j], rd[i]) || overlap(wr[j], wr[i]) || overlap(rd[j], wr[i]))
            {
                op.waitOp = j;
                waited[s] = j;
                pl.ops[j].signals = true;
                break;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Demucs v3 (hdemucs_mmi). Restates /root/reference/src/model_inference.cpp:477-856 with its blocks
// src/encdec.cpp:363-863 and src/layers.cpp:533-1113, src/lstm.cpp:68-147. Levels 0-3 of both branches are
// the v4 encoder layers with DConv hidden width C/4; the time branch's level 4 is a bare conv injected into the
// frequency branch's level 4; levels 4 / 5 carry GroupNorm(4 groups) and a DConv with BiLSTM + LocalState;
// decoders have no DConv; decoder 0 / 1 and tdecoder 0 carry GroupNorm(4 groups).
i64 lstm_sync_floats(int B, int H)
{
    // h exchange granules of the cooperative LSTM kernel (lstm.hip): [2 directions][batch groups of 16][2 parities][H][16]
    // x 8 bytes {value, tag}
    const i64 nbg = (B + 15) / 16;
    return 2 * nbg * 2 * (i64)H * 16 * 2;
}
i64 lstm_xchg_floats(int B, int T, int H)
{
    // EXPERIMENT (DMX_LSTM_XCHG=x4): the 4-byte exchange image [2 directions x batch groups of 16][T][H][16] floats,
    // sentinel-filled by the launcher; never smaller than the granule area (either form may be selected at run time)
    const i64 nbg = (B + 15) / 16;
    const i64 x = 2 * nbg * (i64)T * H * 16;
    return x > lstm_sync_floats(B, H) ? x : lstm_sync_floats(B, H);
}

void build_plan_v3(const PackedModel &pm, i64 seg, int B, Plan &pl, const PlanOpts &opts)
{
    Builder b(pm, pl, opts);
    pl.B = B;
    pl.geo = make_geo(seg);
    pl.S = 4;
    pl.D = 0;
    const Geo &G = pl.geo;
    const int T = (int)G.le, S = 4;
    const int ch[4] = {48, 96, 192, 384};
    const int Fl[5] = {2048, 512, 128, 32, 8};
    const int L3 = (int)G.Lt[4];
    const int T5 = (T - 2 + 1) / 2 + 1; // Conv1d k4 s2 p1, ceil form (Q5): ceil((T + 2 - 3 - 1) / 2) + 1

    // ------------------------------------------------------------------ constants
    pl.zeroOff = b.alloc(64);
    const i64 cWindow = b.alloc(4096);
    const i64 cTwiddle = b.alloc(2 * 2048);
    const int nfr = T + 4;
    const i64 wssLen = 4096 + 1024 * (i64)(nfr - 1);
    const i64 cWss = b.alloc(wssLen);
    const i64 cRden = b.alloc(wssLen);
    pl.constants.assign((size_t)b.top, 0.0f);
    {
        float *win = &pl.constants[(size_t)cWindow];
        static constexpr float PI = 3.14159265359F;
        float floatN = (float)(4096 + 1);
        for (int n = 0; n < 4096; ++n)
            win[n] = 0.5F * (1.0F - cosf(2.0F * PI * (float)n / (floatN - 1)));
        float *tw = &pl.constants[(size_t)cTwiddle];
        for (int k = 0; k < 2048; ++k)
        {
            double a = -2.0 * M_PI * (double)k / 4096.0;
            tw[2 * k] = (float)cos(a);
            tw[2 * k + 1] = (float)sin(a);
        }
        float *wss = &pl.constants[(size_t)cWss];
        for (int i = 0; i < nfr; ++i)
            for (int j = 0; j < 4096; ++j)
                wss[(i64)i * 1024 + j] += win[j] * win[j];
        float *rden = &pl.constants[(size_t)cRden];
        for (i64 n = 0; n < wssLen; ++n)
            rden[n] = (1.0f / 4096.0f) / (wss[n] + 1e-8f);
    }

    // ------------------------------------------------------------------ activations
    pl.mixOff = b.alloc((i64)B * seg * 2);
    pl.outOff = b.alloc((i64)B * S * 2 * seg);
    const i64 aXcac = b.alloc((i64)B * T * 2048 * 4);
    const i64 aRsX = b.alloc((i64)B * T * 2), aRsT = b.alloc((i64)B * T * 2);
    const i64 aStF = b.alloc((i64)B * 4), aStT = b.alloc((i64)B * 4);
    b.redScratch[0] = b.alloc((i64)B * 256 * 4);
    b.redScratch[1] = b.alloc((i64)B * 256 * 4);
    i64 aY[4], aX[4], aYt[4], aXt[4];
    for (int i = 0; i < 4; ++i)
    {
        aY[i] = b.alloc((i64)B * T * Fl[i + 1] * ch[i]);
        aX[i] = b.alloc((i64)B * T * Fl[i + 1] * ch[i]);
        aYt[i] = b.alloc((i64)B * G.Lt[i + 1] * ch[i]);
        aXt[i] = b.alloc((i64)B * G.Lt[i + 1] * ch[i]);
    }
    i64 maxRowsF = 0, maxHF = 0, maxRowsT = 0, maxHT = 0;
    for (int i = 0; i < 4; ++i)
    {
        i64 rf = (i64)B * T * Fl[i + 1], rt = (i64)B * G.Lt[i + 1];
        maxRowsF = std::max(maxRowsF, rf);
        maxRowsT = std::max(maxRowsT, rt);
        maxHF = std::max(maxHF, rf * rup(ch[i] / 4, 4));
        maxHT = std::max(maxHT, rt * rup(ch[i] / 4, 4));
    }
    const int kMaxNB = 16;
    const i64 aHf = b.alloc(maxHF), aHt = b.alloc(maxHT);
    const i64 aRsF = b.alloc(maxRowsF * kMaxNB * 2);
    const i64 aRsTt = b.alloc(maxRowsT * kMaxNB * 2);
    const i64 aSt1F = b.alloc((i64)B * 512 * 4), aSt2F = b.alloc((i64)B * 512 * 4);
    const i64 aSt1T = b.alloc((i64)B * 4), aSt2T = b.alloc((i64)B * 4);
    // levels 4 / 5 ([B][T][C] / [B][T5][C], channels last)
    const i64 aXt4 = b.alloc((i64)B * T * 768);
    const i64 aE4 = b.alloc((i64)B * T * 768), aE4n = b.alloc((i64)B * T * 768);
    const i64 aR4 = b.alloc((i64)B * T * 1536), aX4 = b.alloc((i64)B * T * 768);
    const i64 aE5 = b.alloc((i64)B * T5 * 1536), aE5n = b.alloc((i64)B * T5 * 1536);
    const i64 aR5 = b.alloc((i64)B * T5 * 3072), aX5 = b.alloc((i64)B * T5 * 1536);
    const i64 rowsH = std::max((i64)T * 192, (i64)T5 * 384); // rows x hidden width of the two LSTM DConvs
    const i64 aLh = b.alloc(B * rowsH), aLym = b.alloc(B * rowsH), aLr = b.alloc(B * rowsH);
    const i64 aLxp = b.alloc(B * rowsH * 8), aLl0 = b.alloc(B * rowsH * 2), aLl1 = b.alloc(B * rowsH * 2);
    const i64 aLqkvd = b.alloc((i64)B * std::max((i64)T * (3 * 192 + 16), (i64)T5 * (3 * 384 + 16)));
    const i64 aLu = b.alloc((i64)B * std::max((i64)T * 1536, (i64)T5 * 3072));
    const i64 aLsync = b.alloc(std::max(lstm_xchg_floats(B, T, 192), lstm_xchg_floats(B, T5, 384)));
    const i64 aStG = b.alloc((i64)B * 4 * 4), aStGt = b.alloc((i64)B * 4 * 4);
    const i64 aGsScr = b.alloc((i64)B * 4 * 32 * 4), aGsScrT = b.alloc((i64)B * 4 * 32 * 4); // chunk partials (doubles), per stream
    // decoders 0 / 1, tdecoder 0
    const int Lz0 = 2 * T5 + 2, Lzt = 4 * T + 4;
    const i64 aD0r = b.alloc((i64)B * T5 * 3072), aD0g = b.alloc((i64)B * T5 * 1536), aD0t = b.alloc((i64)B * Lz0 * 768);
    const i64 aD1in = b.alloc((i64)B * T * 768), aD1r = b.alloc((i64)B * T * 1536), aPre = b.alloc((i64)B * T * 768);
    const i64 aD1t = b.alloc((i64)B * T * 8 * 384), aTD0t = b.alloc((i64)B * Lzt * 384);
    // common decoders
    i64 aDin[5], aG[4], aTDin[5], aTG[4];
    for (int k = 0; k < 4; ++k)
    {
        int Cd = ch[3 - k];
        aDin[k] = b.alloc((i64)B * T * Fl[4 - k] * Cd);
        aG[k] = b.alloc((i64)B * T * Fl[4 - k] * Cd);
        aTDin[k] = b.alloc((i64)B * G.Lt[4 - k] * Cd);
        aTG[k] = b.alloc((i64)B * G.Lt[4 - k] * Cd);
    }
    aDin[4] = b.alloc((i64)B * T * 2048 * 4 * S);
    aTDin[4] = b.alloc((i64)B * seg * 2 * S);
    const i64 aFrames = b.alloc((i64)B * S * 2 * T * 4096);

    // ------------------------------------------------------------------ small op builders
    auto gstats = [&](const std::string &name, int stream, i64 x, int rows, int C, int Gn) {
        Op op;
        op.kind = OP_GROUP_STATS;
        op.stream = stream;
        op.name = name;
        op.gs = GroupStats{x, aStG, B, rows, C, Gn, 1e-5f, aGsScr};
        pl.ops.push_back(op);
    };
    auto gnact = [&](const std::string &name, int stream, i64 x, i64 y, int rowsIn, int C, int Gn, int mode, i64 w, i64 bs,
                     i64 scale, i64 res, int rowOff, int rowsOut) {
        Op op;
        op.kind = OP_GN_ACT;
        op.stream = stream;
        op.name = name;
        op.ga = GnAct{x, y, aStG, res, w, bs, scale, B, rowsIn, C, Gn, mode, rowOff, rowsOut};
        pl.ops.push_back(op);
    };
    // rows x K linear layer on [B][rows][K] (1x1 conv), optional residual
    auto linear = [&](const std::string &name, int stream, i64 x, int rows, int K, i64 w, i64 bias, int N, i64 y, i64 res) {
        IGemm g = b.base_gemm();
        g.B = B, g.P1 = rows, g.P0 = 1;
        g.x = x, g.L1 = rows, g.L0 = 1, g.Cin = K;
        g.seg0 = K;
        g.w_w = w, g.bias_w = bias, g.N = N;
        g.epi = EPI_LINEAR, g.act = 0;
        g.y = y, g.ldy = N, g.yBatchStride = (i64)rows * N;
        g.res = res;
        b.finish(g, false);
        b.push_gemm(name, stream, g);
    };
    // Conv1d k3 over the rows of [B][rows][C] (dilation d, "same" padding)
    auto conv_k3 = [&](const std::string &name, int stream, i64 x, int rows, int C, int d, i64 w, i64 bias, int N, i64 y) {
        IGemm g = b.base_gemm();
        g.B = B, g.P1 = rows, g.P0 = 1;
        g.x = x, g.L1 = rows, g.L0 = 1, g.Cin = C;
        g.S1 = 3, g.dil1 = d, g.pad1 = d;
        g.seg0 = C;
        g.w_w = w, g.bias_w = bias, g.N = N;
        g.epi = EPI_LINEAR, g.act = 0;
        g.y = y, g.ldy = N, g.yBatchStride = (i64)rows * N;
        b.finish(g, false);
        b.push_gemm(name, stream, g);
    };
    // DConv with BiLSTM + LocalState, in place on y [B][rows][C]; layers.cpp:877-1113
    auto dconv_lstm = [&](const std::string &p, i64 y, int rows, int C, const std::string &tapName) {
        const int H = C / 4, ld = 3 * H + 16;
        for (int j = 0; j < 2; ++j)
        {
            const std::string w = p + ".dconv." + std::to_string(j) + ".", nm = p + ".dconv" + std::to_string(j);
            // LSTM and LocalState outputs of every layer keep their own (small) buffers: they are debug taps
            const i64 aLa = b.alloc((i64)B * rows * H), aLa2 = b.alloc((i64)B * rows * H);
            conv_k3(nm + ".k1", 0, y, rows, C, j == 0 ? 1 : 2, b.W(w + "k1.Wt"), b.W(w + "k1.b"), H, aLh);
            gstats(nm + ".gn1.stats", 0, aLh, rows, H, 1);
            gnact(nm + ".gn1", 0, aLh, aLym, rows, H, 1, 1, b.W(w + "gn1.w"), b.W(w + "gn1.b"), -1, -1, 0, rows);
            i64 in = aLym;
            int In = H;
            for (int layer = 0; layer < 2; ++layer)
            {
                const std::string lw = w + "lstm" + std::to_string(layer);
                linear(nm + ".lstm" + std::to_string(layer) + ".ih", 0, in, rows, In, b.W(lw + ".ih.Wt"), b.W(lw + ".ih.b"), 8 * H,
                       aLxp, -1);
                Op op;
                op.kind = OP_LSTM;
                op.stream = 0;
                op.name = nm + ".lstm" + std::to_string(layer);
                op.lstm = Lstm{aLxp, b.W(lw + ".hh"), layer == 0 ? aLl0 : aLl1, aLsync, B, rows, H};
                pl.ops.push_back(op);
                in = layer == 0 ? aLl0 : aLl1;
                In = 2 * H;
            }
            linear(nm + ".lin", 0, aLl1, rows, 2 * H, b.W(w + "lin.Wt"), b.W(w + "lin.b"), H, aLa, aLym); // + skip
            b.push_tap(tapName + "_lstm" + std::to_string(j), aLa, {rows, H}, (i64)rows * H);
            linear(nm + ".qkvd", 0, aLa, rows, H, b.W(w + "qkvd.Wt"), b.W(w + "qkvd.b"), ld, aLqkvd, -1);
            {
                Op op;
                op.kind = OP_LOCAL_ATTN;
                op.stream = 0;
                op.name = nm + ".attn";
                op.la = LocalAttn{aLqkvd, aLr, B, rows, H, ld};
                pl.ops.push_back(op);
            }
            linear(nm + ".proj", 0, aLr, rows, H, b.W(w + "proj.Wt"), b.W(w + "proj.b"), H, aLa2, aLa); // x + proj(result)
            b.push_tap(tapName + "_attn" + std::to_string(j), aLa2, {rows, H}, (i64)rows * H);
            linear(nm + ".k2", 0, aLa2, rows, H, b.W(w + "k2.Wt"), b.W(w + "k2.b"), 2 * C, aLu, -1);
            gstats(nm + ".gn2.stats", 0, aLu, rows, 2 * C, 1);
            gnact(nm + ".gn2", 0, aLu, y, rows, 2 * C, 1, 2, b.W(w + "gn2.w"), b.W(w + "gn2.b"), b.W(w + "scale"), y, 0, rows);
        }
    };

    // ------------------------------------------------------------------ ops: front end
    {
        Op op;
        op.kind = OP_STFT;
        op.stream = 0;
        op.name = "stft";
        op.stft = Stft{pl.mixOff, aXcac, aRsX, aRsT, B, T, (int)seg, (int)G.pad, cWindow, cTwiddle};
        pl.ops.push_back(op);
    }
    b.push_reduce("znorm.freq", 0, aRsX, aStF, B, T, 1, 1, (double)4 * 2048 * T, MODE_ZNORM);
    b.push_reduce("znorm.time", 1, aRsT, aStT, B, T, 1, 1, (double)2 * seg, MODE_ZNORM);
    b.push_tap("x_cac", aXcac, {T, 2048, 4}, (i64)T * 2048 * 4);

    // ------------------------------------------------------------------ encoders 0-3 (encdec.cpp:363-524)
    for (int i = 0; i < 4; ++i)
    {
        const int C = ch[i], Fin = Fl[i], Fo = Fl[i + 1];
        const int cinF = i == 0 ? 4 : ch[i - 1], cinT = i == 0 ? 2 : ch[i - 1];
        const i64 Lin = G.Lt[i], Lo = G.Lt[i + 1];
        std::string pe = "encoder." + std::to_string(i), pt = "tencoder." + std::to_string(i);
        {
            IGemm g = b.base_gemm();
            g.B = B, g.P1 = 1, g.P0 = (int)Lo;
            g.x = i == 0 ? pl.mixOff : aXt[i - 1];
            g.L1 = 1, g.L0 = (int)Lin, g.Cin = cinT;
            g.seg0 = 8 * cinT, g.stride0 = 4, g.pad0 = 2;
            if (i == 0)
                g.pro = PRO_AFFINE, g.proStats = aStT;
            g.w_w = b.W(pt + ".conv.Wt"), g.bias_w = b.W(pt + ".conv.b");
            g.N = C;
            g.epi = EPI_LINEAR, g.act = 1;
            g.y = aYt[i], g.ldy = C, g.yBatchStride = Lo * C;
            b.finish(g, false);
            b.push_gemm(pt + ".conv", 1, g);
            b.dconv(pt, 1, aYt[i], B, (int)Lo, 1, C, aHt, aRsTt, aSt1T, aSt2T);
            IGemm r = b.base_gemm();
            r.B = B, r.P1 = (int)Lo, r.P0 = 1;
            r.x = aYt[i], r.L1 = (int)Lo, r.L0 = 1, r.Cin = C;
            r.seg0 = C;
            r.w_w = b.W(pt + ".rewrite.Wt"), r.bias_w = b.W(pt + ".rewrite.b");
            r.N = 2 * C;
            r.epi = EPI_GLU;
            r.y = aXt[i], r.ldy = C, r.yBatchStride = Lo * C;
            b.finish(r, true);
            b.push_gemm(pt + ".rewrite", 1, r);
        }
        {
            IGemm g = b.base_gemm();
            g.B = B, g.P1 = T, g.P0 = Fo;
            g.x = i == 0 ? aXcac : aX[i - 1];
            g.L1 = T, g.L0 = Fin, g.Cin = cinF;
            g.seg0 = 8 * cinF, g.stride0 = 4, g.pad0 = 2;
            if (i == 0)
                g.pro = PRO_AFFINE, g.proStats = aStF;
            g.w_w = b.W(pe + ".conv.Wt"), g.bias_w = b.W(pe + ".conv.b");
            g.N = C;
            g.epi = EPI_LINEAR, g.act = 1;
            g.y = aY[i], g.ldy = C, g.yBatchStride = (i64)T * Fo * C;
            b.finish(g, false);
            b.push_gemm(pe + ".conv", 0, g);
            b.dconv(pe, 0, aY[i], B, T, Fo, C, aHf, aRsF, aSt1F, aSt2F);
            IGemm r = b.base_gemm();
            r.B = B, r.P1 = T, r.P0 = Fo;
            r.x = aY[i], r.L1 = T, r.L0 = Fo, r.Cin = C;
            r.seg0 = C;
            r.w_w = b.W(pe + ".rewrite.Wt"), r.bias_w = b.W(pe + ".rewrite.b");
            r.N = 2 * C;
            r.epi = EPI_GLU;
            if (i == 0)
                r.table_w = b.W("freq_emb.table"), r.tableScale = 10.0f * 0.2f; // model_inference.cpp:599-618
            r.y = aX[i], r.ldy = C, r.yBatchStride = (i64)T * Fo * C;
            b.finish(r, true);
            b.push_gemm(pe + ".rewrite", 0, r);
        }
        b.push_tap("x_" + std::to_string(i), aX[i], {T, Fo, C}, (i64)T * Fo * C);
        b.push_tap("xt_" + std::to_string(i), aXt[i], {(int)Lo, C}, Lo * C);
    }

    // ------------------------------------------------------------------ tencoder 4 (bare conv; encdec.cpp:526-537)
    {
        IGemm g = b.base_gemm();
        g.B = B, g.P1 = 1, g.P0 = T;
        g.x = aXt[3], g.L1 = 1, g.L0 = L3, g.Cin = 384;
        g.seg0 = 8 * 384, g.stride0 = 4, g.pad0 = 2;
        g.w_w = b.W("tencoder.4.conv.Wt"), g.bias_w = b.W("tencoder.4.conv.b");
        g.N = 768;
        g.epi = EPI_LINEAR, g.act = 0;
        g.y = aXt4, g.ldy = 768, g.yBatchStride = (i64)T * 768;
        b.finish(g, false);
        b.push_gemm("tencoder.4.conv", 1, g);
        b.push_tap("xt_4", aXt4, {T, 768}, (i64)T * 768);
    }
    // ------------------------------------------------------------------ encoder 4 (encdec.cpp:539-581)
    // Conv2d (8,1)/(4,1), no padding, on the 8 frequency rows of a frame: one run of 8*384 floats per (b, t);
    // the time branch's level-4 output is injected as the residual of the same GEMM
    linear("encoder.4.conv", 0, aX[3], T, 8 * 384, b.W("encoder.4.conv.Wt"), b.W("encoder.4.conv.b"), 768, aE4, aXt4);
    gstats("encoder.4.norm1.stats", 0, aE4, T, 768, 4);
    gnact("encoder.4.norm1", 0, aE4, aE4n, T, 768, 4, 1, b.W("encoder.4.norm1.w"), b.W("encoder.4.norm1.b"), -1, -1, 0, T);
    dconv_lstm("encoder.4", aE4n, T, 768, "e4");
    linear("encoder.4.rewrite", 0, aE4n, T, 768, b.W("encoder.4.rewrite.Wt"), b.W("encoder.4.rewrite.b"), 1536, aR4, -1);
    gstats("encoder.4.norm2.stats", 0, aR4, T, 1536, 4);
    gnact("encoder.4.norm2", 0, aR4, aX4, T, 1536, 4, 2, b.W("encoder.4.norm2.w"), b.W("encoder.4.norm2.b"), -1, -1, 0, T);
    b.push_tap("x_4", aX4, {T, 768}, (i64)T * 768);
    // ------------------------------------------------------------------ encoder 5, shared (encdec.cpp:583-623)
    {
        IGemm g = b.base_gemm(); // Conv1d(768 -> 1536, k4, s2, p1)
        g.B = B, g.P1 = 1, g.P0 = T5;
        g.x = aX4, g.L1 = 1, g.L0 = T, g.Cin = 768;
        g.seg0 = 4 * 768, g.stride0 = 2, g.pad0 = 1;
        g.w_w = b.W("encoder.5.conv.Wt"), g.bias_w = b.W("encoder.5.conv.b");
        g.N = 1536;
        g.epi = EPI_LINEAR, g.act = 0;
        g.y = aE5, g.ldy = 1536, g.yBatchStride = (i64)T5 * 1536;
        b.finish(g, false);
        b.push_gemm("encoder.5.conv", 0, g);
    }
    gstats("encoder.5.norm1.stats", 0, aE5, T5, 1536, 4);
    gnact("encoder.5.norm1", 0, aE5, aE5n, T5, 1536, 4, 1, b.W("encoder.5.norm1.w"), b.W("encoder.5.norm1.b"), -1, -1, 0, T5);
    dconv_lstm("encoder.5", aE5n, T5, 1536, "e5");
    linear("encoder.5.rewrite", 0, aE5n, T5, 1536, b.W("encoder.5.rewrite.Wt"), b.W("encoder.5.rewrite.b"), 3072, aR5, -1);
    gstats("encoder.5.norm2.stats", 0, aR5, T5, 3072, 4);
    gnact("encoder.5.norm2", 0, aR5, aX5, T5, 3072, 4, 2, b.W("encoder.5.norm2.w"), b.W("encoder.5.norm2.b"), -1, -1, 0, T5);
    b.push_tap("x_5", aX5, {T5, 1536}, (i64)T5 * 1536);

    // ------------------------------------------------------------------ decoder 0, shared (encdec.cpp:625-663)
    conv_k3("decoder.0.rewrite", 0, aX5, T5, 1536, 1, b.W("decoder.0.rewrite.Wt"), b.W("decoder.0.rewrite.b"), 3072, aD0r);
    gstats("decoder.0.norm1.stats", 0, aD0r, T5, 3072, 4);
    gnact("decoder.0.norm1", 0, aD0r, aD0g, T5, 3072, 4, 2, b.W("decoder.0.norm1.w"), b.W("decoder.0.norm1.b"), -1, -1, 0, T5);
    {
        IGemm t = b.base_gemm(); // ConvTranspose1d(1536 -> 768, k4, s2): 2*T5 + 2 outputs, all of them normalised
        t.B = B, t.P1 = 1, t.P0 = T5 + 1;
        t.x = aD0g, t.L1 = 1, t.L0 = T5, t.Cin = 1536;
        t.seg0 = 2 * 1536, t.pad0 = 1;
        t.w_w = b.W("decoder.0.conv_tr.Wt"), t.bias_w = b.W("decoder.0.conv_tr.b");
        t.N = 2 * 768;
        t.epi = EPI_TRCONV, t.act = 0;
        t.Lout = Lz0, t.Cout = 768, t.trS = 2, t.trOff = 0;
        t.y = aD0t, t.ldy = 768, t.yBatchStride = (i64)Lz0 * 768;
        b.finish(t, false);
        b.push_gemm("decoder.0.conv_tr", 0, t);
    }
    gstats("decoder.0.norm2.stats", 0, aD0t, Lz0, 768, 4);
    // GELU, crop [1, 1+T), and the skip add of decoder 1 (x + saved_4; encdec.cpp:673)
    gnact("decoder.0.norm2", 0, aD0t, aD1in, Lz0, 768, 4, 1, b.W("decoder.0.norm2.w"), b.W("decoder.0.norm2.b"), -1, aX4, 1, T);
    b.push_tap("d1_in", aD1in, {T, 768}, (i64)T * 768);
    // ------------------------------------------------------------------ decoder 1 (encdec.cpp:665-705)
    conv_k3("decoder.1.rewrite", 0, aD1in, T, 768, 1, b.W("decoder.1.rewrite.Wt"), b.W("decoder.1.rewrite.b"), 1536, aD1r);
    gstats("decoder.1.norm1.stats", 0, aD1r, T, 1536, 4);
    gnact("decoder.1.norm1", 0, aD1r, aPre, T, 1536, 4, 2, b.W("decoder.1.norm1.w"), b.W("decoder.1.norm1.b"), -1, -1, 0, T);
    {
        IGemm t = b.base_gemm(); // ConvTranspose2d (8,1)/(4,1) on ONE frequency row -> 8 rows, no crop
        t.B = B, t.P1 = T, t.P0 = 2;
        t.x = aPre, t.L1 = T, t.L0 = 1, t.Cin = 768;
        t.seg0 = 2 * 768, t.pad0 = 1;
        t.w_w = b.W("decoder.1.conv_tr.Wt"), t.bias_w = b.W("decoder.1.conv_tr.b");
        t.N = 4 * 384;
        t.epi = EPI_TRCONV, t.act = 0;
        t.Lout = 8, t.Cout = 384, t.trS = 4, t.trOff = 0;
        t.y = aD1t, t.ldy = 384, t.yBatchStride = (i64)T * 8 * 384;
        b.finish(t, false);
        b.push_gemm("decoder.1.conv_tr", 0, t);
    }
    gstats("decoder.1.norm2.stats", 0, aD1t, T * 8, 384, 4);
    gnact("decoder.1.norm2", 0, aD1t, aDin[0], T * 8, 384, 4, 1, b.W("decoder.1.norm2.w"), b.W("decoder.1.norm2.b"), -1, aX[3], 0,
          T * 8);
    b.push_tap("dec_in", aDin[0], {T, 8, 384}, (i64)T * 8 * 384);
    // ------------------------------------------------------------------ tdecoder 0 (encdec.cpp:707-725)
    {
        IGemm t = b.base_gemm(); // ConvTranspose1d(768 -> 384, k8, s4) on decoder 1's "pre": 4T + 4 outputs
        t.B = B, t.P1 = 1, t.P0 = T + 1;
        t.x = aPre, t.L1 = 1, t.L0 = T, t.Cin = 768;
        t.seg0 = 2 * 768, t.pad0 = 1;
        t.w_w = b.W("tdecoder.0.conv_tr.Wt"), t.bias_w = b.W("tdecoder.0.conv_tr.b");
        t.N = 4 * 384;
        t.epi = EPI_TRCONV, t.act = 0;
        t.Lout = Lzt, t.Cout = 384, t.trS = 4, t.trOff = 0;
        t.y = aTD0t, t.ldy = 384, t.yBatchStride = (i64)Lzt * 384;
        b.finish(t, false);
        b.push_gemm("tdecoder.0.conv_tr", 1, t);
    }
    {
        // the one GroupNorm of the time branch runs on stream 1: its statistics record is its own
        Op op;
        op.kind = OP_GROUP_STATS;
        op.stream = 1;
        op.name = "tdecoder.0.norm2.stats";
        op.gs = GroupStats{aTD0t, aStGt, B, Lzt, 384, 4, 1e-5f, aGsScrT};
        pl.ops.push_back(op);
        // GELU, crop [2, 2 + L3), and the skip add of tdecoder 1
        Op o2;
        o2.kind = OP_GN_ACT;
        o2.stream = 1;
        o2.name = "tdecoder.0.norm2";
        o2.ga = GnAct{aTD0t, aTDin[0], aStGt, aXt[3], b.W("tdecoder.0.norm2.w"), b.W("tdecoder.0.norm2.b"), -1, B, Lzt, 384, 4, 1, 2, L3};
        pl.ops.push_back(o2);
    }
    b.push_tap("tdec_in", aTDin[0], {L3, 384}, (i64)L3 * 384);

    // ------------------------------------------------------------------ decoders 2-5 / tdecoders 1-4 (encdec.cpp:727-863)
    for (int k = 0; k < 4; ++k)
    {
        const int Cd = ch[3 - k], F = Fl[4 - k];
        const int coutF = k < 3 ? ch[2 - k] : 4 * S, coutT = k < 3 ? ch[2 - k] : 2 * S;
        const i64 L = G.Lt[4 - k], Lout = G.Lt[3 - k];
        std::string pd = "decoder." + std::to_string(k + 2), ptd = "tdecoder." + std::to_string(k + 1);
        {
            IGemm g = b.base_gemm(); // Conv2d 3x3 pad 1 + GLU
            g.B = B, g.P1 = T, g.P0 = F;
            g.x = aDin[k], g.L1 = T, g.L0 = F, g.Cin = Cd;
            g.S1 = 3, g.pad1 = 1;
            g.seg0 = 3 * Cd, g.pad0 = 1;
            g.w_w = b.W(pd + ".rewrite.Wt"), g.bias_w = b.W(pd + ".rewrite.b");
            g.N = 2 * Cd;
            g.epi = EPI_GLU;
            g.y = aG[k], g.ldy = Cd, g.yBatchStride = (i64)T * F * Cd;
            b.finish(g, true);
            b.push_gemm(pd + ".rewrite", 0, g);
            IGemm t = b.base_gemm(); // ConvTranspose2d (8,1)/(4,1) (+GELU) + crop + next skip
            t.B = B, t.P1 = T, t.P0 = F + 1;
            t.x = aG[k], t.L1 = T, t.L0 = F, t.Cin = Cd;
            t.seg0 = 2 * Cd, t.pad0 = 1;
            t.w_w = b.W(pd + ".conv_tr.Wt"), t.bias_w = b.W(pd + ".conv_tr.b");
            t.N = 4 * coutF;
            t.epi = EPI_TRCONV, t.act = k < 3 ? 1 : 0;
            t.Lout = 4 * F, t.Cout = coutF;
            t.res = k < 3 ? aX[2 - k] : -1;
            t.y = aDin[k + 1], t.ldy = coutF, t.yBatchStride = (i64)T * 4 * F * coutF;
            b.finish(t, false);
            b.push_gemm(pd + ".conv_tr", 0, t);
            b.push_tap("dec_" + std::to_string(k), aDin[k + 1], {T, 4 * F, coutF}, (i64)T * 4 * F * coutF);
        }
        {
            IGemm g = b.base_gemm(); // Conv1d k3 pad 1 + GLU
            g.B = B, g.P1 = (int)L, g.P0 = 1;
            g.x = aTDin[k], g.L1 = (int)L, g.L0 = 1, g.Cin = Cd;
            g.S1 = 3, g.pad1 = 1;
            g.seg0 = Cd;
            g.w_w = b.W(ptd + ".rewrite.Wt"), g.bias_w = b.W(ptd + ".rewrite.b");
            g.N = 2 * Cd;
            g.epi = EPI_GLU;
            g.y = aTG[k], g.ldy = Cd, g.yBatchStride = L * Cd;
            b.finish(g, true);
            b.push_gemm(ptd + ".rewrite", 1, g);
            IGemm t = b.base_gemm();
            t.B = B, t.P1 = 1, t.P0 = (int)L + 1;
            t.x = aTG[k], t.L1 = 1, t.L0 = (int)L, t.Cin = Cd;
            t.seg0 = 2 * Cd, t.pad0 = 1;
            t.w_w = b.W(ptd + ".conv_tr.Wt"), t.bias_w = b.W(ptd + ".conv_tr.b");
            t.N = 4 * coutT;
            t.epi = EPI_TRCONV, t.act = k < 3 ? 1 : 0;
            t.Lout = (int)Lout, t.Cout = coutT;
            t.res = k < 3 ? aXt[2 - k] : -1;
            t.y = aTDin[k + 1], t.ldy = coutT, t.yBatchStride = Lout * coutT;
            b.finish(t, false);
            b.push_gemm(ptd + ".conv_tr", 1, t);
            b.push_tap("tdec_" + std::to_string(k), aTDin[k + 1], {(int)Lout, coutT}, Lout * coutT);
        }
    }

    // ------------------------------------------------------------------ ISTFT + sum (model_inference.cpp:719-855)
    {
        Op op;
        op.kind = OP_ISTFT;
        op.stream = 0;
        op.name = "istft";
        op.istft = Istft{aDin[4], aStF, aFrames, B, T, S, cWindow, cTwiddle, 1};
        pl.ops.push_back(op);
        Op o2;
        o2.kind = OP_OLA;
        o2.stream = 0;
        o2.name = "ola";
        o2.ola = Ola{aFrames, aTDin[4], aStT, cWss, pl.outOff, B, T, S, (int)seg, (int)G.pad, aDin[4], aStF, cWindow, cTwiddle, cRden};
        pl.ops.push_back(o2);
    }
    pl.arenaFloats = b.top + 64;
    compute_deps(pl);
}

} // namespace dmx
