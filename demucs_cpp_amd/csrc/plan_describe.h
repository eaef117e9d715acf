// plan_describe.h — one op of a plan as a line of key=value words: what dmx_debug_op_info (debug_api.cpp) reports and what
// tests/cpu_interp.cpp reports for its own plan, so that the two plans can be compared word by word. Plain C++, no HIP.
#pragma once
#include "attention_select.h"
#include "gemm_tiles.h"
#include <algorithm>
#include <cstdio>
#include <string>

namespace dmx
{
inline std::string describe_choice(const IGemm &g)
{
    char t[256];
    snprintf(t, sizeof(t), "cfg=%d family=%d arith=%d wnf=%d label=%s BM=%d BN=%d NB=%d", g.cfg, g.choice.family, g.choice.arith, g.choice.wnf,
             g.choice.label ? g.choice.label : "-", kTileCfgs[g.cfg].BM, kTileCfgs[g.cfg].BN, g.NB);
    return t;
}

// name kind stream reads= writes= scratch= (arena ranges lo:hi, ... : op_access, and what the kernel may write beyond its results),
// then the words of the op's kind: the GEMM's shape, epilogue and kernel choice; elsewhere label= and the sizes (K: the longest
// sum, T: steps) the error bounds of tests/op_reference.py are derived from
inline std::string describe_op(const Op &op)
{
    std::vector<Range> rd, wr, scr;
    op_access(op, rd, wr);
    if (op.kind == OP_STATS_REDUCE && op.sr.scratch >= 0)
        scr.push_back(Range{op.sr.scratch, op.sr.scratch + (i64)op.sr.B * op.sr.nchunk * 4});
    if (op.kind == OP_GROUP_STATS && op.gs.scratch >= 0)
        scr.push_back(Range{op.gs.scratch, op.gs.scratch + (i64)op.gs.B * op.gs.G * 32 * 4});
    if (op.kind == OP_LSTM && op.lstm.sync >= 0)
        scr.push_back(Range{op.lstm.sync, op.lstm.sync + lstm_xchg_floats(op.lstm.B, op.lstm.T, op.lstm.H)});
    std::string all = "name=" + op.name + " kind=" + std::to_string(op.kind) + " stream=" + std::to_string(op.stream);
    const std::vector<Range> *lists[3] = {&rd, &wr, &scr};
    const char *keys[3] = {" reads=", " writes=", " scratch="};
    for (int k = 0; k < 3; ++k)
    {
        all += keys[k];
        for (const Range &r : *lists[k])
            all += std::to_string(r.lo) + ":" + std::to_string(r.hi) + ",";
    }
    auto word = [&](const char *k, i64 v) { all += std::string(" ") + k + "=" + std::to_string(v); };
    switch (op.kind)
    {
    case OP_IGEMM:
    {
        const IGemm &g = op.g;
        const i64 M = (i64)g.B * g.P1 * g.P0;
        word("K", g.K), word("N", g.N), word("M", M), word("pro", g.pro), word("epi", g.epi), word("act", g.act), word("res", g.res >= 0);
        word("stat", g.rowstat >= 0), word("hterms", g.hterms);
        word("y", g.y), word("ldy", g.ldy), word("Kp", g.Kp), word("w_w", g.w_w), word("bias_w", g.bias_w), word("kvCol0", g.kvCol0);
        all += " " + describe_choice(g);
        if (g.rowstat >= 0)
            all += " rowstat=" + std::to_string(g.rowstat) + ":" + std::to_string(g.rowstat + M * std::max(g.NB, 1) * 2);
        if (g.kv >= 0)
            word("kv", g.kv), word("kvPlane", (i64)g.B * g.kvT * g.kvH * g.kvHs);
        break;
    }
    case OP_ATTENTION:
        all += std::string(" label=") + (op.at.split ? "attention_split" : "attention");
        word("K", op.at.hs), word("T", op.at.Tk), word("split", op.at.split), word("planes", op.at.kpl >= 0);
        word("Tq", op.at.Tq), word("H", op.at.H), word("B", op.at.B);
        all += std::string(" form=") + att_form_name(op.at.form);
        {
            char sc[32];
            snprintf(sc, sizeof(sc), " scale=%.9g", (double)op.at.scale);
            all += sc;
        }
        if (op.at.kpl >= 0)
            word("kpl", op.at.kpl), word("vt", op.at.vt), word("kvPlane", (i64)op.at.B * op.at.Tk * op.at.H * op.at.hs);
        break;
    case OP_STATS_REDUCE: all += " label=stats_reduce", word("K", (i64)op.sr.R * op.sr.NB); break;
    case OP_STFT: all += " label=stft", word("K", 4096); break;
    case OP_LAYERNORM: all += " label=layernorm", word("K", op.ln.D); break;
    case OP_GN_APPLY: all += " label=gn_apply"; break;
    case OP_ISTFT: all += " label=istft", word("K", 4096), word("fused", op.istft.fused); break;
    case OP_OLA: all += op.ola.x >= 0 ? " label=istft_ola" : " label=ola", word("K", 4096), word("fused", op.ola.x >= 0); break;
    case OP_GROUP_STATS: all += " label=group_stats", word("K", (i64)op.gs.rows * (op.gs.C / op.gs.G)); break;
    case OP_GN_ACT: all += " label=gn_act", word("mode", op.ga.mode); break;
    case OP_LSTM: all += " label=lstm", word("K", op.lstm.H), word("T", op.lstm.T); break;
    case OP_LOCAL_ATTN: all += " label=local_attn", word("K", op.la.H / 4), word("T", op.la.T); break;
    case OP_DCONV_ROW: all += " label=dconv_row", word("K", 3 * op.dr.C), word("T", op.dr.T), word("H", op.dr.hid); break;
    default: all += " label=tap"; break;
    }
    return all;
}
} // namespace dmx
