// attention_select_harness.cpp — csrc/attention_select.h (host arithmetic, no HIP) as a stand-alone CPU program
// (tests/test_attention_select_cpu.py).
//   attention_select_harness barriers NTMAX
//       one line per nt = 1 .. NTMAX: nt, barriers of half A, barriers of half B (att_pair_barriers)
//   attention_select_harness plans MODEL SEG:BATCH:GEMM ...
//       the plan a context of that GEMM mode builds (gemm_select.h build_chosen_plan, as exec.cpp dmx_get_plan calls it; every weight
//       exact), one line per OP_ATTENTION: seg batch gemm name Tq Tk H hs planes, then att_select_form under DMX_ATT_PAIR = 0, unset, 2
//   attention_select_harness form TQ TK H B HS PLANES MODE
//       att_select_form of a hand-made shape
#include "../demucs_cpp_amd/csrc/model_pack.cpp"
#include "../demucs_cpp_amd/csrc/plan.cpp"
#include "../demucs_cpp_amd/csrc/gemm_select.cpp"
#include "../demucs_cpp_amd/csrc/attention_select.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dmx;

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "barriers"))
    {
        for (int nt = 1; nt <= atoi(argv[2]); ++nt)
            printf("%d %d %d\n", nt, att_pair_barriers(nt, 0), att_pair_barriers(nt, 1));
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "form"))
    {
        printf("%s\n", att_form_name(att_select_form(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]) != 0,
                                                     atoi(argv[8]))));
        return 0;
    }
    if (argc < 4 || strcmp(argv[1], "plans"))
        return 2;
    PackedModel pm;
    std::string err;
    if (!load_and_pack(argv[2], pm, err))
    {
        fprintf(stderr, "%s\n", err.c_str());
        return 3;
    }
    const std::vector<i64> none;
    GemmModelFacts f;
    f.bf16Planes = f.fp16Plane = true;
    f.planeDelta = (i64)pm.blob.size() + 512;
    f.inexactW = f.inexactH = &none;
    for (int a = 3; a < argc; ++a)
    {
        long long seg;
        int B, gemm;
        if (sscanf(argv[a], "%lld:%d:%d", &seg, &B, &gemm) != 3)
            return 4;
        Plan pl;
        build_chosen_plan(pm, seg, B, gemm, gemm != GEMM_F32 && pm.arch != 3, f, 1, pl);
        for (const Op &op : pl.ops)
            if (op.kind == OP_ATTENTION)
            {
                const Attention &t = op.at;
                const bool planes = t.kpl >= 0 && t.vt >= 0;
                printf("%lld %d %d %s %d %d %d %d %d", seg, B, gemm, op.name.c_str(), t.Tq, t.Tk, t.H, t.hs, planes ? 1 : 0);
                for (int mode = 0; mode < 3; ++mode)
                    printf(" %s", att_form_name(att_select_form(t.Tq, t.Tk, t.H, t.B, t.hs, planes, mode)));
                printf("\n");
            }
    }
    return 0;
}
