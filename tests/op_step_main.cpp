// op_step_main.cpp — the step interface of tests/cpu_interp.cpp as a stand-alone program, for a run under AddressSanitizer / UBSan
// (tests/test_op_reference_cpu.py builds it with -fsanitize=address,undefined and starts it as a child process).
//   op_step_main MODEL SEG BATCH GEMM KVPLANES
// steps every op of the plan in fp32 and in double (a fused inverse STFT + overlap-add chained), writes the operands of every
// attention op through interp_set_attention first, and reads every accessor.
#include "cpu_interp.cpp"

#include <random>

int main(int argc, char **argv)
{
    if (argc < 6)
        return 2;
    void *h = interp_create_chosen(argv[1], atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (!h)
        return 3;
    Interp *it = (Interp *)h;
    std::mt19937 rng(7);
    std::normal_distribution<float> nd(0.f, 0.1f);
    for (i64 i = 0; i < (i64)it->pl.B * it->pl.geo.seg * 2; ++i)
        interp_arena(h)[interp_mix_off(h) + i] = nd(rng);
    const int n = interp_n_ops(h);
    char buf[4096];
    double sum = 0;
    i64 writes = 0;
    for (int i = 0; i < n; ++i)
    {
        const Op &op = it->pl.ops[(size_t)i];
        if (interp_op_info(h, i, buf, sizeof(buf)) <= 0)
            return 4;
        if (op.kind == OP_TAP)
            continue;
        if (op.kind == OP_ATTENTION || op.kind == OP_LOCAL_ATTN)
        {
            // interp_set_attention: dense operands written over what the chain left in the op's read ranges
            const bool loc = op.kind == OP_LOCAL_ATTN;
            const i64 nq = loc ? (i64)op.la.B * op.la.T * op.la.H : (i64)op.at.B * op.at.Tq * op.at.H * op.at.hs;
            const i64 nk = loc ? nq : (i64)op.at.B * op.at.Tk * op.at.H * op.at.hs;
            std::normal_distribution<float> unit(0.f, 1.f);
            std::vector<float> q((size_t)nq), k((size_t)nk), v((size_t)nk), d(loc ? (size_t)op.la.B * op.la.T * 16 : 0);
            for (std::vector<float> *a : {&q, &k, &v, &d})
                for (float &x : *a)
                    x = unit(rng);
            if (interp_set_attention(h, i, q.data(), k.data(), v.data(), loc ? d.data() : nullptr) != 0)
                return 9;
            if (interp_set_attention(h, i, q.data(), k.data(), v.data(), loc ? nullptr : q.data()) != -1) // decay of the other kind
                return 10;
        }
        else if (interp_set_attention(h, i, nullptr, nullptr, nullptr, nullptr) != -1)
            return 11;
        if (interp_step(h, i, 0) != 0)
            return 6;
        const bool chained = op.kind == OP_OLA && op.ola.x >= 0 && i > 0 && it->pl.ops[(size_t)i - 1].kind == OP_ISTFT;
        if (interp_step(h, i, 1 | (op.kind == OP_IGEMM && op.g.hterms ? 2 : 0) | (chained ? 4 : 0)) != 0)
            return 7;
        const unsigned char *mask = interp_mask(h);
        const double *r = interp_precise(h);
        const float *s = interp_magnitude(h);
        for (i64 k = 0; k < interp_arena_floats(h); ++k)
            if (mask[k])
                sum += r[k] + s[k], ++writes;
        // interp_census: the counters of the precise step; interp_operands: every role's range lies inside the arena (W. words:
        // inside the packed weights) - the crafted-operand tests write through them
        long long cen[64];
        const int nc = interp_census(cen, 64);
        if (nc <= 0 || nc > 64)
            return 12;
        for (int k = 0; k < nc; ++k)
            sum += (double)cen[k] * 1e-9;
        char roles[1024];
        if (interp_operands(h, i, roles, sizeof(roles)) < 0)
            return 13;
        for (char *w = strtok(roles, " "); w; w = strtok(nullptr, " "))
        {
            long long f[6];
            char role[32];
            if (sscanf(w, "%31[^=]=%lld:%lld:%lld:%lld:%lld:%lld", role, f, f + 1, f + 2, f + 3, f + 4, f + 5) != 7)
                continue; // (conv= has more fields and names no range)
            if (!strcmp(role, "rows") || !strcmp(role, "reduce"))
                continue;
            const i64 last = f[0] + (f[5] - 1) * f[4] + (f[1] - 1) * f[3] + f[2];
            const i64 cap = strncmp(role, "W.", 2) ? interp_arena_floats(h) : interp_weight_floats(h);
            if (f[0] < 0 || last > cap)
                return 14;
        }
        double *pr;
        float *ps;
        const i64 np = interp_planes(h, &pr, &ps);
        for (i64 k = 0; k < np; ++k)
            sum += pr[k] + ps[k];
    }
    std::vector<float> out((size_t)((i64)it->pl.B * it->pl.S * 2 * it->pl.geo.seg));
    std::memcpy(out.data(), interp_arena(h) + interp_out_off(h), out.size() * sizeof(float));
    for (float v : out)
        sum += v;
    sum += interp_weights(h)[interp_weight_floats(h) - 1];
    interp_free(h);
    printf("steps ok: %d ops, %lld elements written, checksum %.6g\n", n, (long long)writes, sum);
    return std::isfinite(sum) ? 0 : 8;
}
