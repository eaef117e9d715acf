// The multi-track plan (demucs_cpp_amd/csrc/tracks_plan.cpp) without a GPU: builds the plan of a case and prints it as JSON.
// A case is the numbers  seg stride B Q N pcm n[T] shifts[T*Q*N]  (T follows from their count), given on the command line
// or one case per line on stdin; one line of JSON per case. The ensemble kernel's tail cap is not applied (it belongs to
// the executor's kernels, not to the plan). Built with g++ alone: make plan_harness. tests/test_tracks_plan_cpu.py reads it.
#include "../demucs_cpp_amd/csrc/tracks_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>

static void print_list(const char *name, const std::vector<int64_t> &v)
{
    printf(",\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i)
        printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]");
}

static void print_plan(const TracksPlan &p)
{
    printf("{\"T\":%d,\"Q\":%d,\"N\":%d,\"B\":%d,\"seg\":%lld,\"stride\":%lld", p.T, p.Q, p.N, p.B, (long long)p.seg, (long long)p.stride);
    printf(",\"ringBlocks\":%lld,\"nSlots\":%d,\"nmax\":%lld,\"Mtot\":%lld", (long long)p.ringBlocks, p.nSlots, (long long)p.nmax, (long long)p.Mtot);
    const char *sep = "";
    printf(",\"jobs\":[");
    for (const TrackJob &j : p.jobs)
        printf("%s{\"n\":%lld,\"kFirst\":%d,\"kLast\":%d,\"slot\":%d,\"takeover\":%d}", sep, (long long)j.n, j.kFirst, j.kLast, j.slot, (int)j.takeover), sep = ",";
    printf("],\"tm\":["), sep = "";
    for (const TrackModel &x : p.tm)
        printf("%s{\"g0\":%lld,\"m\":%lld,\"c0\":%d,\"nMin\":%d,\"nMax\":%d}", sep, (long long)x.g0, (long long)x.m, x.c0, x.nMin, x.nMax), sep = ",";
    printf("],\"copies\":["), sep = "";
    for (const TrackCopy &c : p.copies)
        printf("%s{\"len\":%lld,\"shift\":%d,\"nseg\":%d}", sep, (long long)c.len, c.shift, c.nseg), sep = ",";
    printf("],\"items\":["), sep = "";
    for (const std::vector<TrackItem> &its : p.items)
    {
        printf("%s[", sep), sep = "";
        for (const TrackItem &it : its)
            printf("%s[%d,%d,%d]", sep, it.t, it.k, it.g), sep = ",";
        printf("]"), sep = ",";
    }
    printf("],\"batches\":["), sep = "";
    for (const TrackBatch &b : p.batches)
        printf("%s{\"q\":%d,\"g0\":%lld,\"nb\":%d}", sep, b.q, (long long)b.g0, b.nb), sep = ",";
    printf("]");
    print_list("cum", p.cum);
    printf(",\"pieces\":["), sep = "";
    for (const std::vector<TrackPiece> &pcs : p.pieces)
    {
        printf("%s[", sep), sep = "";
        for (const TrackPiece &pc : pcs)
        {
            printf("%s{\"t\":%d,\"lo\":%lld,\"hi\":%lld,\"itemLo\":[", sep, pc.t, (long long)pc.lo, (long long)pc.hi);
            for (int q = 0; q < p.Q; ++q)
                printf("%s%lld", q ? "," : "", (long long)p.pieceItems[pc.item0 + (size_t)q]);
            printf("]}"), sep = ",";
        }
        printf("]"), sep = ",";
    }
    printf("]");
    print_list("M", p.M), print_list("R", p.R), print_list("ringOff", p.ringOff);
    printf(",\"pcm\":["), sep = "";
    for (const std::vector<PcmRange> &rs : p.pcm)
    {
        printf("%s[", sep), sep = "";
        for (const PcmRange &r : rs)
            printf("%s[%d,%lld,%lld]", sep, r.t, (long long)r.lo, (long long)r.hi), sep = ",";
        printf("]"), sep = ",";
    }
    printf("]}\n");
}

static int run_case(const std::vector<long long> &v)
{
    if (v.size() < 6 || v[0] < 1 || v[1] < 1 || v[2] < 1 || v[3] < 1 || v[4] < 1 || (v.size() - 6) % (size_t)(1 + v[3] * v[4]) != 0 ||
        v.size() == 6)
    {
        fprintf(stderr, "tracks_plan_harness: a case is  seg stride B Q N pcm n[T] shifts[T*Q*N]\n");
        return 2;
    }
    const int B = (int)v[2], Q = (int)v[3], N = (int)v[4], T = (int)((v.size() - 6) / (size_t)(1 + Q * N));
    std::vector<int64_t> n((size_t)T);
    std::vector<int> shifts((size_t)T * Q * N);
    for (int t = 0; t < T; ++t)
        n[(size_t)t] = v[6 + (size_t)t];
    for (size_t i = 0; i < shifts.size(); ++i)
        shifts[i] = (int)v[6 + (size_t)T + i];
    for (int t = 0; t < T; ++t)
        if (n[(size_t)t] < 2)
            return fprintf(stderr, "tracks_plan_harness: n[%d] < 2\n", t), 2;
    for (int s : shifts)
        if (s < 0 || s >= DMX_MAX_SHIFT)
            return fprintf(stderr, "tracks_plan_harness: shift %d not in [0, %d)\n", s, DMX_MAX_SHIFT), 2;
    TracksPlan p;
    std::string err;
    const int rc = tracks_plan_build(p, T, n.data(), Q, N, shifts.data(), v[0], v[1], B, v[5] != 0, -1, err);
    if (rc != DMX_OK)
        printf("{\"error\":%d,\"message\":\"%s\"}\n", rc, err.c_str());
    else
        print_plan(p);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1)
    {
        std::vector<long long> v;
        for (int i = 1; i < argc; ++i)
            v.push_back(atoll(argv[i]));
        return run_case(v);
    }
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        std::vector<long long> v;
        for (long long x; in >> x;)
            v.push_back(x);
        if (v.empty())
            continue;
        if (int rc = run_case(v))
            return rc;
    }
    return 0;
}
