// The multi-track plan of a call with tracks at other sample rates (demucs_cpp_amd/csrc/tracks_plan.cpp) without a GPU: prints
// the 44.1 kHz pieces, the native-rate ranges and the PCM ranges of a case as JSON.
// A case is the numbers  seg stride B Q N pcm T  m[T] rate[T]  shifts[T*Q*N]  on the command line or one case per line on
// stdin; one line of JSON per case. Built with g++ from tracks_plan.cpp alone: make rates_harness
// (CXXFLAGS_RATES=-fsanitize=address,undefined RATES_OUT=... builds the sanitizer form). tests/test_track_rates_cpu.py reads it.
#include "../demucs_cpp_amd/csrc/tracks_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <sstream>

static void print_ranges(const char *name, const std::vector<std::vector<PcmRange>> &v)
{
    printf(",\"%s\":[", name);
    const char *sep = "";
    for (const std::vector<PcmRange> &rs : v)
    {
        printf("%s[", sep), sep = "";
        for (const PcmRange &r : rs)
            printf("%s[%d,%lld,%lld]", sep, r.t, (long long)r.lo, (long long)r.hi), sep = ",";
        printf("]"), sep = ",";
    }
    printf("]");
}

static int run_case(const std::vector<long long> &v)
{
    const size_t T = v.size() > 6 && v[6] > 0 ? (size_t)v[6] : 0;
    if (T == 0 || v[0] < 1 || v[1] < 1 || v[2] < 1 || v[3] < 1 || v[4] < 1 || v.size() != 7 + 2 * T + T * (size_t)(v[3] * v[4]))
    {
        fprintf(stderr, "track_rates_harness: a case is  seg stride B Q N pcm T  m[T] rate[T]  shifts[T*Q*N]\n");
        return 2;
    }
    const int B = (int)v[2], Q = (int)v[3], N = (int)v[4];
    std::vector<int64_t> m(T), n44(T);
    std::vector<int> rates(T), shifts(T * (size_t)(Q * N));
    for (size_t t = 0; t < T; ++t)
    {
        m[t] = v[7 + t], rates[t] = (int)v[7 + T + t];
        if (m[t] < 1 || rates[t] < 1)
            return fprintf(stderr, "track_rates_harness: track %zu: %lld frames at %d Hz\n", t, (long long)m[t], rates[t]), 2;
        const int64_t g = std::gcd(rates[t], 44100), up = 44100 / g, down = rates[t] / g;
        n44[t] = (m[t] * up + down - 1) / down; // dmx_resample_length
        if (n44[t] < 2)
            return fprintf(stderr, "track_rates_harness: track %zu leaves %lld frames at 44100 Hz\n", t, (long long)n44[t]), 2;
    }
    for (size_t i = 0; i < shifts.size(); ++i)
    {
        shifts[i] = (int)v[7 + 2 * T + i];
        if (shifts[i] < 0 || shifts[i] >= DMX_MAX_SHIFT)
            return fprintf(stderr, "track_rates_harness: shift %d not in [0, %d)\n", shifts[i], DMX_MAX_SHIFT), 2;
    }
    TracksPlan p;
    std::string err;
    const int rc = tracks_plan_build(p, (int)T, n44.data(), Q, N, shifts.data(), v[0], v[1], B, v[5] != 0, -1, err, rates.data(), m.data());
    if (rc != DMX_OK)
    {
        printf("{\"error\":%d,\"message\":\"%s\"}\n", rc, err.c_str());
        return 0;
    }
    printf("{\"mmax\":%lld,\"nmax\":%lld,\"jobs\":[", (long long)p.mmax, (long long)p.nmax);
    const char *sep = "";
    for (const TrackJob &j : p.jobs)
        printf("%s{\"n\":%lld,\"m\":%lld,\"rate\":%d,\"kFirst\":%d,\"kLast\":%d}", sep, (long long)j.n, (long long)j.m, j.rate, j.kFirst, j.kLast), sep = ",";
    printf("],\"pieces\":["), sep = "";
    for (const std::vector<TrackPiece> &pcs : p.pieces)
    {
        printf("%s[", sep), sep = "";
        for (const TrackPiece &pc : pcs)
            printf("%s[%d,%lld,%lld]", sep, pc.t, (long long)pc.lo, (long long)pc.hi), sep = ",";
        printf("]"), sep = ",";
    }
    printf("]");
    print_ranges("native", p.native);
    print_ranges("pcm", p.pcm);
    printf("}\n");
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
