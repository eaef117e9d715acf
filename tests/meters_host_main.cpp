// The meters' kernel text (csrc/meters.hip) as host code: the staged tiles with their halo, the lane's window, the integer
// histogram and its walk, thread by thread on the CPU (tests/test_meters_cpu.py; the Makefile's meters_host and
// meters_host_asan). The hop energies come from the loudness stage's kernel text, compiled the same way.
//   meters_host_main tp FILE RATE INTERLEAVED CUT     FILE: raw fp32, planar [2][n] or interleaved [n][2]; CUT: 0, or the
//       frame (a multiple of 4) at which the signal is cut into two pieces. Prints the bit pattern of TP as 8 hex digits
//   meters_host_main meters FILE RATE INTERLEAVED     prints "lra_c <int> max_momentary_c <int> max_short_c <int>"
//   meters_host_main filter RATE                      prints F and then the 12 F + 1 taps, one %a per line
#define DMX_LOUDNESS_HOST 1
#define DMX_METERS_HOST 1
#include "../demucs_cpp_amd/csrc/loudness.hip"
#include "../demucs_cpp_amd/csrc/meters.hip"

#include <cstdio>
#include <cstdlib>
#include <string>

static bool read_floats(const char *path, std::vector<float> &x)
{
    FILE *f = std::fopen(path, "rb");
    if (!f)
        return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    x.resize((size_t)bytes / sizeof(float));
    const bool ok = std::fread(x.data(), sizeof(float), x.size(), f) == x.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "filter" && argc == 3)
    {
        dmx::TpFilter f;
        dmx::tp_filter(std::atoi(argv[2]), &f);
        std::printf("%d\n", f.F);
        for (int k = 0; k <= dmx::kTpTaps * f.F; ++k)
            std::printf("%a\n", (double)f.h[k]);
        return 0;
    }
    if (cmd == "tp" && argc == 6)
    {
        std::vector<float> x;
        if (!read_floats(argv[2], x) || x.size() < 2)
            return 2;
        const float tp = dmx::tp_host_measure(x.data(), std::atoi(argv[4]) != 0, (int64_t)(x.size() / 2), std::atoi(argv[3]), std::atoll(argv[5]));
        unsigned u;
        std::memcpy(&u, &tp, sizeof u);
        std::printf("%08x\n", u);
        return 0;
    }
    if (cmd == "meters" && argc == 5)
    {
        std::vector<float> x;
        if (!read_floats(argv[2], x) || x.size() < 2)
            return 2;
        const int rate = std::atoi(argv[3]);
        double L = 0.0;
        int lufsC = 0, lra = 0, maxM = 0, maxS = 0;
        std::vector<double> e;
        if (dmx::loud_host_measure(x.data(), std::atoi(argv[4]) != 0, (int64_t)(x.size() / 2), rate, &L, &lufsC, e) != 0)
            return 2;
        e.push_back(0.0); // H may be 0: keep the pointer valid
        dmx::meters_host(e.data(), (rate + 5) / 10, (int)((e.size() - 1) / 2), &lra, &maxM, &maxS);
        std::printf("lra_c %d max_momentary_c %d max_short_c %d\n", lra, maxM, maxS);
        return 0;
    }
    std::fprintf(stderr, "usage: meters_host_main tp FILE RATE INTERLEAVED CUT | meters FILE RATE INTERLEAVED | filter RATE\n");
    return 1;
}
