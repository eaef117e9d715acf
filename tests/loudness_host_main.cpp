// The loudness stage's kernel text (csrc/loudness.hip) as host code: the chunked state-space scan, the hop straddle and the
// fixed-order sums, lane by lane on the CPU (tests/test_loudness_cpu.py; the Makefile's loudness_host and loudness_host_asan).
//   loudness_host_main measure FILE RATE INTERLEAVED   FILE: raw fp32, planar [2][n] or interleaved [n][2]
//       prints "L <%a> lufs_c <int> H <int>" and then the 2 H hop energies e[c][j], one %a per line
//   loudness_host_main coef RATE                       prints the ten coefficients, one %a per line
//   loudness_host_main table FILE                      writes the gain table, 12001 floats
#define DMX_LOUDNESS_HOST 1
#include "../demucs_cpp_amd/csrc/loudness.hip"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "coef" && argc == 3)
    {
        const int rate = std::atoi(argv[2]);
        if (rate < dmx::kLoudMinRate)
            return 2;
        double c[10];
        dmx::loud_coefficients(rate, c);
        for (double v : c)
            std::printf("%a\n", v);
        return 0;
    }
    if (cmd == "table" && argc == 3)
    {
        std::vector<float> T(dmx::kLoudGainSteps);
        dmx::loud_gain_table(T.data());
        FILE *f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(T.data(), sizeof(float), T.size(), f) != T.size())
            return 2;
        std::fclose(f);
        return 0;
    }
    if (cmd == "measure" && argc == 5)
    {
        FILE *f = std::fopen(argv[2], "rb");
        if (!f)
            return 2;
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        std::vector<float> x((size_t)bytes / sizeof(float));
        if (std::fread(x.data(), sizeof(float), x.size(), f) != x.size())
            return 2;
        std::fclose(f);
        const int64_t n = (int64_t)(x.size() / 2);
        double L = 0.0;
        int lufsC = 0;
        std::vector<double> e;
        if (dmx::loud_host_measure(x.data(), std::atoi(argv[4]) != 0, n, std::atoi(argv[3]), &L, &lufsC, e) != 0)
            return 2;
        std::printf("L %a lufs_c %d H %d\n", L, lufsC, (int)(e.size() / 2));
        for (double v : e)
            std::printf("%a\n", v);
        return 0;
    }
    std::fprintf(stderr, "usage: loudness_host_main measure FILE RATE INTERLEAVED | coef RATE | table FILE\n");
    return 1;
}
