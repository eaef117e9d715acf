// The limiter's kernel text (csrc/limiter.hip) as host code: the level, the required reduction, the tiles' aggregates, the
// carry sweeps and the two scans, thread by thread on the CPU (tests/test_limiter_cpu.py; the Makefile's limiter_host and
// limiter_host_asan). The true-peak phases come from the meters' kernel text, compiled the same way.
//   limiter_host_main run FILE RATE INTERLEAVED GAIN CEILING TP QA QR OUT    FILE: raw fp32, planar [2][n] or interleaved
//       [n][2]; GAIN and CEILING: the bit patterns of the floats as 8 hex digits; TP: 1 takes the interpolated phases. Writes
//       M (int32 [n]) and then the gain plane (fp32 [n]) to OUT and prints
//       "peak_out <8 hex> true_peak_out <8 hex> max_reduction <int> limited_frames <int>"
//   limiter_host_main tables OUT            writes LUT (int32 [4096]), THI (fp32 [385]) and TLO (fp32 [4096]) to OUT
//   limiter_host_main slopes RATE ATTACK_MS RELEASE_MS     prints "qa <int> qr <int>", or "error"
//   limiter_host_main workspace N           prints the bytes
#define DMX_METERS_HOST 1
#define DMX_LIMITER_HOST 1
#include "../demucs_cpp_amd/csrc/meters.hip"
#include "../demucs_cpp_amd/csrc/limiter.hip"

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
static float float_of_hex(const char *s)
{
    const unsigned u = (unsigned)std::strtoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}
static unsigned bits_of(float f)
{
    unsigned u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char **argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "run" && argc == 11)
    {
        std::vector<float> x;
        if (!read_floats(argv[2], x) || x.size() < 2)
            return 2;
        const int64_t n = (int64_t)(x.size() / 2);
        std::vector<unsigned char> work;
        dmx::LimHostResult r;
        dmx::lim_host_run(x.data(), std::atoi(argv[4]) != 0, n, std::atoi(argv[3]), float_of_hex(argv[5]), float_of_hex(argv[6]),
                          std::atoi(argv[7]) != 0, std::atoi(argv[8]), std::atoi(argv[9]), work, &r);
        FILE *f = std::fopen(argv[10], "wb");
        if (!f)
            return 2;
        const bool ok = std::fwrite(work.data(), 4, (size_t)n, f) == (size_t)n &&
                        std::fwrite(work.data() + dmx::lim_ws_gain_offset(n), 4, (size_t)n, f) == (size_t)n;
        std::fclose(f);
        if (!ok)
            return 2;
        std::printf("peak_out %08x true_peak_out %08x max_reduction %d limited_frames %lld\n", bits_of(r.peakOut), bits_of(r.truePeakOut),
                    (int)r.maxReduction, (long long)r.limitedFrames);
        return 0;
    }
    if (cmd == "tables" && argc == 3)
    {
        std::vector<int32_t> lut(dmx::kLimLut);
        std::vector<float> thi(dmx::kLimHi), tlo(dmx::kLimLo);
        dmx::lim_tables(lut.data(), thi.data(), tlo.data());
        FILE *f = std::fopen(argv[2], "wb");
        if (!f)
            return 2;
        std::fwrite(lut.data(), 4, lut.size(), f);
        std::fwrite(thi.data(), 4, thi.size(), f);
        std::fwrite(tlo.data(), 4, tlo.size(), f);
        std::fclose(f);
        return 0;
    }
    if (cmd == "slopes" && argc == 5)
    {
        int qa = 0, qr = 0;
        if (dmx::lim_slopes(std::atoi(argv[2]), std::atof(argv[3]), std::atof(argv[4]), &qa, &qr) != 0)
            std::printf("error\n");
        else
            std::printf("qa %d qr %d\n", qa, qr);
        return 0;
    }
    if (cmd == "workspace" && argc == 3)
    {
        std::printf("%lld\n", (long long)dmx::lim_workspace_bytes(std::atoll(argv[2])));
        return 0;
    }
    std::fprintf(stderr, "usage: limiter_host_main run FILE RATE INTERLEAVED GAIN CEILING TP QA QR OUT | tables OUT | slopes RATE ATTACK_MS "
                         "RELEASE_MS | workspace N\n");
    return 1;
}
