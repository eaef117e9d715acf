// The FLAC output stage's kernel text (csrc/flac.hip) compiled as host code, as a stand-alone program: no GPU, no HIP.
// Built plain and with -fsanitize=address,undefined (make flac_host / flac_host_asan); tests/test_flac_lpc_cpu.py runs it
// over the crafted inputs and compares with the specification's bytes (tests/flac_spec.py, tests/flac_lpc_spec.py).
//
//   flac_host_main LIST        LIST: one job per line, "<bits 16|24> <level 0|1|2> <rate> <PCM file> <output file>"
//
// The PCM file holds the interleaved little-endian bytes that csrc/pcm.hip writes; the output file is the .flac file. The
// PCM, the workspace and the output live in heap blocks of exactly their sizes (the PCM rounded up to 16 bytes, as the
// PCM stage pads it), so that a load or store past an end is a sanitizer report.
#define DMX_FLAC_HOST 1
#include "../demucs_cpp_amd/csrc/flac.hip"

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

static int run(int bits, int level, int rate, const std::string &in, const std::string &outPath)
{
    std::ifstream fi(in, std::ios::binary);
    if (!fi)
        return 2;
    std::string data((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int frameBytes = 2 * bits / 8;
    if ((bits != 16 && bits != 24) || data.empty() || data.size() % (size_t)frameBytes)
        return 3;
    const int64_t n = (int64_t)(data.size() / (size_t)frameBytes);
    const int64_t bound = dmx::flac_bound(bits, n), workBytes = dmx::flac_workspace_bytes(bits, n);
    if (bound < 0 || workBytes < 0)
        return 4;
    const size_t pcmBytes = (data.size() + 15) / 16 * 16;
    unsigned char *pcm = (unsigned char *)aligned_alloc(16, pcmBytes);
    memset(pcm, 0, pcmBytes);
    memcpy(pcm, data.data(), data.size());
    unsigned char *work = (unsigned char *)aligned_alloc(16, (size_t)workBytes); // not initialised, as on the device
    unsigned char *out = (unsigned char *)malloc((size_t)bound + 3);
    memset(out, 0x5a, (size_t)bound + 3);
    long long size = -1;
    int rc = dmx::flac_host_encode(pcm, bits, n, rate, level, out + 3, &size, work) ? 5 : 0; // an output at an odd address
    if (!rc && (size < 42 || size > bound))
        rc = 6;
    for (int i = 0; !rc && i < 3; ++i)
        if (out[i] != 0x5a)
            rc = 7;
    for (int64_t i = size; !rc && i < bound; ++i)
        if (out[3 + i] != 0x5a)
            rc = 7; // a store behind the file
    if (!rc)
    {
        std::ofstream fo(outPath, std::ios::binary);
        fo.write((const char *)out + 3, (std::streamsize)size);
    }
    free(out), free(work), free(pcm);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc != 2)
    {
        std::cerr << "usage: " << argv[0] << " LIST\n";
        return 64;
    }
    std::ifstream list(argv[1]);
    std::string line;
    int jobs = 0;
    while (std::getline(list, line))
    {
        std::istringstream ls(line);
        int bits, level, rate;
        std::string in, out;
        if (!(ls >> bits >> level >> rate >> in >> out))
            continue;
        const int rc = run(bits, level, rate, in, out);
        if (rc)
        {
            std::cerr << "job failed (" << rc << "): " << line << "\n";
            return 1;
        }
        ++jobs;
    }
    std::cout << jobs << " jobs\n";
    return 0;
}
