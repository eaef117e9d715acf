// The FLAC input stage's kernel text (csrc/flac_in.hip) compiled as host code, as a stand-alone program: no GPU, no HIP.
// Built plain and with -fsanitize=address,undefined (make flac_in_host / flac_in_host_asan); tests/test_flac_in_cpu.py runs
// it over a corpus and compares with the reference decoder of tests/flac_in_spec.py.
//
//   flac_in_host_main LIST        LIST: one job per line, "<encoding 0|1|2> <input file> <output file>"
//
// Output file: four int64 {rc, status, good, n} and then, for rc 0, the n frames in the encoding asked for; rc 1: the probe
// refused the file and its message follows as text. The file, the workspace and the output live in heap blocks of exactly
// their sizes, so that a load or store past an end is a sanitizer report.
#define DMX_FLAC_IN_HOST 1
#include "../demucs_cpp_amd/csrc/flac_in.hip"

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

static int run(int encoding, const std::string &in, const std::string &outPath)
{
    std::ifstream fi(in, std::ios::binary);
    if (!fi)
        return 2;
    std::string data((std::istreambuf_iterator<char>(fi)), std::istreambuf_iterator<char>());
    const int64_t bytes = (int64_t)data.size();
    unsigned char *file = (unsigned char *)malloc(bytes ? (size_t)bytes : 1);
    memcpy(file, data.data(), (size_t)bytes);
    std::ofstream fo(outPath, std::ios::binary);
    dmx_flac_info info;
    memset(&info, 0, sizeof info);
    char msg[160] = "";
    int64_t head[4] = {0, 0, 0, 0};
    if (dmx::flac_in_probe(file, bytes, &info, msg, sizeof msg) != 0)
    {
        head[0] = 1;
        fo.write((const char *)head, sizeof head);
        fo.write(msg, (std::streamsize)strlen(msg));
        free(file);
        return 0;
    }
    const int64_t workBytes = dmx::flac_in_workspace_bytes(&info, bytes);
    if (workBytes < 0)
    {
        free(file);
        return 3;
    }
    const size_t frameBytes = encoding == DMX_PCM_F32 ? 8 : encoding == DMX_PCM_S16 ? 4 : 6;
    const size_t outBytes = DMX_OUTPUT_STRIDE((size_t)info.total_samples * frameBytes);
    void *work = malloc((size_t)workBytes); // not initialised, as on the device
    unsigned char *out = (unsigned char *)malloc(outBytes);
    memset(out, 0xa5, outBytes);
    long long status[2] = {-1, -1};
    const int rc = dmx::flac_in_host_decode(file, bytes, &info, encoding, out, status, work);
    head[0] = rc ? 4 : 0, head[1] = status[0], head[2] = status[1], head[3] = info.total_samples;
    fo.write((const char *)head, sizeof head);
    fo.write((const char *)out, (std::streamsize)((size_t)info.total_samples * frameBytes));
    free(out), free(work), free(file);
    return 0;
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
        int enc;
        std::string in, out;
        if (!(ls >> enc >> in >> out))
            continue;
        const int rc = run(enc, in, out);
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
