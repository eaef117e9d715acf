// Test helper for demucscpp::parse_remix / remix_two_stems (demucscpp_hip.hpp), no GPU:
//   remix_parse_harness parse <nb_sources> <text>              -> one line per output: NAME then the row's gains as fp32 bit patterns (hex)
//   remix_parse_harness two_stems <nb_sources> <stem> <method> -> the same for remix_two_stems
// exit 2 and the exception's message on stderr when the text is refused
#include <cstdio>
#include <cstring>

#include "demucscpp_hip.hpp"

int main(int argc, char **argv)
{
    if (argc < 4)
        return 1;
    const int S = std::atoi(argv[2]);
    demucscpp::remix_options ro;
    try
    {
        if (std::string(argv[1]) == "parse")
            ro = demucscpp::parse_remix(argv[3], S);
        else if (std::string(argv[1]) == "two_stems" && argc >= 5)
            ro = demucscpp::remix_two_stems(S, std::atoi(argv[3]), std::atoi(argv[4]));
        else
            return 1;
    }
    catch (const std::exception &e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    for (size_t o = 0; o < ro.names.size(); ++o)
    {
        std::printf("%s", ro.names[o].c_str());
        for (int s = 0; s <= S; ++s)
        {
            unsigned u;
            std::memcpy(&u, &ro.gains[o * (size_t)(S + 1) + (size_t)s], 4);
            std::printf(" %08x", u);
        }
        std::printf("\n");
    }
    return 0;
}
