// pcm_wav_harness — wraps raw PCM bytes (as the PCM output stage produces them) into a WAV file with the CLI's writer
// (cli/wav.hpp write_pcm_file), reads the file back with the CLI's reader and dumps the decoded samples as raw float32
// (interleaved stereo): lets the CPU tests check the header and the round trip of every output encoding.
//   pcm_wav_harness <encoding 0|1|2> <rate> <in.raw> <out.wav> <dump.f32>
#include "wav.hpp"

int main(int argc, const char **argv)
{
    if (argc != 6)
        return 2;
    const int encoding = atoi(argv[1]), rate = atoi(argv[2]);
    FILE *f = fopen(argv[3], "rb");
    if (!f)
        return 3;
    std::vector<unsigned char> raw;
    for (int ch; (ch = fgetc(f)) != EOF;)
        raw.push_back((unsigned char)ch);
    fclose(f);
    const dmx_output_spec spec{encoding, DMX_CLIP_NONE, -1};
    const int64_t per = dmx_output_bytes(&spec, 1);
    if (per <= 0 || raw.size() % (size_t)per)
        return 4;
    const int64_t n = (int64_t)(raw.size() / (size_t)per);
    if (!wavio::write_pcm_file(raw.data(), n, encoding, argv[4], rate))
        return 5;
    demucscpp::StereoMatrix audio;
    int got = 0;
    setenv("DMX_RESAMPLE", "0", 1);
    if (rate == demucscpp::SUPPORTED_SAMPLE_RATE)
    {
        if (!wavio::load_audio_file(argv[4], audio, &got))
            return 1;
        f = fopen(argv[5], "wb");
        if (!f)
            return 3;
        fwrite(audio.data.data(), sizeof(float), audio.data.size(), f);
        fclose(f);
    }
    std::cout << "frames " << n << std::endl;
    return 0;
}
