// demucs_batch.cpp.main — many tracks in one call (no reference counterpart: the reference's CLIs take one file):
//   demucs_batch.cpp.main [--shifts N] [--overlap F] [--shift-offsets a,b,...] [--two-stems NAME]
//                         [--other-method add|minus|none] [--remix NAME=TERMS,...]
//                         [--clip-mode rescale|clamp|none] [--int16|--int24|--float32] [--flac] [--flac-level N] [--bag-weights w00,w01,...]
//                         [--loudnorm LUFS | --loudnorm-each LUFS | --loudness] [--max-peak DB] [--true-peak] [--meters]
//                         [--limit] [--limit-attack MS] [--limit-release MS]
//                         <model> <out dir> <wav or flac file>...
// An input whose content begins with "fLaC" (or an ID3v2 tag and "fLaC") is a FLAC file. When every input is a FLAC file
// (at 44.1 kHz, or with DMX_RESAMPLE=1 at any rate) the files go to the GPU as they are and are decoded there
// (dmx_tracks_infer_from_flac, dmx_tracks_infer_from_flac_rates; csrc/flac_in.hip) - the outputs are those of the equivalent
// WAV inputs; otherwise a FLAC file is decoded on the GPU (dmx_flac_decode) and treated as a WAV file of its rate (DMX_RESAMPLE).
// -> <out dir>/<wav file stem>/target_{i}_{drums|bass|other|vocals|guitar|piano}.wav (stereo float32), every file
// byte-identical to what demucs.cpp.main / demucs_v3.cpp.main writes for that input alone. The model's architecture
// (HTDemucs v4 4s / 6s, or Demucs v3) is read from the file; the segments of all tracks share batches
// (dmx_tracks_infer through demucscpp::demucs_inference_batch / demucscpp_v3::demucs_v3_inference_batch).
// Environment: DMX_DEVICE (GPU index), DMX_SHIFT_OFFSET (fixed shift instead of rand(), drawn per track in order),
// DMX_BATCH (segments in flight), DMX_RESAMPLE (wav.hpp).
// Options (demucs's --shifts / --overlap; dmx_tracks_infer_opts through the demucscpp::inference_options overloads):
//   --shifts N               run each track as N shifted copies and average them (1 <= N <= 32; default 1)
//   --overlap F              segment overlap, 0 <= F <= 0.9 (default 0.25)
//   --shift-offsets a,b,...  the N copies' shift offsets in [0, 22050), applied to every track
// Output options (demucs's; the stems are encoded on the GPU and leave it as WAV data: dmx_tracks_infer_pcm through
// demucscpp::demucs_inference_batch_pcm):
//   --two-stems NAME         write target_0_NAME.wav and target_1_no_NAME.wav (the sum of the other stems); NAME is a stem
//                            of the loaded model
//   --other-method METHOD    what --two-stems writes beside the stem (demucs's option; it needs --two-stems): add (the
//                            default: the sum of the other stems), minus (target_1_no_NAME.wav = the original mixture minus
//                            the stem: it keeps what the model attributed to no stem) or none (target_0_NAME.wav only)
//   --remix NAME=TERMS[,NAME=TERMS...]   outputs mixed on the GPU from the stems and the original mixture, written as
//                            target_{o}_{NAME}.wav (at most 8). TERMS is a sequence of [+|-][GAIN*]SOURCE; SOURCE is a stem
//                            of the loaded model or mix (the input track); GAIN is a decimal number or NdB (10^(N/20)); behind
//                            a term's sign a GAIN may carry a minus of its own:
//                              --remix karaoke=mix-vocals,backing=drums+bass+other+-12dB*vocals
//                            Not together with --two-stems. (minus, none and --remix go through dmx_tracks_infer_remix and
//                            demucscpp::demucs_inference_batch_remix.)
//   --clip-mode MODE         rescale (divide a stem whose peak exceeds 1 / 1.01 by 1.01 peak), clamp (to +-0.99) or none
//   --int16 --int24 --float32  sample format of the files (these take no value)
//   --flac                   write target_*.flac instead of target_*.wav (demucs's option; it takes no value): the same samples,
//                            losslessly coded on the GPU (dmx_tracks_infer_flac; csrc/flac.hip), 16 bit by default, 24 bit
//                            with --int24; --float32 --flac is an error. It combines with every option above and with bags.
//   --loudnorm LUFS          bring every track's MIXTURE to LUFS (integrated loudness, ITU-R BS.1770; -70 .. 0) with one gain for all
//                            of its outputs, so that the stems keep their balance (DMX_LOUD_MIXTURE); --loudnorm-each LUFS gives
//                            every output its own gain (DMX_LOUD_EACH); --loudness only measures. --max-peak DB (default -1) is the
//                            ceiling of the sample peak: the gain is reduced where it would be exceeded. A line per output is
//                            printed: "vocals: -14.23 LUFS, gain +3.10 dB". They combine with every option above.
//   --limit                  the look-ahead peak limiter holds --max-peak (DMX_LOUD_LIMIT): with --loudnorm or
//                            --loudnorm-each the ceiling no longer lowers the gain, so the target is reached; on its own (or as
//                            --clip-mode limit) it limits the stems as they are (DMX_LOUD_UNITY). --limit-attack MS (default 5) and
//                            --limit-release MS (default 100) are the times in which the reduction moves by 10 dB, 0.1 .. 10000. The
//                            report gains a part such as "limited 1234 frames, max -5.21 dB, peak -1.00 dBFS".
//   --true-peak              with --loudnorm or --loudnorm-each: --max-peak is a ceiling of the TRUE peak (4x oversampled below
//                            96 kHz; DMX_LOUD_TRUE_PEAK), -1 dBTP by default. --meters (with any of the three flags above) extends
//                            the line: "vocals: -14.23 LUFS, gain +3.10 dB, TP -1.00 dBTP, LRA 6.20 LU, max M -9.80, max S -11.42",
//                            TP the true peak of what leaves, LRA the loudness range, M and S the largest momentary and short-term
//                            loudness in LUFS of the output as measured. These two take no value.
//   --flac-level N           with --flac: 0 (default) FIXED predictors alone, 1 adds an LPC predictor of order 8, 2 orders 8
//                            and 12 (smaller files, the same samples); without --flac it changes nothing
// With any of them the defaults are demucs's: rescale, 16 bit. Without any of them the files are float32 as before.
// A track at another rate (DMX_RESAMPLE=1) takes them at its own rate: the library converts inside the track path
// (dmx_tracks_infer_rates, dmx_tracks_infer_from_flac_rates) and the outputs are the stems at the file's rate.
// <model> may also be a bag of models (dmx_tracks_infer_bag through the demucscpp::demucs_bag overloads; every option
// above still applies, and every model gets the same offsets, from --shift-offsets or DMX_SHIFT_OFFSET):
//   a directory              scanned as demucs_ft.cpp.main scans it (file names containing htdemucs_ft_{drums,bass,other,
//                            vocals}): the fine-tuned bag, stem i from model i; every file byte-identical to what
//                            demucs_ft.cpp.main writes for that input alone
//   file1,file2,...          up to 8 models of one architecture, averaged with equal weights, or with
//   --bag-weights w00,w01,.. the weight of (model q, stem s) at position q * stems + s: finite, >= 0, every stem with a
//                            model and every model with a weight (a single model file may be given with it, too)
// With N > 1, DMX_SHIFT_OFFSET is ambiguous without --shift-offsets and is refused. Without options the call and its output
// are those of the plain batch call.
#include <cerrno>
#include <cmath>
#include <filesystem>
#include <fstream>
#include <iomanip>

#include "wav.hpp"

using namespace demucscpp;

[[noreturn]] static void usage(const char *argv0)
{
    std::cerr << "Usage: " << argv0 << " [--shifts N] [--overlap F] [--shift-offsets a,b,...] [--two-stems NAME]"
              << " [--other-method add|minus|none] [--remix NAME=[+|-][GAIN*]SOURCE...,...]"
              << " [--clip-mode rescale|clamp|none] [--int16|--int24|--float32] [--flac] [--flac-level 0|1|2] [--bag-weights w00,w01,...]"
              << " [--loudnorm LUFS | --loudnorm-each LUFS | --loudness] [--max-peak DB] [--true-peak] [--meters]"
              << " [--limit] [--limit-attack MS] [--limit-release MS] (--clip-mode limit: --limit without loudnorm)"
              << " <model file | ft model dir | file1,file2,...> <out dir> <wav file>..." << std::endl;
    exit(1);
}

static bool parse_int(const std::string &s, long lo, long hi, int &v)
{
    if (s.empty())
        return false;
    char *end = nullptr;
    errno = 0;
    const long x = std::strtol(s.c_str(), &end, 10);
    if (errno || *end || x < lo || x > hi)
        return false;
    v = (int)x;
    return true;
}

// a comma-separated list, strictly: an empty value (leading, doubled or trailing comma) is an error
static bool split_list(const std::string &val, std::vector<std::string> &items)
{
    items.clear();
    for (size_t pos = 0;;)
    {
        const size_t comma = val.find(',', pos);
        items.push_back(val.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos));
        if (items.back().empty())
            return false;
        if (comma == std::string::npos)
            return true;
        pos = comma + 1;
    }
}

int main(int argc, const char **argv)
{
    std::vector<float> bag_weights;
    bool with_bag_weights = false;
    inference_options opts;
    output_options out_opts; // demucs's defaults: 16 bit, rescale
    bool with_opts = false, with_out_opts = false, flac = false, float32_given = false;
    std::string two_stems, remix_text;
    int other_method = -1; // DMX_OTHER_*, -1: not given
    int flac_level = 0;
    int loud_mode = -1; // DMX_LOUD_*, -1: not given
    float loud_target = -14.0f, max_peak_db = -1.0f;
    LoudnessReport loud_report; // filled by the remix calls when a loudness flag is given
    bool true_peak = false, with_meters = false;
    MetersReport meters_report; // filled as well with --meters
    bool limit = false, clip_limit = false, limit_times = false;
    float limit_attack = DMX_LIMIT_ATTACK_MS, limit_release = DMX_LIMIT_RELEASE_MS;
    LimitReport limit_report; // filled as well with --limit
    int a = 1;
    for (; a < argc && std::string(argv[a]).rfind("--", 0) == 0; a += 2)
    {
        const std::string opt = argv[a];
        if (opt == "--int16" || opt == "--int24" || opt == "--float32") // no value: step back so that a += 2 moves by one
        {
            out_opts.encoding = opt == "--int16" ? DMX_PCM_S16 : opt == "--int24" ? DMX_PCM_S24 : DMX_PCM_F32;
            float32_given = opt == "--float32";
            with_out_opts = true;
            --a;
            continue;
        }
        if (opt == "--flac") // no value either
        {
            flac = with_out_opts = true;
            --a;
            continue;
        }
        if (opt == "--true-peak" || opt == "--meters") // no value; what they need is checked behind the loop
        {
            (opt == "--meters" ? with_meters : true_peak) = true;
            --a;
            continue;
        }
        if (opt == "--limit") // no value; what it goes with is checked behind the loop
        {
            limit = true;
            --a;
            continue;
        }
        if (opt == "--loudness") // no value: measure and report, the bytes stay
        {
            loud_mode = DMX_LOUD_MEASURE, with_out_opts = true;
            --a;
            continue;
        }
        if (a + 1 >= argc)
            usage(argv[0]);
        const std::string val = argv[a + 1];
        if (opt == "--loudnorm" || opt == "--loudnorm-each" || opt == "--max-peak")
        {
            char *end = nullptr;
            errno = 0;
            const float v = std::strtof(val.c_str(), &end);
            if (val.empty() || errno || *end || !std::isfinite(v))
                usage(argv[0]);
            if (opt == "--max-peak")
                max_peak_db = v;
            else if (v < -70.0f || v > 0.0f) // the library's range for a target in LUFS
                usage(argv[0]);
            else
                loud_target = v, loud_mode = opt == "--loudnorm" ? DMX_LOUD_MIXTURE : DMX_LOUD_EACH, with_out_opts = true;
            continue;
        }
        if (opt == "--limit-attack" || opt == "--limit-release")
        {
            char *end = nullptr;
            errno = 0;
            const float v = std::strtof(val.c_str(), &end);
            if (val.empty() || errno || *end || !std::isfinite(v) || v < 0.1f || v > 10000.0f) // the library's range
                usage(argv[0]);
            (opt == "--limit-attack" ? limit_attack : limit_release) = v, limit_times = true;
            continue;
        }
        if (opt == "--two-stems")
        {
            if (stem_index(val) < 0)
                usage(argv[0]);
            two_stems = val, out_opts.two_stems = stem_index(val), with_out_opts = true;
            continue;
        }
        if (opt == "--flac-level") // the level alone asks for nothing: without --flac it is not used
        {
            if (!parse_int(val, 0, 2, flac_level))
                usage(argv[0]);
            continue;
        }
        if (opt == "--other-method")
        {
            other_method = val == "add" ? DMX_OTHER_ADD : val == "minus" ? DMX_OTHER_MINUS : val == "none" ? DMX_OTHER_NONE : -1;
            if (other_method < 0)
                usage(argv[0]);
            with_out_opts = true;
            continue;
        }
        if (opt == "--remix")
        {
            try // the grammar now, against every stem name; against the loaded model's stems once it is known
            {
                parse_remix(val, 6);
            }
            catch (const std::exception &e)
            {
                std::cerr << "--remix: " << e.what() << std::endl;
                usage(argv[0]);
            }
            remix_text = val, with_out_opts = true;
            continue;
        }
        if (opt == "--clip-mode")
        {
            if (val == "rescale")
                out_opts.clip = DMX_CLIP_RESCALE;
            else if (val == "clamp")
                out_opts.clip = DMX_CLIP_CLAMP;
            else if (val == "none")
                out_opts.clip = DMX_CLIP_NONE;
            else if (val == "limit") // --limit without loudnorm: nothing is left to clip under the ceiling
                out_opts.clip = DMX_CLIP_NONE, limit = clip_limit = true;
            else
                usage(argv[0]);
            with_out_opts = true;
            continue;
        }
        if (opt == "--bag-weights")
        {
            std::vector<std::string> items;
            if (!split_list(val, items))
                usage(argv[0]);
            bag_weights.clear();
            for (const std::string &it : items)
            {
                char *end = nullptr;
                errno = 0;
                const float w = std::strtof(it.c_str(), &end);
                if (errno || *end || !std::isfinite(w) || w < 0.0f)
                    usage(argv[0]);
                bag_weights.push_back(w);
            }
            with_bag_weights = true;
            continue;
        }
        with_opts = true;
        if (opt == "--shifts")
        {
            if (!parse_int(val, 1, DMX_MAX_SHIFTS, opts.shifts))
                usage(argv[0]);
        }
        else if (opt == "--overlap")
        {
            char *end = nullptr;
            errno = 0;
            opts.overlap = std::strtof(val.c_str(), &end);
            if (val.empty() || errno || *end || !std::isfinite(opts.overlap) || opts.overlap < 0.0f || opts.overlap > DMX_MAX_OVERLAP)
                usage(argv[0]);
        }
        else if (opt == "--shift-offsets")
        {
            // every comma separates two values: an empty value (leading, doubled or trailing comma) is an error
            opts.shift_offsets.clear();
            for (size_t pos = 0;;)
            {
                const size_t comma = val.find(',', pos);
                int v = 0;
                if (!parse_int(val.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos), 0, DMX_MAX_SHIFT - 1, v))
                    usage(argv[0]);
                opts.shift_offsets.push_back(v);
                if (comma == std::string::npos)
                    break;
                pos = comma + 1;
            }
        }
        else
            usage(argv[0]);
    }
    if (argc - a < 3)
        usage(argv[0]);
    if (other_method >= 0 && two_stems.empty())
    {
        std::cerr << "--other-method needs --two-stems" << std::endl;
        usage(argv[0]);
    }
    if (!remix_text.empty() && !two_stems.empty())
    {
        std::cerr << "--remix and --two-stems exclude each other" << std::endl;
        usage(argv[0]);
    }
    if (limit_times && !limit)
    {
        std::cerr << "--limit-attack and --limit-release need --limit" << std::endl;
        usage(argv[0]);
    }
    if (limit && (loud_mode == DMX_LOUD_MEASURE || (clip_limit && loud_mode >= 0)))
    {
        std::cerr << (clip_limit ? "--clip-mode limit is --limit without loudnorm: give --limit beside --loudnorm or --loudnorm-each"
                                 : "--limit changes the samples and --loudness only measures: they exclude each other")
                  << std::endl;
        usage(argv[0]);
    }
    if (limit && loud_mode < 0) // the limiter alone under --max-peak
        loud_mode = DMX_LOUD_UNITY, with_out_opts = true;
    if (true_peak && !limit && loud_mode != DMX_LOUD_MIXTURE && loud_mode != DMX_LOUD_EACH)
    {
        std::cerr << "--true-peak needs --loudnorm, --loudnorm-each or --limit: it is the ceiling of their gain" << std::endl;
        usage(argv[0]);
    }
    if (with_meters && loud_mode < 0)
    {
        std::cerr << "--meters needs --loudnorm, --loudnorm-each or --loudness: it extends their report" << std::endl;
        usage(argv[0]);
    }
    if (flac && (float32_given || out_opts.encoding == DMX_PCM_F32))
    {
        std::cerr << "--float32 and --flac exclude each other: FLAC holds integer samples (--int16, the default, or --int24)" << std::endl;
        usage(argv[0]);
    }
    // minus, none, --remix and --flac leave through the remix entry points; everything else as before
    const bool with_remix = !remix_text.empty() || other_method == DMX_OTHER_MINUS || other_method == DMX_OTHER_NONE || flac || loud_mode >= 0;
    remix_options remix;
    bool flac_in = false; // every input is a .flac file the GPU takes as it is (decided once the inputs have been looked at):
                          // at 44.1 kHz, or with DMX_RESAMPLE=1 at any rate
    bool any_rate = false; // DMX_RESAMPLE=1 and an input at another rate: the tracks go to the library with their rates
    auto make_remix = [&](int nb_sources) { // once the model's stems are known
        if (with_out_opts && out_opts.two_stems >= nb_sources)
        {
            std::cerr << "--two-stems " << two_stems << ": the loaded model has no such stem (" << nb_sources << " sources)" << std::endl;
            exit(1);
        }
        if (!with_remix && !flac_in && !any_rate)
            return;
        try
        {
            if (!remix_text.empty())
                remix = parse_remix(remix_text, nb_sources);
            else if (out_opts.two_stems >= 0)
                remix = remix_two_stems(nb_sources, out_opts.two_stems, other_method < 0 ? DMX_OTHER_ADD : other_method);
            else // --flac alone: every stem, through 0 / 1 gains (the bytes of the output spec)
            {
                static const char *stems[6] = {"drums", "bass", "other", "vocals", "guitar", "piano"};
                remix.gains.assign((size_t)nb_sources * (size_t)(nb_sources + 1), 0.0f);
                for (int s = 0; s < nb_sources; ++s)
                    remix.names.push_back(stems[s]), remix.gains[(size_t)s * (size_t)(nb_sources + 1) + (size_t)s] = 1.0f;
            }
        }
        catch (const std::exception &e)
        {
            std::cerr << (remix_text.empty() ? "--other-method: " : "--remix: ") << e.what() << std::endl;
            exit(1);
        }
        remix.encoding = out_opts.encoding, remix.clip = out_opts.clip, remix.flac = flac, remix.flac_level = flac_level;
        if (loud_mode >= 0)
        {
            remix.loudness.on = true, remix.loudness.mode = loud_mode, remix.loudness.target_lufs = loud_target;
            remix.loudness.max_peak = (float)std::pow(10.0, (double)max_peak_db / 20.0);
            remix.loudness.true_peak = true_peak;
            remix.loudness.meters = with_meters ? &meters_report : nullptr;
            remix.loudness.limit = limit, remix.loudness.attack_ms = limit_attack, remix.loudness.release_ms = limit_release;
            remix.loudness.limit_report = limit ? &limit_report : nullptr;
        }
        if (!with_out_opts) // FLAC inputs or other rates without an output option: the float32 stems, through unit gains
            remix.encoding = DMX_PCM_F32, remix.clip = DMX_CLIP_NONE;
    };
    if (!opts.shift_offsets.empty() && (int)opts.shift_offsets.size() != opts.shifts)
    {
        std::cerr << "--shift-offsets: " << opts.shift_offsets.size() << " values for --shifts " << opts.shifts << std::endl;
        usage(argv[0]);
    }
    if (opts.shifts > 1 && opts.shift_offsets.empty() && std::getenv("DMX_SHIFT_OFFSET"))
    {
        std::cerr << "DMX_SHIFT_OFFSET with --shifts " << opts.shifts << " is ambiguous: give the copies' offsets with --shift-offsets"
                  << std::endl;
        exit(1);
    }
    argv += a - 1, argc -= a - 1; // the positional arguments as without options
    std::cout << "demucs_batch.cpp Main driver program (MI355X HIP path)" << std::endl;
    const std::string model_file = argv[1], out_dir = argv[2];
    const int n_files = argc - 3;
    // a bag: a directory of fine-tuned models, a comma-separated list of files, or --bag-weights
    std::vector<std::string> bag_files;
    bool ft_dir = false;
    {
        std::error_code ec;
        if (std::filesystem::is_directory(model_file, ec))
        {
            if (with_bag_weights)
            {
                std::cerr << "--bag-weights: a directory is the fine-tuned bag (stem i from model i) and takes no weights" << std::endl;
                usage(argv[0]);
            }
            static const char *keys[4] = {"htdemucs_ft_drums", "htdemucs_ft_bass", "htdemucs_ft_other", "htdemucs_ft_vocals"};
            static const char *ft_names[4] = {"drums", "bass", "other", "vocals"};
            bag_files.assign(4, std::string());
            bool have[4] = {false, false, false, false};
            for (const auto &entry : std::filesystem::directory_iterator(model_file))
                for (int i = 0; i < 4; ++i)
                    if (!have[i] && entry.path().string().find(keys[i]) != std::string::npos)
                    {
                        bag_files[(size_t)i] = entry.path().string();
                        std::cout << "Loading ft model " << entry.path().string() << " for " << ft_names[i] << std::endl;
                        have[i] = true;
                        break;
                    }
            for (int i = 0; i < 4; ++i)
                if (!have[i])
                {
                    std::cerr << "Error: no model file containing '" << keys[i] << "' in " << model_file << std::endl;
                    exit(1);
                }
            ft_dir = true;
        }
        else if (model_file.find(',') != std::string::npos || with_bag_weights)
        {
            if (!split_list(model_file, bag_files) || bag_files.size() > (size_t)DMX_MAX_BAG)
            {
                std::cerr << "<model>: a list of 1 to " << DMX_MAX_BAG << " model files separated by single commas" << std::endl;
                usage(argv[0]);
            }
        }
    }
    const bool bag_mode = !bag_files.empty();
    int arch = 0;
    if (!bag_mode)
    {
        const char *d = std::getenv("DMX_DEVICE");
        dmx_model *m = nullptr;
        if (dmx_model_load(model_file.c_str(), d ? std::atoi(d) : 0, &m) != DMX_OK)
        {
            std::cerr << "Error loading model: " << dmx_last_error() << std::endl;
            exit(1);
        }
        arch = dmx_model_arch(m);
        dmx_model_free(m);
    }
    std::vector<StereoMatrix> tracks((size_t)n_files);
    std::vector<int> native_rate((size_t)n_files, SUPPORTED_SAMPLE_RATE); // != 44100 only with DMX_RESAMPLE=1 (wav.hpp)
    // FLAC inputs (the content decides, not the name). When EVERY input is a .flac file - at 44.1 kHz, or with DMX_RESAMPLE=1
    // at any rate - the bytes go to the GPU as they are (dmx_tracks_infer_from_flac, dmx_tracks_infer_from_flac_rates);
    // otherwise a .flac file is decoded on the GPU (dmx_flac_decode) and then takes the way of a WAV file of its rate.
    // With DMX_RESAMPLE=1 a track at another rate goes to the library as it is, with its rate (dmx_tracks_infer_rates): both
    // conversions run inside the track path, and every output option applies to the stems at the file's rate.
    std::vector<FlacFile> flac_files((size_t)n_files);
    std::vector<int64_t> flac_frames;
    int n_flac = 0, n_flac_441 = 0;
    for (int i = 0; i < n_files; ++i)
    {
        std::vector<uint8_t> head(16);
        FILE *fh = fopen(argv[3 + i], "rb");
        const size_t got = fh ? fread(head.data(), 1, head.size(), fh) : 0;
        if (fh)
            fclose(fh);
        head.resize(got);
        if (!(got >= 4 && (memcmp(head.data(), "fLaC", 4) == 0 || memcmp(head.data(), "ID3", 3) == 0)))
            continue;
        if (!wavio::read_file_bytes(argv[3 + i], flac_files[(size_t)i]))
            exit(1);
        if (!wavio::is_flac_image(flac_files[(size_t)i]))
        {
            flac_files[(size_t)i].clear();
            continue;
        }
        ++n_flac;
        dmx_flac_info info;
        if (dmx_flac_probe(flac_files[(size_t)i].data(), (int64_t)flac_files[(size_t)i].size(), &info) != DMX_OK)
        {
            std::cerr << "[ERROR] " << argv[3 + i] << ": " << dmx_last_error() << std::endl;
            exit(1);
        }
        n_flac_441 += info.sample_rate == SUPPORTED_SAMPLE_RATE;
    }
    const char *rs_env = std::getenv("DMX_RESAMPLE");
    const bool resample = rs_env && std::atoi(rs_env) == 1;
    flac_in = n_flac == n_files && (n_flac_441 == n_files || resample);
    any_rate = flac_in && n_flac_441 != n_files;
    // without DMX_RESAMPLE=1 another rate is refused here with the reference's message; with it the track stays at its rate
    for (int i = 0; i < n_files && !flac_in; ++i)
    {
        if (!(flac_files[(size_t)i].empty()
                  ? wavio::load_audio_file(argv[3 + i], tracks[(size_t)i], &native_rate[(size_t)i], nullptr, true)
                  : wavio::load_flac_image(argv[3 + i], flac_files[(size_t)i], tracks[(size_t)i], &native_rate[(size_t)i], nullptr, true)))
            exit(1);
        any_rate = any_rate || native_rate[(size_t)i] != SUPPORTED_SAMPLE_RATE;
    }
    std::cout << std::fixed << std::setprecision(3);
    ProgressCallback cb = [](float progress, const std::string &msg) {
        std::cout << "(" << std::setw(3) << std::setfill(' ') << progress * 100.0f << "%) " << msg << std::endl;
    };
    std::vector<StemTensor> outs;
    PcmOutputs pcm_outs;
    auto remix_or = [&](int encoding) { return flac_in || any_rate ? remix.encoding : encoding; };
    int nb_sources = 4;
    if (bag_mode)
    {
        demucs_bag bag;
        if (!load_demucs_bag(bag_files, &bag))
        {
            std::cerr << "Error loading model" << std::endl;
            exit(1);
        }
        nb_sources = bag.nb_sources;
        std::vector<float> weights; // empty: the diagonal
        if (with_bag_weights)
        {
            if (bag_weights.size() != bag_files.size() * (size_t)nb_sources)
            {
                std::cerr << "--bag-weights: " << bag_weights.size() << " values for " << bag_files.size() << " models x " << nb_sources
                          << " stems" << std::endl;
                usage(argv[0]);
            }
            weights = bag_weights;
        }
        else if (!ft_dir)
            weights.assign(bag_files.size() * (size_t)nb_sources, 1.0f);
        if (dmx_bag_weights((int)bag_files.size(), nb_sources, weights.empty() ? nullptr : weights.data(), nullptr, nullptr) != DMX_OK)
        {
            std::cerr << dmx_last_error() << std::endl;
            usage(argv[0]);
        }
        std::cout << "Starting Demucs bag (" << bag_files.size() << " models, " << nb_sources << "-source) inference of " << n_files
                  << " tracks" << std::endl;
        make_remix(nb_sources);
        if (flac_in && any_rate)
            pcm_outs = demucs_inference_batch_remix(bag, flac_files, native_rate, cb, weights, opts, remix, nullptr, &flac_frames, &loud_report);
        else if (flac_in)
            pcm_outs = demucs_inference_batch_remix(bag, flac_files, cb, weights, opts, remix, nullptr, &flac_frames, &loud_report);
        else if (any_rate)
            pcm_outs = demucs_inference_batch_remix(bag, tracks, native_rate, cb, weights, opts, remix, nullptr, &loud_report);
        else if (with_remix)
            pcm_outs = demucs_inference_batch_remix(bag, tracks, cb, weights, opts, remix, nullptr, &loud_report);
        else if (with_out_opts)
            pcm_outs = demucs_inference_batch_pcm(bag, tracks, cb, weights, opts, out_opts);
        else
            outs = demucs_inference_batch(bag, tracks, cb, weights, opts);
    }
    else if (arch == 3)
    {
        demucscpp_v3::demucs_v3_model model;
        if (!demucscpp_v3::load_demucs_v3_model(model_file, &model))
        {
            std::cerr << "Error loading model" << std::endl;
            exit(1);
        }
        std::cout << "Starting Demucs v3 MMI inference of " << n_files << " tracks" << std::endl;
        make_remix(nb_sources);
        if (flac_in && any_rate)
            pcm_outs = demucscpp_v3::demucs_v3_inference_batch_remix(model, flac_files, native_rate, cb, opts, remix, nullptr, &flac_frames, &loud_report);
        else if (flac_in)
            pcm_outs = demucscpp_v3::demucs_v3_inference_batch_remix(model, flac_files, cb, opts, remix, nullptr, &flac_frames, &loud_report);
        else if (any_rate)
            pcm_outs = demucscpp_v3::demucs_v3_inference_batch_remix(model, tracks, native_rate, cb, opts, remix, nullptr, &loud_report);
        else if (with_remix)
            pcm_outs = demucscpp_v3::demucs_v3_inference_batch_remix(model, tracks, cb, opts, remix, nullptr, &loud_report);
        else if (with_out_opts)
            pcm_outs = demucscpp_v3::demucs_v3_inference_batch_pcm(model, tracks, cb, opts, out_opts);
        else
            outs = with_opts ? demucscpp_v3::demucs_v3_inference_batch(model, tracks, cb, opts)
                             : demucscpp_v3::demucs_v3_inference_batch(model, tracks, cb);
    }
    else
    {
        demucs_model model;
        if (!load_demucs_model(model_file, &model))
        {
            std::cerr << "Error loading model" << std::endl;
            exit(1);
        }
        nb_sources = model.is_4sources ? 4 : 6;
        std::cout << "Starting Demucs (" << nb_sources << "-source) inference of " << n_files << " tracks" << std::endl;
        make_remix(nb_sources);
        if (flac_in && any_rate)
            pcm_outs = demucs_inference_batch_remix(model, flac_files, native_rate, cb, opts, remix, nullptr, &flac_frames, &loud_report);
        else if (flac_in)
            pcm_outs = demucs_inference_batch_remix(model, flac_files, cb, opts, remix, nullptr, &flac_frames, &loud_report);
        else if (any_rate)
            pcm_outs = demucs_inference_batch_remix(model, tracks, native_rate, cb, opts, remix, nullptr, &loud_report);
        else if (with_remix)
            pcm_outs = demucs_inference_batch_remix(model, tracks, cb, opts, remix, nullptr, &loud_report);
        else if (with_out_opts)
            pcm_outs = demucs_inference_batch_pcm(model, tracks, cb, opts, out_opts);
        else
            outs = with_opts ? demucs_inference_batch(model, tracks, cb, opts) : demucs_inference_batch(model, tracks, cb);
    }
    static const char *names[6] = {"drums", "bass", "other", "vocals", "guitar", "piano"};
    for (int f = 0; f < n_files; ++f)
    {
        const StereoMatrix &audio = tracks[(size_t)f];
        std::filesystem::path p = std::filesystem::path(out_dir) / std::filesystem::path(argv[3 + f]).stem();
        std::filesystem::create_directories(p);
        if (with_out_opts || flac_in || any_rate) // the bytes are WAV data already
        {
            const int64_t frames = flac_in ? flac_frames[(size_t)f] : audio.cols();
            const auto &po = pcm_outs[(size_t)f];
            for (size_t o = 0; loud_mode >= 0 && o <= po.size(); ++o) // the report: the outputs, then the mixture
            {
                const dmx_loudness_result &lr = loud_report[(size_t)f][o];
                char line[160];
                const std::string who = o < po.size() ? remix.names[o] : std::string("mixture");
                if (lr.lufs_c == DMX_LUFS_UNMEASURABLE)
                    snprintf(line, sizeof line, "%s: unmeasurable", who.c_str());
                else
                    snprintf(line, sizeof line, "%s: %.2f LUFS", who.c_str(), lr.lufs_c / 100.0);
                std::cout << line;
                if (o < po.size())
                {
                    snprintf(line, sizeof line, ", gain %+.2f dB", 20.0 * std::log10((double)lr.gain));
                    std::cout << line;
                }
                if (limit && o < po.size()) // what the limiter did to the output (1 unit = 1 / 65536 octave)
                {
                    const dmx_limit_result &li = limit_report[(size_t)f][o];
                    char peak[48];
                    if (li.peak_out > 0.0f)
                        snprintf(peak, sizeof peak, "%.2f dBFS", 20.0 * std::log10((double)li.peak_out));
                    else
                        snprintf(peak, sizeof peak, "-inf dBFS");
                    snprintf(line, sizeof line, ", limited %lld frames, max %.2f dB, peak %s", (long long)li.limited_frames,
                             -(double)li.max_reduction / 65536.0 * 20.0 * std::log10(2.0), peak);
                    std::cout << line;
                }
                if (with_meters) // the true peak of what leaves (the mixture: as measured), then the meters of the signal as measured
                {
                    const dmx_meters_result &mr = meters_report[(size_t)f][o];
                    // (behind the limiter with --true-peak: the true peak of the limited output)
                    const float tp = o < po.size() ? (limit && true_peak ? limit_report[(size_t)f][o].true_peak_out : lr.gain * mr.true_peak)
                                                   : mr.true_peak;
                    auto lu = [](int32_t c, const char *unit) {
                        char b[48];
                        if (c == DMX_LUFS_UNMEASURABLE)
                            snprintf(b, sizeof b, "n/a");
                        else
                            snprintf(b, sizeof b, "%.2f%s", c / 100.0, unit);
                        return std::string(b);
                    };
                    if (tp > 0.0f)
                        snprintf(line, sizeof line, ", TP %.2f dBTP", 20.0 * std::log10((double)tp));
                    else
                        snprintf(line, sizeof line, ", TP -inf dBTP");
                    std::cout << line << ", LRA " << lu(mr.lra_c, " LU") << ", max M " << lu(mr.max_momentary_c, "") << ", max S "
                              << lu(mr.max_short_c, "");
                }
                std::cout << std::endl;
            }
            for (size_t target = 0; target < po.size(); ++target)
            {
                const std::string name = with_remix || flac_in || any_rate ? remix.names[target]
                                         : out_opts.two_stems < 0 ? names[target]
                                                                  : (target == 0 ? two_stems : "no_" + two_stems);
                auto p_target = p / ("target_" + std::to_string(target) + "_" + name + (flac ? ".flac" : ".wav"));
                std::cout << "Writing " << (flac ? "flac" : "wav") << " file " << p_target << std::endl;
                bool ok;
                if (flac) // a complete file already
                {
                    std::ofstream f(p_target.string(), std::ios::binary);
                    f.write(reinterpret_cast<const char *>(po[target].data()), (std::streamsize)po[target].size());
                    ok = (bool)f;
                }
                else
                    ok = wavio::write_pcm_file(po[target].data(), frames, remix_or(out_opts.encoding), p_target.string(), native_rate[(size_t)f]);
                if (!ok)
                {
                    std::cerr << "Error writing " << p_target << std::endl;
                    exit(1);
                }
            }
            continue;
        }
        const StemTensor &out = outs[(size_t)f];
        std::vector<float> wave((size_t)(2 * audio.cols()));
        for (int target = 0; target < nb_sources; ++target)
        {
            auto p_target = p / ("target_" + std::to_string(target) + "_" + names[target] + ".wav");
            std::cout << "Writing wav file " << p_target << std::endl;
            for (int64_t i = 0; i < audio.cols(); ++i)
            {
                wave[(size_t)(2 * i)] = out(target, 0, i);
                wave[(size_t)(2 * i + 1)] = out(target, 1, i);
            }
            if (!wavio::write_audio_file(wave.data(), audio.cols(), p_target.string())) // (every track is at 44.1 kHz here)
            {
                std::cerr << "Error writing " << p_target << std::endl;
                exit(1);
            }
        }
    }
    return 0;
}
