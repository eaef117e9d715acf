// demucs_batch.cpp.main — many tracks in one call (no reference counterpart: the reference's CLIs take one file):
//   demucs_batch.cpp.main <model file> <out dir> <wav file>...
// -> <out dir>/<wav file stem>/target_{i}_{drums|bass|other|vocals|guitar|piano}.wav (stereo float32), every file
// byte-identical to what demucs.cpp.main / demucs_v3.cpp.main writes for that input alone. The model's architecture
// (HTDemucs v4 4s / 6s, or Demucs v3) is read from the file; the segments of all tracks share batches
// (dmx_tracks_infer through demucscpp::demucs_inference_batch / demucscpp_v3::demucs_v3_inference_batch).
// Environment: DMX_DEVICE (GPU index), DMX_SHIFT_OFFSET (fixed shift instead of rand(), drawn per track in order),
// DMX_BATCH (segments in flight), DMX_RESAMPLE (wav.hpp).
#include <filesystem>
#include <iomanip>

#include "wav.hpp"

using namespace demucscpp;

int main(int argc, const char **argv)
{
    if (argc < 4)
    {
        std::cerr << "Usage: " << argv[0] << " <model file> <out dir> <wav file>..." << std::endl;
        exit(1);
    }
    std::cout << "demucs_batch.cpp Main driver program (MI355X HIP path)" << std::endl;
    const std::string model_file = argv[1], out_dir = argv[2];
    const int n_files = argc - 3;
    int arch = 0;
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
    std::vector<int64_t> native_frames((size_t)n_files, -1);
    for (int i = 0; i < n_files; ++i)
        if (!wavio::load_audio_file(argv[3 + i], tracks[(size_t)i], &native_rate[(size_t)i], &native_frames[(size_t)i]))
            exit(1);
    std::cout << std::fixed << std::setprecision(3);
    ProgressCallback cb = [](float progress, const std::string &msg) {
        std::cout << "(" << std::setw(3) << std::setfill(' ') << progress * 100.0f << "%) " << msg << std::endl;
    };
    std::vector<StemTensor> outs;
    int nb_sources = 4;
    if (arch == 3)
    {
        demucscpp_v3::demucs_v3_model model;
        if (!demucscpp_v3::load_demucs_v3_model(model_file, &model))
        {
            std::cerr << "Error loading model" << std::endl;
            exit(1);
        }
        std::cout << "Starting Demucs v3 MMI inference of " << n_files << " tracks" << std::endl;
        outs = demucscpp_v3::demucs_v3_inference_batch(model, tracks, cb);
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
        outs = demucs_inference_batch(model, tracks, cb);
    }
    static const char *names[6] = {"drums", "bass", "other", "vocals", "guitar", "piano"};
    for (int f = 0; f < n_files; ++f)
    {
        const StereoMatrix &audio = tracks[(size_t)f];
        const StemTensor &out = outs[(size_t)f];
        std::filesystem::path p = std::filesystem::path(out_dir) / std::filesystem::path(argv[3 + f]).stem();
        std::filesystem::create_directories(p);
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
            if (!wavio::write_audio_file(wave.data(), audio.cols(), p_target.string(), native_rate[(size_t)f], native_frames[(size_t)f]))
            {
                std::cerr << "Error writing " << p_target << std::endl;
                exit(1);
            }
        }
    }
    return 0;
}
