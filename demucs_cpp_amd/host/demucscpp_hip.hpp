// demucscpp_hip.hpp — header-only C++17 mirror of the reference's public API for the hot
// path, on top of the C ABI (include/demucs_hip.h). Same names, argument meaning and
// error behaviour as /root/reference/src/model.hpp:
//
//   bool  demucscpp::load_demucs_model(const std::string&, demucs_model*)      :649-650
//   <S,2,N> demucscpp::demucs_inference(const demucs_model&, <2,N>, ProgressCallback) :658-660
//   void  demucscpp::model_inference(const demucs_model&, demucs_segment_buffers&,
//                                    stft_buffers&, ProgressCallback, float, float) :662-666
// and, for Demucs v3 (hdemucs_mmi), namespace demucscpp_v3 (src/model.hpp:668-1415):
//   bool  load_demucs_v3_model(const std::string&, demucs_v3_model*)                     :1396-1397
//   <4,2,N> demucs_v3_inference(const demucs_v3_model&, <2,N>, ProgressCallback)          :1405-1408
//   void  model_v3_inference(const demucs_v3_model&, demucs_v3_segment_buffers&, stft_buffers&, ...) :1410-1414
// plus, with no reference counterpart (the reference's CLIs take one file), demucs_inference_batch /
// demucs_v3_inference_batch: many tracks in one call, their segments sharing batches (dmx_tracks_infer), and their overloads
// taking demucscpp::inference_options: demucs's shifts ensemble and segment overlap (dmx_tracks_infer_opts); and
// demucs_inference_batch_pcm / demucs_v3_inference_batch_pcm with demucscpp::output_options: the stems as 16-bit / 24-bit /
// float32 WAV data, two-stems and clip mode applied on the GPU (dmx_tracks_infer_pcm); and their overloads taking a
// demucscpp::demucs_bag: several models with a weight per (model, stem) - the fine-tuned bag, ensembles (dmx_tracks_infer_bag);
// and demucs_inference_batch_remix / demucs_v3_inference_batch_remix with demucscpp::remix_options: outputs mixed on the GPU
// from the stems and the original mixture - demucs's --other-method minus / none, stem gains, mix-minus (dmx_tracks_infer_remix).
//
// Eigen is not required: the two tensor types below have exactly the memory image of
// the reference's column-major Eigen::MatrixXf(2,N) and Eigen::Tensor3dXf(S,2,N), so a
// project that has Eigen can wrap them zero-copy with Eigen::Map / Eigen::TensorMap
// (see INTEGRATION.md). Define DEMUCSCPP_HIP_WITH_EIGEN before including this header to
// get overloads that take and return the Eigen types themselves.
#pragma once
#include "demucs_hip.h"

#include <cmath>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <algorithm>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef DEMUCSCPP_HIP_WITH_EIGEN
#include <Eigen/Dense>
#include <unsupported/Eigen/CXX11/Tensor>
#endif

namespace demucscpp
{

using ProgressCallback = std::function<void(float, const std::string &)>; // src/model.hpp:17

const int SUPPORTED_SAMPLE_RATE = 44100; // src/dsp.hpp:14
const float SEGMENT_LEN_SECS = 7.8f;     // src/model.hpp:652
const float MAX_SHIFT_SECS = 0.5f;       // src/model.hpp:654
const float OVERLAP = 0.25f;             // src/model.hpp:655

// (2, N) column-major == interleaved stereo; element (c, i) at c + 2*i
struct StereoMatrix
{
    int64_t n = 0;
    std::vector<float> data;
    StereoMatrix() {}
    explicit StereoMatrix(int64_t cols) : n(cols), data((size_t)(2 * cols), 0.0f) {}
    int64_t rows() const { return 2; }
    int64_t cols() const { return n; }
    float &operator()(int c, int64_t i) { return data[(size_t)(c + 2 * i)]; }
    float operator()(int c, int64_t i) const { return data[(size_t)(c + 2 * i)]; }
};

// (S, 2, N) column-major; element (s, c, i) at s + S*(c + 2*i)
struct StemTensor
{
    int S = 0;
    int64_t n = 0;
    std::vector<float> data;
    StemTensor() {}
    StemTensor(int s, int64_t cols) : S(s), n(cols), data((size_t)(s * 2 * cols), 0.0f) {}
    int64_t dimension(int d) const { return d == 0 ? S : (d == 1 ? 2 : n); }
    float &operator()(int s, int c, int64_t i) { return data[(size_t)(s + (int64_t)S * (c + 2 * i))]; }
    float operator()(int s, int c, int64_t i) const { return data[(size_t)(s + (int64_t)S * (c + 2 * i))]; }
};

// weight container: resident in HBM (on every device of the engine) behind an opaque handle
// (src/model.hpp:285-554). One engine = weights + activation arena(s) + streams; see include/demucs_hip.h.
//
// Re-entrancy: the reference's contract is concurrent demucs_inference calls on ONE shared const model
// (cli-apps/threaded_inference.hpp:105-123 runs N std::threads on it). Calls on one demucs_model are
// serialised here by `lock` (one GPU context already keeps every CU busy, so nothing is lost); results are
// bit-identical to sequential calls. tests/threaded_harness.cpp runs exactly that pattern.
struct engine_model // what a loaded model is on this side of the boundary, whatever its architecture
{
    std::vector<int> devices;  // HIP devices (env DMX_DEVICES="0,1,..."; "all"; default: device DMX_DEVICE or 0)
    int shift_offset = -1;     // -1: rand() % 22050 like src/model_apply.cpp:114; else fixed
    int max_batch = 12;        // segments in flight per device (7.8 GB of arena; 3.33 ms per segment, 3.9 at 4, 3.22 at 24: DMX_BATCH)
    dmx_engine *engine = nullptr;
    mutable std::mutex lock;
    engine_model() {}
    engine_model(const engine_model &) = delete;
    engine_model &operator=(const engine_model &) = delete;
    ~engine_model()
    {
        if (engine)
            dmx_engine_free(engine);
    }
};
struct demucs_model : engine_model
{
    bool is_4sources = true;
};

namespace detail
{
// DMX_DEVICES: comma-separated HIP device ids, or "all"; DMX_DEVICE: one id (kept from round 1)
inline std::vector<int> devices_from_env()
{
    std::vector<int> d;
    if (const char *e = std::getenv("DMX_DEVICES"))
    {
        std::string s(e);
        if (s == "all")
        {
            for (int i = 0; i < dmx_device_count(); ++i)
                d.push_back(i);
            return d;
        }
        std::stringstream ss(s);
        std::string tok;
        while (std::getline(ss, tok, ','))
            if (!tok.empty())
                d.push_back(std::atoi(tok.c_str()));
    }
    if (d.empty())
    {
        const char *one = std::getenv("DMX_DEVICE");
        d.push_back(one ? std::atoi(one) : 0);
    }
    return d;
}
inline void read_env(int &shift_offset, int &max_batch)
{
    if (const char *so = std::getenv("DMX_SHIFT_OFFSET"))
        shift_offset = std::atoi(so);
    if (const char *mb = std::getenv("DMX_BATCH"))
        max_batch = std::max(1, std::atoi(mb));
}
struct CbThunk
{
    const ProgressCallback *cb;
};
// remix_options::flac_level around one track call: the context's level is put back when the call has returned
struct FlacLevelGuard
{
    dmx_ctx *c;
    int before;
    bool ok;
    FlacLevelGuard(dmx_ctx *ctx, int level) : c(ctx), before(ctx ? dmx_ctx_flac_level(ctx) : 0), ok(ctx && dmx_ctx_set_flac_level(ctx, level) == DMX_OK) {}
    ~FlacLevelGuard()
    {
        if (c)
            (void)dmx_ctx_set_flac_level(c, before);
    }
    FlacLevelGuard(const FlacLevelGuard &) = delete;
    FlacLevelGuard &operator=(const FlacLevelGuard &) = delete;
};
inline void progress_thunk(float p, const char *msg, void *user)
{
    const ProgressCallback *cb = static_cast<CbThunk *>(user)->cb;
    if (cb && *cb)
        (*cb)(p, std::string(msg));
}
[[noreturn]] inline void die(const char *where)
{
    // the reference has no error channel in inference (std::exit(1), src/layers.cpp:98-103)
    std::cerr << where << ": " << dmx_last_error() << std::endl;
    std::exit(1);
}
} // namespace detail

// src/model.hpp:649-650. Returns false and reports on stderr exactly when the reference
// loader does (src/model_load.cpp:64-69,97-102,1065-1070,1096-1105), and additionally
// when no HIP device is usable (there is no CPU fallback).
namespace detail
{
// arch: 4 = dmc4 / dmc6 file (HTDemucs v4), 3 = dmc3 (Demucs v3). A file of the other family is "bad magic" to the
// reference's loaders (src/model_load.cpp:79-102 / :1335-1340).
inline bool load_engine(const char *who, const std::string &model_file, engine_model *model, int arch)
{
    if (model->devices.empty())
        model->devices = devices_from_env();
    read_env(model->shift_offset, model->max_batch);
    const char *files[1] = {model_file.c_str()};
    if (dmx_engine_create(files, 1, model->devices.data(), (int)model->devices.size(), model->max_batch, DMX_TRANSPORT_AUTO,
                          &model->engine) != DMX_OK)
    {
        std::cerr << who << ": " << dmx_last_error() << std::endl;
        return false;
    }
    if (dmx_engine_arch(model->engine) != arch)
    {
        std::cerr << who << ": invalid model data (bad magic)" << std::endl;
        dmx_engine_free(model->engine);
        model->engine = nullptr;
        return false;
    }
    return true;
}
} // namespace detail
inline bool load_demucs_model(const std::string &model_file, demucs_model *model)
{
    if (!detail::load_engine("load_demucs_model", model_file, model, 4))
        return false;
    model->is_4sources = dmx_engine_n_sources(model->engine) == 4;
    return true;
}

// src/model.hpp:658-660, src/model_apply.cpp:60-91. With several devices the overlapping-segment loop is
// sharded over them (csrc/engine.cpp); the result is bit-identical to one device.
inline StemTensor demucs_inference(const demucs_model &model, const StereoMatrix &full_audio, ProgressCallback cb)
{
    const int S = model.is_4sources ? 4 : 6;
    StemTensor out(S, full_audio.cols());
    detail::CbThunk th{&cb};
    std::lock_guard<std::mutex> guard(model.lock);
    if (dmx_engine_track_infer(model.engine, full_audio.data.data(), full_audio.cols(), &model.shift_offset, out.data.data(),
                               DMX_LAYOUT_EIGEN, detail::progress_thunk, &th) != DMX_OK)
        detail::die("demucs_inference");
    return out;
}

// demucs's inference-time quality options (PyTorch demucs apply_model(shifts=, overlap=); the reference fixes 1 and 0.25) for
// the batch calls (dmx_tracks_infer_opts). shift_offsets: empty (model.shift_offset for every copy; -1: rand() % 22050 drawn
// per (track, copy)), `shifts` values applied to every track, or tracks x shifts values, row-major.
struct inference_options
{
    int shifts = 1;
    float overlap = 0.25f;
    std::vector<int> shift_offsets;
};
namespace detail
{
// what a batch call runs on: the root context of a model's engine (models NULL, Q 0), or a bag's context, models and weights
struct Target
{
    dmx_ctx *c;
    dmx_model *const *models;
    int Q;
    const float *w;
    int S;
};
inline Target root_target(const engine_model &model, int S) // under model.lock
{
    return Target{dmx_engine_root_ctx(model.engine, 0), nullptr, 0, nullptr, S};
}
// tracks x shifts offsets from the options, or with a bag (Q >= 0) tracks x models x shifts: empty (`fill` everywhere),
// `shifts` values (for every track and model) or all of them, row-major
inline std::vector<int> expand_shifts(const char *who, int fill, size_t T, int Q, const inference_options &opts)
{
    const size_t N = (size_t)std::max(opts.shifts, 0), all = T * (Q < 0 ? 1 : (size_t)Q) * N;
    std::vector<int> shifts(all, fill);
    if (opts.shift_offsets.size() == N)
        for (size_t i = 0; i < shifts.size(); ++i)
            shifts[i] = opts.shift_offsets[i % N];
    else if (opts.shift_offsets.size() == all)
        shifts = opts.shift_offsets;
    else if (!opts.shift_offsets.empty())
    {
        std::cerr << who << ": " << opts.shift_offsets.size() << " shift offsets for " << T << " tracks x ";
        if (Q >= 0)
            std::cerr << Q << " models x ";
        std::cerr << N << " shifts" << std::endl;
        std::exit(1);
    }
    return shifts;
}
struct TrackInputs // the tracks as the ABI takes them
{
    std::vector<const float *> in;
    std::vector<int64_t> n;
    explicit TrackInputs(const std::vector<StereoMatrix> &tracks)
    {
        for (const StereoMatrix &t : tracks)
            in.push_back(t.data.data()), n.push_back(t.cols());
    }
};
// fp32 stems of many tracks in one call; each result is bit-identical to demucs_inference of that track alone. opts NULL:
// dmx_tracks_infer, one offset per track; else dmx_tracks_infer_opts, or with a bag dmx_tracks_infer_bag
inline std::vector<StemTensor> fp32_call(const char *who, const Target &g, const std::vector<StereoMatrix> &tracks, const std::vector<int> &shifts,
                                         const ProgressCallback &cb, const inference_options *opts)
{
    const int T = (int)tracks.size();
    const TrackInputs x(tracks);
    std::vector<StemTensor> out;
    out.reserve(tracks.size());
    std::vector<float *> dst;
    for (const StereoMatrix &t : tracks)
    {
        out.emplace_back(g.S, t.cols());
        dst.push_back(out.back().data.data());
    }
    const std::vector<void *> vdst(dst.begin(), dst.end());
    CbThunk th{&cb};
    auto run = [&]() -> int {
        if (g.models)
            return dmx_tracks_infer_bag(g.c, g.models, g.Q, g.w, T, x.in.data(), x.n.data(), opts->shifts, opts->overlap, shifts.data(), nullptr,
                                        vdst.data(), nullptr, DMX_LAYOUT_EIGEN, progress_thunk, &th);
        if (opts)
            return dmx_tracks_infer_opts(g.c, T, x.in.data(), x.n.data(), opts->shifts, opts->overlap, shifts.data(), dst.data(), DMX_LAYOUT_EIGEN,
                                         progress_thunk, &th);
        return dmx_tracks_infer(g.c, T, x.in.data(), x.n.data(), shifts.data(), dst.data(), DMX_LAYOUT_EIGEN, progress_thunk, &th);
    };
    if (!g.c || run() != DMX_OK)
        die(who);
    return out;
}
// on the model's first device (the root context of its engine). model.shift_offset applies to every track and copy
// (-1: rand() % 22050 drawn per (track, copy), in order)
inline std::vector<StemTensor> batch_call(const char *who, const engine_model &model, int S, const std::vector<StereoMatrix> &tracks,
                                          const ProgressCallback &cb, const inference_options *opts = nullptr)
{
    if (tracks.empty())
        return std::vector<StemTensor>();
    const std::vector<int> shifts = expand_shifts(who, model.shift_offset, tracks.size(), -1, opts ? *opts : inference_options());
    std::lock_guard<std::mutex> guard(model.lock);
    return fp32_call(who, root_target(model, S), tracks, shifts, cb, opts);
}
} // namespace detail
inline std::vector<StemTensor> demucs_inference_batch(const demucs_model &model, const std::vector<StereoMatrix> &tracks, ProgressCallback cb)
{
    return detail::batch_call("demucs_inference_batch", model, model.is_4sources ? 4 : 6, tracks, cb);
}
inline std::vector<StemTensor> demucs_inference_batch(const demucs_model &model, const std::vector<StereoMatrix> &tracks, ProgressCallback cb,
                                                      const inference_options &opts)
{
    return detail::batch_call("demucs_inference_batch", model, model.is_4sources ? 4 : 6, tracks, cb, &opts);
}

// Stems as WAV-ready PCM, encoded on the GPU (dmx_tracks_infer_pcm): demucs's --two-stems, --clip-mode and --int24 /
// --float32. The defaults are demucs's: 16 bit, rescale, all stems. two_stems: -1, or the index of the stem to isolate
// (stem_index("vocals")): output 0 is that stem, output 1 the sum of the others.
struct output_options
{
    int encoding = DMX_PCM_S16;
    int clip = DMX_CLIP_RESCALE;
    int two_stems = -1;
};
// drums 0, bass 1, other 2, vocals 3, guitar 4, piano 5 (the order of the stems in every result); -1: no such stem
inline int stem_index(const std::string &name)
{
    static const char *names[6] = {"drums", "bass", "other", "vocals", "guitar", "piano"};
    for (int i = 0; i < 6; ++i)
        if (name == names[i])
            return i;
    return -1;
}
// result[t][o]: the bytes of the WAV data chunk of output o of track t (interleaved stereo, little-endian, 24 bit packed)
using PcmOutputs = std::vector<std::vector<std::vector<unsigned char>>>;
namespace detail
{
// what a PCM / remix / FLAC call writes: one flat buffer per track (a track's n_out outputs are consecutive across the ABI,
// `per` bytes apart), the peaks and, for .flac files, the sizes
struct TrackOutputs
{
    int n_out;
    std::vector<std::vector<unsigned char>> flat;
    std::vector<void *> dst;
    std::vector<int64_t> per, sizes;
    std::vector<float> pk;
    TrackOutputs(size_t T, int n) : n_out(n), sizes(T * (size_t)n, 0), pk(T * (size_t)n, 0.0f) { flat.reserve(T); }
    void add(const char *who, int64_t bytes) // the next track: `bytes` per output, as the library sized it
    {
        if (bytes < 0)
            die(who);
        per.push_back(bytes);
        flat.emplace_back((size_t)(std::max<int64_t>(bytes, 1) * n_out));
        dst.push_back(flat.back().data());
    }
    // result[t][o]: the `per` bytes of the output, or for .flac files the first sizes[t * n_out + o] of them; then the peaks
    PcmOutputs cut(std::vector<std::vector<float>> *peaks, bool flac = false)
    {
        const size_t T = flat.size();
        PcmOutputs out(T);
        for (size_t t = 0; t < T; ++t)
        {
            for (int o = 0; o < n_out; ++o)
            {
                const auto first = flat[t].begin() + (size_t)o * (size_t)per[t];
                out[t].emplace_back(first, first + (size_t)(flac ? sizes[t * (size_t)n_out + o] : per[t]));
            }
            flat[t] = std::vector<unsigned char>();
        }
        if (peaks)
        {
            peaks->assign(T, std::vector<float>());
            for (size_t t = 0; t < T; ++t)
                (*peaks)[t].assign(pk.begin() + t * (size_t)n_out, pk.begin() + (t + 1) * (size_t)n_out);
        }
        return out;
    }
};
// dmx_tracks_infer_pcm, or with a bag dmx_tracks_infer_bag
inline PcmOutputs pcm_call(const char *who, const Target &g, const std::vector<StereoMatrix> &tracks, const std::vector<int> &shifts,
                           const ProgressCallback &cb, const inference_options &opts, const output_options &oo,
                           std::vector<std::vector<float>> *peaks)
{
    const int T = (int)tracks.size();
    const dmx_output_spec spec{oo.encoding, oo.clip, oo.two_stems};
    const TrackInputs x(tracks);
    TrackOutputs y(tracks.size(), oo.two_stems < 0 ? g.S : 2);
    for (int64_t n : x.n)
        y.add(who, dmx_output_bytes(&spec, n));
    CbThunk th{&cb};
    if (!g.c || (g.models ? dmx_tracks_infer_bag(g.c, g.models, g.Q, g.w, T, x.in.data(), x.n.data(), opts.shifts, opts.overlap, shifts.data(), &spec,
                                                 y.dst.data(), y.pk.data(), DMX_LAYOUT_EIGEN, progress_thunk, &th)
                          : dmx_tracks_infer_pcm(g.c, T, x.in.data(), x.n.data(), opts.shifts, opts.overlap, shifts.data(), &spec, y.dst.data(),
                                                 y.pk.data(), DMX_LAYOUT_EIGEN, progress_thunk, &th)) != DMX_OK)
        die(who);
    return y.cut(peaks);
}
inline PcmOutputs batch_call_pcm(const char *who, const engine_model &model, const std::vector<StereoMatrix> &tracks, const ProgressCallback &cb,
                                 const inference_options &opts, const output_options &oo, std::vector<std::vector<float>> *peaks)
{
    if (tracks.empty())
        return PcmOutputs();
    const std::vector<int> shifts = expand_shifts(who, model.shift_offset, tracks.size(), -1, opts);
    std::lock_guard<std::mutex> guard(model.lock);
    return pcm_call(who, root_target(model, dmx_engine_n_sources(model.engine)), tracks, shifts, cb, opts, oo, peaks);
}
} // namespace detail
inline PcmOutputs demucs_inference_batch_pcm(const demucs_model &model, const std::vector<StereoMatrix> &tracks, ProgressCallback cb,
                                             const inference_options &opts, const output_options &out_opts,
                                             std::vector<std::vector<float>> *peaks = nullptr)
{
    return detail::batch_call_pcm("demucs_inference_batch_pcm", model, tracks, cb, opts, out_opts, peaks);
}

// what remix_options::loudness.meters receives (dmx_tracks_infer_meters): per track the library's n_out + 1 entries, the outputs
// and then the mixture
using MetersReport = std::vector<std::vector<dmx_meters_result>>;
// what remix_options::loudness.limit_report receives (dmx_tracks_infer_limit): per track the library's n_out entries
using LimitReport = std::vector<std::vector<dmx_limit_result>>;
// Outputs mixed on the GPU from the stems and the original mixture (dmx_tracks_infer_remix; include/demucs_hip.h
// dmx_remix_spec): output o is names[o], its row of gains is gains[o * (nb_sources + 1) ...], the last entry of a row the
// gain of the mixture. The defaults are demucs's: 16 bit, rescale.
struct remix_options
{
    int encoding = DMX_PCM_S16;
    int clip = DMX_CLIP_RESCALE;
    std::vector<std::string> names;
    std::vector<float> gains;
    // demucs's --flac (dmx_tracks_infer_flac): the outputs are complete .flac files instead of WAV data, 16 bit for
    // DMX_PCM_S16 and 24 bit for DMX_PCM_S24 (DMX_PCM_F32 is refused); sample_rate is written into their headers
    bool flac = false;
    int sample_rate = 44100;
    // the compression level of those files (dmx_ctx_set_flac_level, applied around the call and put back behind it):
    // 0 FIXED predictors alone, 1 + LPC order 8, 2 + LPC orders 8 and 12; it means nothing without flac
    int flac_level = 0;
    // the loudness stage (dmx_tracks_infer_loud / dmx_tracks_infer_from_flac_loud), off by default: mode
    // DMX_LOUD_MEASURE | DMX_LOUD_MIXTURE | DMX_LOUD_EACH, the target in LUFS, the ceiling of the sample peak as a linear value
    // (-1 dBFS; infinity: none). The overloads that take these options have a last argument, LoudnessReport *loudness_report,
    // that receives the report. With flac and without rates the files are taken to be at 44100 Hz (sample_rate must say so).
    // true_peak: max_peak is a ceiling of the TRUE peak (DMX_LOUD_TRUE_PEAK), -1 dBTP. meters: null, or
    // where the call leaves its meters report (dmx_tracks_infer_meters / dmx_tracks_infer_from_flac_meters): per track n_out + 1
    // entries, the outputs and then the mixture, each with its true peak, loudness range and momentary and short-term maxima.
    struct loudness_options
    {
        bool on = false;
        int mode = DMX_LOUD_MIXTURE;
        float target_lufs = -14.0f, max_peak = 0.8912509f;
        bool true_peak = false;
        MetersReport *meters = nullptr;
        // the look-ahead peak limiter (DMX_LOUD_LIMIT): the ceiling no longer lowers the gain, the limiter
        // holds max_peak. With mode DMX_LOUD_UNITY it is the limiter without loudnorm. attack_ms / release_ms: the times in which
        // the reduction moves by 10 dB. limit_report: null, or where the call leaves the limiter's report, per track n_out entries.
        bool limit = false;
        float attack_ms = DMX_LIMIT_ATTACK_MS, release_ms = DMX_LIMIT_RELEASE_MS;
        LimitReport *limit_report = nullptr;
    };
    loudness_options loudness;
};
// what a call with remix_options::loudness on reports: per track the library's n_out + 1 entries, the outputs and then the mixture
using LoudnessReport = std::vector<std::vector<dmx_loudness_result>>;
// the image of a .flac file, for the overloads that take tracks as files (dmx_tracks_infer_from_flac)
using FlacFile = std::vector<unsigned char>;
// demucs's --two-stems NAME with --other-method add | minus | none (DMX_OTHER_*): outputs "NAME" and, except for none,
// "no_NAME" (add: the other stems added; minus: mixture - stem). Throws std::invalid_argument with the library's message.
inline remix_options remix_two_stems(int nb_sources, int stem, int method)
{
    static const char *stems[6] = {"drums", "bass", "other", "vocals", "guitar", "piano"};
    float g[2 * 8];
    int n_out = 0;
    if (nb_sources > 6 || dmx_remix_two_stems(nb_sources, stem, method, g, &n_out) != DMX_OK)
        throw std::invalid_argument(nb_sources > 6 ? std::string("remix_two_stems: more than 6 sources") : std::string(dmx_last_error()));
    remix_options ro;
    ro.gains.assign(g, g + n_out * (nb_sources + 1));
    ro.names.push_back(stems[stem]);
    if (n_out == 2)
        ro.names.push_back(std::string("no_") + stems[stem]);
    return ro;
}
// The batch CLI's --remix grammar: NAME=TERMS[,NAME=TERMS...], TERMS a sequence of [+|-][GAIN*]SOURCE (the sign may be left
// out in front of the first term only). SOURCE: a stem name of an nb_sources-source model, or "mix" (the original mixture).
// GAIN: a decimal number (digits with at most one point), or NdB = 10^(N/20) evaluated in double and rounded to fp32; behind
// a term's sign a GAIN may carry a minus of its own ("+-12dB*vocals": 12 dB down; "-12dB*vocals" is minus 12 dB UP).
// "karaoke=mix-vocals,backing=drums+bass+other+-12dB*vocals" -> two outputs. A source may appear once per output; names
// are file name parts: not empty, no '/', no duplicates. Throws std::invalid_argument naming the bad term.
inline remix_options parse_remix(const std::string &text, int nb_sources)
{
    static const char *stems[6] = {"drums", "bass", "other", "vocals", "guitar", "piano"};
    auto bad = [](const std::string &what) -> std::invalid_argument { return std::invalid_argument("remix: " + what); };
    if (nb_sources < 1 || nb_sources > 6)
        throw bad("nb_sources " + std::to_string(nb_sources) + " (1 to 6)");
    remix_options ro;
    const size_t W = (size_t)nb_sources + 1;
    for (size_t pos = 0;;)
    {
        const size_t comma = text.find(',', pos);
        const std::string item = text.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
        const size_t eq = item.find('=');
        if (eq == std::string::npos)
            throw bad("'" + item + "': expected NAME=TERMS");
        const std::string name = item.substr(0, eq), terms = item.substr(eq + 1);
        if (name.empty())
            throw bad("'" + item + "': empty output name");
        if (name.find('/') != std::string::npos)
            throw bad("output name '" + name + "' contains '/'");
        if (std::find(ro.names.begin(), ro.names.end(), name) != ro.names.end())
            throw bad("output name '" + name + "' given twice");
        if (terms.empty())
            throw bad("output '" + name + "': no terms");
        if ((int)ro.names.size() == DMX_MAX_OUTPUTS)
            throw bad("more than " + std::to_string(DMX_MAX_OUTPUTS) + " outputs");
        std::vector<float> row(W, 0.0f);
        std::vector<bool> seen(W, false);
        for (size_t i = 0; i < terms.size();)
        {
            const size_t t0 = i;
            float sign = 1.0f;
            if (terms[i] == '+' || terms[i] == '-')
                sign = terms[i++] == '-' ? -1.0f : 1.0f;
            else if (i != 0)
                throw bad("output '" + name + "': internal error"); // cannot happen: a term ends at a sign
            bool gneg = false;
            if (i < terms.size() && terms[i] == '-' && i > t0) // the gain's own minus, behind the term's sign
                gneg = true, ++i;
            size_t e = i;
            while (e < terms.size() && terms[e] != '+' && terms[e] != '-')
                ++e;
            const std::string term = terms.substr(t0, e - t0), body = terms.substr(i, e - i);
            const size_t star = body.find('*');
            std::string source = body;
            double gain = 1.0;
            if (star != std::string::npos)
            {
                source = body.substr(star + 1);
                std::string num = body.substr(0, star);
                const bool db = num.size() >= 2 && num.compare(num.size() - 2, 2, "dB") == 0;
                if (db)
                    num.resize(num.size() - 2);
                size_t digits = 0, points = 0;
                for (char ch : num)
                    digits += ch >= '0' && ch <= '9', points += ch == '.';
                if (digits == 0 || points > 1 || digits + points != num.size())
                    throw bad("output '" + name + "', term '" + term + "': bad gain '" + body.substr(0, star) + "'");
                gain = std::strtod(num.c_str(), nullptr);
                if (gneg)
                    gain = -gain;
                if (db)
                    gain = std::pow(10.0, gain / 20.0);
            }
            else if (gneg)
                throw bad("output '" + name + "', term '" + term + "': bad gain '-'");
            const float g = sign * (float)gain;
            if (!std::isfinite(g))
                throw bad("output '" + name + "', term '" + term + "': the gain is not finite");
            int src = -1;
            if (source == "mix")
                src = nb_sources;
            else
                for (int k = 0; k < nb_sources; ++k)
                    if (source == stems[k])
                        src = k;
            if (src < 0)
                throw bad("output '" + name + "', term '" + term + "': unknown source '" + source + "' (a stem of the " +
                          std::to_string(nb_sources) + "-source model, or mix)");
            if (seen[(size_t)src])
                throw bad("output '" + name + "', term '" + term + "': source '" + source + "' appears twice");
            seen[(size_t)src] = true, row[(size_t)src] = g;
            i = e;
        }
        ro.names.push_back(name);
        ro.gains.insert(ro.gains.end(), row.begin(), row.end());
        if (comma == std::string::npos)
            break;
        pos = comma + 1;
    }
    return ro;
}
namespace detail
{
// the dmx_remix_spec of the options (it points into them), checked against a model of S stems
inline dmx_remix_spec remix_spec(const char *who, int S, const remix_options &ro)
{
    const int n_out = (int)ro.names.size();
    if (ro.gains.size() != (size_t)n_out * (size_t)(S + 1))
    {
        std::cerr << who << ": " << ro.gains.size() << " gains for " << n_out << " outputs x (" << S << " stems + the mixture)" << std::endl;
        std::exit(1);
    }
    const dmx_remix_spec spec{ro.encoding, ro.clip, n_out, ro.gains.data()};
    if (dmx_remix_check(S, &spec) != DMX_OK)
        die(who);
    return spec;
}
// bytes of one output of n frames: its WAV data, or the bound of its .flac file
inline int64_t remix_bytes(const remix_options &ro, int64_t n)
{
    const dmx_output_spec ospec{ro.encoding, ro.clip, -1};
    return ro.flac ? dmx_flac_bound(ro.encoding == DMX_PCM_S16 ? 16 : 24, n) : dmx_output_bytes(&ospec, n);
}
// the flat report of a call with ro.loudness.on, cut per track into *report
inline void loudness_report_cut(const remix_options &ro, const std::vector<dmx_loudness_result> &rep, size_t T, int n_out, LoudnessReport *report)
{
    if (!ro.loudness.on || !report)
        return;
    report->assign(T, std::vector<dmx_loudness_result>());
    for (size_t t = 0; t < T; ++t)
        (*report)[t].assign(rep.begin() + (std::ptrdiff_t)(t * (size_t)(n_out + 1)),
                                        rep.begin() + (std::ptrdiff_t)((t + 1) * (size_t)(n_out + 1)));
}
// the loudness spec of a call, and the flat meters report it fills (empty: none asked for), cut per track behind the call
inline dmx_loudness_spec loudness_spec_of(const remix_options &ro)
{
    return dmx_loudness_spec{ro.loudness.mode | (ro.loudness.true_peak ? DMX_LOUD_TRUE_PEAK : 0) | (ro.loudness.limit ? DMX_LOUD_LIMIT : 0),
                             ro.loudness.target_lufs, ro.loudness.max_peak};
}
inline dmx_limiter_spec limiter_spec_of(const remix_options &ro) { return dmx_limiter_spec{ro.loudness.attack_ms, ro.loudness.release_ms}; }
inline void limit_report_cut(const remix_options &ro, const std::vector<dmx_limit_result> &rep, size_t T, int n_out)
{
    if (!ro.loudness.on || !ro.loudness.limit_report)
        return;
    ro.loudness.limit_report->assign(T, std::vector<dmx_limit_result>());
    for (size_t t = 0; t < T; ++t)
        (*ro.loudness.limit_report)[t].assign(rep.begin() + (std::ptrdiff_t)(t * (size_t)n_out), rep.begin() + (std::ptrdiff_t)((t + 1) * (size_t)n_out));
}
inline void meters_report_cut(const remix_options &ro, const std::vector<dmx_meters_result> &rep, size_t T, int n_out)
{
    if (!ro.loudness.on || !ro.loudness.meters)
        return;
    ro.loudness.meters->assign(T, std::vector<dmx_meters_result>());
    for (size_t t = 0; t < T; ++t)
        (*ro.loudness.meters)[t].assign(rep.begin() + (std::ptrdiff_t)(t * (size_t)(n_out + 1)),
                                        rep.begin() + (std::ptrdiff_t)((t + 1) * (size_t)(n_out + 1)));
}
// one call of dmx_tracks_infer_remix, or for ro.flac dmx_tracks_infer_flac; shifts as the caller's path lays them out.
// rates: track t is at (*rates)[t] Hz (dmx_tracks_infer_rates)
inline PcmOutputs remix_call(const char *who, const Target &g, const std::vector<StereoMatrix> &tracks, const std::vector<int> &shifts,
                             const ProgressCallback &cb, const inference_options &opts, const remix_options &ro,
                             std::vector<std::vector<float>> *peaks, const std::vector<int> *rates = nullptr, LoudnessReport *report = nullptr)
{
    const int T = (int)tracks.size();
    if (rates && rates->size() != tracks.size())
    {
        std::cerr << who << ": " << rates->size() << " rates for " << T << " tracks" << std::endl;
        std::exit(1);
    }
    const dmx_remix_spec spec = remix_spec(who, g.S, ro);
    if (ro.flac && ro.encoding != DMX_PCM_S16 && ro.encoding != DMX_PCM_S24)
    {
        std::cerr << who << ": remix_options.flac needs encoding DMX_PCM_S16 or DMX_PCM_S24" << std::endl;
        std::exit(1);
    }
    const TrackInputs x(tracks);
    TrackOutputs y(tracks.size(), spec.n_out);
    for (int64_t n : x.n)
        y.add(who, remix_bytes(ro, n));
    if (ro.loudness.on && ro.flac && !rates && ro.sample_rate != 44100)
    {
        std::cerr << who << ": remix_options.loudness with flac takes the tracks to be at 44100 Hz (pass their rates instead)" << std::endl;
        std::exit(1);
    }
    CbThunk th{&cb};
    FlacLevelGuard level(g.c, ro.flac ? ro.flac_level : 0);
    const dmx_loudness_spec lspec = loudness_spec_of(ro);
    std::vector<dmx_loudness_result> rep(ro.loudness.on ? (size_t)T * (size_t)(spec.n_out + 1) : 0);
    std::vector<dmx_meters_result> mrep(ro.loudness.on && ro.loudness.meters ? rep.size() : 0);
    const dmx_limiter_spec lim = limiter_spec_of(ro);
    std::vector<dmx_limit_result> lrep(ro.loudness.on && ro.loudness.limit_report ? (size_t)T * (size_t)spec.n_out : 0);
    auto run = [&]() -> int {
        if (ro.loudness.on) // (null meters and limiter reports: dmx_tracks_infer_loud)
            return dmx_tracks_infer_limit(g.c, g.models, g.Q, g.w, T, x.in.data(), x.n.data(), rates ? rates->data() : nullptr, opts.shifts,
                                           opts.overlap, shifts.data(), &spec, ro.flac ? 1 : 0, y.dst.data(), ro.flac ? y.sizes.data() : nullptr,
                                           y.pk.data(), DMX_LAYOUT_EIGEN, progress_thunk, &th, &lspec, rep.data(),
                                           mrep.empty() ? nullptr : mrep.data(), &lim, lrep.empty() ? nullptr : lrep.data());
        if (rates)
            return dmx_tracks_infer_rates(g.c, g.models, g.Q, g.w, T, x.in.data(), x.n.data(), rates->data(), opts.shifts, opts.overlap, shifts.data(),
                                          &spec, ro.flac ? 1 : 0, y.dst.data(), ro.flac ? y.sizes.data() : nullptr, y.pk.data(), DMX_LAYOUT_EIGEN,
                                          progress_thunk, &th);
        if (ro.flac)
            return dmx_tracks_infer_flac(g.c, g.models, g.Q, g.w, T, x.in.data(), x.n.data(), opts.shifts, opts.overlap, shifts.data(), &spec,
                                         ro.sample_rate, y.dst.data(), y.sizes.data(), y.pk.data(), DMX_LAYOUT_EIGEN, progress_thunk, &th);
        return dmx_tracks_infer_remix(g.c, g.models, g.Q, g.w, T, x.in.data(), x.n.data(), opts.shifts, opts.overlap, shifts.data(), &spec,
                                      y.dst.data(), y.pk.data(), DMX_LAYOUT_EIGEN, progress_thunk, &th);
    };
    if (!g.c || !level.ok || run() != DMX_OK)
        die(who);
    loudness_report_cut(ro, rep, tracks.size(), spec.n_out, report);
    meters_report_cut(ro, mrep, tracks.size(), spec.n_out);
    limit_report_cut(ro, lrep, tracks.size(), spec.n_out);
    return y.cut(peaks, ro.flac);
}
// the same on tracks given as the images of .flac files (dmx_tracks_infer_from_flac): ro.flac chooses the output form.
// frames (optional) receives each track's sample count. A file the probe refuses, a rate other than 44100 Hz or a stream
// that breaks inside ends the process with the library's message, which names the track. rates (optional) receives the
// files' sample rates and lets every track run at its own (dmx_tracks_infer_from_flac_rates; .flac outputs carry it).
inline PcmOutputs flac_files_call(const char *who, const Target &g, const std::vector<FlacFile> &files, const std::vector<int> &shifts,
                                  const ProgressCallback &cb, const inference_options &opts, const remix_options &ro,
                                  std::vector<std::vector<float>> *peaks, std::vector<int64_t> *frames, std::vector<int> *rates = nullptr, LoudnessReport *report = nullptr)
{
    const size_t T = files.size();
    const dmx_remix_spec spec = remix_spec(who, g.S, ro);
    if (ro.flac && (ro.encoding != DMX_PCM_S16 && ro.encoding != DMX_PCM_S24 || (!rates && ro.sample_rate != 44100)))
    {
        std::cerr << who << ": remix_options.flac needs encoding DMX_PCM_S16 or DMX_PCM_S24 and sample_rate 44100" << std::endl;
        std::exit(1);
    }
    std::vector<const void *> in(T);
    std::vector<int64_t> bytes(T), n(T);
    TrackOutputs y(T, spec.n_out);
    for (size_t t = 0; t < T; ++t)
    {
        dmx_flac_info info;
        in[t] = files[t].data(), bytes[t] = (int64_t)files[t].size();
        if (dmx_flac_probe(in[t], bytes[t], &info) != DMX_OK)
        {
            std::cerr << who << ": track " << t << ": " << dmx_last_error() << std::endl;
            std::exit(1);
        }
        n[t] = info.total_samples;
        if (rates)
            rates->resize(T), (*rates)[t] = info.sample_rate;
        y.add(who, remix_bytes(ro, n[t]));
    }
    std::vector<int64_t> status(2 * T, 0);
    CbThunk th{&cb};
    FlacLevelGuard level(g.c, ro.flac ? ro.flac_level : 0);
    const dmx_loudness_spec lspec = loudness_spec_of(ro);
    std::vector<dmx_loudness_result> rep(ro.loudness.on ? T * (size_t)(spec.n_out + 1) : 0);
    std::vector<dmx_meters_result> mrep(ro.loudness.on && ro.loudness.meters ? rep.size() : 0);
    const dmx_limiter_spec lim = limiter_spec_of(ro);
    std::vector<dmx_limit_result> lrep(ro.loudness.on && ro.loudness.limit_report ? T * (size_t)spec.n_out : 0);
    if (!g.c || !level.ok ||
        (ro.loudness.on
             ? dmx_tracks_infer_from_flac_limit(g.c, g.models, g.Q, g.w, (int)T, in.data(), bytes.data(), opts.shifts, opts.overlap,
                                                 shifts.data(), &spec, ro.flac ? 1 : 0, y.dst.data(), y.sizes.data(), y.pk.data(), status.data(),
                                                 progress_thunk, &th, &lspec, rep.data(), mrep.empty() ? nullptr : mrep.data(), &lim,
                                                lrep.empty() ? nullptr : lrep.data())
             : (rates ? dmx_tracks_infer_from_flac_rates : dmx_tracks_infer_from_flac)(g.c, g.models, g.Q, g.w, (int)T, in.data(), bytes.data(),
                                                                                       opts.shifts, opts.overlap, shifts.data(), &spec,
                                                                                       ro.flac ? 1 : 0, y.dst.data(), y.sizes.data(), y.pk.data(),
                                                                                       status.data(), progress_thunk, &th)) != DMX_OK)
        die(who);
    loudness_report_cut(ro, rep, T, spec.n_out, report);
    meters_report_cut(ro, mrep, T, spec.n_out);
    limit_report_cut(ro, lrep, T, spec.n_out);
    if (frames)
        *frames = n;
    return y.cut(peaks, ro.flac);
}
inline PcmOutputs batch_call_from_flac(const char *who, const engine_model &model, const std::vector<FlacFile> &files,
                                       const ProgressCallback &cb, const inference_options &opts, const remix_options &ro,
                                       std::vector<std::vector<float>> *peaks, std::vector<int64_t> *frames, std::vector<int> *rates = nullptr, LoudnessReport *report = nullptr)
{
    if (files.empty())
        return PcmOutputs();
    const std::vector<int> shifts = expand_shifts(who, model.shift_offset, files.size(), -1, opts);
    std::lock_guard<std::mutex> guard(model.lock);
    return flac_files_call(who, root_target(model, dmx_engine_n_sources(model.engine)), files, shifts, cb, opts, ro, peaks, frames, rates, report);
}
inline PcmOutputs batch_call_remix(const char *who, const engine_model &model, const std::vector<StereoMatrix> &tracks,
                                   const ProgressCallback &cb, const inference_options &opts, const remix_options &ro,
                                   std::vector<std::vector<float>> *peaks, const std::vector<int> *rates = nullptr, LoudnessReport *report = nullptr)
{
    if (tracks.empty())
        return PcmOutputs();
    const std::vector<int> shifts = expand_shifts(who, model.shift_offset, tracks.size(), -1, opts);
    std::lock_guard<std::mutex> guard(model.lock);
    return remix_call(who, root_target(model, dmx_engine_n_sources(model.engine)), tracks, shifts, cb, opts, ro, peaks, rates, report);
}
} // namespace detail
inline PcmOutputs demucs_inference_batch_remix(const demucs_model &model, const std::vector<StereoMatrix> &tracks, ProgressCallback cb,
                                               const inference_options &opts, const remix_options &remix,
                                               std::vector<std::vector<float>> *peaks = nullptr, LoudnessReport *loudness_report = nullptr)
{
    return detail::batch_call_remix("demucs_inference_batch_remix", model, tracks, cb, opts, remix, peaks, nullptr, loudness_report);
}

// tracks given as .flac files (44100 Hz; decoded on the GPU): frames (optional) receives each track's sample count
inline PcmOutputs demucs_inference_batch_remix(const demucs_model &model, const std::vector<FlacFile> &files, ProgressCallback cb,
                                               const inference_options &opts, const remix_options &remix,
                                               std::vector<std::vector<float>> *peaks = nullptr, std::vector<int64_t> *frames = nullptr, LoudnessReport *loudness_report = nullptr)
{
    return detail::batch_call_from_flac("demucs_inference_batch_remix (flac files)", model, files, cb, opts, remix, peaks, frames, nullptr, loudness_report);
}

// Tracks at their own sample rates (dmx_tracks_infer_rates): tracks[t] holds the caller's frames at rates[t] Hz, the outputs
// have those frames and that rate, and both conversions run on the device inside the track path. For .flac files `rates`
// RECEIVES the files' rates, and remix.sample_rate is not read: every .flac output carries its track's rate.
inline PcmOutputs demucs_inference_batch_remix(const demucs_model &model, const std::vector<StereoMatrix> &tracks, const std::vector<int> &rates,
                                               ProgressCallback cb, const inference_options &opts, const remix_options &remix,
                                               std::vector<std::vector<float>> *peaks = nullptr, LoudnessReport *loudness_report = nullptr)
{
    return detail::batch_call_remix("demucs_inference_batch_remix (rates)", model, tracks, cb, opts, remix, peaks, &rates, loudness_report);
}
inline PcmOutputs demucs_inference_batch_remix(const demucs_model &model, const std::vector<FlacFile> &files, std::vector<int> &rates,
                                               ProgressCallback cb, const inference_options &opts, const remix_options &remix,
                                               std::vector<std::vector<float>> *peaks = nullptr, std::vector<int64_t> *frames = nullptr, LoudnessReport *loudness_report = nullptr)
{
    return detail::batch_call_from_flac("demucs_inference_batch_remix (flac files, rates)", model, files, cb, opts, remix, peaks, frames, &rates, loudness_report);
}

// The fine-tuned bag (cli-apps/demucs_ft.cpp:136-241): four 4-source models, stem i from model i. The
// reference runs four demucs_inference calls back to back; calling demucs_inference on four demucs_model
// objects still works here, but one bag engine deals all (model, segment) items over the devices at once
// (168 items on 8 GPUs = 21 each, instead of four rounds of 42 = 6 + 6 + 5 + ...).
struct demucs_ft_bag
{
    std::vector<int> devices;
    int shift_offsets[4] = {-1, -1, -1, -1}; // -1: successive rand() % 22050 draws, like four demucs_inference calls
    int max_batch = 12;
    dmx_engine *engine = nullptr;
    mutable std::mutex lock;
    demucs_ft_bag() {}
    demucs_ft_bag(const demucs_ft_bag &) = delete;
    demucs_ft_bag &operator=(const demucs_ft_bag &) = delete;
    ~demucs_ft_bag()
    {
        if (engine)
            dmx_engine_free(engine);
    }
};
// model_files: drums, bass, other, vocals (the order of cli-apps/demucs_ft.cpp:141-168)
inline bool load_demucs_ft_bag(const std::vector<std::string> &model_files, demucs_ft_bag *bag)
{
    if (model_files.size() != 4)
    {
        std::cerr << "load_demucs_ft_bag: four model files are required" << std::endl;
        return false;
    }
    if (bag->devices.empty())
        bag->devices = detail::devices_from_env();
    int so = -1;
    detail::read_env(so, bag->max_batch);
    if (so >= 0)
        for (int &v : bag->shift_offsets)
            v = so;
    const char *files[4] = {model_files[0].c_str(), model_files[1].c_str(), model_files[2].c_str(), model_files[3].c_str()};
    if (dmx_engine_create(files, 4, bag->devices.data(), (int)bag->devices.size(), bag->max_batch, DMX_TRANSPORT_AUTO, &bag->engine) !=
        DMX_OK)
    {
        std::cerr << "load_demucs_ft_bag: " << dmx_last_error() << std::endl;
        return false;
    }
    return true;
}
inline StemTensor demucs_ft_inference(const demucs_ft_bag &bag, const StereoMatrix &full_audio, ProgressCallback cb)
{
    StemTensor out(4, full_audio.cols());
    detail::CbThunk th{&cb};
    std::lock_guard<std::mutex> guard(bag.lock);
    if (dmx_engine_track_infer(bag.engine, full_audio.data.data(), full_audio.cols(), bag.shift_offsets, out.data.data(), DMX_LAYOUT_EIGEN,
                               detail::progress_thunk, &th) != DMX_OK)
        detail::die("demucs_ft_inference");
    return out;
}

// A bag of models on the batch path (dmx_tracks_infer_bag): Q models of one architecture on one
// device, one context, a weight per (model, stem). The fine-tuned bag is the diagonal (no weights: stem i from model i);
// equal weights average the models. shift_offset applies to every (track, model, copy); -1: rand() % 22050 drawn in that
// order. The tracks' segments share batches per model, and every option of the single-model batch calls applies.
struct demucs_bag
{
    int device = -1;       // -1: DMX_DEVICE, else 0
    int shift_offset = -1; // DMX_SHIFT_OFFSET
    int max_batch = 12;    // DMX_BATCH
    int arch = 0, nb_sources = 0;
    std::vector<dmx_model *> models;
    dmx_ctx *ctx = nullptr;
    mutable std::mutex lock;
    demucs_bag() {}
    demucs_bag(const demucs_bag &) = delete;
    demucs_bag &operator=(const demucs_bag &) = delete;
    ~demucs_bag()
    {
        if (ctx)
            dmx_ctx_free(ctx);
        for (dmx_model *m : models)
            dmx_model_free(m);
    }
};
inline bool load_demucs_bag(const std::vector<std::string> &model_files, demucs_bag *bag)
{
    if (model_files.empty() || model_files.size() > (size_t)DMX_MAX_BAG)
    {
        std::cerr << "load_demucs_bag: 1 to " << DMX_MAX_BAG << " model files are required, got " << model_files.size() << std::endl;
        return false;
    }
    if (bag->device < 0)
    {
        const char *one = std::getenv("DMX_DEVICE");
        bag->device = one ? std::atoi(one) : 0;
    }
    detail::read_env(bag->shift_offset, bag->max_batch);
    for (const std::string &f : model_files)
    {
        dmx_model *m = nullptr;
        if (dmx_model_load(f.c_str(), bag->device, &m) != DMX_OK)
        {
            std::cerr << "load_demucs_bag: " << f << ": " << dmx_last_error() << std::endl;
            return false;
        }
        bag->models.push_back(m);
    }
    bag->arch = dmx_model_arch(bag->models[0]), bag->nb_sources = dmx_model_n_sources(bag->models[0]);
    if (dmx_ctx_create(bag->models[0], 0, bag->max_batch, &bag->ctx) != DMX_OK)
    {
        std::cerr << "load_demucs_bag: " << dmx_last_error() << std::endl;
        return false;
    }
    return true;
}
namespace detail
{
// weights: empty (the diagonal) or models x stems
inline const float *bag_weights(const char *who, const demucs_bag &bag, const std::vector<float> &weights)
{
    if (weights.empty())
        return nullptr;
    if (weights.size() != bag.models.size() * (size_t)bag.nb_sources)
    {
        std::cerr << who << ": " << weights.size() << " weights for " << bag.models.size() << " models x " << bag.nb_sources << " stems"
                  << std::endl;
        std::exit(1);
    }
    return weights.data();
}
// the prologue of every call on a bag: the shift offsets (tracks x models x shifts; the bag's shift_offset where the options
// give none), then the weights are checked, then the bag's lock is taken and held
struct BagCall
{
    std::vector<int> shifts;
    Target g;
    std::lock_guard<std::mutex> guard;
    BagCall(const char *who, const demucs_bag &bag, size_t T, const std::vector<float> &weights, const inference_options &opts)
        : shifts(expand_shifts(who, bag.shift_offset, T, (int)bag.models.size(), opts)),
          g{bag.ctx, bag.models.data(), (int)bag.models.size(), bag_weights(who, bag, weights), bag.nb_sources}, guard(bag.lock)
    {
    }
};
} // namespace detail
// weights: empty (the diagonal: needs as many models as stems) or models x stems, row-major
inline std::vector<StemTensor> demucs_inference_batch(const demucs_bag &bag, const std::vector<StereoMatrix> &tracks, ProgressCallback cb,
                                                      const std::vector<float> &weights = std::vector<float>(),
                                                      const inference_options &opts = inference_options())
{
    const char *who = "demucs_inference_batch (bag)";
    if (tracks.empty())
        return std::vector<StemTensor>();
    const detail::BagCall b(who, bag, tracks.size(), weights, opts);
    return detail::fp32_call(who, b.g, tracks, b.shifts, cb, &opts);
}
inline PcmOutputs demucs_inference_batch_pcm(const demucs_bag &bag, const std::vector<StereoMatrix> &tracks, ProgressCallback cb,
                                             const std::vector<float> &weights, const inference_options &opts, const output_options &oo,
                                             std::vector<std::vector<float>> *peaks = nullptr)
{
    const char *who = "demucs_inference_batch_pcm (bag)";
    if (tracks.empty())
        return PcmOutputs();
    const detail::BagCall b(who, bag, tracks.size(), weights, opts);
    return detail::pcm_call(who, b.g, tracks, b.shifts, cb, opts, oo, peaks);
}
inline PcmOutputs demucs_inference_batch_remix(const demucs_bag &bag, const std::vector<StereoMatrix> &tracks, ProgressCallback cb,
                                               const std::vector<float> &weights, const inference_options &opts, const remix_options &remix,
                                               std::vector<std::vector<float>> *peaks = nullptr, LoudnessReport *loudness_report = nullptr)
{
    const char *who = "demucs_inference_batch_remix (bag)";
    if (tracks.empty())
        return PcmOutputs();
    const detail::BagCall b(who, bag, tracks.size(), weights, opts);
    return detail::remix_call(who, b.g, tracks, b.shifts, cb, opts, remix, peaks, nullptr, loudness_report);
}
inline PcmOutputs demucs_inference_batch_remix(const demucs_bag &bag, const std::vector<FlacFile> &files, ProgressCallback cb,
                                               const std::vector<float> &weights, const inference_options &opts, const remix_options &remix,
                                               std::vector<std::vector<float>> *peaks = nullptr, std::vector<int64_t> *frames = nullptr, LoudnessReport *loudness_report = nullptr)
{
    const char *who = "demucs_inference_batch_remix (bag, flac files)";
    if (files.empty())
        return PcmOutputs();
    const detail::BagCall b(who, bag, files.size(), weights, opts);
    return detail::flac_files_call(who, b.g, files, b.shifts, cb, opts, remix, peaks, frames, nullptr, loudness_report);
}
// the same with tracks at their own rates (see the demucs_model overloads)
inline PcmOutputs demucs_inference_batch_remix(const demucs_bag &bag, const std::vector<StereoMatrix> &tracks, const std::vector<int> &rates,
                                               ProgressCallback cb, const std::vector<float> &weights, const inference_options &opts,
                                               const remix_options &remix, std::vector<std::vector<float>> *peaks = nullptr, LoudnessReport *loudness_report = nullptr)
{
    const char *who = "demucs_inference_batch_remix (bag, rates)";
    if (tracks.empty())
        return PcmOutputs();
    const detail::BagCall b(who, bag, tracks.size(), weights, opts);
    return detail::remix_call(who, b.g, tracks, b.shifts, cb, opts, remix, peaks, &rates, loudness_report);
}
inline PcmOutputs demucs_inference_batch_remix(const demucs_bag &bag, const std::vector<FlacFile> &files, std::vector<int> &rates,
                                               ProgressCallback cb, const std::vector<float> &weights, const inference_options &opts,
                                               const remix_options &remix, std::vector<std::vector<float>> *peaks = nullptr,
                                               std::vector<int64_t> *frames = nullptr, LoudnessReport *loudness_report = nullptr)
{
    const char *who = "demucs_inference_batch_remix (bag, flac files, rates)";
    if (files.empty())
        return PcmOutputs();
    const detail::BagCall b(who, bag, files.size(), weights, opts);
    return detail::flac_files_call(who, b.g, files, b.shifts, cb, opts, remix, peaks, frames, &rates, loudness_report);
}

// segment-level surface; src/model.hpp:569-647 (only the boundary members are kept:
// `mix` in, `targets_out` out - every intermediate lives in the HBM arena)
// Under DEMUCSCPP_HIP_WITH_EIGEN the reference's name `demucs_segment_buffers` IS the Eigen-typed struct further
// down (a caller that keeps `demucscpp::demucs_segment_buffers buffers(2, n, S); buffers.mix(i, j) = ...` with Eigen
// semantics, src/model.hpp:569-647, must get Eigen members); this container-typed one is then reachable as
// demucs_segment_buffers_plain only.
struct demucs_segment_buffers_plain
{
    int segment_samples;
    StereoMatrix mix;
    StemTensor targets_out;
    demucs_segment_buffers_plain(int /*nb_channels*/, int segment_samples_, int nb_sources)
        : segment_samples(segment_samples_), mix(segment_samples_), targets_out(nb_sources, segment_samples_)
    {
    }
};
#ifndef DEMUCSCPP_HIP_WITH_EIGEN
typedef demucs_segment_buffers_plain demucs_segment_buffers;
#endif
struct stft_buffers // kept for signature compatibility (src/dsp.hpp:20-101); the STFT state lives on the GPU
{
    explicit stft_buffers(int /*n_samples*/) {}
};

namespace detail
{
inline void segment_call(const engine_model &model, int segment_samples, const float *mix, float *targets_out, const ProgressCallback &cb,
                         float current_progress, float segment_progress)
{
    if (segment_samples != DMX_SEGMENT_SAMPLES)
    {
        std::cerr << "model_inference: segment must be " << DMX_SEGMENT_SAMPLES << " samples" << std::endl;
        std::exit(1);
    }
    if (cb)
        cb(current_progress, "3., apply_model mix shape: (2, " + std::to_string(segment_samples) + ")");
    {
        std::lock_guard<std::mutex> guard(model.lock);
        dmx_ctx *ctx = dmx_engine_root_ctx(model.engine, 0);
        if (!ctx || dmx_segment_infer(ctx, mix, targets_out, DMX_LAYOUT_EIGEN) != DMX_OK)
            die("model_inference");
    }
    if (cb)
        cb(current_progress + segment_progress, "Mask + istft");
}
} // namespace detail

// src/model.hpp:662-666, src/model_inference.cpp:48-475
inline void model_inference(const demucs_model &model, demucs_segment_buffers_plain &buffers, stft_buffers & /*stft_buf*/,
                            ProgressCallback cb, float current_progress, float segment_progress)
{
    detail::segment_call(model, buffers.segment_samples, buffers.mix.data.data(), buffers.targets_out.data.data(), cb, current_progress,
                         segment_progress);
}

#ifdef DEMUCSCPP_HIP_WITH_EIGEN
// Exact reference signatures on the Eigen types themselves (zero-copy in, written in place out): a
// caller that keeps /root/reference/src/model.hpp:569-666 as it is compiles against these.
typedef Eigen::Tensor<float, 3> Tensor3dXf; // src/tensor.hpp

inline Tensor3dXf demucs_inference(const demucs_model &model, const Eigen::MatrixXf &full_audio, ProgressCallback cb)
{
    const int S = model.is_4sources ? 4 : 6;
    Tensor3dXf out(S, 2, full_audio.cols());
    detail::CbThunk th{&cb};
    std::lock_guard<std::mutex> guard(model.lock);
    if (dmx_engine_track_infer(model.engine, full_audio.data(), full_audio.cols(), &model.shift_offset, out.data(), DMX_LAYOUT_EIGEN,
                               detail::progress_thunk, &th) != DMX_OK)
        detail::die("demucs_inference");
    return out;
}

// src/model.hpp:569-647: the boundary members with the reference's names and types. The reference's
// intermediates (x, xt, saved_*, ... :583-647) live in the HBM arena and have no host image.
struct demucs_segment_buffers // the reference's name and member types
{
    int segment_samples;
    Eigen::MatrixXf mix;     // (nb_channels, segment_samples)
    Tensor3dXf targets_out;  // (nb_sources, nb_channels, segment_samples)
    demucs_segment_buffers(int nb_channels, int segment_samples_, int nb_sources)
        : segment_samples(segment_samples_), mix(nb_channels, segment_samples_), targets_out(nb_sources, nb_channels, segment_samples_)
    {
        mix.setZero();
        targets_out.setZero();
    }
};
typedef demucs_segment_buffers demucs_segment_buffers_eigen; // round-2 name
inline void model_inference(const demucs_model &model, demucs_segment_buffers &buffers, stft_buffers & /*stft_buf*/,
                            ProgressCallback cb, float current_progress, float segment_progress)
{
    detail::segment_call(model, buffers.segment_samples, buffers.mix.data(), buffers.targets_out.data(), cb, current_progress,
                         segment_progress);
}
#endif

} // namespace demucscpp

// ---------------------------------------------------------------------------------------------
// Demucs v3 (hdemucs_mmi): /root/reference/src/model.hpp:668-1415, cli-apps/demucs_v3.cpp. Same engine, same
// threading contract; the weight file carries the "dmc3" magic (README.md:82 ggml-model-hdemucs_mmi-v3-f16.bin).
namespace demucscpp_v3
{
using demucscpp::ProgressCallback;
using demucscpp::StemTensor;
using demucscpp::StereoMatrix;

struct demucs_v3_model : demucscpp::engine_model // src/model.hpp:694-1236: the weights live in HBM
{
};

// src/model.hpp:1396-1397, src/model_load.cpp:1302-2166
inline bool load_demucs_v3_model(const std::string &model_file, demucs_v3_model *model)
{
    return demucscpp::detail::load_engine("load_demucs_v3_model", model_file, model, 3);
}

// src/model.hpp:1405-1408, src/model_apply.cpp:307-339
inline StemTensor demucs_v3_inference(const demucs_v3_model &model, const StereoMatrix &full_audio, ProgressCallback cb)
{
    StemTensor out(4, full_audio.cols());
    demucscpp::detail::CbThunk th{&cb};
    std::lock_guard<std::mutex> guard(model.lock);
    if (dmx_engine_track_infer(model.engine, full_audio.data.data(), full_audio.cols(), &model.shift_offset, out.data.data(),
                               DMX_LAYOUT_EIGEN, demucscpp::detail::progress_thunk, &th) != DMX_OK)
        demucscpp::detail::die("demucs_v3_inference");
    return out;
}

inline std::vector<StemTensor> demucs_v3_inference_batch(const demucs_v3_model &model, const std::vector<StereoMatrix> &tracks,
                                                         ProgressCallback cb)
{
    return demucscpp::detail::batch_call("demucs_v3_inference_batch", model, 4, tracks, cb);
}
inline std::vector<StemTensor> demucs_v3_inference_batch(const demucs_v3_model &model, const std::vector<StereoMatrix> &tracks,
                                                         ProgressCallback cb, const demucscpp::inference_options &opts)
{
    return demucscpp::detail::batch_call("demucs_v3_inference_batch", model, 4, tracks, cb, &opts);
}

inline demucscpp::PcmOutputs demucs_v3_inference_batch_pcm(const demucs_v3_model &model, const std::vector<StereoMatrix> &tracks,
                                                           ProgressCallback cb, const demucscpp::inference_options &opts,
                                                           const demucscpp::output_options &out_opts,
                                                           std::vector<std::vector<float>> *peaks = nullptr)
{
    return demucscpp::detail::batch_call_pcm("demucs_v3_inference_batch_pcm", model, tracks, cb, opts, out_opts, peaks);
}
inline demucscpp::PcmOutputs demucs_v3_inference_batch_remix(const demucs_v3_model &model, const std::vector<StereoMatrix> &tracks,
                                                             ProgressCallback cb, const demucscpp::inference_options &opts,
                                                             const demucscpp::remix_options &remix,
                                                             std::vector<std::vector<float>> *peaks = nullptr, demucscpp::LoudnessReport *loudness_report = nullptr)
{
    return demucscpp::detail::batch_call_remix("demucs_v3_inference_batch_remix", model, tracks, cb, opts, remix, peaks, nullptr, loudness_report);
}
inline demucscpp::PcmOutputs demucs_v3_inference_batch_remix(const demucs_v3_model &model, const std::vector<demucscpp::FlacFile> &files,
                                                             ProgressCallback cb, const demucscpp::inference_options &opts,
                                                             const demucscpp::remix_options &remix,
                                                             std::vector<std::vector<float>> *peaks = nullptr,
                                                             std::vector<int64_t> *frames = nullptr, demucscpp::LoudnessReport *loudness_report = nullptr)
{
    return demucscpp::detail::batch_call_from_flac("demucs_v3_inference_batch_remix (flac files)", model, files, cb, opts, remix, peaks, frames, nullptr, loudness_report);
}
// the same with tracks at their own rates (see demucscpp::demucs_inference_batch_remix)
inline demucscpp::PcmOutputs demucs_v3_inference_batch_remix(const demucs_v3_model &model, const std::vector<StereoMatrix> &tracks,
                                                             const std::vector<int> &rates, ProgressCallback cb,
                                                             const demucscpp::inference_options &opts, const demucscpp::remix_options &remix,
                                                             std::vector<std::vector<float>> *peaks = nullptr, demucscpp::LoudnessReport *loudness_report = nullptr)
{
    return demucscpp::detail::batch_call_remix("demucs_v3_inference_batch_remix (rates)", model, tracks, cb, opts, remix, peaks, &rates, loudness_report);
}
inline demucscpp::PcmOutputs demucs_v3_inference_batch_remix(const demucs_v3_model &model, const std::vector<demucscpp::FlacFile> &files,
                                                             std::vector<int> &rates, ProgressCallback cb,
                                                             const demucscpp::inference_options &opts, const demucscpp::remix_options &remix,
                                                             std::vector<std::vector<float>> *peaks = nullptr,
                                                             std::vector<int64_t> *frames = nullptr, demucscpp::LoudnessReport *loudness_report = nullptr)
{
    return demucscpp::detail::batch_call_from_flac("demucs_v3_inference_batch_remix (flac files, rates)", model, files, cb, opts, remix, peaks,
                                                   frames, &rates, loudness_report);
}

// src/model.hpp:1238-1394: the boundary members (`mix` in, `targets_out` out); LSTM state, decay tables and every
// intermediate live in the HBM arena
typedef demucscpp::demucs_segment_buffers_plain demucs_v3_segment_buffers_plain;
#ifndef DEMUCSCPP_HIP_WITH_EIGEN
typedef demucscpp::demucs_segment_buffers_plain demucs_v3_segment_buffers;
#endif

// src/model.hpp:1410-1414, src/model_inference.cpp:477-856
inline void model_v3_inference(const demucs_v3_model &model, demucs_v3_segment_buffers_plain &buffers, demucscpp::stft_buffers & /*stft_buf*/,
                               ProgressCallback cb, float current_progress, float segment_progress)
{
    demucscpp::detail::segment_call(model, buffers.segment_samples, buffers.mix.data.data(), buffers.targets_out.data.data(), cb,
                                    current_progress, segment_progress);
}

#ifdef DEMUCSCPP_HIP_WITH_EIGEN
inline demucscpp::Tensor3dXf demucs_v3_inference(const demucs_v3_model &model, const Eigen::MatrixXf &full_audio, ProgressCallback cb)
{
    demucscpp::Tensor3dXf out(4, 2, full_audio.cols());
    demucscpp::detail::CbThunk th{&cb};
    std::lock_guard<std::mutex> guard(model.lock);
    if (dmx_engine_track_infer(model.engine, full_audio.data(), full_audio.cols(), &model.shift_offset, out.data(), DMX_LAYOUT_EIGEN,
                               demucscpp::detail::progress_thunk, &th) != DMX_OK)
        demucscpp::detail::die("demucs_v3_inference");
    return out;
}
typedef demucscpp::demucs_segment_buffers demucs_v3_segment_buffers; // Eigen-typed mix / targets_out
inline void model_v3_inference(const demucs_v3_model &model, demucs_v3_segment_buffers &buffers, demucscpp::stft_buffers & /*stft_buf*/,
                               ProgressCallback cb, float current_progress, float segment_progress)
{
    demucscpp::detail::segment_call(model, buffers.segment_samples, buffers.mix.data(), buffers.targets_out.data(), cb, current_progress,
                                    segment_progress);
}
#endif
} // namespace demucscpp_v3
