// codec_api.cpp — the codecs as entry points of their own: PCM / remix encoding (pcm.hip), FLAC output (flac.hip) and
// FLAC input (flac_in.hip) on buffers the caller names, on the device or, through a scratch copy, on the host.
#include "api_internal.h"

#include <climits>
#include <cmath>

using namespace dmx;

extern "C" int dmx_pcm_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                     const dmx_output_spec *spec, void *d_out, float *d_peaks, void *stream)
{
    const char *fn = "dmx_pcm_encode_device";
    if (n_sources < 1 || n_sources > 64)
        return fail(DMX_ERR_ARG, "%s: n_sources %d", fn, n_sources);
    DMXCHK(dmx_pcm_check_spec(fn, spec, n_sources));
    if (!d_planes || !d_out || !d_peaks)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_planes ? "d_planes" : !d_out ? "d_out" : "d_peaks");
    if (n < 1 || plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (1 <= n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    if (((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_planes & 3) != 0 || ((uintptr_t)d_peaks & 3) != 0)
        return fail(DMX_ERR_ARG, "%s: d_out must be 16-byte aligned, d_planes and d_peaks 4-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const int nOut = spec->stem < 0 ? n_sources : 2;
    HIPCHK(hipMemsetAsync(d_peaks, 0, sizeof(float) * (size_t)nOut, s));
    const PcmPiece pp{d_planes, (unsigned char *)d_out, (unsigned *)d_peaks, n, plane_stride,
                      DMX_OUTPUT_STRIDE(n * dmx_pcm_frame_bytes(spec->encoding)), 0, n};
    launch_pcm_peak(&pp, 1, n_sources, spec->stem, s);
    launch_pcm_encode(&pp, 1, n_sources, spec->stem, spec->encoding, spec->clip, s);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

// the end of dmx_pcm_encode and dmx_remix_encode: wait for the kernels, then the nOut outputs and the peaks leave
static int pcm_download(const char *fn, void *out, float *peaks, const unsigned char *dOut, const float *dPeaks, int nOut, i64 bytes,
                        i64 devStride)
{
    if (hipDeviceSynchronize() != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    for (int o = 0; o < nOut; ++o)
        if (hipMemcpy((unsigned char *)out + (size_t)(o * bytes), dOut + (size_t)(o * devStride), (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(DMX_ERR_HIP, "%s: download failed", fn);
    if (peaks && hipMemcpy(peaks, dPeaks, sizeof(float) * (size_t)nOut, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: download failed", fn);
    return DMX_OK;
}

extern "C" int dmx_pcm_encode(int device, const float *planes, int n_sources, int64_t n, const dmx_output_spec *spec, void *out,
                              float *peaks)
{
    const char *fn = "dmx_pcm_encode";
    if (n_sources < 1 || n_sources > 64)
        return fail(DMX_ERR_ARG, "%s: n_sources %d", fn, n_sources);
    DMXCHK(dmx_pcm_check_spec(fn, spec, n_sources));
    if (!planes || !out || n < 1)
        return fail(DMX_ERR_ARG, "%s: invalid argument (null pointer or n < 1)", fn);
    HIPCHK(hipSetDevice(device));
    const int nOut = spec->stem < 0 ? n_sources : 2;
    const i64 bytes = n * dmx_pcm_frame_bytes(spec->encoding), devStride = DMX_OUTPUT_STRIDE(bytes);
    const size_t inBytes = sizeof(float) * (size_t)n_sources * 2 * (size_t)n;
    DevScratch d;
    float *dIn = (float *)d.get(inBytes);
    unsigned char *dOut = (unsigned char *)d.get((size_t)(nOut * devStride));
    float *dPeaks = (float *)d.get(sizeof(float) * (size_t)nOut);
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (hipMemcpy(dIn, planes, inBytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: upload failed", fn);
    DMXCHK(dmx_pcm_encode_device(device, dIn, n_sources, n, n, spec, dOut, dPeaks, nullptr));
    return pcm_download(fn, out, peaks, dOut, dPeaks, nOut, bytes, devStride);
}

static bool remix_uses_mix(const PcmGains &G)
{
    for (int o = 0; o < G.nOut; ++o)
        if (G.g[o][G.S] != 0.0f)
            return true;
    return false;
}

extern "C" int dmx_remix_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                       const float *d_mix, const dmx_remix_spec *spec, void *d_out, float *d_peaks, void *stream)
{
    const char *fn = "dmx_remix_encode_device";
    PcmGains G;
    DMXCHK(dmx_remix_check_spec(fn, n_sources, spec, &G, false));
    if (!d_planes || !d_out || !d_peaks)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_planes ? "d_planes" : !d_out ? "d_out" : "d_peaks");
    if (!d_mix && remix_uses_mix(G))
        return fail(DMX_ERR_ARG, "%s: null d_mix pointer, and the mixture column of the gains is not all zero", fn);
    if (n < 1 || plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (1 <= n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    if (((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_planes & 3) != 0 || ((uintptr_t)d_peaks & 3) != 0 || ((uintptr_t)d_mix & 3) != 0)
        return fail(DMX_ERR_ARG, "%s: d_out must be 16-byte aligned, d_planes, d_mix and d_peaks 4-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_peaks, 0, sizeof(float) * (size_t)G.nOut, s));
    RemixPiece pp{PcmPiece{d_planes, (unsigned char *)d_out, (unsigned *)d_peaks, n, plane_stride,
                           DMX_OUTPUT_STRIDE(n * dmx_pcm_frame_bytes(spec->encoding)), 0, n},
                  d_mix};
    launch_remix_peak(&pp, 1, G, s);
    launch_remix_encode(&pp, 1, G, spec->encoding, spec->clip, s);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_remix_encode(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                                void *out, float *peaks)
{
    const char *fn = "dmx_remix_encode";
    PcmGains G;
    DMXCHK(dmx_remix_check_spec(fn, n_sources, spec, &G, false));
    if (!planes || !out || n < 1)
        return fail(DMX_ERR_ARG, "%s: invalid argument (null pointer or n < 1)", fn);
    if (!mix && remix_uses_mix(G))
        return fail(DMX_ERR_ARG, "%s: null mix pointer, and the mixture column of the gains is not all zero", fn);
    HIPCHK(hipSetDevice(device));
    const int nOut = G.nOut;
    const i64 bytes = n * dmx_pcm_frame_bytes(spec->encoding), devStride = DMX_OUTPUT_STRIDE(bytes);
    const size_t inBytes = sizeof(float) * (size_t)n_sources * 2 * (size_t)n, mixBytes = sizeof(float) * 2 * (size_t)n;
    DevScratch d;
    float *dIn = (float *)d.get(inBytes);
    unsigned char *dOut = (unsigned char *)d.get((size_t)(nOut * devStride));
    float *dPeaks = (float *)d.get(sizeof(float) * (size_t)nOut);
    float *dMix = mix ? (float *)d.get(mixBytes) : nullptr;
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (hipMemcpy(dIn, planes, inBytes, hipMemcpyHostToDevice) != hipSuccess ||
        (mix && hipMemcpy(dMix, mix, mixBytes, hipMemcpyHostToDevice) != hipSuccess))
        return fail(DMX_ERR_HIP, "%s: upload failed", fn);
    DMXCHK(dmx_remix_encode_device(device, dIn, n_sources, n, n, dMix, spec, dOut, dPeaks, nullptr));
    return pcm_download(fn, out, peaks, dOut, dPeaks, nOut, bytes, devStride);
}

// --------------------------------------------------------------------------- loudness (loudness.hip)
extern "C" int dmx_loudness_coefficients(int rate, double *coef)
{
    if (!coef)
        return fail(DMX_ERR_ARG, "dmx_loudness_coefficients: null coef pointer");
    if (rate < DMX_LOUD_MIN_RATE)
        return fail(DMX_ERR_ARG, "dmx_loudness_coefficients: rate %d is below %d Hz", rate, DMX_LOUD_MIN_RATE);
    loud_coefficients(rate, coef);
    return DMX_OK;
}
extern "C" int dmx_loudness_gain_table(float *table)
{
    if (!table)
        return fail(DMX_ERR_ARG, "dmx_loudness_gain_table: null table pointer");
    loud_gain_table(table);
    return DMX_OK;
}
extern "C" int64_t dmx_loudness_workspace_bytes(int64_t n) { return loud_workspace_bytes(n); }

// the one validator of a loudness spec. limiter: the spec may carry DMX_LOUD_LIMIT or be DMX_LOUD_UNITY (sections 2.16), and
// the limiter's times are checked (lim NULL: the defaults); else the modes of section 2.15 alone, as dmx_loudness_check's
// contract has it
static int loud_check_impl(const char *fn, const dmx_loudness_spec *spec, const dmx_limiter_spec *lim, int rate, int track, bool limiter)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: null loudness spec", fn);
    const int flags = DMX_LOUD_TRUE_PEAK | (limiter ? DMX_LOUD_LIMIT : 0), base = spec->mode & ~flags;
    const bool limit = limiter && spec->mode >= 0 && (spec->mode & DMX_LOUD_LIMIT) != 0;
    const bool okBase = base == DMX_LOUD_MEASURE || base == DMX_LOUD_MIXTURE || base == DMX_LOUD_EACH || (limiter && base == DMX_LOUD_UNITY);
    if (spec->mode < 0 || !okBase || (limit && base == DMX_LOUD_MEASURE) || (!limit && base == DMX_LOUD_UNITY))
        return fail(DMX_ERR_ARG, "%s: loudness spec: mode %d (DMX_LOUD_MEASURE 0, DMX_LOUD_MIXTURE 1, DMX_LOUD_EACH 2, each alone or with DMX_LOUD_TRUE_PEAK 0x100%s)",
                    fn, spec->mode, limiter ? "; DMX_LOUD_LIMIT 0x200 with DMX_LOUD_MIXTURE, DMX_LOUD_EACH or DMX_LOUD_UNITY 3, which needs it" : "");
    if (!std::isfinite(spec->target_lufs) || spec->target_lufs < -70.0f || spec->target_lufs > 0.0f)
        return fail(DMX_ERR_ARG, "%s: loudness spec: target_lufs %g is not in [-70, 0]", fn, (double)spec->target_lufs);
    if (!(spec->max_peak > 0.0f))
        return fail(DMX_ERR_ARG, "%s: loudness spec: max_peak %g is not above 0", fn, (double)spec->max_peak);
    if (limit && !std::isfinite(spec->max_peak))
        return fail(DMX_ERR_ARG, "%s: loudness spec: max_peak %g with DMX_LOUD_LIMIT: the limiter needs a finite ceiling", fn, (double)spec->max_peak);
    if (rate < DMX_LOUD_MIN_RATE && track >= 0)
        return fail(DMX_ERR_ARG, "%s: track %d: loudness: rate %d is below %d Hz", fn, track, rate, DMX_LOUD_MIN_RATE);
    if (rate < DMX_LOUD_MIN_RATE)
        return fail(DMX_ERR_ARG, "%s: loudness: rate %d is below %d Hz", fn, rate, DMX_LOUD_MIN_RATE);
    if (!limiter)
        return DMX_OK;
    const double ms[2] = {lim ? (double)lim->attack_ms : kLimAttackMs, lim ? (double)lim->release_ms : kLimReleaseMs};
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(ms[k]) || ms[k] < kLimMinMs || ms[k] > kLimMaxMs)
            return fail(DMX_ERR_ARG, "%s: limiter spec: %s %g is not in [0.1, 10000]", fn, k ? "release_ms" : "attack_ms", ms[k]);
    return DMX_OK;
}
int dmx_loud_check_spec(const char *fn, const dmx_loudness_spec *spec, int rate, int track)
{
    return loud_check_impl(fn, spec, nullptr, rate, track, false);
}
int dmx_limit_check_spec(const char *fn, const dmx_loudness_spec *spec, const dmx_limiter_spec *lim, int rate, int track)
{
    return loud_check_impl(fn, spec, lim, rate, track, true);
}
static int loud_check(const char *fn, const dmx_loudness_spec *spec, int rate) { return dmx_loud_check_spec(fn, spec, rate, -1); }
extern "C" int dmx_loudness_check(const dmx_loudness_spec *spec, int rate) { return loud_check("dmx_loudness_check", spec, rate); }

// the stage alone has no context to own its tables: one copy per device, made on first use (a blocking upload) and kept for the
// life of the process (the gain table: 48 KB; the limiter's: 34 KB; the track path keeps its own in the context)
namespace
{
struct DeviceTable
{
    size_t words;
    void (*fill)(int32_t *);
    const char *uploadFailed;
    std::mutex mu;
    std::map<int, int32_t *> copies;
    int get(int device, const void **T)
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = copies.find(device);
        if (it == copies.end())
        {
            std::vector<int32_t> h(words, 0);
            fill(h.data());
            int32_t *d = nullptr;
            HIPCHK(hipMalloc(&d, sizeof(int32_t) * words));
            if (hipMemcpy(d, h.data(), sizeof(int32_t) * words, hipMemcpyHostToDevice) != hipSuccess)
            {
                (void)hipFree(d);
                return fail(DMX_ERR_HIP, "%s", uploadFailed);
            }
            it = copies.emplace(device, d).first;
        }
        *T = it->second;
        return DMX_OK;
    }
};
DeviceTable g_loudTable{kLoudGainSteps, [](int32_t *h) { loud_gain_table(reinterpret_cast<float *>(h)); }, "loudness: the gain table's upload failed"};
DeviceTable g_limTables{kLimTableWords,
                        [](int32_t *h) { lim_tables(h, reinterpret_cast<float *>(h + kLimLut), reinterpret_cast<float *>(h + kLimLut + kLimHiPad)); },
                        "limiter: the tables' upload failed"};

// the events of a timed entry point: made by create(), destroyed with the object
template <int N>
struct Events
{
    const char *fn;
    hipEvent_t ev[N] = {};
    explicit Events(const char *f) : fn(f) {}
    Events(const Events &) = delete;
    ~Events()
    {
        for (hipEvent_t e : ev)
            if (e)
                (void)hipEventDestroy(e);
    }
    int create()
    {
        for (hipEvent_t &e : ev)
            if (hipEventCreate(&e) != hipSuccess)
                return fail(DMX_ERR_HIP, "%s: hipEventCreate failed", fn);
        return DMX_OK;
    }
    int elapsed(int i, int j, float *ms) const
    {
        if (hipEventElapsedTime(ms, ev[i], ev[j]) != hipSuccess)
            return fail(DMX_ERR_HIP, "%s: hipEventElapsedTime failed", fn);
        return DMX_OK;
    }
    // the wait of a timed call on its last event
    int wait(int i) const
    {
        if (hipEventSynchronize(ev[i]) != hipSuccess)
            return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return DMX_OK;
    }
};
} // namespace
static int loud_table(int device, const float **T) { return g_loudTable.get(device, reinterpret_cast<const void **>(T)); }
int dmx_limiter_device_tables(int device, const int32_t **T) { return g_limTables.get(device, reinterpret_cast<const void **>(T)); }

// one stereo signal as a one-row gain table: planar through source 0 of one "stem", interleaved through the mixture column
static void loud_signal(const float *d_x, int64_t n, int64_t plane_stride, RemixPiece *pc, PcmGains *G)
{
    *G = PcmGains{};
    G->nOut = 1, G->S = plane_stride ? 1 : 0;
    G->g[0][0] = 1.0f;
    *pc = RemixPiece{PcmPiece{plane_stride ? d_x : nullptr, nullptr, nullptr, n, plane_stride, 0, 0, n}, plane_stride ? nullptr : d_x};
}

// the loudness and the limiter timed calls: `run` enqueues the call with five events around its launches, then one stereo
// sample-peak launch reads the same signal between two more; synchronised. ms[0..4): the call's launches, ms[4]: the peak kernel
template <class Run>
static int timed_beside_peak(const char *fn, int device, const float *d_x, int64_t n, int64_t plane_stride, void *stream, float *ms, Run run)
{
    if (!ms)
        return fail(DMX_ERR_ARG, "%s: null ms pointer", fn);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Events<7> ev(fn);
    DMXCHK(ev.create());
    DevScratch d;
    unsigned *dPeak = (unsigned *)d.get(sizeof(unsigned));
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    DMXCHK(run(fn, ev.ev));
    RemixPiece pc;
    PcmGains G;
    loud_signal(d_x, n, plane_stride, &pc, &G);
    pc.peaks = dPeak;
    (void)hipMemsetAsync(dPeak, 0, sizeof(unsigned), s);
    (void)hipEventRecord(ev.ev[5], s);
    launch_remix_peak(&pc, 1, G, s);
    (void)hipEventRecord(ev.ev[6], s);
    DMXCHK(ev.wait(6));
    for (int i = 0; i < 4; ++i)
        DMXCHK(ev.elapsed(i, i + 1, &ms[i]));
    return ev.elapsed(5, 6, &ms[4]);
}

// marks: null, or five events around the four launches
static int loudness_device(const char *fn, int device, const float *d_x, int64_t n, int64_t plane_stride, int rate,
                           dmx_loudness_result *d_result, double *d_e, void *d_work, void *stream, hipEvent_t *marks)
{
    if (rate < DMX_LOUD_MIN_RATE)
        return fail(DMX_ERR_ARG, "%s: rate %d is below %d Hz", fn, rate, DMX_LOUD_MIN_RATE);
    if (n < 1 || n >= (int64_t)1 << 36 || (plane_stride != 0 && plane_stride < n))
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (1 <= n < 2^36; plane_stride 0 or >= n)", fn, (long long)n,
                    (long long)plane_stride);
    if (!d_x || !d_result || !d_work)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_x ? "d_x" : !d_result ? "d_result" : "d_work");
    if (((uintptr_t)d_x & 3) != 0 || ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_result & 7) != 0 || ((uintptr_t)d_e & 7) != 0)
        return fail(DMX_ERR_ARG, "%s: d_x must be 4-byte aligned, d_work 16-byte aligned, d_result and d_e 8-byte aligned", fn);
    LoudPlan lp;
    if (loud_plan(rate, n, &lp) != 0)
        return fail(DMX_ERR_ARG, "%s: no plan for rate %d, n %lld", fn, rate, (long long)n);
    HIPCHK(hipSetDevice(device));
    RemixPiece pc;
    PcmGains G;
    loud_signal(d_x, n, plane_stride, &pc, &G);
    launch_loud_measure(pc, G, lp, (unsigned char *)d_work, 0, d_e, d_result, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_loudness_device(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, dmx_loudness_result *d_result,
                                   double *d_e, void *d_work, void *stream)
{
    return loudness_device("dmx_loudness_device", device, d_x, n, plane_stride, rate, d_result, d_e, d_work, stream, nullptr);
}

extern "C" int dmx_loudness_device_timed(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate,
                                         dmx_loudness_result *d_result, double *d_e, void *d_work, void *stream, float *ms)
{
    return timed_beside_peak("dmx_loudness_device_timed", device, d_x, n, plane_stride, stream, ms, [&](const char *fn, hipEvent_t *marks) {
        return loudness_device(fn, device, d_x, n, plane_stride, rate, d_result, d_e, d_work, stream, marks);
    });
}

static int meters_device(const char *fn, int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, dmx_loudness_result *d_result,
                         double *d_e, void *d_work, void *stream, dmx_meters_result *d_meters);

// dmx_loudness and, with its entry `meters` on the host, dmx_meters: the upload, the scratch and the download
static int loudness_host(const char *fn, int device, const float *x, int64_t n, int interleaved, int rate, dmx_loudness_result *result, double *e,
                         dmx_meters_result *meters, bool withMeters)
{
    if (rate < DMX_LOUD_MIN_RATE)
        return fail(DMX_ERR_ARG, "%s: rate %d is below %d Hz", fn, rate, DMX_LOUD_MIN_RATE);
    if (!x || !result || (withMeters && !meters) || n < 1 || n >= (int64_t)1 << 36)
        return fail(DMX_ERR_ARG, "%s: invalid argument (null pointer, n < 1 or n >= 2^36)", fn);
    HIPCHK(hipSetDevice(device));
    const size_t inBytes = sizeof(float) * 2 * (size_t)n, eBytes = sizeof(double) * 2 * (size_t)(n / ((rate + 5) / 10));
    DevScratch d;
    float *dX = (float *)d.get(inBytes);
    void *dWork = d.get((size_t)(loud_workspace_bytes(n) + (withMeters ? meters_workspace_bytes(n) : 0)));
    unsigned char *dRes = (unsigned char *)d.get(64); // the loudness result, then the meters
    dmx_meters_result *dMeters = (dmx_meters_result *)(dRes + sizeof(dmx_loudness_result));
    double *dE = e && eBytes ? (double *)d.get(eBytes) : nullptr;
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (hipMemcpy(dX, x, inBytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: upload failed", fn);
    DMXCHK(withMeters ? meters_device(fn, device, dX, n, interleaved ? 0 : n, rate, (dmx_loudness_result *)dRes, dE, dWork, nullptr, dMeters)
                      : loudness_device(fn, device, dX, n, interleaved ? 0 : n, rate, (dmx_loudness_result *)dRes, dE, dWork, nullptr, nullptr));
    if (hipDeviceSynchronize() != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    if (hipMemcpy(result, dRes, sizeof(dmx_loudness_result), hipMemcpyDeviceToHost) != hipSuccess ||
        (withMeters && hipMemcpy(meters, dMeters, sizeof(dmx_meters_result), hipMemcpyDeviceToHost) != hipSuccess) ||
        (dE && hipMemcpy(e, dE, eBytes, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(DMX_ERR_HIP, "%s: download failed", fn);
    return DMX_OK;
}
extern "C" int dmx_loudness(int device, const float *x, int64_t n, int interleaved, int rate, dmx_loudness_result *result, double *e)
{
    return loudness_host("dmx_loudness", device, x, n, interleaved, rate, result, e, nullptr, false);
}

static_assert(kChainMaxOut == PcmGains::kMaxOut && kChainReportBytes == sizeof(dmx_loudness_result) &&
                  kChainReportBytes == sizeof(dmx_meters_result) && kChainLimResBytes >= (int)sizeof(dmx_limit_result),
              "loud_chain.h restates these sizes");

int dmx_loud_chain_enqueue(const LoudChainJob &job, hipStream_t s, LimitPiece *piece)
{
    const RemixPiece &pp = job.pp;
    const PcmGains &G = *job.G;
    const LoudPlan &lp = *job.lp;
    const LoudChain &L = job.L;
    const dmx_loudness_spec &loud = *job.loud;
    const int base = loud.mode & ~(DMX_LOUD_TRUE_PEAK | DMX_LOUD_LIMIT), targetC = (int)rintf(100.0f * loud.target_lufs);
    const bool byTp = (loud.mode & DMX_LOUD_TRUE_PEAK) != 0, limited = (loud.mode & DMX_LOUD_LIMIT) != 0;
    unsigned char *work = job.work;
    float *gains = (float *)(work + L.gains);
    unsigned *tp = (unsigned *)(work + L.truePeaks);
    PcmGains M{}; // the mixture as a one-row table of its own: its slot is the last
    M.nOut = 1, M.S = G.S;
    M.g[0][G.S] = 1.0f;
    launch_loud_measure(pp, G, lp, work, 0, nullptr, nullptr, s);
    launch_loud_measure(pp, M, lp, work, G.nOut, nullptr, nullptr, s);
    TpFilter f;
    if (L.tpWords || limited)
        tp_filter(job.rate, &f);
    if (L.tpWords)
    {
        // the true peaks of the whole track's outputs, and for a meters report the mixture's and the hop meters
        HIPCHK(hipMemsetAsync(tp, 0, sizeof(unsigned) * (size_t)L.tpWords, s));
        RemixPiece tq = pp;
        tq.peaks = tp;
        launch_true_peak(&tq, 1, G, f, s);
        if (job.meters)
        {
            tq.peaks = tp + G.nOut;
            launch_true_peak(&tq, 1, M, f, s);
            launch_meters(work, 0, G.nOut + 1, lp, tp, job.meters, s);
        }
    }
    static_cast<RemixPiece &>(*piece) = pp;
    piece->gains = gains;
    piece->gplane = nullptr, piece->gplaneStride = 0;
    if (!limited)
    {
        if (byTp)
            launch_loud_gain_tp(work, L.slotBytes, G.nOut, pp.peaks, tp, base, targetC, loud.max_peak, job.loudTable, gains, job.report, s);
        else
            launch_loud_gain(work, L.slotBytes, G.nOut, pp.peaks, base, targetC, loud.max_peak, job.loudTable, gains, job.report, s);
        return DMX_OK;
    }
    // the gain without a ceiling (the peaks are zero: nothing to cap, nothing to scale; DMX_LOUD_UNITY: g = 1, as under MEASURE),
    // then the limiter under that gain: its envelopes, the limited peaks in place of the gained ones, and the results
    launch_loud_gain(work, L.slotBytes, G.nOut, pp.peaks, base == DMX_LOUD_UNITY ? DMX_LOUD_MEASURE : base, targetC, INFINITY, job.loudTable, gains,
                     job.report, s);
    LimJob lj{};
    (void)lim_slopes(job.rate, job.lim ? (double)job.lim->attack_ms : kLimAttackMs, job.lim ? (double)job.lim->release_ms : kLimReleaseMs, &lj.qa,
                     &lj.qr);
    dmx_limit_result *limRes = (dmx_limit_result *)(work + L.limRes);
    lj.pc = pp, lj.G = G, lj.gains = gains, lj.gainImm = 1.0f, lj.ceiling = loud.max_peak;
    lj.link = base == DMX_LOUD_MIXTURE, lj.work = work + L.lim, lj.tables = job.limTables, lj.res = limRes;
    launch_limit(lj, f, byTp, s);
    HIPCHK(hipMemcpy2DAsync(pp.peaks, sizeof(float), &limRes->peak_out, sizeof(dmx_limit_result), sizeof(float), (size_t)G.nOut,
                            hipMemcpyDeviceToDevice, s));
    piece->gplane = (const float *)(lj.work + lim_ws_gain_offset(lp.n));
    piece->gplaneStride = lj.link ? 0 : L.envBytes / 4;
    return DMX_OK;
}

// the entry points of this section and of the meters' are the limiter's without its two arguments
static int loud_encode_limit_device(const char *fn, int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                    const float *d_mix, const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out,
                                    float *d_peaks, dmx_loudness_result *d_report, void *d_work, void *stream, dmx_meters_result *d_meters,
                                    const dmx_limiter_spec *lim, dmx_limit_result *d_limit);
static int loud_encode_limit_host(const char *fn, int device, const float *planes, int n_sources, int64_t n, const float *mix,
                                  const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *out, float *peaks,
                                  dmx_loudness_result *report, dmx_meters_result *meters, const dmx_limiter_spec *lim, dmx_limit_result *limit);

extern "C" int dmx_loud_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride, const float *d_mix,
                                      const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out, float *d_peaks,
                                      dmx_loudness_result *d_report, void *d_work, void *stream)
{
    return loud_encode_limit_device("dmx_loud_encode_device", device, d_planes, n_sources, n, plane_stride, d_mix, spec, loud, rate, d_out,
                                    d_peaks, d_report, d_work, stream, nullptr, nullptr, nullptr);
}

extern "C" int dmx_loud_encode_meters_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                             const float *d_mix, const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out,
                                             float *d_peaks, dmx_loudness_result *d_report, void *d_work, void *stream,
                                             dmx_meters_result *d_meters)
{
    const char *fn = "dmx_loud_encode_meters_device";
    if (!d_meters)
        return fail(DMX_ERR_ARG, "%s: null d_meters pointer", fn);
    return loud_encode_limit_device(fn, device, d_planes, n_sources, n, plane_stride, d_mix, spec, loud, rate, d_out, d_peaks, d_report, d_work,
                                    stream, d_meters, nullptr, nullptr);
}

extern "C" int dmx_loud_encode(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                               const dmx_loudness_spec *loud, int rate, void *out, float *peaks, dmx_loudness_result *report)
{
    return loud_encode_limit_host("dmx_loud_encode", device, planes, n_sources, n, mix, spec, loud, rate, out, peaks, report, nullptr, nullptr, nullptr);
}

extern "C" int dmx_loud_encode_meters(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                                      const dmx_loudness_spec *loud, int rate, void *out, float *peaks, dmx_loudness_result *report,
                                      dmx_meters_result *meters)
{
    return loud_encode_limit_host("dmx_loud_encode_meters", device, planes, n_sources, n, mix, spec, loud, rate, out, peaks, report, meters, nullptr,
                                  nullptr);
}

// --------------------------------------------------------------------------- meters (meters.hip)
extern "C" int dmx_true_peak_filter(int rate, int *factor, float *taps)
{
    if (rate < 1)
        return fail(DMX_ERR_ARG, "dmx_true_peak_filter: rate %d", rate);
    if (!factor)
        return fail(DMX_ERR_ARG, "dmx_true_peak_filter: null factor pointer");
    TpFilter f;
    tp_filter(rate, &f);
    *factor = f.F;
    if (taps)
        std::memcpy(taps, f.h, sizeof(float) * (size_t)(kTpTaps * f.F + 1));
    return DMX_OK;
}
extern "C" int64_t dmx_meters_workspace_bytes(int64_t n) { return meters_workspace_bytes(n); }

static int meters_device(const char *fn, int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, dmx_loudness_result *d_result,
                         double *d_e, void *d_work, void *stream, dmx_meters_result *d_meters)
{
    if (!d_meters || ((uintptr_t)d_meters & 3) != 0)
        return fail(DMX_ERR_ARG, "%s: d_meters is null or not 4-byte aligned", fn);
    DMXCHK(loudness_device(fn, device, d_x, n, plane_stride, rate, d_result, d_e, d_work, stream, nullptr));
    LoudPlan lp;
    (void)loud_plan(rate, n, &lp); // checked by the measurement
    hipStream_t s = (hipStream_t)stream;
    unsigned *tp = (unsigned *)((unsigned char *)d_work + loud_workspace_bytes(n));
    RemixPiece pc;
    PcmGains G;
    loud_signal(d_x, n, plane_stride, &pc, &G);
    pc.peaks = tp;
    TpFilter f;
    tp_filter(rate, &f);
    HIPCHK(hipMemsetAsync(tp, 0, sizeof(unsigned), s));
    launch_true_peak(&pc, 1, G, f, s);
    launch_meters((const unsigned char *)d_work, 0, 1, lp, tp, d_meters, s);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_meters_device(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, dmx_loudness_result *d_result,
                                 double *d_e, void *d_work, void *stream, dmx_meters_result *d_meters)
{
    return meters_device("dmx_meters_device", device, d_x, n, plane_stride, rate, d_result, d_e, d_work, stream, d_meters);
}

extern "C" int dmx_meters_device_timed(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, void *d_work, void *stream,
                                       float *ms)
{
    const char *fn = "dmx_meters_device_timed";
    if (!ms)
        return fail(DMX_ERR_ARG, "%s: null ms pointer", fn);
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Events<6> ev(fn);
    DMXCHK(ev.create());
    DevScratch d;
    unsigned char *dSmall = (unsigned char *)d.get(64); // a loudness result, a meters result, a sample peak
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    DMXCHK(loudness_device(fn, device, d_x, n, plane_stride, rate, (dmx_loudness_result *)dSmall, nullptr, d_work, stream, nullptr));
    LoudPlan lp;
    (void)loud_plan(rate, n, &lp);
    unsigned *tp = (unsigned *)((unsigned char *)d_work + loud_workspace_bytes(n));
    RemixPiece pc;
    PcmGains G;
    loud_signal(d_x, n, plane_stride, &pc, &G);
    TpFilter f;
    tp_filter(rate, &f);
    (void)hipMemsetAsync(tp, 0, sizeof(unsigned), s);
    (void)hipMemsetAsync(dSmall + 48, 0, sizeof(unsigned), s);
    pc.peaks = tp;
    (void)hipEventRecord(ev.ev[0], s);
    launch_true_peak(&pc, 1, G, f, s);
    (void)hipEventRecord(ev.ev[1], s);
    pc.peaks = (unsigned *)(dSmall + 48);
    (void)hipEventRecord(ev.ev[2], s);
    launch_remix_peak(&pc, 1, G, s);
    (void)hipEventRecord(ev.ev[3], s);
    (void)hipEventRecord(ev.ev[4], s);
    launch_meters((const unsigned char *)d_work, 0, 1, lp, tp, dSmall + 16, s);
    (void)hipEventRecord(ev.ev[5], s);
    DMXCHK(ev.wait(5));
    for (int i = 0; i < 3; ++i)
        DMXCHK(ev.elapsed(2 * i, 2 * i + 1, &ms[i]));
    return DMX_OK;
}

extern "C" int dmx_meters(int device, const float *x, int64_t n, int interleaved, int rate, dmx_loudness_result *result, double *e,
                          dmx_meters_result *meters)
{
    return loudness_host("dmx_meters", device, x, n, interleaved, rate, result, e, meters, true);
}

// --------------------------------------------------------------------------- limiter (limiter.hip)
extern "C" int dmx_limiter_tables(int32_t *lut, float *thi, float *tlo)
{
    if (!lut || !thi || !tlo)
        return fail(DMX_ERR_ARG, "dmx_limiter_tables: null %s pointer", !lut ? "lut" : !thi ? "thi" : "tlo");
    lim_tables(lut, thi, tlo);
    return DMX_OK;
}
static int limiter_slopes(const char *fn, int rate, double attack_ms, double release_ms, int *qa, int *qr)
{
    if (rate < 1)
        return fail(DMX_ERR_ARG, "%s: limiter spec: rate %d", fn, rate);
    if (!std::isfinite(attack_ms) || attack_ms < kLimMinMs || attack_ms > kLimMaxMs)
        return fail(DMX_ERR_ARG, "%s: limiter spec: attack_ms %g is not in [0.1, 10000]", fn, attack_ms);
    if (!std::isfinite(release_ms) || release_ms < kLimMinMs || release_ms > kLimMaxMs)
        return fail(DMX_ERR_ARG, "%s: limiter spec: release_ms %g is not in [0.1, 10000]", fn, release_ms);
    (void)lim_slopes(rate, attack_ms, release_ms, qa, qr);
    return DMX_OK;
}
extern "C" int dmx_limiter_slopes(int rate, double attack_ms, double release_ms, int32_t *qa, int32_t *qr)
{
    if (!qa || !qr)
        return fail(DMX_ERR_ARG, "dmx_limiter_slopes: null %s pointer", !qa ? "qa" : "qr");
    return limiter_slopes("dmx_limiter_slopes", rate, attack_ms, release_ms, qa, qr);
}
extern "C" int64_t dmx_limiter_workspace_bytes(int64_t n) { return lim_workspace_bytes(n); }

// what the stage refuses before any GPU work, and the slopes
static int limit_check(const char *fn, int rate, float max_peak, const dmx_limiter_spec *lim, int *qa, int *qr)
{
    DMXCHK(limiter_slopes(fn, rate, lim ? (double)lim->attack_ms : kLimAttackMs, lim ? (double)lim->release_ms : kLimReleaseMs, qa, qr));
    if (!(max_peak > 0.0f) || !std::isfinite(max_peak))
        return fail(DMX_ERR_ARG, "%s: max_peak %g is not finite and above 0", fn, (double)max_peak);
    return DMX_OK;
}

// marks: null, or five events around the launches
static int limit_device(const char *fn, int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, float gain, float max_peak,
                        int true_peak, const dmx_limiter_spec *lim, dmx_limit_result *d_result, void *d_work, void *stream, hipEvent_t *marks)
{
    LimJob job{};
    DMXCHK(limit_check(fn, rate, max_peak, lim, &job.qa, &job.qr));
    if (n < 1 || n >= (int64_t)1 << 36 || (plane_stride != 0 && plane_stride < n))
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (1 <= n < 2^36; plane_stride 0 or >= n)", fn, (long long)n,
                    (long long)plane_stride);
    if (!d_x || !d_result || !d_work)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_x ? "d_x" : !d_result ? "d_result" : "d_work");
    if (((uintptr_t)d_x & 3) != 0 || ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_result & 7) != 0)
        return fail(DMX_ERR_ARG, "%s: d_x must be 4-byte aligned, d_work 16-byte aligned, d_result 8-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    DMXCHK(dmx_limiter_device_tables(device, &job.tables));
    loud_signal(d_x, n, plane_stride, &job.pc, &job.G);
    job.gains = nullptr, job.gainImm = gain, job.ceiling = max_peak, job.link = 0;
    job.work = (unsigned char *)d_work, job.res = d_result;
    TpFilter f;
    tp_filter(rate, &f);
    launch_limit(job, f, true_peak != 0, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_limit_device(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, float gain, float max_peak,
                                int true_peak, const dmx_limiter_spec *lim, dmx_limit_result *d_result, void *d_work, void *stream)
{
    return limit_device("dmx_limit_device", device, d_x, n, plane_stride, rate, gain, max_peak, true_peak, lim, d_result, d_work, stream, nullptr);
}

extern "C" int dmx_limit_device_timed(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, float gain, float max_peak,
                                      int true_peak, const dmx_limiter_spec *lim, dmx_limit_result *d_result, void *d_work, void *stream,
                                      float *ms)
{
    return timed_beside_peak("dmx_limit_device_timed", device, d_x, n, plane_stride, stream, ms, [&](const char *fn, hipEvent_t *marks) {
        return limit_device(fn, device, d_x, n, plane_stride, rate, gain, max_peak, true_peak, lim, d_result, d_work, stream, marks);
    });
}

extern "C" int dmx_limit(int device, const float *x, int64_t n, int interleaved, int rate, float gain, float max_peak, int true_peak,
                         const dmx_limiter_spec *lim, int32_t *m, float *gain_plane, dmx_limit_result *result)
{
    const char *fn = "dmx_limit";
    if (!x || !result || n < 1 || n >= (int64_t)1 << 36)
        return fail(DMX_ERR_ARG, "%s: invalid argument (null pointer, n < 1 or n >= 2^36)", fn);
    int qa, qr;
    DMXCHK(limit_check(fn, rate, max_peak, lim, &qa, &qr));
    HIPCHK(hipSetDevice(device));
    const size_t inBytes = sizeof(float) * 2 * (size_t)n;
    DevScratch d;
    float *dX = (float *)d.get(inBytes);
    unsigned char *dWork = (unsigned char *)d.get((size_t)lim_workspace_bytes(n));
    dmx_limit_result *dRes = (dmx_limit_result *)d.get(sizeof(dmx_limit_result));
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (hipMemcpy(dX, x, inBytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: upload failed", fn);
    DMXCHK(limit_device(fn, device, dX, n, interleaved ? 0 : n, rate, gain, max_peak, true_peak, lim, dRes, dWork, nullptr, nullptr));
    if (hipDeviceSynchronize() != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    if (hipMemcpy(result, dRes, sizeof(dmx_limit_result), hipMemcpyDeviceToHost) != hipSuccess ||
        (m && hipMemcpy(m, dWork, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) ||
        (gain_plane && hipMemcpy(gain_plane, dWork + lim_ws_gain_offset(n), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(DMX_ERR_HIP, "%s: download failed", fn);
    return DMX_OK;
}

static int limiter_check(const char *fn, const dmx_loudness_spec *spec, const dmx_limiter_spec *lim, int rate)
{
    return dmx_limit_check_spec(fn, spec, lim, rate, -1);
}
extern "C" int dmx_limiter_check(const dmx_loudness_spec *spec, const dmx_limiter_spec *lim, int rate)
{
    return limiter_check("dmx_limiter_check", spec, lim, rate);
}

static LoudChain stage_layout(int nOut, int64_t n, bool meters, int mode)
{
    return loud_chain_layout(nOut, n, LoudChainMode{meters, (mode & DMX_LOUD_TRUE_PEAK) != 0, (mode & DMX_LOUD_LIMIT) != 0, nOut, false});
}

// d_meters: null (the workspace is the one without meters), or n_out + 1 entries on the device; d_limit: null, or n_out entries
static int loud_encode_limit_device(const char *fn, int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                    const float *d_mix, const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out,
                                    float *d_peaks, dmx_loudness_result *d_report, void *d_work, void *stream, dmx_meters_result *d_meters,
                                    const dmx_limiter_spec *lim, dmx_limit_result *d_limit)
{
    PcmGains G;
    DMXCHK(dmx_remix_check_spec(fn, n_sources, spec, &G, false));
    DMXCHK(limiter_check(fn, loud, lim, rate));
    if (((uintptr_t)d_limit & 7) != 0)
        return fail(DMX_ERR_ARG, "%s: d_limit must be 8-byte aligned", fn);
    if (!d_planes || !d_out || !d_peaks || !d_mix || !d_report || !d_work)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn,
                    !d_planes ? "d_planes" : !d_out ? "d_out" : !d_peaks ? "d_peaks" : !d_mix ? "d_mix" : !d_report ? "d_report" : "d_work");
    if (n < 1 || n >= (int64_t)1 << 36 || plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (1 <= n <= plane_stride, n < 2^36)", fn, (long long)n,
                    (long long)plane_stride);
    if (((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_planes & 3) != 0 || ((uintptr_t)d_peaks & 3) != 0 || ((uintptr_t)d_mix & 3) != 0 ||
        ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_report & 7) != 0 || ((uintptr_t)d_meters & 3) != 0)
        return fail(DMX_ERR_ARG, "%s: d_out and d_work must be 16-byte aligned, d_report 8-byte aligned, d_planes, d_mix, d_peaks and d_meters 4-byte aligned",
                    fn);
    LoudPlan lp;
    if (loud_plan(rate, n, &lp) != 0)
        return fail(DMX_ERR_ARG, "%s: no plan for rate %d, n %lld", fn, rate, (long long)n);
    HIPCHK(hipSetDevice(device));
    const bool limited = (loud->mode & DMX_LOUD_LIMIT) != 0;
    LoudChainJob job{};
    DMXCHK(loud_table(device, &job.loudTable));
    if (limited)
        DMXCHK(dmx_limiter_device_tables(device, &job.limTables));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_peaks, 0, sizeof(float) * (size_t)G.nOut, s));
    job.pp = RemixPiece{PcmPiece{d_planes, (unsigned char *)d_out, (unsigned *)d_peaks, n, plane_stride,
                                 DMX_OUTPUT_STRIDE(n * dmx_pcm_frame_bytes(spec->encoding)), 0, n},
                        d_mix};
    job.G = &G, job.lp = &lp, job.rate = rate, job.loud = loud, job.lim = lim;
    job.work = (unsigned char *)d_work, job.L = stage_layout(G.nOut, n, d_meters != nullptr, loud->mode);
    job.report = d_report, job.meters = d_meters;
    if (!limited) // (the limiter measures the peaks of what it leaves: the peak kernel is not needed)
        launch_remix_peak(&job.pp, 1, G, s);
    LimitPiece piece;
    DMXCHK(dmx_loud_chain_enqueue(job, s, &piece));
    if (limited)
        launch_limit_encode(&piece, 1, G, spec->encoding, spec->clip, s);
    else if ((loud->mode & ~DMX_LOUD_TRUE_PEAK) == DMX_LOUD_MEASURE)
        launch_remix_encode(&piece, 1, G, spec->encoding, spec->clip, s);
    else
        launch_loud_encode(&piece, 1, G, spec->encoding, spec->clip, s);
    if (d_limit && limited)
        HIPCHK(hipMemcpyAsync(d_limit, job.work + job.L.limRes, sizeof(dmx_limit_result) * (size_t)G.nOut, hipMemcpyDeviceToDevice, s));
    else if (d_limit) // a mode without DMX_LOUD_LIMIT: the call as it was, and d_limit zeroed
        HIPCHK(hipMemsetAsync(d_limit, 0, sizeof(dmx_limit_result) * (size_t)G.nOut, s));
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_loud_encode_limit_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                            const float *d_mix, const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out,
                                            float *d_peaks, dmx_loudness_result *d_report, void *d_work, void *stream,
                                            dmx_meters_result *d_meters, const dmx_limiter_spec *lim, dmx_limit_result *d_limit)
{
    return loud_encode_limit_device("dmx_loud_encode_limit_device", device, d_planes, n_sources, n, plane_stride, d_mix, spec, loud, rate, d_out,
                                    d_peaks, d_report, d_work, stream, d_meters, lim, d_limit);
}

extern "C" int dmx_loud_encode_limit(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                                     const dmx_loudness_spec *loud, int rate, void *out, float *peaks, dmx_loudness_result *report,
                                     dmx_meters_result *meters, const dmx_limiter_spec *lim, dmx_limit_result *limit)
{
    return loud_encode_limit_host("dmx_loud_encode_limit", device, planes, n_sources, n, mix, spec, loud, rate, out, peaks, report, meters, lim,
                                  limit);
}

// host buffers: meters NULL or n_out + 1 entries, limit NULL or n_out entries
static int loud_encode_limit_host(const char *fn, int device, const float *planes, int n_sources, int64_t n, const float *mix,
                                  const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *out, float *peaks,
                                  dmx_loudness_result *report, dmx_meters_result *meters, const dmx_limiter_spec *lim, dmx_limit_result *limit)
{
    PcmGains G;
    DMXCHK(dmx_remix_check_spec(fn, n_sources, spec, &G, false));
    DMXCHK(limiter_check(fn, loud, lim, rate));
    if (!planes || !out || !mix || n < 1 || n >= (int64_t)1 << 36)
        return fail(DMX_ERR_ARG, "%s: invalid argument (null planes, mix or out pointer, n < 1 or n >= 2^36)", fn);
    HIPCHK(hipSetDevice(device));
    const int nOut = G.nOut;
    const i64 bytes = n * dmx_pcm_frame_bytes(spec->encoding), devStride = DMX_OUTPUT_STRIDE(bytes);
    const size_t inBytes = sizeof(float) * (size_t)n_sources * 2 * (size_t)n, mixBytes = sizeof(float) * 2 * (size_t)n;
    const size_t workBytes = (size_t)stage_layout(nOut, n, meters != nullptr, loud->mode).total;
    const size_t reportBytes = sizeof(dmx_loudness_result) * (size_t)(nOut + 1), metersBytes = sizeof(dmx_meters_result) * (size_t)(nOut + 1),
                 limitBytes = sizeof(dmx_limit_result) * (size_t)nOut;
    DevScratch d;
    float *dIn = (float *)d.get(inBytes + DMX_OUTPUT_STRIDE(mixBytes)); // the planes, then the mixture
    unsigned char *dOut = (unsigned char *)d.get((size_t)(nOut * devStride));
    unsigned char *dSmall = (unsigned char *)d.get(256 + reportBytes + metersBytes + 16 + limitBytes); // the peaks, the reports
    void *dWork = d.get(workBytes);
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    float *dMix = dIn + (size_t)n_sources * 2 * (size_t)n;
    float *dPeaks = (float *)dSmall;
    dmx_loudness_result *dReport = (dmx_loudness_result *)(dSmall + 256);
    dmx_meters_result *dMeters = meters ? (dmx_meters_result *)(dSmall + 256 + reportBytes) : nullptr;
    dmx_limit_result *dLimit = (dmx_limit_result *)(dSmall + ((256 + reportBytes + metersBytes + 15) & ~(size_t)15));
    if (hipMemcpy(dIn, planes, inBytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dMix, mix, mixBytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: upload failed", fn);
    DMXCHK(loud_encode_limit_device(fn, device, dIn, n_sources, n, n, dMix, spec, loud, rate, dOut, dPeaks, dReport, dWork, nullptr, dMeters, lim,
                                    limit ? dLimit : nullptr));
    DMXCHK(pcm_download(fn, out, peaks, dOut, dPeaks, nOut, bytes, devStride));
    if ((report && hipMemcpy(report, dReport, reportBytes, hipMemcpyDeviceToHost) != hipSuccess) ||
        (meters && hipMemcpy(meters, dMeters, metersBytes, hipMemcpyDeviceToHost) != hipSuccess) ||
        (limit && hipMemcpy(limit, dLimit, limitBytes, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(DMX_ERR_HIP, "%s: download failed", fn);
    return DMX_OK;
}

// --------------------------------------------------------------------------- FLAC output (flac.hip)
extern "C" int64_t dmx_flac_bound(int bits, int64_t n) { return flac_bound(bits, n); }
extern "C" int64_t dmx_flac_workspace_bytes(int bits, int64_t n) { return flac_workspace_bytes(bits, n); }

static int flac_check(const char *fn, int bits, int64_t n, int sample_rate)
{
    if (bits != 16 && bits != 24)
        return fail(DMX_ERR_ARG, "%s: bits %d (16 or 24)", fn, bits);
    if (n < 1 || n >= (int64_t)1 << 36)
        return fail(DMX_ERR_ARG, "%s: n = %lld, must be in [1, 2^36)", fn, (long long)n);
    if (sample_rate < 1 || sample_rate > 655350)
        return fail(DMX_ERR_ARG, "%s: sample_rate %d not in [1, 655350]", fn, sample_rate);
    return DMX_OK;
}

static int flac_level_check(const char *fn, int level)
{
    if (level < 0 || level > 2)
        return fail(DMX_ERR_ARG, "%s: level %d (0, 1 or 2)", fn, level);
    return DMX_OK;
}

// marks: null, or four events recorded around the three launches (dmx_flac_encode_device_timed)
static int flac_encode_device(const char *fn, int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                              int64_t *d_size, void *d_work, void *stream, hipEvent_t *marks)
{
    DMXCHK(flac_check(fn, bits, n, sample_rate));
    DMXCHK(flac_level_check(fn, level));
    if (!d_pcm || !d_out || !d_size || !d_work)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_pcm ? "d_pcm" : !d_out ? "d_out" : !d_size ? "d_size" : "d_work");
    if (((uintptr_t)d_pcm & 15) != 0 || ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_size & 7) != 0)
        return fail(DMX_ERR_ARG, "%s: d_pcm and d_work must be 16-byte aligned, d_size 8-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    launch_flac_encode((const unsigned char *)d_pcm, 0, bits, n, sample_rate, 1, (unsigned char *)d_out, 0, (long long *)d_size,
                       (unsigned char *)d_work, (hipStream_t)stream, level, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_flac_encode_device(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, void *d_out, int64_t *d_size,
                                      void *d_work, void *stream)
{
    return flac_encode_device("dmx_flac_encode_device", device, d_pcm, bits, n, sample_rate, 0, d_out, d_size, d_work, stream, nullptr);
}
extern "C" int dmx_flac_encode_device_level(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                                            int64_t *d_size, void *d_work, void *stream)
{
    return flac_encode_device("dmx_flac_encode_device_level", device, d_pcm, bits, n, sample_rate, level, d_out, d_size, d_work, stream,
                              nullptr);
}
// measurement (tools/flac_bench.py): the call above, synchronised, with the three kernels' times between HIP events in ms[0..3)
extern "C" int dmx_flac_encode_device_timed(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                                            int64_t *d_size, void *d_work, void *stream, float *ms)
{
    const char *fn = "dmx_flac_encode_device_timed";
    if (!ms)
        return fail(DMX_ERR_ARG, "%s: null ms pointer", fn);
    HIPCHK(hipSetDevice(device));
    Events<4> ev(fn);
    DMXCHK(ev.create());
    DMXCHK(flac_encode_device(fn, device, d_pcm, bits, n, sample_rate, level, d_out, d_size, d_work, stream, ev.ev));
    DMXCHK(ev.wait(3));
    for (int i = 0; i < 3; ++i)
        DMXCHK(ev.elapsed(i, i + 1, &ms[i]));
    return DMX_OK;
}

static int flac_encode_host(const char *fn, int device, const void *pcm, int bits, int64_t n, int sample_rate, int level, void *out,
                            int64_t *size)
{
    DMXCHK(flac_check(fn, bits, n, sample_rate));
    DMXCHK(flac_level_check(fn, level));
    if (!pcm || !out || !size)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !pcm ? "pcm" : !out ? "out" : "size");
    HIPCHK(hipSetDevice(device));
    const size_t inBytes = (size_t)n * 2 * (size_t)(bits / 8);
    const i64 bound = flac_bound(bits, n), workBytes = flac_workspace_bytes(bits, n);
    DevScratch d;
    void *dIn = d.get(DMX_OUTPUT_STRIDE(inBytes)), *dOut = d.get((size_t)bound), *dWork = d.get((size_t)workBytes);
    int64_t *dSize = (int64_t *)d.get(sizeof(int64_t));
    int64_t got = 0;
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (hipMemcpy(dIn, pcm, inBytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: upload failed", fn);
    DMXCHK(flac_encode_device(fn, device, dIn, bits, n, sample_rate, level, dOut, dSize, dWork, nullptr, nullptr));
    if (hipDeviceSynchronize() != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    if (hipMemcpy(&got, dSize, sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: download failed", fn);
    if (got < 42 || got > bound)
        return fail(DMX_ERR_HIP, "%s: internal error (%lld encoded bytes, bound %lld)", fn, (long long)got, (long long)bound);
    if (hipMemcpy(out, dOut, (size_t)got, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: download failed", fn);
    *size = got;
    return DMX_OK;
}
extern "C" int dmx_flac_encode(int device, const void *pcm, int bits, int64_t n, int sample_rate, void *out, int64_t *size)
{
    return flac_encode_host("dmx_flac_encode", device, pcm, bits, n, sample_rate, 0, out, size);
}
extern "C" int dmx_flac_encode_level(int device, const void *pcm, int bits, int64_t n, int sample_rate, int level, void *out, int64_t *size)
{
    return flac_encode_host("dmx_flac_encode_level", device, pcm, bits, n, sample_rate, level, out, size);
}

extern "C" int dmx_ctx_set_flac_level(dmx_ctx *c, int level)
{
    if (!c)
        return fail(DMX_ERR_ARG, "dmx_ctx_set_flac_level: null context");
    DMXCHK(flac_level_check("dmx_ctx_set_flac_level", level));
    c->flacLevel = level;
    return DMX_OK;
}
extern "C" int dmx_ctx_flac_level(const dmx_ctx *c) { return c ? c->flacLevel : -1; }

// --------------------------------------------------------------------------- FLAC input (flac_in.hip)
extern "C" int dmx_flac_probe(const void *file, int64_t bytes, dmx_flac_info *info)
{
    if (!file || !info)
        return fail(DMX_ERR_ARG, "dmx_flac_probe: null %s pointer", !file ? "file" : "info");
    char msg[160];
    if (flac_in_probe(file, bytes, info, msg, sizeof msg) != 0)
        return fail(DMX_ERR_FORMAT, "dmx_flac_probe: %s", msg);
    return DMX_OK;
}
extern "C" int64_t dmx_flac_decode_workspace_bytes(const dmx_flac_info *info, int64_t bytes) { return flac_in_workspace_bytes(info, bytes); }

static int flac_in_check(const char *fn, int64_t bytes, const dmx_flac_info *info, int encoding)
{
    if (!info)
        return fail(DMX_ERR_ARG, "%s: null info pointer", fn);
    if (flac_in_workspace_bytes(info, bytes) < 0)
        return fail(DMX_ERR_ARG, "%s: info is not what dmx_flac_probe returns for a file of %lld bytes", fn, (long long)bytes);
    if (info->bits != 8 && info->bits != 12 && info->bits != 16 && info->bits != 20 && info->bits != 24)
        return fail(DMX_ERR_ARG, "%s: %d bits per sample (8, 12, 16, 20 or 24)", fn, info->bits);
    if (encoding != DMX_PCM_F32 && encoding != DMX_PCM_S16 && encoding != DMX_PCM_S24)
        return fail(DMX_ERR_ARG, "%s: encoding %d (DMX_PCM_F32 0, DMX_PCM_S16 1, DMX_PCM_S24 2)", fn, encoding);
    if (encoding != DMX_PCM_F32 && (info->channels != 2 || info->bits != (encoding == DMX_PCM_S16 ? 16 : 24)))
        return fail(DMX_ERR_ARG, "%s: encoding %s needs a stereo stream of exactly that depth (this one: %d channel(s), %d bits)", fn,
                    encoding == DMX_PCM_S16 ? "DMX_PCM_S16" : "DMX_PCM_S24", info->channels, info->bits);
    return DMX_OK;
}

extern "C" int dmx_flac_decode_device(int device, const void *d_file, int64_t bytes, const dmx_flac_info *info, int encoding, void *d_out,
                                      int64_t *d_status, void *d_work, void *stream)
{
    const char *fn = "dmx_flac_decode_device";
    DMXCHK(flac_in_check(fn, bytes, info, encoding));
    if (!d_file || !d_out || !d_status || !d_work)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !d_file ? "d_file" : !d_out ? "d_out" : !d_status ? "d_status" : "d_work");
    if (((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_status & 7) != 0)
        return fail(DMX_ERR_ARG, "%s: d_out and d_work must be 16-byte aligned, d_status 8-byte aligned", fn);
    HIPCHK(hipSetDevice(device));
    if (launch_flac_decode((const unsigned char *)d_file, bytes, info, encoding, d_out, (long long *)d_status, d_work, (hipStream_t)stream) != 0)
        return fail(DMX_ERR_ARG, "%s: info rejected", fn);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_flac_decode(int device, const void *file, int64_t bytes, const dmx_flac_info *info, int encoding, void *out, int64_t *status)
{
    const char *fn = "dmx_flac_decode";
    DMXCHK(flac_in_check(fn, bytes, info, encoding));
    if (!file || !out || !status)
        return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, !file ? "file" : !out ? "out" : "status");
    HIPCHK(hipSetDevice(device));
    const size_t outBytes = (size_t)info->total_samples * (encoding == DMX_PCM_F32 ? 8 : encoding == DMX_PCM_S16 ? 4 : 6);
    const i64 workBytes = flac_in_workspace_bytes(info, bytes);
    DevScratch d;
    void *dIn = d.get((size_t)bytes), *dOut = d.get(DMX_OUTPUT_STRIDE(outBytes)), *dWork = d.get((size_t)workBytes);
    int64_t *dStatus = (int64_t *)d.get(2 * sizeof(int64_t));
    if (!d.ok)
        return fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    if (hipMemcpy(dIn, file, (size_t)bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: upload failed", fn);
    DMXCHK(dmx_flac_decode_device(device, dIn, bytes, info, encoding, dOut, dStatus, dWork, nullptr));
    if (hipDeviceSynchronize() != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    if (hipMemcpy(status, dStatus, 2 * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: download failed", fn);
    return DMX_OK;
}

// measurement aid (tools/flac_in_bench.py): dmx_flac_decode_device with HIP events around each of the five launches;
// ms[0..5): candidates, scan, chain, decode, finish. Synchronises the stream.
extern "C" int dmx_flac_decode_profile(int device, const void *d_file, int64_t bytes, const dmx_flac_info *info, int encoding, void *d_out,
                                       int64_t *d_status, void *d_work, void *stream, float *ms)
{
    const char *fn = "dmx_flac_decode_profile";
    DMXCHK(flac_in_check(fn, bytes, info, encoding));
    if (!d_file || !d_out || !d_status || !d_work || !ms)
        return fail(DMX_ERR_ARG, "%s: null pointer", fn);
    HIPCHK(hipSetDevice(device));
    Events<6> ev(fn);
    DMXCHK(ev.create());
    if (launch_flac_decode((const unsigned char *)d_file, bytes, info, encoding, d_out, (long long *)d_status, d_work, (hipStream_t)stream, ev.ev) != 0)
        return fail(DMX_ERR_ARG, "%s: info rejected", fn);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError()));
    for (int k = 0; k < 5; ++k)
        DMXCHK(ev.elapsed(k, k + 1, &ms[k]));
    return DMX_OK;
}
