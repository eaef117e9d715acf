// analysis_api.cpp — what is computed on finished stems, as entry points of their own: BSS Eval v4 (bss.hip), the Wiener
// post-filter (wiener.hip), the WPE de-reverberation (dereverb.hip), the time stretch and pitch shift (stretch.hip), the
// harmonic/percussive split (hpss.hip), the log-mel features (logmel.hip) and the .npy writer of their results.
#include "api_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

using namespace dmx;

// --------------------------------------------------------------------------- BSS Eval v4 (bss.hip)
static int bss_check(const char *fn, const dmx_bss_spec *spec)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: null spec pointer", fn);
    if (spec->window < 1)
        return fail(DMX_ERR_ARG, "%s: bss spec: window %lld is below 1", fn, (long long)spec->window);
    if (spec->hop < 1)
        return fail(DMX_ERR_ARG, "%s: bss spec: hop %lld is below 1", fn, (long long)spec->hop);
    if (spec->filters_len < 1 || spec->filters_len > kBssMaxFilter)
        return fail(DMX_ERR_ARG, "%s: bss spec: filters_len %d is not in [1, %d]", fn, spec->filters_len, kBssMaxFilter);
    return DMX_OK;
}
extern "C" int dmx_bss_check(const dmx_bss_spec *spec) { return bss_check("dmx_bss_check", spec); }
extern "C" int64_t dmx_bss_windows(int64_t n, int64_t window, int64_t hop) { return bss_windows(n, window, hop); }
extern "C" int64_t dmx_bss_eval_workspace_bytes(int n_sources, int channels, int64_t n, int filters_len)
{
    return bss_workspace_bytes(n_sources, channels, n, filters_len);
}

static int bss_shape(const char *fn, int J, int C, int64_t n, const dmx_bss_spec *spec)
{
    DMXCHK(bss_check(fn, spec));
    if (!bss_shape_ok(J, C, n, spec->filters_len))
        return fail(DMX_ERR_ARG, "%s: n_sources %d, channels %d, n %lld, filters_len %d (1 .. %d sources, 1 | 2 channels, 1 <= n < 2^31, "
                    "n_sources channels filters_len <= %d)", fn, J, C, (long long)n, spec->filters_len, kBssMaxSources, kBssMaxOrder);
    return DMX_OK;
}

// marks: null, or seven events around the six stages
static int bss_device(const char *fn, int device, const float *d_refs, const float *d_ests, int J, int C, int64_t n, int64_t plane_stride,
                      const dmx_bss_spec *spec, double *d_metrics, int *d_status, double *d_filters, void *d_work, void *stream,
                      hipEvent_t *marks)
{
    DMXCHK(bss_shape(fn, J, C, n, spec));
    if (plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    DMXCHK(first_null(fn, {{"d_refs", d_refs}, {"d_ests", d_ests}, {"d_metrics", d_metrics}, {"d_status", d_status}, {"d_work", d_work}}));
    if ((((uintptr_t)d_refs | (uintptr_t)d_ests | (uintptr_t)d_status) & 3) != 0 || (((uintptr_t)d_metrics | (uintptr_t)d_filters) & 7) != 0 ||
        ((uintptr_t)d_work & 255) != 0)
        return fail(DMX_ERR_ARG, "%s: d_refs, d_ests and d_status must be 4-byte aligned, d_metrics and d_filters 8-byte, d_work 256-byte", fn);
    HIPCHK(hipSetDevice(device));
    const BssJob job{d_refs, d_ests, J, C, spec->filters_len, n, plane_stride, spec->window, spec->hop, d_metrics, d_status, d_filters,
                     (unsigned char *)d_work};
    launch_bss(job, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_bss_eval_device(int device, const float *d_refs, const float *d_ests, int n_sources, int channels, int64_t n,
                                   int64_t plane_stride, const dmx_bss_spec *spec, double *d_metrics, int *d_status, double *d_filters,
                                   void *d_work, void *stream)
{
    return bss_device("dmx_bss_eval_device", device, d_refs, d_ests, n_sources, channels, n, plane_stride, spec, d_metrics, d_status, d_filters,
                      d_work, stream, nullptr);
}

extern "C" int dmx_bss_eval_device_timed(int device, const float *d_refs, const float *d_ests, int n_sources, int channels, int64_t n,
                                         int64_t plane_stride, const dmx_bss_spec *spec, double *d_metrics, int *d_status, double *d_filters,
                                         void *d_work, void *stream, float *ms)
{
    const char *fn = "dmx_bss_eval_device_timed";
    float gaps[6];
    DMXCHK(timed_call<7>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        return bss_device(fn, device, d_refs, d_ests, n_sources, channels, n, plane_stride, spec, d_metrics, d_status, d_filters, d_work, stream,
                          marks);
    }));
    std::copy(gaps, gaps + 6, ms);
    return DMX_OK;
}

extern "C" int dmx_bss_eval(int device, const float *refs, const float *ests, int n_sources, int channels, int64_t n, const dmx_bss_spec *spec,
                            double *metrics, int *status, double *filters)
{
    const char *fn = "dmx_bss_eval";
    DMXCHK(bss_shape(fn, n_sources, channels, n, spec));
    DMXCHK(first_null(fn, {{"refs", refs}, {"ests", ests}, {"metrics", metrics}, {"status", status}}));
    HIPCHK(hipSetDevice(device));
    const int M = n_sources * channels;
    const size_t inBytes = sizeof(float) * (size_t)M * (size_t)n;
    const size_t outBytes = sizeof(double) * 4 * (size_t)n_sources * (size_t)bss_windows(n, spec->window, spec->hop);
    const size_t filtBytes = sizeof(double) * (size_t)n_sources * (size_t)M * (size_t)spec->filters_len * (size_t)channels;
    HostTrip t(fn);
    float *dIn;
    unsigned char *dOut; // the metrics, then the status
    double *dFilt = nullptr;
    void *dWork;
    DMXCHK(t.alloc(&dIn, 2 * inBytes));
    DMXCHK(t.alloc(&dOut, outBytes + 256));
    if (filters)
        DMXCHK(t.alloc(&dFilt, filtBytes));
    DMXCHK(t.alloc(&dWork, (size_t)bss_workspace_bytes(n_sources, channels, n, spec->filters_len)));
    int *dStatus = (int *)(dOut + ((outBytes + 255) & ~(size_t)255));
    DMXCHK(t.up(dIn, refs, inBytes));
    DMXCHK(t.up(dIn + (size_t)M * (size_t)n, ests, inBytes));
    DMXCHK(bss_device(fn, device, dIn, dIn + (size_t)M * (size_t)n, n_sources, channels, n, n, spec, (double *)dOut, dStatus, dFilt, dWork, nullptr,
                      nullptr));
    DMXCHK(t.wait());
    DMXCHK(t.down(metrics, dOut, outBytes));
    DMXCHK(t.down(status, dStatus, sizeof(int)));
    if (filters)
        DMXCHK(t.down(filters, dFilt, filtBytes));
    return DMX_OK;
}

// --------------------------------------------------------------------------- Wiener post-filter (wiener.hip)
static int wiener_check(const char *fn, const dmx_wiener_spec *spec, int J, int C, int64_t n)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: null spec pointer", fn);
    if (spec->iterations < 1 || spec->iterations > kWienerMaxIter)
        return fail(DMX_ERR_ARG, "%s: wiener spec: iterations %d is not in [1, %d]", fn, spec->iterations, kWienerMaxIter);
    if (spec->residual != 0 && spec->residual != 1)
        return fail(DMX_ERR_ARG, "%s: wiener spec: residual %d is not 0 or 1", fn, spec->residual);
    if (spec->win_len < 1)
        return fail(DMX_ERR_ARG, "%s: wiener spec: win_len %d is below 1", fn, spec->win_len);
    if (J < 1 || J > kWienerMaxSources)
        return fail(DMX_ERR_ARG, "%s: n_sources %d is not in [1, %d]", fn, J, kWienerMaxSources);
    if (C != 1 && C != 2)
        return fail(DMX_ERR_ARG, "%s: channels %d is not 1 or 2", fn, C);
    if (!wiener_shape_ok(J, C, n))
        return fail(DMX_ERR_ARG, "%s: n %lld is not in (%d, 2^31)", fn, (long long)n, kWienerPad);
    return DMX_OK;
}
extern "C" int dmx_wiener_check(const dmx_wiener_spec *spec, int n_sources, int channels, int64_t n)
{
    return wiener_check("dmx_wiener_check", spec, n_sources, channels, n);
}
extern "C" int64_t dmx_wiener_workspace_bytes(const dmx_wiener_spec *spec, int n_sources, int channels, int64_t n)
{
    if (wiener_check("dmx_wiener_workspace_bytes", spec, n_sources, channels, n) != DMX_OK)
        return -1;
    return wiener_workspace_bytes(n_sources, channels, n, spec->residual);
}

// marks: null, or iterations + 3 events around the stages
static int wiener_device(const char *fn, int device, const float *d_mix, const float *d_ests, int J, int C, int64_t n, int64_t plane_stride,
                         const dmx_wiener_spec *spec, float *d_out, void *d_work, int64_t work_bytes, void *stream, hipEvent_t *marks)
{
    DMXCHK(wiener_check(fn, spec, J, C, n));
    if (plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    DMXCHK(first_null(fn, {{"d_mix", d_mix}, {"d_ests", d_ests}, {"d_out", d_out}, {"d_work", d_work}}));
    if ((((uintptr_t)d_mix | (uintptr_t)d_ests | (uintptr_t)d_out) & 3) != 0 || ((uintptr_t)d_work & 255) != 0)
        return fail(DMX_ERR_ARG, "%s: d_mix, d_ests and d_out must be 4-byte aligned, d_work 256-byte", fn);
    const int64_t need = wiener_workspace_bytes(J, C, n, spec->residual);
    if (work_bytes < need)
        return fail(DMX_ERR_ARG, "%s: work_bytes %lld is below dmx_wiener_workspace_bytes = %lld", fn, (long long)work_bytes, (long long)need);
    HIPCHK(hipSetDevice(device));
    const WienerJob job{d_mix, d_ests, d_out, J, C, spec->iterations, spec->residual, spec->win_len, n, plane_stride, (unsigned char *)d_work};
    launch_wiener(job, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_wiener_device(int device, const float *d_mix, const float *d_ests, int n_sources, int channels, int64_t n,
                                 int64_t plane_stride, const dmx_wiener_spec *spec, float *d_out, void *d_work, int64_t work_bytes, void *stream)
{
    return wiener_device("dmx_wiener_device", device, d_mix, d_ests, n_sources, channels, n, plane_stride, spec, d_out, d_work, work_bytes,
                         stream, nullptr);
}

extern "C" int dmx_wiener_device_timed(int device, const float *d_mix, const float *d_ests, int n_sources, int channels, int64_t n,
                                       int64_t plane_stride, const dmx_wiener_spec *spec, float *d_out, void *d_work, int64_t work_bytes,
                                       void *stream, float *ms)
{
    const char *fn = "dmx_wiener_device_timed";
    float gaps[kWienerMaxIter + 2];
    int stages = 0; // iterations + 2, once wiener_device has checked the spec: the last event recorded, not the array's last
    DMXCHK(timed_call<kWienerMaxIter + 3>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        DMXCHK(wiener_device(fn, device, d_mix, d_ests, n_sources, channels, n, plane_stride, spec, d_out, d_work, work_bytes, stream, marks));
        stages = spec->iterations + 2;
        return DMX_OK;
    }, &stages));
    std::copy(gaps, gaps + stages, ms);
    return DMX_OK;
}

extern "C" int dmx_wiener(int device, const float *mix, const float *ests, int n_sources, int channels, int64_t n, const dmx_wiener_spec *spec,
                          float *out)
{
    const char *fn = "dmx_wiener";
    DMXCHK(wiener_check(fn, spec, n_sources, channels, n));
    DMXCHK(first_null(fn, {{"mix", mix}, {"ests", ests}, {"out", out}}));
    HIPCHK(hipSetDevice(device));
    const size_t plane = sizeof(float) * (size_t)n, M = (size_t)n_sources * (size_t)channels;
    const int64_t workBytes = wiener_workspace_bytes(n_sources, channels, n, spec->residual);
    HostTrip t(fn);
    float *dIn, *dOut;
    void *dWork;
    DMXCHK(t.alloc(&dIn, ((size_t)channels + M) * plane));
    DMXCHK(t.alloc(&dOut, M * plane));
    DMXCHK(t.alloc(&dWork, (size_t)workBytes));
    float *dEsts = dIn + (size_t)channels * (size_t)n;
    DMXCHK(t.up(dIn, mix, (size_t)channels * plane));
    DMXCHK(t.up(dEsts, ests, M * plane));
    DMXCHK(wiener_device(fn, device, dIn, dEsts, n_sources, channels, n, n, spec, dOut, dWork, workBytes, nullptr, nullptr));
    DMXCHK(t.wait());
    return t.down(out, dOut, M * plane);
}

// --------------------------------------------------------------------------- WPE de-reverberation (dereverb.hip)
static int dereverb_check(const char *fn, const dmx_dereverb_spec *spec, int J, int C, int64_t n)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: null spec pointer", fn);
    if (spec->taps < 1 || spec->taps > kDrvMaxTaps)
        return fail(DMX_ERR_ARG, "%s: dereverb spec: taps %d is not in [1, %d]", fn, spec->taps, kDrvMaxTaps);
    if (spec->delay < 1 || spec->delay > kDrvMaxDelay)
        return fail(DMX_ERR_ARG, "%s: dereverb spec: delay %d is not in [1, %d]", fn, spec->delay, kDrvMaxDelay);
    if (spec->iterations < 1 || spec->iterations > kDrvMaxIter)
        return fail(DMX_ERR_ARG, "%s: dereverb spec: iterations %d is not in [1, %d]", fn, spec->iterations, kDrvMaxIter);
    if (!(spec->eps > 0.0 && spec->eps < 1.0))
        return fail(DMX_ERR_ARG, "%s: dereverb spec: eps %g is not in (0, 1)", fn, spec->eps);
    if (!(spec->reg >= 0.0 && spec->reg < 1.0))
        return fail(DMX_ERR_ARG, "%s: dereverb spec: reg %g is not in [0, 1)", fn, spec->reg);
    if (J < 1 || J > kDrvMaxSources)
        return fail(DMX_ERR_ARG, "%s: n_sources %d is not in [1, %d]", fn, J, kDrvMaxSources);
    if (C != 1 && C != 2)
        return fail(DMX_ERR_ARG, "%s: channels %d is not 1 or 2", fn, C);
    if (!dereverb_shape_ok(J, C, n))
        return fail(DMX_ERR_ARG, "%s: n %lld is not in (%d, 2^31)", fn, (long long)n, kWienerPad);
    return DMX_OK;
}
extern "C" int dmx_dereverb_check(const dmx_dereverb_spec *spec, int n_sources, int channels, int64_t n)
{
    return dereverb_check("dmx_dereverb_check", spec, n_sources, channels, n);
}
extern "C" int64_t dmx_dereverb_workspace_bytes(const dmx_dereverb_spec *spec, int n_sources, int channels, int64_t n)
{
    if (dereverb_check("dmx_dereverb_workspace_bytes", spec, n_sources, channels, n) != DMX_OK)
        return -1;
    return dereverb_workspace_bytes(n_sources, channels, n, spec->taps);
}

// marks: null, or iterations + 3 events around the stages
static int dereverb_device(const char *fn, int device, const float *d_stems, int J, int C, int64_t n, int64_t plane_stride,
                           const dmx_dereverb_spec *spec, float *d_out, void *d_work, int64_t work_bytes, void *stream, hipEvent_t *marks)
{
    DMXCHK(dereverb_check(fn, spec, J, C, n));
    if (plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    DMXCHK(first_null(fn, {{"d_stems", d_stems}, {"d_out", d_out}, {"d_work", d_work}}));
    if ((((uintptr_t)d_stems | (uintptr_t)d_out) & 3) != 0 || ((uintptr_t)d_work & 255) != 0)
        return fail(DMX_ERR_ARG, "%s: d_stems and d_out must be 4-byte aligned, d_work 256-byte", fn);
    const int64_t need = dereverb_workspace_bytes(J, C, n, spec->taps);
    if (work_bytes < need)
        return fail(DMX_ERR_ARG, "%s: work_bytes %lld is below dmx_dereverb_workspace_bytes = %lld", fn, (long long)work_bytes, (long long)need);
    HIPCHK(hipSetDevice(device));
    const DereverbJob job{d_stems, d_out, J, C, DrvSpec{spec->taps, spec->delay, spec->iterations, spec->eps, spec->reg}, n, plane_stride,
                          (unsigned char *)d_work};
    launch_dereverb(job, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_dereverb_device(int device, const float *d_stems, int n_sources, int channels, int64_t n, int64_t plane_stride,
                                   const dmx_dereverb_spec *spec, float *d_out, void *d_work, int64_t work_bytes, void *stream)
{
    return dereverb_device("dmx_dereverb_device", device, d_stems, n_sources, channels, n, plane_stride, spec, d_out, d_work, work_bytes, stream,
                           nullptr);
}

extern "C" int dmx_dereverb_device_timed(int device, const float *d_stems, int n_sources, int channels, int64_t n, int64_t plane_stride,
                                         const dmx_dereverb_spec *spec, float *d_out, void *d_work, int64_t work_bytes, void *stream, float *ms)
{
    const char *fn = "dmx_dereverb_device_timed";
    float gaps[kDrvMaxIter + 2];
    int stages = 0; // iterations + 2, once dereverb_device has checked the spec: the last event recorded, not the array's last
    DMXCHK(timed_call<kDrvMaxIter + 3>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        DMXCHK(dereverb_device(fn, device, d_stems, n_sources, channels, n, plane_stride, spec, d_out, d_work, work_bytes, stream, marks));
        stages = spec->iterations + 2;
        return DMX_OK;
    }, &stages));
    std::copy(gaps, gaps + stages, ms);
    return DMX_OK;
}

extern "C" int dmx_dereverb(int device, const float *stems, int n_sources, int channels, int64_t n, const dmx_dereverb_spec *spec, float *out)
{
    const char *fn = "dmx_dereverb";
    DMXCHK(dereverb_check(fn, spec, n_sources, channels, n));
    DMXCHK(first_null(fn, {{"stems", stems}, {"out", out}}));
    HIPCHK(hipSetDevice(device));
    const size_t bytes = sizeof(float) * (size_t)n * (size_t)n_sources * (size_t)channels;
    const int64_t workBytes = dereverb_workspace_bytes(n_sources, channels, n, spec->taps);
    HostTrip t(fn);
    float *dIn, *dOut;
    void *dWork;
    DMXCHK(t.alloc(&dIn, bytes));
    DMXCHK(t.alloc(&dOut, bytes));
    DMXCHK(t.alloc(&dWork, (size_t)workBytes));
    DMXCHK(t.up(dIn, stems, bytes));
    DMXCHK(dereverb_device(fn, device, dIn, n_sources, channels, n, n, spec, dOut, dWork, workBytes, nullptr, nullptr));
    DMXCHK(t.wait());
    return t.down(out, dOut, bytes);
}

// --------------------------------------------------------------------------- time stretch and pitch shift (stretch.hip)
static StretchSpec stretch_spec(const dmx_stretch_spec *s) { return StretchSpec{s->num, s->den, s->pitch_num, s->pitch_den}; }
static int stretch_check(const char *fn, const dmx_stretch_spec *spec, int J, int C, int64_t n)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: null spec pointer", fn);
    const std::pair<const char *, int> terms[] = {{"num", spec->num}, {"den", spec->den}, {"pitch_num", spec->pitch_num}, {"pitch_den", spec->pitch_den}};
    for (const auto &t : terms)
        if (t.second < 1 || t.second > kStretchMaxTerm)
            return fail(DMX_ERR_ARG, "%s: stretch spec: %s %d is not in [1, %d]", fn, t.first, t.second, kStretchMaxTerm);
    const StretchSpec s = stretch_spec(spec);
    if (!stretch_spec_ok(s))
        return fail(DMX_ERR_ARG, "%s: stretch spec: the rate num / den = %d / %d is not in [1/%d, %d]", fn, s.num, s.den, kStretchMaxRate, kStretchMaxRate);
    if (J < 1 || J > kStretchMaxSources)
        return fail(DMX_ERR_ARG, "%s: n_sources %d is not in [1, %d]", fn, J, kStretchMaxSources);
    if (C != 1 && C != 2)
        return fail(DMX_ERR_ARG, "%s: channels %d is not 1 or 2", fn, C);
    if (!wiener_shape_ok(1, C, n))
        return fail(DMX_ERR_ARG, "%s: n %lld is not in (%d, 2^31)", fn, (long long)n, kWienerPad);
    if (!stretch_shape_ok(J, C, n, s))
        return fail(DMX_ERR_ARG, "%s: the stretched length ceil(n den / num) = %lld is not in (%d, 2^31)", fn, (long long)stretch_mid_length(n, s),
                    kWienerPad);
    if (stretch_converts(s) && resample_check(s.pnum, s.pden, J * C) != DMX_OK)
    {
        const std::string why = dmx_err_string(); // the converter's own refusal, passed on
        return fail(DMX_ERR_ARG, "%s: stretch spec: pitch_num / pitch_den = %d / %d: %s", fn, s.pnum, s.pden, why.c_str());
    }
    return DMX_OK;
}
extern "C" int dmx_stretch_check(const dmx_stretch_spec *spec, int n_sources, int channels, int64_t n)
{
    return stretch_check("dmx_stretch_check", spec, n_sources, channels, n);
}
extern "C" int64_t dmx_stretch_length(const dmx_stretch_spec *spec, int64_t n)
{
    if (!spec || !stretch_spec_ok(stretch_spec(spec)) || n < 0 || n >= ((int64_t)1 << 31))
        return -1;
    const int64_t mid = stretch_mid_length(n, stretch_spec(spec));
    return spec->pitch_num == spec->pitch_den ? mid : dmx_resample_length(mid, spec->pitch_num, spec->pitch_den);
}
extern "C" int64_t dmx_stretch_workspace_bytes(const dmx_stretch_spec *spec, int n_sources, int channels, int64_t n)
{
    if (stretch_check("dmx_stretch_workspace_bytes", spec, n_sources, channels, n) != DMX_OK)
        return -1;
    return stretch_workspace_bytes(n_sources, channels, n, stretch_spec(spec));
}

// The fraction nearest to `value` among those with a denominator of at most max_den; of two equally near, the smaller
// denominator. Exact: value = M / 2^k with M below 2^53, so |value - n / d| = |M d - n 2^k| / (d 2^k), and two of them are
// compared by cross-multiplying in 128-bit integers (M d < 2^73; a numerator |M d - n 2^k| <= 2^(k - 1) times d <= 2^20).
extern "C" int dmx_stretch_ratio(double value, int max_den, int *num, int *den)
{
    const char *fn = "dmx_stretch_ratio";
    DMXCHK(first_null(fn, {{"num", num}, {"den", den}}));
    if (!(value >= 1.0 / 1024 && value <= 1024.0))
        return fail(DMX_ERR_ARG, "%s: value %g is not in [1/1024, 1024]", fn, value);
    if (max_den < 1 || max_den > kStretchMaxTerm)
        return fail(DMX_ERR_ARG, "%s: max_den %d is not in [1, %d]", fn, max_den, kStretchMaxTerm);
    typedef unsigned __int128 u128;
    int e = 0;
    const u128 M = (u128)std::ldexp(std::frexp(value, &e), 53); // value = M 2^(e - 53), an integer below 2^53
    const int k = 53 - e;                                      // 42 .. 62
    u128 bestErr = 0;
    int64_t bestN = 0, bestD = 0;
    for (int64_t d = 1; d <= max_den; ++d)
    {
        const u128 Md = M * (u128)d;
        u128 n = (Md + ((u128)1 << (k - 1))) >> k; // the integer nearest to value d, at least 1
        if (n == 0)
            n = 1;
        const u128 err = Md > (n << k) ? Md - (n << k) : (n << k) - Md;
        if (bestD == 0 || err * (u128)bestD < bestErr * (u128)d) // err / d < bestErr / bestD: strictly nearer only
            bestErr = err, bestN = (int64_t)n, bestD = d;
    }
    *num = (int)bestN, *den = (int)bestD;
    return DMX_OK;
}

// marks: null, or 5 events around the stages. *stages, where given: the index of the last event recorded
static int stretch_device(const char *fn, int device, const float *d_stems, int J, int C, int64_t n, int64_t plane_stride,
                          const dmx_stretch_spec *spec, float *d_out, int64_t out_stride, void *d_work, int64_t work_bytes, void *stream,
                          hipEvent_t *marks, int *stages = nullptr)
{
    DMXCHK(stretch_check(fn, spec, J, C, n));
    const int64_t nOut = dmx_stretch_length(spec, n);
    if (plane_stride < n || out_stride < nOut)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld, dmx_stretch_length = %lld, out_stride = %lld (n <= plane_stride, "
                    "the length <= out_stride)", fn, (long long)n, (long long)plane_stride, (long long)nOut, (long long)out_stride);
    DMXCHK(first_null(fn, {{"d_stems", d_stems}, {"d_out", d_out}, {"d_work", d_work}}));
    if ((((uintptr_t)d_stems | (uintptr_t)d_out) & 3) != 0 || ((uintptr_t)d_work & 255) != 0)
        return fail(DMX_ERR_ARG, "%s: d_stems and d_out must be 4-byte aligned, d_work 256-byte", fn);
    const StretchSpec s = stretch_spec(spec);
    const int64_t need = stretch_workspace_bytes(J, C, n, s);
    if (work_bytes < need)
        return fail(DMX_ERR_ARG, "%s: work_bytes %lld is below dmx_stretch_workspace_bytes = %lld", fn, (long long)work_bytes, (long long)need);
    HIPCHK(hipSetDevice(device));
    if (stretch_converts(s)) // the filter's upload blocks: ahead of the launches
        DMXCHK(resample_prepare(device, s.pnum, s.pden));
    const StretchJob job{d_stems, d_out, J, C, s, n, plane_stride, out_stride, (unsigned char *)d_work};
    launch_stretch(job, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    if (stages)
        *stages = 3;
    if (!stretch_converts(s))
        return DMX_OK;
    const StretchLayout l = stretch_layout(J, C, n, s);
    DMXCHK(dmx_resample_device(device, (const float *)((unsigned char *)d_work + l.tmp), l.n2, J * C, l.mid, 1, s.pnum, s.pden, d_out, out_stride,
                               1, stream));
    if (marks)
        HIPCHK(hipEventRecord(marks[4], (hipStream_t)stream));
    if (stages)
        *stages = 4;
    return DMX_OK;
}

extern "C" int dmx_stretch_device(int device, const float *d_stems, int n_sources, int channels, int64_t n, int64_t plane_stride,
                                  const dmx_stretch_spec *spec, float *d_out, int64_t out_stride, void *d_work, int64_t work_bytes, void *stream)
{
    return stretch_device("dmx_stretch_device", device, d_stems, n_sources, channels, n, plane_stride, spec, d_out, out_stride, d_work, work_bytes,
                          stream, nullptr);
}

extern "C" int dmx_stretch_device_timed(int device, const float *d_stems, int n_sources, int channels, int64_t n, int64_t plane_stride,
                                        const dmx_stretch_spec *spec, float *d_out, int64_t out_stride, void *d_work, int64_t work_bytes,
                                        void *stream, float *ms)
{
    const char *fn = "dmx_stretch_device_timed";
    float gaps[4] = {0.f, 0.f, 0.f, 0.f}; // the converter's entry stays 0 where there is none
    int stages = 0;
    DMXCHK(timed_call<5>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        return stretch_device(fn, device, d_stems, n_sources, channels, n, plane_stride, spec, d_out, out_stride, d_work, work_bytes, stream, marks,
                              &stages);
    }, &stages));
    std::copy(gaps, gaps + 4, ms);
    return DMX_OK;
}

extern "C" int dmx_stretch(int device, const float *stems, int n_sources, int channels, int64_t n, const dmx_stretch_spec *spec, float *out)
{
    const char *fn = "dmx_stretch";
    DMXCHK(stretch_check(fn, spec, n_sources, channels, n));
    DMXCHK(first_null(fn, {{"stems", stems}, {"out", out}}));
    HIPCHK(hipSetDevice(device));
    const size_t planes = (size_t)n_sources * (size_t)channels;
    const int64_t nOut = dmx_stretch_length(spec, n), workBytes = stretch_workspace_bytes(n_sources, channels, n, stretch_spec(spec));
    HostTrip t(fn);
    float *dIn, *dOut;
    void *dWork;
    DMXCHK(t.alloc(&dIn, sizeof(float) * planes * (size_t)n));
    DMXCHK(t.alloc(&dOut, sizeof(float) * planes * (size_t)nOut));
    DMXCHK(t.alloc(&dWork, (size_t)workBytes));
    DMXCHK(t.up(dIn, stems, sizeof(float) * planes * (size_t)n));
    DMXCHK(stretch_device(fn, device, dIn, n_sources, channels, n, n, spec, dOut, nOut, dWork, workBytes, nullptr, nullptr));
    DMXCHK(t.wait());
    return t.down(out, dOut, sizeof(float) * planes * (size_t)nOut);
}

// --------------------------------------------------------------------------- harmonic/percussive split (hpss.hip)
static HpssSpec hpss_spec(const dmx_hpss_spec *s) { return HpssSpec{s->kernel_h, s->kernel_p, s->power, s->residual, s->margin_h, s->margin_p}; }
static int hpss_spec_check(const char *fn, const dmx_hpss_spec *spec)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: null spec pointer", fn);
    const std::pair<const char *, int> windows[] = {{"kernel_h", spec->kernel_h}, {"kernel_p", spec->kernel_p}};
    for (const auto &w : windows)
        if (!hpss_kernel_ok(w.second))
            return fail(DMX_ERR_ARG, "%s: hpss spec: %s %d is not odd and in [3, %d]", fn, w.first, w.second, kHpssMaxKernel);
    if (spec->power < 1 || spec->power > kHpssMaxPower)
        return fail(DMX_ERR_ARG, "%s: hpss spec: power %d is not in [1, %d]", fn, spec->power, kHpssMaxPower);
    const std::pair<const char *, double> margins[] = {{"margin_h", spec->margin_h}, {"margin_p", spec->margin_p}};
    for (const auto &m : margins)
        if (!hpss_margin_ok(m.second))
            return fail(DMX_ERR_ARG, "%s: hpss spec: %s %g is not in [1, %g]", fn, m.first, m.second, kHpssMaxMargin);
    if (spec->residual != 0 && spec->residual != 1)
        return fail(DMX_ERR_ARG, "%s: hpss spec: residual %d is not 0 or 1", fn, spec->residual);
    return DMX_OK;
}
static int hpss_check(const char *fn, const dmx_hpss_spec *spec, int J, int C, int64_t n)
{
    DMXCHK(hpss_spec_check(fn, spec));
    if (J < 1 || J > kHpssMaxSources)
        return fail(DMX_ERR_ARG, "%s: n_sources %d is not in [1, %d]", fn, J, kHpssMaxSources);
    if (C != 1 && C != 2)
        return fail(DMX_ERR_ARG, "%s: channels %d is not 1 or 2", fn, C);
    if (!hpss_shape_ok(J, C, n))
        return fail(DMX_ERR_ARG, "%s: n %lld is not in (%d, 2^31)", fn, (long long)n, kWienerPad);
    return DMX_OK;
}
extern "C" int dmx_hpss_check(const dmx_hpss_spec *spec, int n_sources, int channels, int64_t n)
{
    return hpss_check("dmx_hpss_check", spec, n_sources, channels, n);
}
extern "C" int64_t dmx_hpss_workspace_bytes(const dmx_hpss_spec *spec, int n_sources, int channels, int64_t n)
{
    if (hpss_check("dmx_hpss_workspace_bytes", spec, n_sources, channels, n) != DMX_OK)
        return -1;
    return hpss_workspace_bytes(n_sources, channels, n);
}
extern "C" int dmx_hpss_geometry(int *tile_frames, int *tile_bins)
{
    DMXCHK(first_null("dmx_hpss_geometry", {{"tile_frames", tile_frames}, {"tile_bins", tile_bins}}));
    *tile_frames = kHpssTileFrames, *tile_bins = kHpssTileBins;
    return DMX_OK;
}

extern "C" int dmx_hpss_filter_device(int device, const void *d_spec, int planes, int frames, int bins, int row, const dmx_hpss_spec *spec,
                                      int what, float *d_a, float *d_b, void *stream)
{
    const char *fn = "dmx_hpss_filter_device";
    DMXCHK(hpss_spec_check(fn, spec));
    if (!hpss_filter_shape_ok(planes, frames, bins, row))
        return fail(DMX_ERR_ARG, "%s: planes = %d, frames = %d, bins = %d, row = %d (1 <= planes <= %d, 1 <= frames <= %d, 1 <= bins <= row <= %d)",
                    fn, planes, frames, bins, row, kHpssMaxPlanes, kHpssMaxFrames, kHpssMaxRow);
    if (what != DMX_HPSS_MASKS && what != DMX_HPSS_MEDIANS)
        return fail(DMX_ERR_ARG, "%s: what %d is not DMX_HPSS_MASKS or DMX_HPSS_MEDIANS", fn, what);
    DMXCHK(first_null(fn, {{"d_spec", d_spec}, {"d_a", d_a}, {"d_b", d_b}}));
    if (((uintptr_t)d_spec & 7) != 0 || (((uintptr_t)d_a | (uintptr_t)d_b) & 3) != 0)
        return fail(DMX_ERR_ARG, "%s: d_spec must be 8-byte aligned, d_a and d_b 4-byte", fn);
    HIPCHK(hipSetDevice(device));
    launch_hpss_filter((const float2 *)d_spec, planes, frames, bins, row, hpss_spec(spec), what, d_a, d_b, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

// marks: null, or 4 events around the stages
static int hpss_device(const char *fn, int device, const float *d_stems, int J, int C, int64_t n, int64_t plane_stride, const dmx_hpss_spec *spec,
                       float *d_out, int64_t out_stride, void *d_work, int64_t work_bytes, void *stream, hipEvent_t *marks)
{
    DMXCHK(hpss_check(fn, spec, J, C, n));
    if (plane_stride < n || out_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld, out_stride = %lld (n <= plane_stride, n <= out_stride)", fn, (long long)n,
                    (long long)plane_stride, (long long)out_stride);
    DMXCHK(first_null(fn, {{"d_stems", d_stems}, {"d_out", d_out}, {"d_work", d_work}}));
    if ((((uintptr_t)d_stems | (uintptr_t)d_out) & 3) != 0 || ((uintptr_t)d_work & 255) != 0)
        return fail(DMX_ERR_ARG, "%s: d_stems and d_out must be 4-byte aligned, d_work 256-byte", fn);
    const int64_t need = hpss_workspace_bytes(J, C, n);
    if (work_bytes < need)
        return fail(DMX_ERR_ARG, "%s: work_bytes %lld is below dmx_hpss_workspace_bytes = %lld", fn, (long long)work_bytes, (long long)need);
    HIPCHK(hipSetDevice(device));
    const HpssJob job{d_stems, d_out, J, C, hpss_spec(spec), n, plane_stride, out_stride, (unsigned char *)d_work};
    launch_hpss(job, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_hpss_device(int device, const float *d_stems, int n_sources, int channels, int64_t n, int64_t plane_stride,
                               const dmx_hpss_spec *spec, float *d_out, int64_t out_stride, void *d_work, int64_t work_bytes, void *stream)
{
    return hpss_device("dmx_hpss_device", device, d_stems, n_sources, channels, n, plane_stride, spec, d_out, out_stride, d_work, work_bytes, stream,
                       nullptr);
}

extern "C" int dmx_hpss_device_timed(int device, const float *d_stems, int n_sources, int channels, int64_t n, int64_t plane_stride,
                                     const dmx_hpss_spec *spec, float *d_out, int64_t out_stride, void *d_work, int64_t work_bytes, void *stream,
                                     float *ms)
{
    const char *fn = "dmx_hpss_device_timed";
    float gaps[3];
    DMXCHK(timed_call<4>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        return hpss_device(fn, device, d_stems, n_sources, channels, n, plane_stride, spec, d_out, out_stride, d_work, work_bytes, stream, marks);
    }));
    std::copy(gaps, gaps + 3, ms);
    return DMX_OK;
}

extern "C" int dmx_hpss(int device, const float *stems, int n_sources, int channels, int64_t n, const dmx_hpss_spec *spec, float *out)
{
    const char *fn = "dmx_hpss";
    DMXCHK(hpss_check(fn, spec, n_sources, channels, n));
    DMXCHK(first_null(fn, {{"stems", stems}, {"out", out}}));
    HIPCHK(hipSetDevice(device));
    const size_t planes = (size_t)n_sources * (size_t)channels, kinds = (size_t)(2 + spec->residual);
    const int64_t workBytes = hpss_workspace_bytes(n_sources, channels, n);
    HostTrip t(fn);
    float *dIn, *dOut;
    void *dWork;
    DMXCHK(t.alloc(&dIn, sizeof(float) * planes * (size_t)n));
    DMXCHK(t.alloc(&dOut, sizeof(float) * planes * kinds * (size_t)n));
    DMXCHK(t.alloc(&dWork, (size_t)workBytes));
    DMXCHK(t.up(dIn, stems, sizeof(float) * planes * (size_t)n));
    DMXCHK(hpss_device(fn, device, dIn, n_sources, channels, n, n, spec, dOut, n, dWork, workBytes, nullptr, nullptr));
    DMXCHK(t.wait());
    return t.down(out, dOut, sizeof(float) * planes * kinds * (size_t)n);
}

// --------------------------------------------------------------------------- log-mel features (logmel.hip)
static LogmelSpec logmel_spec(const dmx_logmel_spec *s)
{
    return LogmelSpec{s->sr, s->n_fft, s->hop, s->n_mels, s->fmin, s->fmax, s->mel_scale, s->mel_norm, s->log_mode, s->chunk_frames,
                      s->amin, s->top_db};
}
// n < 0: the spec alone
static int logmel_check(const char *fn, const dmx_logmel_spec *spec, int64_t n)
{
    if (!spec)
        return fail(DMX_ERR_ARG, "%s: null spec pointer", fn);
    const LogmelSpec s = logmel_spec(spec);
    if (const char *why = logmel_spec_error(s))
        return fail(DMX_ERR_ARG, "%s: logmel spec: %s", fn, why);
    if (n >= 0 && !logmel_length_ok(s, n))
        return fail(DMX_ERR_ARG, "%s: n %lld is not in (%d, 2^31)", fn, (long long)n, s.chunk_frames > 0 ? 0 : s.n_fft / 2);
    if (n >= 0 && logmel_frames(s, n).chunks > 65535)
        return fail(DMX_ERR_ARG, "%s: n %lld gives more than 65535 chunks", fn, (long long)n);
    return DMX_OK;
}
extern "C" int dmx_logmel_check(const dmx_logmel_spec *spec, int64_t n) { return logmel_check("dmx_logmel_check", spec, n); }

extern "C" int dmx_logmel_preset(const char *name, dmx_logmel_spec *spec)
{
    if (!name || !spec)
        return fail(DMX_ERR_ARG, "dmx_logmel_preset: null %s pointer", !name ? "name" : "spec");
    const std::string p = name;
    if (p == "whisper" || p == "whisper128")
        *spec = dmx_logmel_spec{16000, 400, 160, p == "whisper" ? 80 : 128, 0.0, 8000.0, DMX_MEL_SLANEY, DMX_MEL_NORM_SLANEY, DMX_LOG_WHISPER,
                                3000, 1e-10, 0.0};
    else if (p == "librosa")
        *spec = dmx_logmel_spec{22050, 2048, 512, 128, 0.0, 11025.0, DMX_MEL_SLANEY, DMX_MEL_NORM_SLANEY, DMX_LOG_DB, 0, 1e-10, 80.0};
    else
        return fail(DMX_ERR_ARG, "dmx_logmel_preset: name \"%s\" is not whisper, whisper128 or librosa", name);
    return DMX_OK;
}

extern "C" int dmx_logmel_frames(const dmx_logmel_spec *spec, int64_t n, int64_t *chunks, int64_t *frames)
{
    if (!chunks || !frames)
        return fail(DMX_ERR_ARG, "dmx_logmel_frames: null %s pointer", !chunks ? "chunks" : "frames");
    DMXCHK(logmel_check("dmx_logmel_frames", spec, n < 0 ? 0 : n));
    const LogmelFrames fr = logmel_frames(logmel_spec(spec), n);
    *chunks = fr.chunks, *frames = fr.frames;
    return DMX_OK;
}

extern "C" int dmx_logmel_filters(const dmx_logmel_spec *spec, double *W)
{
    if (!W)
        return fail(DMX_ERR_ARG, "dmx_logmel_filters: null W pointer");
    DMXCHK(logmel_check("dmx_logmel_filters", spec, -1));
    logmel_filters(logmel_spec(spec), W);
    return DMX_OK;
}

extern "C" int dmx_logmel_geometry(const dmx_logmel_spec *spec, int *tile_frames, int *slab_depth, int64_t *lds_bytes)
{
    if (!tile_frames || !slab_depth || !lds_bytes)
        return fail(DMX_ERR_ARG, "dmx_logmel_geometry: null output pointer");
    DMXCHK(logmel_check("dmx_logmel_geometry", spec, -1));
    const LogmelTile t = logmel_tile(spec->n_fft, spec->hop);
    *tile_frames = t.ft, *slab_depth = t.K, *lds_bytes = t.ldsBytes;
    return DMX_OK;
}

extern "C" int64_t dmx_logmel_workspace_bytes(const dmx_logmel_spec *spec, int planes, int64_t n)
{
    const char *fn = "dmx_logmel_workspace_bytes";
    if (logmel_check(fn, spec, n < 0 ? 0 : n) != DMX_OK)
        return -1;
    if (planes < 1 || planes > 65535)
        return fail(DMX_ERR_ARG, "%s: planes %d is not in [1, 65535]", fn, planes), -1;
    return logmel_layout(logmel_spec(spec), planes, n).bytes;
}

// the host-made tables of a spec (logmel_host_tables), made once per process and kept: the copy a launch enqueues may read them
// after the call has returned
static const unsigned char *logmel_tables(const LogmelSpec &s)
{
    static std::mutex mu;
    static std::map<std::string, std::vector<unsigned char>> made;
    const std::string key((const char *)&s, sizeof(s));
    std::lock_guard<std::mutex> lock(mu);
    std::vector<unsigned char> &h = made[key];
    if (h.empty())
    {
        const LogmelLayout l = logmel_layout(s, 1, s.n_fft);
        h.resize((size_t)l.hostBytes);
        logmel_host_tables(s, l, h.data());
    }
    return h.data();
}

// marks: null, or 4 events around the stages
static int logmel_device(const char *fn, int device, const float *d_planes, int planes, int64_t n, int64_t plane_stride,
                         const dmx_logmel_spec *spec, float *d_out, void *d_work, int64_t work_bytes, void *stream, hipEvent_t *marks)
{
    DMXCHK(logmel_check(fn, spec, n < 0 ? 0 : n));
    if (planes < 1 || planes > 65535)
        return fail(DMX_ERR_ARG, "%s: planes %d is not in [1, 65535]", fn, planes);
    if (plane_stride < n)
        return fail(DMX_ERR_ARG, "%s: n = %lld, plane_stride = %lld (n <= plane_stride)", fn, (long long)n, (long long)plane_stride);
    DMXCHK(first_null(fn, {{"d_planes", d_planes}, {"d_out", d_out}, {"d_work", d_work}}));
    if ((((uintptr_t)d_planes | (uintptr_t)d_out) & 3) != 0 || ((uintptr_t)d_work & 255) != 0)
        return fail(DMX_ERR_ARG, "%s: d_planes and d_out must be 4-byte aligned, d_work 256-byte", fn);
    LogmelSpec s = logmel_spec(spec);
    if (s.log_mode != DMX_LOG_DB) // the fields the mode does not read take no part in the tables' key
        s.amin = 0.0, s.top_db = 0.0;
    const int64_t need = logmel_layout(s, planes, n).bytes;
    if (work_bytes < need)
        return fail(DMX_ERR_ARG, "%s: work_bytes %lld is below dmx_logmel_workspace_bytes = %lld", fn, (long long)work_bytes, (long long)need);
    HIPCHK(hipSetDevice(device));
    const LogmelJob job{d_planes, d_out, planes, n, plane_stride, s, (unsigned char *)d_work, logmel_tables(s)};
    launch_logmel(job, (hipStream_t)stream, marks);
    HIPCHK(hipGetLastError());
    return DMX_OK;
}

extern "C" int dmx_logmel_device(int device, const float *d_planes, int planes, int64_t n, int64_t plane_stride, const dmx_logmel_spec *spec,
                                 float *d_out, void *d_work, int64_t work_bytes, void *stream)
{
    return logmel_device("dmx_logmel_device", device, d_planes, planes, n, plane_stride, spec, d_out, d_work, work_bytes, stream, nullptr);
}

extern "C" int dmx_logmel_device_timed(int device, const float *d_planes, int planes, int64_t n, int64_t plane_stride,
                                       const dmx_logmel_spec *spec, float *d_out, void *d_work, int64_t work_bytes, void *stream, float *ms)
{
    const char *fn = "dmx_logmel_device_timed";
    float gaps[3];
    DMXCHK(timed_call<4>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        return logmel_device(fn, device, d_planes, planes, n, plane_stride, spec, d_out, d_work, work_bytes, stream, marks);
    }));
    std::copy(gaps, gaps + 3, ms);
    return DMX_OK;
}

// planes on the device (dIn, stride n, in the scratch of t) -> out on the host
static int logmel_to_host(const char *fn, int device, const float *dIn, int planes, int64_t n, const dmx_logmel_spec *spec, HostTrip &t,
                          float *out)
{
    const LogmelFrames fr = logmel_frames(logmel_spec(spec), n);
    const size_t outBytes = sizeof(float) * (size_t)planes * (size_t)(fr.chunks * spec->n_mels * fr.frames);
    const int64_t workBytes = dmx_logmel_workspace_bytes(spec, planes, n);
    if (workBytes < 0)
        return DMX_ERR_ARG;
    float *dOut;
    void *dWork;
    DMXCHK(t.alloc(&dOut, outBytes));
    DMXCHK(t.alloc(&dWork, (size_t)workBytes));
    DMXCHK(logmel_device(fn, device, dIn, planes, n, n, spec, dOut, dWork, workBytes, nullptr, nullptr));
    DMXCHK(t.wait());
    return t.down(out, dOut, outBytes);
}

extern "C" int dmx_logmel(int device, const float *planes, int n_planes, int64_t n, const dmx_logmel_spec *spec, float *out)
{
    const char *fn = "dmx_logmel";
    DMXCHK(logmel_check(fn, spec, n < 0 ? 0 : n));
    if (!planes || !out || n_planes < 1 || n_planes > 65535)
        return fail(DMX_ERR_ARG, "%s: %s", fn, !planes ? "null planes pointer" : !out ? "null out pointer" : "n_planes is not in [1, 65535]");
    HIPCHK(hipSetDevice(device));
    HostTrip t(fn);
    const size_t inBytes = sizeof(float) * (size_t)n_planes * (size_t)n;
    float *dIn;
    DMXCHK(t.alloc(&dIn, inBytes));
    DMXCHK(t.up(dIn, planes, inBytes));
    return logmel_to_host(fn, device, dIn, n_planes, n, spec, t, out);
}

extern "C" int dmx_logmel_from_stems(int device, const float *stems, int n_sources, int channels, int64_t n, int rate_in,
                                     const dmx_logmel_spec *spec, float *out)
{
    const char *fn = "dmx_logmel_from_stems";
    DMXCHK(logmel_check(fn, spec, -1));
    DMXCHK(first_null(fn, {{"stems", stems}, {"out", out}}));
    if (n_sources < 1 || n_sources > 65535 || (channels != 1 && channels != 2) || n < 1)
        return fail(DMX_ERR_ARG, "%s: n_sources %d, channels %d (1 | 2), n %lld", fn, n_sources, channels, (long long)n);
    const int64_t m = dmx_resample_length(n, rate_in, spec->sr);
    if (m < 0)
        return fail(DMX_ERR_ARG, "%s: invalid rates %d -> %d", fn, rate_in, spec->sr);
    DMXCHK(logmel_check(fn, spec, m));
    HIPCHK(hipSetDevice(device));
    HostTrip t(fn);
    const size_t S = (size_t)n_sources, inFloats = S * (size_t)channels * (size_t)n;
    float *dIn;
    DMXCHK(t.alloc(&dIn, sizeof(float) * (inFloats + S * (size_t)n + S * (size_t)m)));
    float *dMono = dIn + inFloats, *dRate = dMono + S * (size_t)n;
    DMXCHK(t.up(dIn, stems, sizeof(float) * inFloats));
    launch_logmel_fold(dIn, dMono, n_sources, channels, n, nullptr);
    DMXCHK(dmx_resample_device(device, dMono, n, n_sources, n, 1, rate_in, spec->sr, dRate, m, 1, nullptr));
    return logmel_to_host(fn, device, dRate, n_sources, m, spec, t, out);
}

extern "C" int dmx_npy_write_f32(const char *path, const float *data, int ndim, const int64_t *shape)
{
    const char *fn = "dmx_npy_write_f32";
    if (!path || !data || !shape || ndim < 1 || ndim > 8)
        return fail(DMX_ERR_ARG, "%s: %s", fn, !path ? "null path" : !data ? "null data pointer" : !shape ? "null shape pointer" : "ndim is not in [1, 8]");
    std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (";
    size_t count = 1;
    for (int i = 0; i < ndim; ++i)
    {
        if (shape[i] < 0)
            return fail(DMX_ERR_ARG, "%s: shape[%d] is negative", fn, i);
        dict += std::to_string(shape[i]) + (ndim == 1 || i + 1 < ndim ? ", " : "");
        count *= (size_t)shape[i];
    }
    dict += "), }";
    while ((10 + dict.size() + 1) % 64) // magic, version and length take 10 bytes; the header ends with a newline on a 64-byte line
        dict += ' ';
    dict += '\n';
    const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(dict.size() & 255), (unsigned char)(dict.size() >> 8)};
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return fail(DMX_ERR_ARG, "%s: cannot open %s", fn, path);
    const bool ok = std::fwrite(head, 1, 10, f) == 10 && std::fwrite(dict.data(), 1, dict.size(), f) == dict.size() &&
                    std::fwrite(data, sizeof(float), count, f) == count;
    if (std::fclose(f) != 0 || !ok)
        return fail(DMX_ERR_ARG, "%s: writing %s failed", fn, path);
    return DMX_OK;
}
