// codec_api.cpp — the codecs as entry points of their own: PCM / remix encoding (pcm.hip), FLAC output (flac.hip) and
// FLAC input (flac_in.hip) on buffers the caller names, on the device or, through a scratch copy, on the host.
#include "api_internal.h"

#include <algorithm>
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
    DMXCHK(first_null(fn, {{"d_planes", d_planes}, {"d_out", d_out}, {"d_peaks", d_peaks}}));
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

// the end of dmx_pcm_encode, dmx_remix_encode and (loud_api.cpp) the dmx_loud_encode* host calls: wait for the kernels, then the
// nOut outputs and the peaks leave
int pcm_download(const HostTrip &t, void *out, float *peaks, const unsigned char *dOut, const float *dPeaks, int nOut, i64 bytes, i64 devStride)
{
    DMXCHK(t.wait());
    for (int o = 0; o < nOut; ++o)
        DMXCHK(t.down((unsigned char *)out + (size_t)(o * bytes), dOut + (size_t)(o * devStride), (size_t)bytes));
    if (peaks)
        DMXCHK(t.down(peaks, dPeaks, sizeof(float) * (size_t)nOut));
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
    HostTrip t(fn);
    float *dIn, *dPeaks;
    unsigned char *dOut;
    DMXCHK(t.alloc(&dIn, inBytes));
    DMXCHK(t.alloc(&dOut, (size_t)(nOut * devStride)));
    DMXCHK(t.alloc(&dPeaks, sizeof(float) * (size_t)nOut));
    DMXCHK(t.up(dIn, planes, inBytes));
    DMXCHK(dmx_pcm_encode_device(device, dIn, n_sources, n, n, spec, dOut, dPeaks, nullptr));
    return pcm_download(t, out, peaks, dOut, dPeaks, nOut, bytes, devStride);
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
    DMXCHK(first_null(fn, {{"d_planes", d_planes}, {"d_out", d_out}, {"d_peaks", d_peaks}}));
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
    HostTrip t(fn);
    float *dIn, *dPeaks, *dMix = nullptr;
    unsigned char *dOut;
    DMXCHK(t.alloc(&dIn, inBytes));
    DMXCHK(t.alloc(&dOut, (size_t)(nOut * devStride)));
    DMXCHK(t.alloc(&dPeaks, sizeof(float) * (size_t)nOut));
    if (mix)
        DMXCHK(t.alloc(&dMix, mixBytes));
    DMXCHK(t.up(dIn, planes, inBytes));
    if (mix)
        DMXCHK(t.up(dMix, mix, mixBytes));
    DMXCHK(dmx_remix_encode_device(device, dIn, n_sources, n, n, dMix, spec, dOut, dPeaks, nullptr));
    return pcm_download(t, out, peaks, dOut, dPeaks, nOut, bytes, devStride);
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
    DMXCHK(first_null(fn, {{"d_pcm", d_pcm}, {"d_out", d_out}, {"d_size", d_size}, {"d_work", d_work}}));
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
    float gaps[3];
    DMXCHK(timed_call<4>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        return flac_encode_device(fn, device, d_pcm, bits, n, sample_rate, level, d_out, d_size, d_work, stream, marks);
    }));
    std::copy(gaps, gaps + 3, ms);
    return DMX_OK;
}

static int flac_encode_host(const char *fn, int device, const void *pcm, int bits, int64_t n, int sample_rate, int level, void *out,
                            int64_t *size)
{
    DMXCHK(flac_check(fn, bits, n, sample_rate));
    DMXCHK(flac_level_check(fn, level));
    DMXCHK(first_null(fn, {{"pcm", pcm}, {"out", out}, {"size", size}}));
    HIPCHK(hipSetDevice(device));
    const size_t inBytes = (size_t)n * 2 * (size_t)(bits / 8);
    const i64 bound = flac_bound(bits, n), workBytes = flac_workspace_bytes(bits, n);
    HostTrip t(fn);
    void *dIn, *dOut, *dWork;
    int64_t *dSize, got = 0;
    DMXCHK(t.alloc(&dIn, DMX_OUTPUT_STRIDE(inBytes)));
    DMXCHK(t.alloc(&dOut, (size_t)bound));
    DMXCHK(t.alloc(&dWork, (size_t)workBytes));
    DMXCHK(t.alloc(&dSize, sizeof(int64_t)));
    DMXCHK(t.up(dIn, pcm, inBytes));
    DMXCHK(flac_encode_device(fn, device, dIn, bits, n, sample_rate, level, dOut, dSize, dWork, nullptr, nullptr));
    DMXCHK(t.wait());
    DMXCHK(t.down(&got, dSize, sizeof(int64_t)));
    if (got < 42 || got > bound)
        return fail(DMX_ERR_HIP, "%s: internal error (%lld encoded bytes, bound %lld)", fn, (long long)got, (long long)bound);
    DMXCHK(t.down(out, dOut, (size_t)got));
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
    DMXCHK(first_null(fn, {{"d_file", d_file}, {"d_out", d_out}, {"d_status", d_status}, {"d_work", d_work}}));
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
    DMXCHK(first_null(fn, {{"file", file}, {"out", out}, {"status", status}}));
    HIPCHK(hipSetDevice(device));
    const size_t outBytes = (size_t)info->total_samples * (encoding == DMX_PCM_F32 ? 8 : encoding == DMX_PCM_S16 ? 4 : 6);
    const i64 workBytes = flac_in_workspace_bytes(info, bytes);
    HostTrip t(fn);
    void *dIn, *dOut, *dWork;
    int64_t *dStatus;
    DMXCHK(t.alloc(&dIn, (size_t)bytes));
    DMXCHK(t.alloc(&dOut, DMX_OUTPUT_STRIDE(outBytes)));
    DMXCHK(t.alloc(&dWork, (size_t)workBytes));
    DMXCHK(t.alloc(&dStatus, 2 * sizeof(int64_t)));
    DMXCHK(t.up(dIn, file, (size_t)bytes));
    DMXCHK(dmx_flac_decode_device(device, dIn, bytes, info, encoding, dOut, dStatus, dWork, nullptr));
    DMXCHK(t.wait());
    DMXCHK(t.down(status, dStatus, 2 * sizeof(int64_t)));
    return t.down(out, dOut, outBytes);
}

// measurement aid (tools/flac_in_bench.py): dmx_flac_decode_device with HIP events around each of the five launches;
// ms[0..5): candidates, scan, chain, decode, finish. Waits for the last event, which synchronises the stream.
extern "C" int dmx_flac_decode_profile(int device, const void *d_file, int64_t bytes, const dmx_flac_info *info, int encoding, void *d_out,
                                       int64_t *d_status, void *d_work, void *stream, float *ms)
{
    const char *fn = "dmx_flac_decode_profile";
    DMXCHK(flac_in_check(fn, bytes, info, encoding));
    if (!d_file || !d_out || !d_status || !d_work || !ms)
        return fail(DMX_ERR_ARG, "%s: null pointer", fn);
    float gaps[5];
    DMXCHK(timed_call<6>(fn, device, ms, gaps, [&](hipEvent_t *marks) {
        if (launch_flac_decode((const unsigned char *)d_file, bytes, info, encoding, d_out, (long long *)d_status, d_work, (hipStream_t)stream, marks) != 0)
            return fail(DMX_ERR_ARG, "%s: info rejected", fn);
        HIPCHK(hipGetLastError());
        return DMX_OK;
    }));
    std::copy(gaps, gaps + 5, ms);
    return DMX_OK;
}
