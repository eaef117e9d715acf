// stage_call.h — the host-side idioms of the stage entry points (codec_api.cpp, loud_api.cpp, analysis_api.cpp), once each: the
// first null pointer of an argument list, the round trip of a host convenience call through device scratch, and the timed form
// of a device call. Included by api_internal.h below what it uses (fail, HIPCHK, DMXCHK, DevScratch).
#pragma once
#include <initializer_list>
#include <utility>

// DMX_OK, or DMX_ERR_ARG naming the first null pointer of `args`, a list of {name, pointer}
inline int first_null(const char *fn, std::initializer_list<std::pair<const char *, const void *>> args)
{
    for (const auto &a : args)
        if (!a.second)
            return fail(DMX_ERR_ARG, "%s: null %s pointer", fn, a.first);
    return DMX_OK;
}

// what a wait that HIP refuses reports
inline int kernels_failed(const char *fn) { return fail(DMX_ERR_HIP, "%s: the kernels failed: %s", fn, hipGetErrorString(hipGetLastError())); }

// The round trip of a host convenience call `fn`: device scratch (at most four pieces, freed when the object goes, whichever way
// the call returns), the uploads, the wait for the kernels, the downloads. Every step is DMX_OK or the call's failure: run each
// under DMXCHK, wait() before the first down(). After a failed alloc nothing more is attempted.
class HostTrip
{
    const char *fn;
    DevScratch d;

public:
    explicit HostTrip(const char *f) : fn(f) {}
    template <class T>
    int alloc(T **p, size_t bytes)
    {
        *p = static_cast<T *>(d.get(bytes));
        return d.ok ? DMX_OK : fail(DMX_ERR_HIP, "%s: hipMalloc failed", fn);
    }
    int up(void *dst, const void *src, size_t bytes) const
    {
        return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? DMX_OK : fail(DMX_ERR_HIP, "%s: upload failed", fn);
    }
    int wait() const { return hipDeviceSynchronize() == hipSuccess ? DMX_OK : kernels_failed(fn); }
    int down(void *dst, const void *src, size_t bytes) const
    {
        return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? DMX_OK : fail(DMX_ERR_HIP, "%s: download failed", fn);
    }
};

// The timed form of a device call `fn`: N events on `device`, destroyed on every path; enqueue(marks) records them around its
// launches (kernels.h: Marks) and returns DMX_OK or its failure; the wait on the last event; gaps[k] = the milliseconds between
// events k and k + 1. last: null, or where the call records fewer than N events the index of its last one, read once enqueue has
// returned: the gaps from there on are not written. The caller copies into ms the gaps its contract names.
template <int N, class Enqueue>
int timed_call(const char *fn, int device, const float *ms, float (&gaps)[N - 1], Enqueue enqueue, const int *last = nullptr)
{
    if (!ms)
        return fail(DMX_ERR_ARG, "%s: null ms pointer", fn);
    HIPCHK(hipSetDevice(device));
    struct Events
    {
        hipEvent_t ev[N] = {};
        ~Events()
        {
            for (hipEvent_t e : ev)
                if (e)
                    (void)hipEventDestroy(e);
        }
    } made;
    for (hipEvent_t &e : made.ev)
        if (hipEventCreate(&e) != hipSuccess)
            return fail(DMX_ERR_HIP, "%s: hipEventCreate failed", fn);
    DMXCHK(enqueue(made.ev));
    const int end = last ? *last : N - 1;
    if (hipEventSynchronize(made.ev[end]) != hipSuccess)
        return kernels_failed(fn);
    for (int k = 0; k < end; ++k)
        if (hipEventElapsedTime(&gaps[k], made.ev[k], made.ev[k + 1]) != hipSuccess)
            return fail(DMX_ERR_HIP, "%s: hipEventElapsedTime failed", fn);
    return DMX_OK;
}
