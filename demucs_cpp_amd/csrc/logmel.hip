// logmel.hip — log-mel features of fp32 planes on the GPU (the specification is restated in
// tests/logmel_spec.py): Whisper's and librosa's front end as two chained binary64 matrix products on v_mfma_f64_16x16x4_f64.
//   tables     the windowed DFT matrix w[n] cos, -w[n] sin (2 pi f n / n_fft) from host-made twiddles and window, written in
//              the order the slabs are staged in: [bin tile][slab][re | im][row][16 bins]
//   power_mel  one workgroup per (plane, chunk, tile of frames), a wave per 16 frames. The samples the tile's frames cover sit
//              in LDS once, as fp32 (reflection and the zero extension by index arithmetic on load). First product,
//              transposed: D[bin][frame] = sum_n table[n][bin] x[frame hop + n]; the table is the A operand, read from a
//              double-buffered LDS slab the waves share, the Toeplitz view of the samples is the B operand, read with
//              overlapping addresses and converted on read. Its accumulator layout (bins 4 r + lane / 16, frame lane % 16) is
//              the B operand layout of the second product M[mel][frame] = sum_bin W[mel][bin] p[bin][frame], so p = re^2 + im^2
//              never leaves the registers; the mel accumulators (8 tiles, 64 VGPRs) stay in registers across all bin tiles,
//              and an all-zero block of the banded W is skipped from a host-made mask.
//   finish     the maximum of a (plane, chunk) over its tiles' maxima, and the clamp in place (DMX_LOG_DB with top_db,
//              DMX_LOG_WHISPER). Rounding to fp32 is monotone, so the clamp of the rounded values is the rounded clamp.
// No atomics, no workgroup waits on another, every sum in a fixed order: equal inputs give equal bits.
#include "kernels.h"

#include <cfloat>

namespace dmx
{
namespace
{
typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// D = A (16 x 4) B (4 x 16) + C. Lane l gives A[l % 16][l / 16] and B[l / 16][l % 16] and holds D[4 r + l / 16][l % 16] in element r
__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

struct LogmelArgs
{
    const float *x;
    float *out;
    const double *tw, *win, *wt, *tmaxIn;
    const int *mask;
    double *table, *tmax;
    i64 n, stride, len, frames, tiles;
    int n_fft, hop, n_mels, log_mode, chunks, ft, K, skew, nft;
    i64 span;
    double amin, top_db;
};

// grid (ceil(nft * n_fft * 32 / 256)): element e of the table
__global__ __launch_bounds__(256) void logmel_tables_kernel(LogmelArgs a)
{
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= (i64)a.nft * a.n_fft * 32)
        return;
    const int lo = (int)(e & 15), k = (int)((e >> 4) % a.K), part = (int)((e >> 4) / a.K & 1);
    const i64 g = e / ((i64)a.K * 32); // the slab: bin tile g / S, rows [s K, (s + 1) K)
    const int S = a.n_fft / a.K, f = (int)(g / S) * 16 + lo, n = (int)(g % S) * a.K + k;
    double v = 0.0;
    if (f <= a.n_fft / 2)
    {
        const int ph = (int)((i64)f * n % a.n_fft);
        v = part == 0 ? a.win[n] * a.tw[2 * ph] : -(a.win[n] * a.tw[2 * ph + 1]);
    }
    a.table[e] = v;
}

// the log of one mel power: what is stored, and (by `key`) what the maximum of the (plane, chunk) is taken over
__device__ inline double logmel_value(const LogmelArgs &a, double m, double *key)
{
    if (a.log_mode == kLogDb)
        return *key = 10.0 * log10(m > a.amin ? m : a.amin);
    if (a.log_mode == kLogWhisper)
    {
        *key = log10(m > 1e-10 ? m : 1e-10);
        return (*key + 4.0) / 4.0;
    }
    return *key = m;
}

template <int NW>
__device__ inline void logmel_fetch(v2d (&pre)[16 / NW], const LogmelArgs &a, i64 g, int slabD2, int tid)
{
    const v2d *src = (const v2d *)(a.table + g * a.K * 32);
#pragma unroll
    for (int q = 0; q < 16 / NW; ++q)
        if (tid + q * 64 * NW < slabD2)
            pre[q] = src[tid + q * 64 * NW];
}
template <int NW>
__device__ inline void logmel_put(const v2d (&pre)[16 / NW], double *slab, int K, i64 g, int slabD2, int tid)
{
    v2d *dst = (v2d *)(slab + (g & 1) * K * 32);
#pragma unroll
    for (int q = 0; q < 16 / NW; ++q)
        if (tid + q * 64 * NW < slabD2)
            dst[tid + q * 64 * NW] = pre[q];
}

// grid (tiles, chunks, planes), NW = ft / 16 waves, dynamic LDS: the samples, then two slabs
template <int NW>
__global__ __launch_bounds__(64 * NW) void logmel_power_mel_kernel(LogmelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ double wmax[4];
    float *smp = (float *)lds;
    const i64 sampleFloats = (a.span + a.skew * ((a.span - 1) / a.hop + 1) + 3) & ~(i64)3;
    double *slab = (double *)(lds + 4 * sampleFloats);
    const int tid = threadIdx.x, nthr = 64 * NW, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const i64 tile = blockIdx.x, chunk = blockIdx.y, plane = blockIdx.z;
    const i64 t0 = tile * a.ft, valid = a.frames - t0 < a.ft ? a.frames - t0 : a.ft; // frames of this tile that exist
    const float *xp = a.x + plane * a.stride;
    const i64 base = chunk * a.len, used = (valid - 1) * a.hop + a.n_fft;
    for (i64 i = tid; i < a.span; i += nthr)
    {
        i64 j = t0 * a.hop + i - a.n_fft / 2; // inside the chunk, reflected about its ends
        j = j < 0 ? -j : j;
        j = j >= a.len ? 2 * (a.len - 1) - j : j;
        const bool in = i < used && j >= 0 && j < a.len && base + j < a.n;
        smp[i + a.skew * (i / a.hop)] = in ? xp[base + j] : 0.0f;
    }
    const int S = a.n_fft / a.K, slabD2 = a.K * 16; // double2 elements of a slab
    const i64 G = (i64)a.nft * S;
    // a slab goes global -> registers before the MFMAs of the slab in use and registers -> LDS behind them
    v2d pre[16 / NW]; // K 16 double2 elements over the threads: at most 4 with four waves, 16 with one
    logmel_fetch<NW>(pre, a, 0, slabD2, tid);
    logmel_put<NW>(pre, slab, a.K, 0, slabD2, tid);
    __syncthreads();
    v4d macc[kLogmelMelTiles], re, im;
#pragma unroll
    for (int m = 0; m < kLogmelMelTiles; ++m)
        macc[m] = v4d{0.0, 0.0, 0.0, 0.0};
    const int frame0 = (wave * 16 + lo) * (a.hop + a.skew); // this lane's frame in the sample image
    int addr = 0, rem = 0, s = 0, ft = 0;
    for (i64 g = 0; g < G; ++g)
    {
        if (g + 1 < G)
            logmel_fetch<NW>(pre, a, g + 1, slabD2, tid);
        if (s == 0)
        {
            re = v4d{0.0, 0.0, 0.0, 0.0}, im = v4d{0.0, 0.0, 0.0, 0.0};
            addr = frame0 + hi + a.skew * (hi / a.hop), rem = hi % a.hop; // sample n = hi of the frame
        }
        const double *sr = slab + (g & 1) * a.K * 32 + hi * 16 + lo, *si = sr + a.K * 16;
        for (int k = 0; k < a.K; k += 4)
        {
            const double xv = (double)smp[addr];
            re = mfma_f64(sr[k * 16], xv, re);
            im = mfma_f64(si[k * 16], xv, im);
            addr += 4, rem += 4;
            while (rem >= a.hop)
                rem -= a.hop, addr += a.skew;
        }
        if (++s == S)
        {
            const v4d p = re * re + im * im;
            const int mk = a.mask[ft];
            const double *w = a.wt + (i64)ft * kLogmelMelTiles * 256 + lane;
#pragma unroll
            for (int m = 0; m < kLogmelMelTiles; ++m)
                if (mk >> m & 1)
                {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        macc[m] = mfma_f64(w[(m * 4 + q) * 64], p[q], macc[m]);
                }
            s = 0, ++ft;
        }
        if (g + 1 < G)
            logmel_put<NW>(pre, slab, a.K, g + 1, slabD2, tid);
        __syncthreads(); // slab g + 1 is written, slab g is read: the next step writes over slab g
    }
    // mel 16 m + 4 r + hi of frame t0 + 16 wave + lo: the frames run along the lanes
    const i64 t = t0 + wave * 16 + lo;
    float *op = a.out + (plane * a.chunks + chunk) * a.n_mels * a.frames;
    double best = -DBL_MAX;
#pragma unroll
    for (int m = 0; m < kLogmelMelTiles; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const int mel = 16 * m + 4 * r + hi;
            if (mel < a.n_mels && t < a.frames)
            {
                double key;
                op[mel * a.frames + t] = (float)logmel_value(a, macc[m][r], &key);
                best = key > best ? key : best;
            }
        }
    for (int d = 32; d > 0; d >>= 1)
    {
        const double o = __shfl_xor(best, d);
        best = o > best ? o : best;
    }
    if (lane == 0)
        wmax[wave] = best;
    __syncthreads();
    if (tid == 0)
    {
        for (int w = 1; w < nthr / 64; ++w)
            best = wmax[w] > best ? wmax[w] : best;
        a.tmax[(plane * a.chunks + chunk) * a.tiles + tile] = best;
    }
}

// grid (ceil(n_mels frames / 1024), chunks, planes)
__global__ __launch_bounds__(256) void logmel_finish_kernel(LogmelArgs a)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const i64 pc = (i64)blockIdx.z * a.chunks + blockIdx.y;
    double best = -DBL_MAX;
    for (i64 i = tid; i < a.tiles; i += 256)
    {
        const double v = a.tmaxIn[pc * a.tiles + i];
        best = v > best ? v : best;
    }
    red[tid] = best;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1)
    {
        if (tid < d)
            red[tid] = red[tid + d] > red[tid] ? red[tid + d] : red[tid];
        __syncthreads();
    }
    const double mx = red[0];
    const float floor32 = a.log_mode == kLogWhisper ? (float)(((mx - 8.0) + 4.0) / 4.0) : (float)(mx - a.top_db);
    float *op = a.out + pc * a.n_mels * a.frames;
    const i64 count = (i64)a.n_mels * a.frames, i0 = (i64)blockIdx.x * 1024;
    for (i64 i = i0 + tid; i < i0 + 1024 && i < count; i += 256)
        op[i] = op[i] > floor32 ? op[i] : floor32;
}

// stems [S][C][n] -> mono [S][n]: 0.5 (L + R) in fp32
__global__ void logmel_fold_kernel(const float *in, float *out, int C, i64 n)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float *p = in + (i64)blockIdx.y * C * n;
    out[(i64)blockIdx.y * n + i] = C == 2 ? 0.5f * (p[i] + p[n + i]) : p[i];
}
} // namespace

void launch_logmel_fold(const float *in, float *out, int sources, int C, i64 n, hipStream_t s)
{
    hipLaunchKernelGGL(logmel_fold_kernel, dim3((unsigned)((n + 255) / 256), sources), dim3(256), 0, s, in, out, C, n);
}

void launch_logmel(const LogmelJob &job, hipStream_t s, hipEvent_t *marks)
{
    const LogmelSpec &sp = job.spec;
    const LogmelLayout l = logmel_layout(sp, job.planes, job.n);
    LogmelArgs a{};
    a.x = job.x, a.out = job.out;
    a.tw = (const double *)(job.work + l.tw), a.win = (const double *)(job.work + l.win), a.wt = (const double *)(job.work + l.wt);
    a.mask = (const int *)(job.work + l.mask);
    a.table = (double *)(job.work + l.table), a.tmax = (double *)(job.work + l.tmax), a.tmaxIn = a.tmax;
    a.n = job.n, a.stride = job.stride, a.len = l.fr.len, a.frames = l.fr.frames, a.tiles = l.tiles;
    a.n_fft = sp.n_fft, a.hop = sp.hop, a.n_mels = sp.n_mels, a.log_mode = sp.log_mode, a.chunks = (int)l.fr.chunks;
    a.ft = l.tile.ft, a.K = l.tile.K, a.skew = l.tile.skew, a.nft = l.tile.nft, a.span = l.tile.span;
    a.amin = sp.amin, a.top_db = sp.top_db;
    Marks mark{marks, s};
    mark();
    (void)hipMemcpyAsync(job.work, job.hostTables, (size_t)l.hostBytes, hipMemcpyHostToDevice, s);
    const i64 elems = (i64)a.nft * a.n_fft * 32;
    hipLaunchKernelGGL(logmel_tables_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, a);
    mark();
    const size_t smem = (size_t)(l.tile.ldsBytes - kLogmelLdsStatic);
    const dim3 grid((unsigned)l.tiles, (unsigned)l.fr.chunks, (unsigned)job.planes);
    auto go = [&](auto kern) {
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLogmelLds - kLogmelLdsStatic);
        hipLaunchKernelGGL(kern, grid, dim3(4 * a.ft), smem, s, a);
    };
    if (a.ft == 64)
        go(logmel_power_mel_kernel<4>);
    else if (a.ft == 32)
        go(logmel_power_mel_kernel<2>);
    else
        go(logmel_power_mel_kernel<1>);
    mark();
    if (logmel_needs_max(sp))
        hipLaunchKernelGGL(logmel_finish_kernel, dim3((unsigned)(((i64)a.n_mels * a.frames + 1023) / 1024), (unsigned)l.fr.chunks, (unsigned)job.planes),
                           dim3(256), 0, s, a);
    mark();
}

} // namespace dmx
