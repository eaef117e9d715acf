// tracks.hip — track-level kernels for gfx950: statistics, the segment gather and the three overlap-add kernels (one copy,
// the shifts ensemble, a bag of models). HBM-bound, fixed summation order => bit-reproducible results. The three overlap-add
// kernels hold the per-sample arithmetic as three texts kept alike: they give the same bits where their specifications
// coincide (DESIGN.md sections 2.7, 2.9). One shared inline body was tried and made the ensemble kernel 9 % slower
// (profiles/track_ola_body_isa.txt, profiles/track_ola_body_ab.txt): change the three together.
//
// Reference semantics:
//   track apply     src/model_apply.cpp:60-288
#include "kernels.h"

namespace dmx
{

// ref = mean over channels; mean / unbiased std of ref (model_apply.cpp:72-82). Track blockIdx.y; every track gets the same
// block decomposition and summation order whatever else shares the launch.
__global__ __launch_bounds__(256) void track_stats_kernel(TrackStatsTable t, double *partials)
{
    __shared__ double red[4][2];
    const int tr = blockIdx.y;
    const float2 *a = reinterpret_cast<const float2 *>(t.audio[tr]);
    const i64 n = t.n[tr];
    double s = 0.0, q = 0.0;
    const i64 per = (n + gridDim.x - 1) / gridDim.x;
    const i64 lo = (i64)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    for (i64 i = lo + threadIdx.x; i < hi; i += 256)
    {
        const float2 v = a[i];
        const float r = (v.x + v.y) / 2.0f;
        s += (double)r;
        q += (double)r * (double)r;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
        s += __shfl_xor(s, off);
        q += __shfl_xor(q, off);
    }
    if ((threadIdx.x & 63) == 0)
    {
        red[threadIdx.x >> 6][0] = s;
        red[threadIdx.x >> 6][1] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double *p = partials + (i64)tr * gridDim.x * 2;
        p[blockIdx.x * 2] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        p[blockIdx.x * 2 + 1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    }
}
// one block per track
__global__ void track_stats_final_kernel(TrackStatsTable t, const double *partials, int nblk)
{
    if (threadIdx.x == 0)
    {
        const int tr = blockIdx.x;
        const double *p = partials + (i64)tr * nblk * 2;
        const i64 n = t.n[tr];
        double s = 0.0, q = 0.0;
        for (int i = 0; i < nblk; ++i)
        {
            s += p[2 * i];
            q += p[2 * i + 1];
        }
        const double mean = s / (double)n;
        double var = (q - (double)n * mean * mean) / (double)(n - 1);
        if (var < 0.0)
            var = 0.0;
        t.stats[tr][0] = (float)mean;
        t.stats[tr][1] = (float)sqrt(var);
    }
}
void launch_track_stats(const TrackStatsTable &t, int T, double *partials, int nblk, hipStream_t s)
{
    if (T > 0)
        hipLaunchKernelGGL(track_stats_kernel, dim3(nblk, T), dim3(256), 0, s, t, partials);
}
void launch_track_stats_final(const TrackStatsTable &t, int T, const double *partials, int nblk, hipStream_t s)
{
    if (T > 0)
        hipLaunchKernelGGL(track_stats_final_kernel, dim3(T), dim3(64), 0, s, t, partials, nblk);
}
void launch_track_stats(const float *audio, i64 n, double *partials, int nblk, hipStream_t s)
{
    TrackStatsTable t{};
    t.audio[0] = audio, t.n[0] = n;
    launch_track_stats(t, 1, partials, nblk, s);
}
void launch_track_stats_final(const double *partials, int nblk, i64 n, float *stats, hipStream_t s)
{
    TrackStatsTable t{};
    t.n[0] = n, t.stats[0] = stats;
    launch_track_stats_final(t, 1, partials, nblk, s);
}

// shift + zero pad + normalise + chunk + centre (model_apply.cpp:21-43,93-138,189-194,250-262).
// The (track, segment) items travel by value in the kernel arguments: no device index buffer, no host
// synchronisation between consecutive gathers.
__global__ __launch_bounds__(256) void track_gather_kernel(TrackSegIdx items, i64 seg, i64 stride, float *mixes)
{
    const int which = blockIdx.y;
    const TrackSegItem &it = items.v[which];
    const i64 maxShift = 22050;
    const i64 n = it.n;
    const int shiftOffset = it.shift;
    const i64 len = n + maxShift - shiftOffset; // dmx_track_geometry
    const i64 off = (i64)it.seg * stride;
    const i64 chunk = seg < len - off ? seg : len - off;
    const i64 left = (seg - chunk) / 2; // floor(total_padding / 2)
    const float mean = it.stats[0], stdv = it.stats[1];
    const float2 *a = reinterpret_cast<const float2 *>(it.audio);
    float2 *dst = reinterpret_cast<float2 *>(mixes) + (i64)which * seg;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < seg; i += (i64)gridDim.x * 256)
    {
        float2 v = make_float2(0.f, 0.f);
        const i64 k = i - left;
        if (k >= 0 && k < chunk)
        {
            const i64 src = off + k + shiftOffset - maxShift; // index into the un-padded track
            if (src >= 0 && src < n)
            {
                const float2 x = a[src];
                v = make_float2((x.x - mean) / stdv, (x.y - mean) / stdv);
            }
        }
        dst[i] = v;
    }
}
void launch_track_gather(const TrackSegItem *items, int nIdx, i64 seg, i64 stride, float *mixes, hipStream_t s)
{
    int gx = (int)((seg + 255) / 256);
    if (gx > 512)
        gx = 512;
    for (int i0 = 0; i0 < nIdx; i0 += TrackSegIdx::kMax)
    {
        TrackSegIdx t{};
        const int nb = nIdx - i0 < TrackSegIdx::kMax ? nIdx - i0 : TrackSegIdx::kMax;
        for (int i = 0; i < nb; ++i)
            t.v[i] = items[i0 + i];
        hipLaunchKernelGGL(track_gather_kernel, dim3(gx, nb), dim3(256), 0, s, t, seg, stride, mixes + (i64)i0 * seg * 2);
    }
}
void launch_track_gather(const float *audio, i64 n, const float *stats, int shiftOffset, i64 seg, i64 stride, i64 len,
                         const int *segIdx, int nIdx, float *mixes, hipStream_t s)
{
    (void)len; // n + DMX_MAX_SHIFT - shiftOffset: the kernel derives it
    for (int i0 = 0; i0 < nIdx; i0 += TrackSegIdx::kMax)
    {
        TrackSegItem it[TrackSegIdx::kMax];
        const int nb = nIdx - i0 < TrackSegIdx::kMax ? nIdx - i0 : TrackSegIdx::kMax;
        for (int i = 0; i < nb; ++i)
            it[i] = TrackSegItem{audio, stats, n, shiftOffset, segIdx[i0 + i]};
        launch_track_gather(it, nb, seg, stride, mixes + (i64)i0 * seg * 2, s);
    }
}

// grid x of a launch over n pieces [i0, i1): 256 samples a block over the longest piece, grid-stride beyond 4096 blocks;
// 0 when no piece has a sample
template <class Piece>
static int ola_grid_x(const Piece *p, int n)
{
    i64 span = 0;
    for (int k = 0; k < n; ++k)
        if (p[k].i1 - p[k].i0 > span)
            span = p[k].i1 - p[k].i0;
    const i64 gx = (span + 255) / 256;
    return (int)(gx > 4096 ? 4096 : gx);
}

// weighted overlap-add in segment order, /sum_weight, trim, de-normalise
// (model_apply.cpp:171-179,207-246,129-135,88). Each output sample is covered by at most
// ceil(seg/stride) = 2 segments; they are accumulated in increasing segment index like the
// reference loop, so the result does not depend on how segments were sharded over GPUs or batched with other tracks.
// planes [planeBase, planeBase + gridDim.y) (plane = s*2 + ch) and samples [i0, i1) of the output of track blockIdx.z are
// produced: the bag takes stem m from model m, and a track can be finished (and copied out) in pieces
// as soon as the segments covering a piece are done.
__global__ __launch_bounds__(256) void track_ola_kernel(TrackOlaTable t, int S, i64 seg, i64 stride, i64 ring, int layout,
                                                        int planeBase)
{
    const TrackOlaEntry &e = t.e[blockIdx.z];
    const int plane = blockIdx.y + planeBase;
    const float mean = e.stats[0], stdv = e.stats[1];
    const i64 maxShift = 22050;
    const float half = (float)(seg / 2);
    const i64 n = e.n, len = e.len;
    const int nSeg = e.nSeg;
    const float *segOut = e.segOut;
    float *out = e.out;
    for (i64 i = e.i0 + (i64)blockIdx.x * 256 + threadIdx.x; i < e.i1; i += (i64)gridDim.x * 256)
    {
        const i64 j = i + maxShift - e.shift; // position in the shifted track
        float acc = 0.f, sw = 0.f;
        i64 first = (j - seg + stride) / stride; // smallest g with g*stride + seg > j
        if (j - seg + 1 <= 0)
            first = 0;
        for (i64 g = first; g < nSeg && g * stride <= j; ++g)
        {
            const i64 off = g * stride;
            const i64 chunk = seg < len - off ? seg : len - off;
            const i64 k = j - off;
            if (k >= chunk)
                continue;
            const i64 left = (seg - chunk) / 2;
            // triangle weight, indexed from 0 even for short chunks (Q8)
            const i64 kk = k < seg / 2 ? k + 1 : seg - k;
            const float w = (float)kk / half;
            i64 blk = e.slot0 + (g - e.gBase);
            if (blk >= ring)
                blk -= ring;
            acc += w * segOut[(blk * S * 2 + plane) * seg + left + k];
            sw += w;
        }
        const float v = (acc / sw) * stdv + mean;
        if (layout == 0)
            out[(i64)plane * n + i] = v;
        else
        {
            const int sIdx = plane >> 1, c = plane & 1;
            out[sIdx + (i64)S * (c + 2 * i)] = v;
        }
    }
}
void launch_track_ola(const TrackOlaEntry *entries, int T, int S, i64 seg, i64 stride, i64 ring, int layout, int planeBase,
                      int nPlanes, hipStream_t s)
{
    if (nPlanes <= 0)
        return;
    for (int t0 = 0; t0 < T; t0 += TrackOlaTable::kMax)
    {
        TrackOlaTable t{};
        int nt = 0;
        for (int k = t0; k < T && k < t0 + TrackOlaTable::kMax; ++k)
            t.e[nt++] = entries[k];
        const int gx = ola_grid_x(t.e, nt);
        if (gx > 0)
            hipLaunchKernelGGL(track_ola_kernel, dim3(gx, nPlanes, nt), dim3(256), 0, s, t, S, seg, stride, ring, layout, planeBase);
    }
}
void launch_track_ola(const float *segOut, int nSeg, int S, i64 seg, i64 stride, i64 len, i64 n, int shiftOffset,
                      const float *stats, float *out, int layout, int planeBase, int nPlanes, i64 i0, i64 i1, hipStream_t s, int gBase)
{
    if (i1 <= i0)
        return;
    TrackOlaEntry e{segOut, stats, out, n, len, i0, i1, gBase, 0, nSeg, shiftOffset};
    launch_track_ola(&e, 1, S, seg, stride, INT64_MAX, layout, planeBase, nPlanes, s);
}

// the shifts ensemble (apply_model(shifts=N): out += shifted_out; out /= shifts, then * std + mean in separate): for each
// copy k in increasing k, exactly track_ola_kernel's normalised value acc / sw on copy k's shifted geometry, summed in fp32;
// then (e / N) * std + mean, written like track_ola_kernel's (acc / sw) * stdv + mean so that both contract alike.
// Grid (x, planes, pieces); the pieces and their copies travel by value (TrackEnsTable).
static_assert(sizeof(TrackEnsTable) <= 3584, "TrackEnsTable must leave room in HIP's 4 KB kernel-argument limit");
__device__ __forceinline__ i64 ens_item(const TrackEnsCopy *cp, int N, int nMin, i64 g, int k)
{
    if (g < nMin)
        return g * N + k;
    i64 it = 0; // the tail rows: copies with nseg <= g are absent
    for (int q = 0; q < N; ++q)
    {
        const i64 nq = cp[q].nseg;
        it += g < nq ? g : nq;
        if (q < k && nq > g)
            ++it;
    }
    return it;
}
__global__ __launch_bounds__(256) void track_ola_ens_kernel(TrackEnsTable t, int N, const float *segOut, int S, i64 seg,
                                                            i64 stride, i64 ring, int layout, int planeBase)
{
    const TrackEnsPiece &p = t.p[blockIdx.z];
    const TrackEnsCopy *cp = t.c + (i64)blockIdx.z * N;
    const int plane = blockIdx.y + planeBase;
    const float mean = p.stats[0], stdv = p.stats[1];
    const i64 maxShift = 22050;
    const float half = (float)(seg / 2);
    const i64 n = p.n;
    float *out = p.out;
    // item(g, k) - nMin N of the tail rows, computed once per block instead of O(N) per segment read
    __shared__ int tail[TrackEnsTable::kMaxTail];
    const int nMin = p.nMin;
    for (int idx = threadIdx.x; idx < p.nTail * N; idx += 256)
        tail[idx] = (int)(ens_item(cp, N, nMin, nMin + idx / N, idx % N) - (i64)nMin * N);
    __syncthreads();
    for (i64 i = p.i0 + (i64)blockIdx.x * 256 + threadIdx.x; i < p.i1; i += (i64)gridDim.x * 256)
    {
        float e = 0.f;
        for (int c = 0; c < N; ++c)
        {
            const int shift = cp[c].shift, nSeg = cp[c].nseg;
            const i64 len = n + maxShift - shift; // dmx_track_geometry_overlap
            const i64 j = i + maxShift - shift;   // position in copy c's shifted track
            float acc = 0.f, sw = 0.f;
            i64 first = (j - seg + stride) / stride; // smallest g with g*stride + seg > j
            if (j - seg + 1 <= 0)
                first = 0;
            for (i64 g = first; g < nSeg && g * stride <= j; ++g)
            {
                const i64 off = g * stride;
                const i64 chunk = seg < len - off ? seg : len - off;
                const i64 k = j - off;
                if (k >= chunk)
                    continue;
                const i64 left = (seg - chunk) / 2;
                // triangle weight, indexed from 0 even for short chunks (Q8)
                const i64 kk = k < seg / 2 ? k + 1 : seg - k;
                const float w = (float)kk / half;
                const i64 it = g < nMin ? g * N + c : (i64)nMin * N + tail[(g - nMin) * N + c];
                i64 blk = p.slotLo + (it - p.itemLo);
                if (blk >= ring)
                    blk -= ring;
                acc += w * segOut[(blk * S * 2 + plane) * seg + left + k];
                sw += w;
            }
            const float v = acc / sw;
            e = c == 0 ? v : e + v;
        }
        const float v = (e / (float)N) * stdv + mean;
        if (layout == 0)
            out[(i64)plane * n + i] = v;
        else
        {
            const int sIdx = plane >> 1, c = plane & 1;
            out[sIdx + (i64)S * (c + 2 * i)] = v;
        }
    }
}
void launch_track_ola_ens(const TrackEnsPiece *pieces, const TrackEnsCopy *copies, int P, int N, const float *segOut, int S,
                          i64 seg, i64 stride, i64 ring, int layout, int planeBase, int nPlanes, hipStream_t s)
{
    if (nPlanes <= 0 || N < 1 || N > TrackEnsTable::kMaxCopies)
        return;
    for (int z = 0; z < P; ++z)
        if (pieces[z].nTail < 0 || pieces[z].nTail * N > TrackEnsTable::kMaxTail)
            return; // the host checks this before any GPU work (tracks_run)
    const int per = TrackEnsTable::kMaxCopies / N < TrackEnsTable::kMaxPieces ? TrackEnsTable::kMaxCopies / N : TrackEnsTable::kMaxPieces;
    for (int z0 = 0; z0 < P; z0 += per)
    {
        TrackEnsTable t{};
        int nz = 0;
        for (int z = z0; z < P && z < z0 + per; ++z, ++nz)
        {
            t.p[nz] = pieces[z];
            for (int k = 0; k < N; ++k)
                t.c[nz * N + k] = copies[(i64)z * N + k];
        }
        const int gx = ola_grid_x(t.p, nz);
        if (gx > 0)
            hipLaunchKernelGGL(track_ola_ens_kernel, dim3(gx, nPlanes, nz), dim3(256), 0, s, t, N, segOut, S, seg, stride, ring,
                               layout, planeBase);
    }
}

// a bag of models (kernels.h TrackBagTable): track_ola_ens_kernel's per-model value from each
// contributing model's own ring, combined with the stem's weights. Grid (x, planes, pieces); everything travels by value.
// The tail tables of the contributing models lie one behind the other in dynamic LDS, in increasing q.
static_assert(sizeof(TrackBagTable) <= 3584, "TrackBagTable must leave room in HIP's 4 KB kernel-argument limit");
__global__ __launch_bounds__(256) void track_ola_bag_kernel(TrackBagTable t, int Q, int N, int S, i64 seg, i64 stride, int layout,
                                                            int planeBase)
{
    extern __shared__ int bagTail[];
    const TrackBagPiece &p = t.p[blockIdx.z];
    const TrackBagModel *pm = t.m + (i64)blockIdx.z * Q;
    const TrackEnsCopy *pc = t.c + (i64)blockIdx.z * Q * N;
    const int plane = blockIdx.y + planeBase;
    const int stem = plane >> 1;
    const float mean = p.stats[0], stdv = p.stats[1];
    const i64 maxShift = 22050;
    const float half = (float)(seg / 2);
    const i64 n = p.n;
    float *out = p.out;
    {
        int toff = 0;
        for (int q = 0; q < Q; ++q)
        {
            if (t.w[q * S + stem] == 0.f)
                continue;
            const TrackEnsCopy *cp = pc + q * N;
            const int nMin = pm[q].nMin, cnt = pm[q].nTail * N;
            for (int idx = threadIdx.x; idx < cnt; idx += 256)
                bagTail[toff + idx] = (int)(ens_item(cp, N, nMin, nMin + idx / N, idx % N) - (i64)nMin * N);
            toff += cnt;
        }
    }
    __syncthreads();
    for (i64 i = p.i0 + (i64)blockIdx.x * 256 + threadIdx.x; i < p.i1; i += (i64)gridDim.x * 256)
    {
        float a = 0.f, W = 0.f;
        bool have = false;
        int toff = 0;
        for (int q = 0; q < Q; ++q)
        {
            const float wq = t.w[q * S + stem];
            if (wq == 0.f)
                continue;
            const TrackEnsCopy *cp = pc + q * N;
            const float *segOut = t.ring[q];
            const i64 ring = t.ringBlocks[q];
            const int nMin = pm[q].nMin;
            const i64 itemLo = pm[q].itemLo, slotLo = pm[q].slotLo;
            float e = 0.f;
            for (int c = 0; c < N; ++c)
            {
                const int shift = cp[c].shift, nSeg = cp[c].nseg;
                const i64 len = n + maxShift - shift; // dmx_track_geometry_overlap
                const i64 j = i + maxShift - shift;   // position in copy c's shifted track
                float acc = 0.f, sw = 0.f;
                i64 first = (j - seg + stride) / stride; // smallest g with g*stride + seg > j
                if (j - seg + 1 <= 0)
                    first = 0;
                for (i64 g = first; g < nSeg && g * stride <= j; ++g)
                {
                    const i64 off = g * stride;
                    const i64 chunk = seg < len - off ? seg : len - off;
                    const i64 k = j - off;
                    if (k >= chunk)
                        continue;
                    const i64 left = (seg - chunk) / 2;
                    // triangle weight, indexed from 0 even for short chunks (Q8)
                    const i64 kk = k < seg / 2 ? k + 1 : seg - k;
                    const float w = (float)kk / half;
                    const i64 it = g < nMin ? g * N + c : (i64)nMin * N + bagTail[toff + (g - nMin) * N + c];
                    i64 blk = slotLo + (it - itemLo);
                    if (blk >= ring)
                        blk -= ring;
                    acc += w * segOut[(blk * S * 2 + plane) * seg + left + k];
                    sw += w;
                }
                const float v = acc / sw;
                e = c == 0 ? v : e + v;
            }
            if (N > 1)
                e = e / (float)N;
            if (!have)
                a = wq * e, W = wq, have = true;
            else
                a = __fmaf_rn(wq, e, a), W = W + wq;
            toff += pm[q].nTail * N;
        }
        const float v = (a / W) * stdv + mean;
        if (layout == 0)
            out[(i64)plane * n + i] = v;
        else
        {
            const int sIdx = plane >> 1, c = plane & 1;
            out[sIdx + (i64)S * (c + 2 * i)] = v;
        }
    }
}
i64 track_ola_bag_tail_entries(const TrackBagModel *models, int P, int Q, int N, int S, const float *w)
{
    if (Q < 1 || Q > TrackBagTable::kMaxBag || S < 1 || S > TrackBagTable::kMaxStems || N < 1 || (i64)Q * N > TrackBagTable::kMaxCopies)
        return -1;
    i64 most = 0;
    for (int z = 0; z < P; ++z)
        for (int s = 0; s < S; ++s)
        {
            i64 cnt = 0;
            for (int q = 0; q < Q; ++q)
            {
                const TrackBagModel &m = models[(i64)z * Q + q];
                if (m.nTail < 0)
                    return -1;
                if (w[q * S + s] != 0.f)
                    cnt += (i64)m.nTail * N;
            }
            if (cnt > TrackBagTable::kMaxTail)
                return -1;
            most = cnt > most ? cnt : most;
        }
    return most;
}
bool launch_track_ola_bag(const TrackBagPiece *pieces, const TrackBagModel *models, const TrackEnsCopy *copies, int P, int Q, int N,
                          const float *w, const float *const *rings, const i64 *ringBlocks, int S, i64 seg, i64 stride, int layout,
                          int planeBase, int nPlanes, hipStream_t s)
{
    if (nPlanes <= 0 || P <= 0)
        return true;
    if (planeBase < 0 || planeBase + nPlanes > 2 * S || track_ola_bag_tail_entries(models, P, Q, N, S, w) < 0)
        return false;
    int per = TrackBagTable::kMaxPieces;
    per = TrackBagTable::kMaxModels / Q < per ? TrackBagTable::kMaxModels / Q : per;
    per = TrackBagTable::kMaxCopies / (Q * N) < per ? TrackBagTable::kMaxCopies / (Q * N) : per;
    for (int z0 = 0; z0 < P; z0 += per)
    {
        TrackBagTable t{};
        for (int q = 0; q < Q; ++q)
        {
            t.ring[q] = rings[q], t.ringBlocks[q] = ringBlocks[q];
            for (int st = 0; st < S; ++st)
                t.w[q * S + st] = w[q * S + st];
        }
        int nz = 0;
        for (int z = z0; z < P && z < z0 + per; ++z, ++nz)
        {
            t.p[nz] = pieces[z];
            for (int q = 0; q < Q; ++q)
            {
                t.m[nz * Q + q] = models[(i64)z * Q + q];
                for (int k = 0; k < N; ++k)
                    t.c[(nz * Q + q) * N + k] = copies[((i64)z * Q + q) * N + k];
            }
        }
        const int gx = ola_grid_x(t.p, nz);
        if (gx <= 0)
            continue;
        const i64 entries = track_ola_bag_tail_entries(models + (i64)z0 * Q, nz, Q, N, S, w);
        hipLaunchKernelGGL(track_ola_bag_kernel, dim3(gx, nPlanes, nz), dim3(256), (size_t)entries * sizeof(int), s, t, Q, N, S, seg,
                           stride, layout, planeBase);
    }
    return true;
}

} // namespace dmx
