// bss.hip — BSS Eval v4 on the GPU: SDR, ISR, SIR and SAR with multichannel distortion filters estimated over the whole track
// (the specification is restated in tests/bss_spec.py). Everything is binary64. The three heavy stages
// are GEMMs on v_mfma_f64_16x16x4_f64 whose Toeplitz operand is never materialised: a tile of lagged samples is read with
// overlapping addresses from a chunk of the plane that sits in LDS with its halo.
//   gram      rho_ab(k) = sum_m a[m] b[m + k]: 16 reference planes x 16 lags per MFMA over 4 samples, accumulators in registers
//             across a chunk, per-chunk partials, a second launch adds them in chunk order
//   fill      the dense lower triangle of G, the own-source diagonal blocks, the right-hand sides
//   cholesky  blocked right-looking: diagonal block in LDS by one workgroup, panel TRSM, MFMA trailing update of the lower tiles;
//             G and the J own-source blocks as one batch over the grid, the host loops over the panels
//   solve     blocked forward and back substitution of all right-hand sides (one MFMA tile wide)
//   project   p = filters (16 output planes) x taps x samples, the reference chunk in LDS with its halo
//   windows   one workgroup per (window, source): the seven energy sums in a fixed order, the silence flags, the four ratios
// No atomics, and no workgroup waits on another: the same input gives the same bits.
// A source whose reference is all zero is DROPPED without a trip to the host: its rows of G become rows of the identity and
// its right-hand sides zero, so its filters are zero, the other sources' systems are what they are without it, and the window
// kernel reports NaN for it.
#include "kernels.h"

#include <cfloat>

namespace dmx
{
namespace
{
typedef double v4d __attribute__((ext_vector_type(4)));

// D = A (16 x 4) B (4 x 16) + C. Lane l gives A[l % 16][l / 16] and B[l / 16][l % 16] and holds D[bss_row(l, r)][l % 16] in
// element r
__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ inline int bss_row(int lane, int r) { return 4 * r + (lane >> 4); }

struct BssMat
{
    double *a, *rhs; // a: [n][ld] row-major, lower triangle; rhs: [n][kBssCols]
    int n, ld;
};
struct BssBatch
{
    BssMat m[kBssMaxSources + 1];
};

__device__ inline bool bss_kept(const double *rho, int j, int C, int Lp)
{
    bool any = false;
    for (int c = 0; c < C; ++c)
    {
        const int p = j * C + c;
        any = any || rho[((int64_t)p * 16 + p) * Lp] != 0.0;
    }
    return any;
}

// ---------------------------------------------------------------------------------------------------------------- gram
// grid (chunks, 2 M planes b). Wave w of 4 owns the lag tiles w, w + 4, ..: at most 8 of 16 lags (L <= 512)
__global__ __launch_bounds__(256) void bss_gram_kernel(const float *refs, const float *ests, int M, int64_t n, int64_t stride, int Lp,
                                                        double *part)
{
    __shared__ double sa[kBssGramSub * 16];                     // [sample][plane]: the A operand's 64 values are contiguous
    __shared__ double sb[kBssGramSub + kBssMaxFilter + 16];     // b[m0 .. m0 + sub + Lp)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const int b = blockIdx.y, nlt = Lp >> 4;
    const float *bp = b < M ? refs + (int64_t)b * stride : ests + (int64_t)(b - M) * stride;
    const int64_t c0 = (int64_t)blockIdx.x * kBssGramChunk, c1 = c0 + kBssGramChunk < n ? c0 + kBssGramChunk : n;
    // two levels of accumulators: the MFMA chain runs over the staged samples only and its sum is then added to the chunk's,
    // which keeps the rounding of a sum of 65536 products near that of 256 + 256 (a single chain cost the filters a digit)
    v4d acc[8], tot[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        tot[q] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int64_t m0 = c0; m0 < c1; m0 += kBssGramSub)
    {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
        __syncthreads();
        for (int idx = tid; idx < kBssGramSub * 16; idx += 256)
        {
            const int p = idx / kBssGramSub, s = idx % kBssGramSub;
            const int64_t m = m0 + s;
            sa[s * 16 + p] = p < M && m < c1 ? (double)refs[(int64_t)p * stride + m] : 0.0; // (beyond the chunk: the next one's)
        }
        for (int idx = tid; idx < kBssGramSub + Lp; idx += 256)
        {
            const int64_t m = m0 + idx;
            sb[idx] = m < n ? (double)bp[m] : 0.0;
        }
        __syncthreads();
        for (int s = 0; s < kBssGramSub; s += 4)
        {
            const double a = sa[(s + hi) * 16 + lo];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (wave + 4 * q < nlt)
                    acc[q] = mfma_f64(a, sb[s + hi + (wave + 4 * q) * 16 + lo], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            tot[q] += acc[q];
    }
    double *out = part + ((int64_t)blockIdx.x * 2 * M + b) * 16 * Lp;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (wave + 4 * q < nlt)
            for (int r = 0; r < 4; ++r)
                out[bss_row(lane, r) * Lp + (wave + 4 * q) * 16 + lo] = tot[q][r];
}

// rho = the chunks' partials added in chunk order; the status starts at DMX_BSS_OK
__global__ void bss_gram_sum_kernel(const double *part, int64_t chunks, int64_t count, double *rho, int *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0)
        *status = 0;
    if (i >= count)
        return;
    double s = 0.0;
    for (int64_t c = 0; c < chunks; ++c)
        s += part[c * count + i];
    rho[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------- fill
// grid (ceil(nG / 256), nG rows): G[row][col] for col <= row, and the same value into the source's own block
__global__ void bss_fill_kernel(const double *rho, int C, int L, int Lp, int nG, double *G, double *Gown)
{
    const int row = blockIdx.y, col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col > row)
        return;
    const int p = row / L, t = row % L, p2 = col / L, t2 = col % L, k = t - t2;
    double v = k >= 0 ? rho[((int64_t)p2 * 16 + p) * Lp + k] : rho[((int64_t)p * 16 + p2) * Lp - k];
    if (!bss_kept(rho, p / C, C, Lp) || !bss_kept(rho, p2 / C, C, Lp))
        v = row == col ? 1.0 : 0.0;
    G[(int64_t)row * nG + col] = v;
    if (p / C == p2 / C)
    {
        const int nOwn = C * L, j = p / C;
        Gown[((int64_t)j * nOwn + (row - j * nOwn)) * nOwn + (col - j * nOwn)] = v;
    }
}

// X[row][(i, c'')] = rho_{r_p, e_ic''}(tau), Y the same inside source i's rows and zero elsewhere
__global__ void bss_rhs_kernel(const double *rho, int C, int L, int Lp, int nG, double *X, double *Y)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nG * kBssCols)
        return;
    const int row = idx / kBssCols, col = idx % kBssCols, p = row / L, t = row % L, M = nG / L;
    double v = 0.0;
    if (col < M && bss_kept(rho, p / C, C, Lp) && bss_kept(rho, col / C, C, Lp))
        v = rho[((int64_t)(M + col) * 16 + p) * Lp + t];
    X[idx] = v;
    Y[idx] = col / C == p / C ? v : 0.0;
}

// ------------------------------------------------------------------------------------------------------------ cholesky
// the diagonal block [k0, k0 + nb) of every matrix of the batch, factored in LDS; a pivot that is not finite and positive
// sets the status and the factorisation goes on (to NaN): no index depends on the data
__global__ __launch_bounds__(256) void bss_potrf_kernel(BssBatch bt, int k0, int *status)
{
    __shared__ double s[kBssPanel * (kBssPanel + 1)];
    const BssMat m = bt.m[blockIdx.x];
    if (k0 >= m.n)
        return;
    const int tid = threadIdx.x, nb = m.n - k0 < kBssPanel ? m.n - k0 : kBssPanel, ldS = kBssPanel + 1;
    for (int idx = tid; idx < nb * nb; idx += 256)
    {
        const int r = idx / nb, c = idx % nb;
        if (c <= r)
            s[r * ldS + c] = m.a[(int64_t)(k0 + r) * m.ld + k0 + c];
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j)
    {
        const double piv = s[j * ldS + j];
        if (tid == 0 && !(piv > 0.0 && piv <= DBL_MAX))
            *status = 1;
        const double d = sqrt(piv);
        __syncthreads();
        if (tid == 0)
            s[j * ldS + j] = d;
        for (int r = j + 1 + tid; r < nb; r += 256)
            s[r * ldS + j] /= d;
        __syncthreads();
        const int w = nb - j - 1;
        for (int idx = tid; idx < w * w; idx += 256)
        {
            const int r = j + 1 + idx / w, c = j + 1 + idx % w;
            if (c <= r)
                s[r * ldS + c] -= s[r * ldS + j] * s[c * ldS + j];
        }
        __syncthreads();
    }
    for (int idx = tid; idx < nb * nb; idx += 256)
    {
        const int r = idx / nb, c = idx % nb;
        if (c <= r)
            m.a[(int64_t)(k0 + r) * m.ld + k0 + c] = s[r * ldS + c];
    }
}

// the panel below the diagonal block: x L11^T = a, one row per thread, 64 rows per workgroup. grid (row blocks, batch)
__global__ __launch_bounds__(64) void bss_trsm_kernel(BssBatch bt, int k0)
{
    // (two 64 x 65 blocks: 66 560 bytes of LDS, inside gfx950's 160 KB per workgroup and above the 64 KB of earlier parts)
    __shared__ double s[kBssPanel * (kBssPanel + 1)], x[kBssPanel * (kBssPanel + 1)];
    const BssMat m = bt.m[blockIdx.y];
    const int i0 = k0 + kBssPanel + blockIdx.x * kBssPanel, tid = threadIdx.x, ldS = kBssPanel + 1, nb = kBssPanel;
    if (i0 >= m.n) // (a panel with rows below it is a full one)
        return;
    for (int idx = tid; idx < nb * nb; idx += 64)
    {
        const int r = idx / nb, c = idx % nb;
        if (c <= r)
            s[r * ldS + c] = m.a[(int64_t)(k0 + r) * m.ld + k0 + c];
        x[r * ldS + c] = i0 + r < m.n ? m.a[(int64_t)(i0 + r) * m.ld + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int c = 0; c < nb; ++c)
    {
        double v = x[tid * ldS + c];
        for (int k = 0; k < c; ++k)
            v -= x[tid * ldS + k] * s[c * ldS + k];
        x[tid * ldS + c] = v / s[c * ldS + c];
    }
    __syncthreads();
    for (int idx = tid; idx < nb * nb; idx += 64)
    {
        const int r = idx / nb, c = idx % nb;
        if (i0 + r < m.n)
            m.a[(int64_t)(i0 + r) * m.ld + k0 + c] = x[r * ldS + c];
    }
}

// the trailing update A22 -= L21 L21^T on the lower 64 x 64 tiles: grid (tiles, tiles, batch), a wave per 16 rows x 64 columns
__global__ __launch_bounds__(256) void bss_syrk_kernel(BssBatch bt, int k0)
{
    if (blockIdx.y > blockIdx.x)
        return;
    const BssMat m = bt.m[blockIdx.z];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
    const int base = k0 + kBssPanel, row0 = base + blockIdx.x * 64 + wave * 16, col0 = base + blockIdx.y * 64;
    if (row0 >= m.n)
        return;
    v4d acc[4];
    for (int t = 0; t < 4; ++t)
        acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int kk = 0; kk < kBssPanel; kk += 4)
    {
        const double a = row0 + lo < m.n ? m.a[(int64_t)(row0 + lo) * m.ld + k0 + kk + hi] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
        {
            const int cb = col0 + t * 16 + lo;
            const double b = cb < m.n ? m.a[(int64_t)cb * m.ld + k0 + kk + hi] : 0.0;
            acc[t] = mfma_f64(a, b, acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        for (int r = 0; r < 4; ++r)
        {
            const int row = row0 + bss_row(lane, r), col = col0 + t * 16 + lo;
            if (row < m.n && col <= row)
                m.a[(int64_t)row * m.ld + col] -= acc[t][r];
        }
}

// --------------------------------------------------------------------------------------------------------------- solve
// the diagonal block of a substitution: L11 x = b (forward) or L11^T x = b (back), 16 columns x 16 row lanes
__global__ __launch_bounds__(256) void bss_subst_diag_kernel(BssBatch bt, int k0, int back)
{
    __shared__ double s[kBssPanel * (kBssPanel + 1)], x[kBssPanel * kBssCols];
    const BssMat m = bt.m[blockIdx.x];
    if (k0 >= m.n)
        return;
    const int tid = threadIdx.x, col = tid & 15, rl = tid >> 4, ldS = kBssPanel + 1, nb = m.n - k0 < kBssPanel ? m.n - k0 : kBssPanel;
    for (int idx = tid; idx < nb * nb; idx += 256)
    {
        const int r = idx / nb, c = idx % nb;
        if (c <= r)
            s[r * ldS + c] = m.a[(int64_t)(k0 + r) * m.ld + k0 + c];
    }
    for (int idx = tid; idx < nb * kBssCols; idx += 256)
        x[idx] = m.rhs[(int64_t)k0 * kBssCols + idx];
    for (int step = 0; step < nb; ++step)
    {
        const int q = back ? nb - 1 - step : step;
        __syncthreads();
        if (rl == 0)
            x[q * kBssCols + col] /= s[q * ldS + q];
        __syncthreads();
        const double xq = x[q * kBssCols + col];
        if (back)
            for (int r = rl; r < q; r += 16)
                x[r * kBssCols + col] -= s[q * ldS + r] * xq;
        else
            for (int r = q + 1 + rl; r < nb; r += 16)
                x[r * kBssCols + col] -= s[r * ldS + q] * xq;
    }
    __syncthreads();
    for (int idx = tid; idx < nb * kBssCols; idx += 256)
        m.rhs[(int64_t)k0 * kBssCols + idx] = x[idx];
}

// behind it the other rows: forward, the rows below: b_i -= L[i][k0 ..] x; back, the rows above: b_i -= L[k0 ..][i]^T x.
// grid (row blocks of 64, batch), a wave per 16 rows
__global__ __launch_bounds__(256) void bss_subst_update_kernel(BssBatch bt, int k0, int back)
{
    const BssMat m = bt.m[blockIdx.y];
    if (k0 >= m.n)
        return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
    const int nb = m.n - k0 < kBssPanel ? m.n - k0 : kBssPanel;
    const int row0 = (back ? 0 : k0 + kBssPanel) + blockIdx.x * 64 + wave * 16, end = back ? k0 : m.n;
    if (row0 >= end)
        return;
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
    for (int kk = 0; kk < nb; kk += 4)
    {
        const int q = kk + hi, i = row0 + lo;
        double a = 0.0, b = 0.0;
        if (q < nb)
        {
            if (i < end)
                a = back ? m.a[(int64_t)(k0 + q) * m.ld + i] : m.a[(int64_t)i * m.ld + k0 + q];
            b = m.rhs[(int64_t)(k0 + q) * kBssCols + lo];
        }
        acc = mfma_f64(a, b, acc);
    }
    for (int r = 0; r < 4; ++r)
    {
        const int row = row0 + bss_row(lane, r);
        if (row < end)
            m.rhs[(int64_t)row * kBssCols + lo] -= acc[r];
    }
}

// ------------------------------------------------------------------------------------------------------------- project
// grid (ceil(n / 256), 2): y = 0 p_all from X, y = 1 p_own from Y, the same sums in the same order (so that one source alone
// gives p_all == p_own bit for bit). A wave per 64 output samples; per reference plane the samples [n0 - Lq, n0 + 256) in LDS
__global__ __launch_bounds__(256) void bss_project_kernel(const float *refs, int M, int64_t n, int64_t stride, int L, const double *X,
                                                           const double *Y, double *proj)
{
    __shared__ double sr[kBssProjTile + kBssMaxFilter];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4, Lq = (L + 3) & ~3;
    const double *F = blockIdx.y ? Y : X;
    const int64_t n0 = (int64_t)blockIdx.x * kBssProjTile;
    v4d acc[4];
    for (int q = 0; q < 4; ++q)
        acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int p = 0; p < M; ++p)
    {
        __syncthreads();
        for (int idx = tid; idx < kBssProjTile + Lq; idx += 256)
        {
            const int64_t mm = n0 - Lq + idx;
            sr[idx] = mm >= 0 && mm < n ? (double)refs[(int64_t)p * stride + mm] : 0.0;
        }
        __syncthreads();
        for (int t0 = 0; t0 < Lq; t0 += 4)
        {
            const int tau = t0 + hi;
            const double a = tau < L ? F[((int64_t)p * L + tau) * kBssCols + lo] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[q] = mfma_f64(a, sr[Lq + (wave * 4 + q) * 16 + lo - tau], acc[q]);
        }
    }
    double *out = proj + (int64_t)blockIdx.y * M * n;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int r = 0; r < 4; ++r)
        {
            const int plane = bss_row(lane, r);
            const int64_t mm = n0 + (wave * 4 + q) * 16 + lo;
            if (plane < M && mm < n)
                out[(int64_t)plane * n + mm] = acc[q][r];
        }
}

// ------------------------------------------------------------------------------------------------------------- windows
__device__ inline double bss_db(double num, double den) { return den == 0.0 ? INFINITY : 10.0 * log10(num / den); }

// grid (windows, J). Every thread adds its samples in order, then the 256 partial sums are added by a fixed tree
__global__ __launch_bounds__(256) void bss_window_kernel(const float *refs, const float *ests, int C, int64_t n, int64_t stride, int64_t W,
                                                          int64_t H, int Lp, const double *rho, const double *proj, double *metrics,
                                                          int *flags)
{
    __shared__ double sh[9][256];
    const int tid = threadIdx.x, j = blockIdx.y, J = gridDim.y, M = J * C;
    const int64_t w = blockIdx.x, nwin = gridDim.x, s0 = w * H, len = n < W ? n : W;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < C; ++c)
    {
        const int p = j * C + c;
        const float *r = refs + (int64_t)p * stride + s0, *e = ests + (int64_t)p * stride + s0;
        const double *pa = proj + (int64_t)p * n + s0, *po = proj + ((int64_t)M + p) * n + s0;
        for (int64_t s = tid; s < len; s += 256)
        {
            const double rv = r[s], ev = e[s], av = pa[s], ov = po[s];
            acc[0] += rv * rv;
            acc[1] += (ev - rv) * (ev - rv);
            acc[2] += (ov - rv) * (ov - rv);
            acc[3] += ov * ov;
            acc[4] += (av - ov) * (av - ov);
            acc[5] += av * av;
            acc[6] += (ev - av) * (ev - av);
            acc[7] += rv != 0.0 ? 1.0 : 0.0;
            acc[8] += ev != 0.0 ? 1.0 : 0.0;
        }
    }
    for (int k = 0; k < 9; ++k)
        sh[k][tid] = acc[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1)
    {
        if (tid < h)
            for (int k = 0; k < 9; ++k)
                sh[k][tid] += sh[k][tid + h];
        __syncthreads();
    }
    if (tid != 0)
        return;
    const bool kept = bss_kept(rho, j, C, Lp);
    const int64_t at = (int64_t)j * nwin + w, plane = (int64_t)J * nwin;
    flags[at] = kept && (sh[7][0] == 0.0 || sh[8][0] == 0.0);
    metrics[at] = kept ? bss_db(sh[0][0], sh[1][0]) : NAN;
    metrics[plane + at] = kept ? bss_db(sh[0][0], sh[2][0]) : NAN;
    metrics[2 * plane + at] = kept ? bss_db(sh[3][0], sh[4][0]) : NAN;
    metrics[3 * plane + at] = kept ? bss_db(sh[5][0], sh[6][0]) : NAN;
}

// the silence rule (one silent kept reference or estimate empties the window for every source) and the failed factorisation
__global__ void bss_finish_kernel(int J, int64_t nwin, const int *flags, const int *status, double *metrics)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwin)
        return;
    bool none = *status != 0;
    for (int j = 0; j < J; ++j)
        none = none || flags[(int64_t)j * nwin + w] != 0;
    if (none)
        for (int k = 0; k < 4 * J; ++k)
            metrics[(int64_t)k * nwin + w] = NAN;
}

// filters[i][row][c''] = X[row][(i, c'')]
__global__ void bss_filters_kernel(const double *X, int J, int C, int nG, double *filters)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)J * nG * C)
        return;
    const int c = idx % C, row = (idx / C) % nG, i = idx / ((int64_t)C * nG);
    filters[idx] = X[(int64_t)row * kBssCols + i * C + c];
}
} // namespace

void launch_bss(const BssJob &job, hipStream_t s, hipEvent_t *marks)
{
    const BssLayout l = bss_layout(job.J, job.C, job.n, job.L);
    unsigned char *w = job.work;
    double *part = (double *)(w + l.part), *rho = (double *)(w + l.rho), *G = (double *)(w + l.G), *Gown = (double *)(w + l.Gown);
    double *X = (double *)(w + l.X), *Y = (double *)(w + l.Y), *proj = (double *)(w + l.proj);
    int *flags = (int *)(w + l.flags);
    const int64_t nwin = bss_windows(job.n, job.window, job.hop), corr = (int64_t)2 * l.M * 16 * l.Lp;
    Marks mark{marks, s};
    mark();
    bss_gram_kernel<<<dim3((unsigned)l.chunks, 2 * l.M), 256, 0, s>>>(job.refs, job.ests, l.M, job.n, job.stride, l.Lp, part);
    bss_gram_sum_kernel<<<(unsigned)((corr + 255) / 256), 256, 0, s>>>(part, l.chunks, corr, rho, job.status);
    mark();
    bss_fill_kernel<<<dim3((l.nG + 255) / 256, l.nG), 256, 0, s>>>(rho, job.C, job.L, l.Lp, l.nG, G, Gown);
    bss_rhs_kernel<<<(l.nG * kBssCols + 255) / 256, 256, 0, s>>>(rho, job.C, job.L, l.Lp, l.nG, X, Y);
    mark();
    BssBatch bt{};
    bt.m[0] = BssMat{G, X, l.nG, l.nG};
    for (int j = 0; j < job.J; ++j)
        bt.m[1 + j] = BssMat{Gown + (int64_t)j * l.nOwn * l.nOwn, Y + (int64_t)j * l.nOwn * kBssCols, l.nOwn, l.nOwn};
    const int batch = 1 + job.J, panels = (l.nG + kBssPanel - 1) / kBssPanel;
    for (int k = 0; k < panels; ++k)
    {
        const int k0 = k * kBssPanel, below = l.nG - k0 - kBssPanel, tiles = (below + 63) / 64;
        bss_potrf_kernel<<<batch, 256, 0, s>>>(bt, k0, job.status);
        if (below > 0)
        {
            bss_trsm_kernel<<<dim3(tiles, batch), 64, 0, s>>>(bt, k0);
            bss_syrk_kernel<<<dim3(tiles, tiles, batch), 256, 0, s>>>(bt, k0);
        }
    }
    mark();
    for (int k = 0; k < panels; ++k)
    {
        const int k0 = k * kBssPanel, below = l.nG - k0 - kBssPanel;
        bss_subst_diag_kernel<<<batch, 256, 0, s>>>(bt, k0, 0);
        if (below > 0)
            bss_subst_update_kernel<<<dim3((below + 63) / 64, batch), 256, 0, s>>>(bt, k0, 0);
    }
    for (int k = panels - 1; k >= 0; --k)
    {
        const int k0 = k * kBssPanel;
        bss_subst_diag_kernel<<<batch, 256, 0, s>>>(bt, k0, 1);
        if (k0 > 0)
            bss_subst_update_kernel<<<dim3(k0 / 64, batch), 256, 0, s>>>(bt, k0, 1);
    }
    mark();
    bss_project_kernel<<<dim3((unsigned)((job.n + kBssProjTile - 1) / kBssProjTile), 2), 256, 0, s>>>(job.refs, l.M, job.n, job.stride, job.L,
                                                                                                      X, Y, proj);
    mark();
    bss_window_kernel<<<dim3((unsigned)nwin, job.J), 256, 0, s>>>(job.refs, job.ests, job.C, job.n, job.stride, job.window, job.hop, l.Lp, rho,
                                                                 proj, job.metrics, flags);
    bss_finish_kernel<<<(unsigned)((nwin + 255) / 256), 256, 0, s>>>(job.J, nwin, flags, job.status, job.metrics);
    if (job.filters)
        bss_filters_kernel<<<(unsigned)(((int64_t)job.J * l.nG * job.C + 255) / 256), 256, 0, s>>>(X, job.J, job.C, l.nG, job.filters);
    mark();
}
} // namespace dmx
