// cpu_interp.cpp — TEST-ONLY CPU interpreter of the execution plan (demucs_cpp_amd/csrc/plan.h).
//
// Purpose: validate, in the build container (no GPU), the host-side half of the product
// - weight repacking (model_pack.cpp) and the op list / descriptors (plan.cpp) - against
// the oracle, and serve as the executable specification of every op the HIP kernels
// implement. It is NOT part of the product: nothing under demucs_cpp_amd/ or cli/ links
// it, and the product fails loudly without a GPU.
//
// Every op is ONE template over its arithmetic T:
//   T = float : the fp32 arithmetic the interpreter always had (interp_run*, interp_step mode 0), bit for bit;
//   T = P     : the same op on the same fp32 inputs evaluated in double (interp_step mode 1). A P carries the value v and a
//               magnitude m >= |v|: the sum of the absolute values of the terms added to form it (a GEMM output: sum |a_k w_k| +
//               |bias| (+ |res|)), carried through products and quotients to first order (|a| m_b + |b| m_a - |a b|) and through
//               the non-linear functions by their local Lipschitz constants. An fp32 evaluation that makes c roundings on the longest path to an element is within
//               c 2^-24 m of v: the bound tests/test_gpu_op_parity.py holds each HIP kernel to.
#include "../demucs_cpp_amd/csrc/model_pack.cpp"
#include "../demucs_cpp_amd/csrc/plan.cpp"
#include "../demucs_cpp_amd/csrc/gemm_select.cpp"
#include "../demucs_cpp_amd/csrc/plan_describe.h"

#include <atomic>
#include <complex>
#include <type_traits>

using namespace dmx;

namespace
{
struct P
{
    double v, m;
    P() : v(0), m(0) {}
    P(double x) : v(x), m(std::fabs(x)) {}
    P(double x, double mm) : v(x), m(mm) {}
};
inline P operator+(P a, P b) { return P(a.v + b.v, a.m + b.m); }
inline P operator-(P a, P b) { return P(a.v - b.v, a.m + b.m); }
inline P operator-(P a) { return P(-a.v, a.m); }
// first order: (|a| + ea)(|b| + eb) without the ea eb term, which is second order in the roundings and, carried through a chain
// of normalisations or a recurrence, would grow until the magnitude bounds nothing. Exact for operands that are plain numbers
inline P operator*(P a, P b) { return P(a.v * b.v, std::fabs(a.v) * b.m + std::fabs(b.v) * a.m - std::fabs(a.v * b.v)); }
inline P operator/(P a, P b)
{
    const double q = a.v / b.v, ab = std::fabs(b.v);
    return P(q, a.m / ab + std::fabs(q) * (b.m - ab) / ab);
}
inline P &operator+=(P &a, P b) { return a = a + b; }
inline P &operator*=(P &a, P b) { return a = a * b; }
inline P &operator/=(P &a, P b) { return a = a / b; }
inline bool operator<(P a, P b) { return a.v < b.v; }

// ---- the census (interp_census): how many evaluations of the LAST precise step fell into each value class. Filled by the P
// overloads of gelu / sigmoidf / tanh_ and by the statistics code in its precise form only; the fp32 arithmetic never looks at it.
// Classes (tests/op_reference.py CENSUS names them in this order):
//   GELU by z = v / sqrt 2, the argument of the device's dmx_erff (kernels.h): sign x {|z| < 0.92, 0.92 <= |z| < 4, |z| >= 4}, and
//     |z| within 2^-10 relative of 0.92, below and above;
//   sigmoid by its argument v: sign x {|v| < 2^-10, < 1, < 9, < 17, < 89, >= 89};  tanh: sign x {|v| < 2^-10, < 1, < 9, >= 9};
//   statistics, per row / group / record formed: all, zero (every element 0), constant (variance 0, mean != 0), |mean| / sigma
//     {< 1, < 64, >= 64}, sigma {< 2^-10, < 2^6, >= 2^6}, "clamped" (the one-pass form q - n mean^2 the device evaluates in double
//     is negative), spike (one element carries more than half of the squared deviations);
//   LSTM cell states with |c| >= 8; the largest number of non-zero operand elements in one GEMM row (a maximum, not a count).
enum
{
    CEN_GELU = 0,
    CEN_SIG = 8,
    CEN_TANH = 20,
    CEN_STAT = 28,
    CEN_C8 = 39,
    CEN_KNZ = 40,
    CEN_N = 41
};
enum
{
    ST_ALL,
    ST_ZERO,
    ST_CONST,
    ST_R0,
    ST_R8,
    ST_R512,
    ST_SIG_SMALL,
    ST_SIG_MID,
    ST_SIG_BIG,
    ST_CLAMPED,
    ST_SPIKE
};
std::atomic<long long> g_census[CEN_N];
inline void census(int k) { g_census[k].fetch_add(1, std::memory_order_relaxed); }
inline void census_gelu(double v)
{
    const double z = std::fabs(v) * std::sqrt(0.5), e = 0.92 * std::ldexp(1.0, -10);
    census(CEN_GELU + (v < 0 ? 0 : 3) + (z < 0.92 ? 0 : z < 4.0 ? 1 : 2));
    if (z >= 0.92 - e && z < 0.92)
        census(CEN_GELU + 6);
    if (z >= 0.92 && z <= 0.92 + e)
        census(CEN_GELU + 7);
}
inline void census_sig(double v)
{
    const double a = std::fabs(v);
    census(CEN_SIG + (v < 0 ? 0 : 6) + (a < std::ldexp(1.0, -10) ? 0 : a < 1 ? 1 : a < 9 ? 2 : a < 17 ? 3 : a < 89 ? 4 : 5));
}
inline void census_tanh(double v)
{
    const double a = std::fabs(v);
    census(CEN_TANH + (v < 0 ? 0 : 4) + (a < std::ldexp(1.0, -10) ? 0 : a < 1 ? 1 : a < 9 ? 2 : 3));
}
// one set of statistics: n values of sum s and sum of squares q (plain doubles, as the device's one-pass form has them), the
// variance the reference formed, the largest squared deviation (< 0: not known, the elements were not seen)
inline void census_stat(double n, double s, double q, double var, double maxdev2)
{
    const double mean = s / n, sd = std::sqrt(var);
    census(CEN_STAT + ST_ALL);
    if (q == 0)
        census(CEN_STAT + ST_ZERO);
    else if (var == 0)
        census(CEN_STAT + ST_CONST);
    else
    {
        const double ratio = std::fabs(mean) / sd;
        census(CEN_STAT + (ratio < 1 ? ST_R0 : ratio < 64 ? ST_R8 : ST_R512));
        census(CEN_STAT + (sd < std::ldexp(1.0, -10) ? ST_SIG_SMALL : sd < 64 ? ST_SIG_MID : ST_SIG_BIG));
        if (maxdev2 > 0.5 * var * (n - 1.0))
            census(CEN_STAT + ST_SPIKE);
    }
    if (q - n * mean * mean < 0)
        census(CEN_STAT + ST_CLAMPED);
}
// ... of rows x cols fp32 elements (leading dimension ld) whose variance the reference formed as var
inline void census_elements(const float *x, int cols, int rows, i64 ld, double n, double var)
{
    double s = 0, q = 0, far = 0;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            s += (double)x[r * ld + c], q += (double)x[r * ld + c] * (double)x[r * ld + c];
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            far = std::max(far, ((double)x[r * ld + c] - s / n) * ((double)x[r * ld + c] - s / n));
    census_stat(n, s, q, var, far);
}

inline float gelu(float v) { return 0.5f * v * (1.0f + std::erf(v / std::sqrt(2.0f))); }
inline float sigmoidf(float v) { return 1.0f / (1.0f + std::exp(-v)); }
inline float exp_(float v) { return std::exp(v); }
inline float tanh_(float v) { return std::tanh(v); }
inline double sqrt_(double v) { return std::sqrt(v); }
inline float fma_(float a, float b, float c) { return std::fmaf(a, b, c); }
inline float max_(float a, float b) { return std::max(a, b); }
inline double max_(double a, double b) { return std::max(a, b); }
// |gelu'| <= 1.13, |sigmoid'| <= 1 / 4, |tanh'| <= 1, exp' = exp, sqrt' = 1 / (2 sqrt)
inline P gelu(P x)
{
    census_gelu(x.v);
    const double f = 0.5 * x.v * (1.0 + std::erf(x.v / std::sqrt(2.0)));
    return P(f, std::fabs(f) + 1.13 * x.m);
}
inline P sigmoidf(P x)
{
    census_sig(x.v);
    const double f = 1.0 / (1.0 + std::exp(-x.v));
    return P(f, f + 0.25 * x.m);
}
inline P exp_(P x)
{
    const double f = std::exp(x.v);
    return P(f, f * (1.0 + x.m));
}
// (tanh is the LSTM's only: the device evaluates it as 2 sigmoid(2 v) - 1 (v3.hip lstm_tanh), whose error is a few u of ONE whatever
// |v| - the "< 2e-7 absolute" its header states. The magnitude therefore carries 1, not |tanh v|)
inline P tanh_(P x)
{
    census_tanh(x.v);
    const double f = std::tanh(x.v);
    return P(f, 1.0 + x.m);
}
inline P sqrt_(P x)
{
    const double f = std::sqrt(x.v);
    return P(f, f + (f > 0 ? 0.5 * x.m / f : 0.0));
}
inline double num(double x) { return x; }
inline double num(P x) { return x.v; }
inline P fma_(P a, P b, P c) { return a * b + c; }
inline P max_(P a, P b) { return a.v < b.v ? b : a; }

// W: the type of the sums the fp32 arithmetic keeps in double; rf: a double result rounded to the arithmetic; wd: widened;
// val: the plain number
template <class T>
struct Tr;
template <>
struct Tr<float>
{
    typedef double W;
    static float rf(double x) { return (float)x; }
    static double wd(float x) { return (double)x; }
    static double val(float x) { return (double)x; }
    static double mag(float x) { return std::fabs((double)x); }
    static float mk(double v, double) { return (float)v; }
    static float rebase(float x) { return x; }
};
template <>
struct Tr<P>
{
    typedef P W;
    static P rf(P x) { return x; }
    static P wd(P x) { return x; }
    static double val(P x) { return x.v; }
    static double mag(P x) { return x.m; }
    static P mk(double v, double m) { return P(v, m); }
    static P rebase(P x) { return P(x.v); } // a state taken as a number of its own: its magnitude starts again at |v|
};

// GroupNorm statistics INSIDE an op (OP_DCONV_ROW) of the values with sums s, q in the wide type: mean and 1 / sqrt(var + eps).
// fp32 arithmetic: the one-pass formula in double, rounded (what the interpreter always did). Precise: the same two numbers, taken
// as numbers of their own (magnitude |v|), exactly as the unfused chain K1 / r1 / K2 / r2 / K3 takes them: there the statistics
// reach the next op as fp32 arena values. The device forms them in double, so their own rounding is one fp32 rounding; what the
// errors of the values do to them is an AVERAGE over >= 100 independent roundings, while carrying magnitudes through
// q - n mean^2 (or its worst-case perturbation) multiplies the bound by the conditioning at every normalisation until it bounds
// nothing (measured: s / |r| of 1e5 and more). The RMS rule of tests/test_gpu_op_parity.py holds the op to what fp32 really gives.
inline void inner_stats(double s, double q, double cnt, float eps, float &mean, float &rstd)
{
    const double m = s / cnt, var = std::max((q - cnt * m * m) / (cnt - 1.0), 0.0);
    mean = (float)m, rstd = (float)(1.0 / std::sqrt(var + (double)eps));
}
inline void inner_stats(P s, P q, double cnt, float eps, P &mean, P &rstd)
{
    const double m = s.v / cnt, var = std::max((q.v - cnt * m * m) / (cnt - 1.0), 0.0);
    census_stat(cnt, s.v, q.v, var, -1.0);
    mean = P(m), rstd = P(1.0 / std::sqrt(var + (double)eps));
}

void fft(std::vector<std::complex<double>> &a, int sign)
{
    int n = (int)a.size();
    for (int i = 1, j = 0; i < n; ++i)
    {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1)
            j ^= bit;
        j ^= bit;
        if (i < j)
            std::swap(a[i], a[j]);
    }
    for (int len = 2; len <= n; len <<= 1)
    {
        double ang = sign * 2.0 * M_PI / len;
        std::complex<double> wl(cos(ang), sin(ang));
        for (int i = 0; i < n; i += len)
        {
            std::complex<double> w(1, 0);
            for (int k = 0; k < len / 2; ++k)
            {
                auto u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
                w *= wl;
            }
        }
    }
}

// round-to-nearest-even bf16 of a finite float, and the three-term split of igemm_common.h split3_pk
inline unsigned short bf16_rn(float x)
{
    unsigned u;
    std::memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
inline float bf16_f(unsigned short h)
{
    unsigned u = (unsigned)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
inline void split3(float x, unsigned short h[3])
{
    h[0] = bf16_rn(x);
    const float r = x - bf16_f(h[0]);
    h[1] = bf16_rn(r);
    const float s = r - bf16_f(h[1]);
    h[2] = bf16_rn(s);
}

struct Interp
{
    PackedModel pm;
    Plan pl;
    std::vector<float> A;
    const float *W;
    std::vector<i64> notFp16; // interp_select_dump: blob offsets of the weights that are not fp16 numbers (filled on first use)
    bool scanned = false;
    // ---- the step interface (interp_step): what the last step wrote, and in the precise arithmetic its unrounded results
    std::vector<unsigned char> mask; // [arenaFloats] 1 = written by the last step (empty: whole-plan runs keep no record)
    std::vector<double> R;           // [arenaFloats] precise result before its one rounding to fp32
    std::vector<float> S;            // [arenaFloats] its magnitude
    std::vector<double> kvR;         // K / V operand planes of the last step (EPI_KPL / EPI_VT): the value whose exact split the
    std::vector<float> kvS;          // planes hold, and its magnitude, indexed like the elements of plane 0
    bool hterms = false;             // the step's GEMM runs on fp16 terms under a per-row scale: the mode's documented allowance
                                     // (2^-39 of the row maximum per dropped remainder, one per k) joins the magnitude
    bool chained = false;            // the step's OP_OLA takes the frames of the OP_ISTFT before it unrounded (the fused GPU kernel)

    void st(i64 off, float v)
    {
        A[(size_t)off] = v;
        if (!mask.empty())
            mask[(size_t)off] = 1;
    }
    void st(i64 off, P v)
    {
        A[(size_t)off] = (float)v.v;
        mask[(size_t)off] = 1, R[(size_t)off] = v.v, S[(size_t)off] = (float)std::min(v.m, 3e38);
    }
    // the bf16 element e of the plane area at float offset kv
    void st_bf16(i64 kv, i64 e, unsigned short h)
    {
        reinterpret_cast<unsigned short *>(&A[(size_t)kv])[e] = h;
        if (!mask.empty())
            mask[(size_t)(kv + e / 2)] = 1;
    }
    float ld_bf16(i64 kv, i64 e) const { return bf16_f(reinterpret_cast<const unsigned short *>(&A[(size_t)kv])[e]); }

    template <class T>
    void run_igemm(const IGemm &g)
    {
        const i64 M = (i64)g.B * g.P1 * g.P0;
        const int BN = kTileCfgs[g.cfg].BN;
        const bool paired = g.epi == EPI_GLU || g.epi == EPI_GN_GLU_SCALE_RES;
        const bool planes = g.epi == EPI_KPL || g.epi == EPI_VT;
        const bool precise = !std::is_same<T, float>::value;
        const i64 rowLen = (i64)g.L0 * g.Cin;
        const i64 kvPlane = (i64)g.B * g.kvT * g.kvH * g.kvHs;
        std::vector<double> wabs; // sum_k |w[n][k]| (fp16-term allowance)
        if (precise && hterms)
        {
            wabs.assign((size_t)g.N, 0.0);
            for (int n = 0; n < g.N; ++n)
                for (int k = 0; k < g.K; ++k)
                    wabs[(size_t)n] += std::fabs((double)W[g.w_w + (i64)n * g.Kp + k]);
        }
        if (precise && planes)
            kvR.assign((size_t)kvPlane, 0.0), kvS.assign((size_t)kvPlane, 0.f);
#pragma omp parallel for schedule(static)
        for (i64 m = 0; m < M; ++m)
        {
            int p0 = (int)(m % g.P0), p1 = (int)((m / g.P0) % g.P1), bb = (int)(m / ((i64)g.P0 * g.P1));
            int grp = bb * g.G0 + (g.G0 > 1 ? p0 : 0);
            std::vector<T> arow((size_t)g.K);
            double rowmax = 0;
            long long knz = 0;
            for (int k = 0; k < g.K; ++k)
            {
                int s1 = k / g.seg0, off = k % g.seg0;
                int in1 = p1 * g.stride1 + s1 * g.dil1 - g.pad1;
                i64 e = (i64)(p0 * g.stride0 - g.pad0) * g.Cin + off;
                T a = 0.f;
                if (in1 >= 0 && in1 < g.L1 && e >= 0 && e < rowLen)
                {
                    a = A[(size_t)(g.x + bb * g.xBatchStride + (i64)in1 * rowLen + e)];
                    if (g.pro == PRO_AFFINE)
                    {
                        const float *st = &A[(size_t)(g.proStats + (i64)bb * 4)];
                        a = (a - st[0]) * st[1];
                    }
                    else if (g.pro == PRO_GN_GELU)
                    {
                        const float *st = &A[(size_t)(g.proStats + (i64)grp * 4)];
                        a = gelu((a - st[0]) * st[1] * W[g.proW_w + k] + W[g.proB_w + k]);
                    }
                }
                arow[(size_t)k] = a;
                rowmax = std::max(rowmax, std::fabs(Tr<T>::val(a)));
                knz += Tr<T>::val(a) != 0;
            }
            if (precise)
            {
                long long seen = g_census[CEN_KNZ].load(std::memory_order_relaxed);
                while (seen < knz && !g_census[CEN_KNZ].compare_exchange_weak(seen, knz, std::memory_order_relaxed))
                    ;
            }
            std::vector<T> v((size_t)g.N);
            for (int n = 0; n < g.N; ++n)
            {
                const float *wr = W + g.w_w + (i64)n * g.Kp;
                T acc = 0.f;
                for (int k = 0; k < g.K; ++k)
                    acc += arow[(size_t)k] * wr[k];
                v[(size_t)n] = acc + W[g.bias_w + n];
                if (precise && hterms)
                    v[(size_t)n] = Tr<T>::mk(Tr<T>::val(v[(size_t)n]), Tr<T>::mag(v[(size_t)n]) + std::ldexp(rowmax * wabs[(size_t)n], -15));
            }
            const i64 yrow = g.y + bb * g.yBatchStride + ((i64)p1 * g.P0 + p0) * g.ldy;
            if (g.epi == EPI_LINEAR)
            {
                for (int n = 0; n < g.N; ++n)
                {
                    T t = v[(size_t)n];
                    if (g.act)
                        t = gelu(t);
                    if (g.res >= 0)
                        t += A[(size_t)(g.res + (yrow - g.y) + n)];
                    v[(size_t)n] = t;
                    st(yrow + n, t);
                }
            }
            else if (g.epi == EPI_SCALE_RES)
            {
                for (int n = 0; n < g.N; ++n)
                {
                    T t = A[(size_t)(g.res + (yrow - g.y) + n)] + v[(size_t)n] * W[g.scale_w + n];
                    v[(size_t)n] = t;
                    st(yrow + n, t);
                }
            }
            else if (paired)
            {
                int C = g.N / 2;
                const float *st4 = g.epi == EPI_GN_GLU_SCALE_RES ? &A[(size_t)(g.epiStats + (i64)grp * 4)] : nullptr;
                for (int c = 0; c < C; ++c)
                {
                    int na = (c / 16) * 32 + (c % 16), nb = na + 16;
                    T a = v[(size_t)na], bq = v[(size_t)nb];
                    if (st4)
                    {
                        a = (a - st4[0]) * st4[1] * W[g.epiW_w + na] + W[g.epiB_w + na];
                        bq = (bq - st4[0]) * st4[1] * W[g.epiW_w + nb] + W[g.epiB_w + nb];
                    }
                    T t = a * sigmoidf(bq);
                    if (g.epi == EPI_GN_GLU_SCALE_RES)
                        t = A[(size_t)(g.res + (yrow - g.y) + c)] + W[g.scale_w + c] * t;
                    else if (g.table_w >= 0)
                        t += g.tableScale * W[g.table_w + (i64)p0 * C + c];
                    st(yrow + c, t);
                }
            }
            else if (g.epi == EPI_TRCONV)
            {
                for (int n = 0; n < g.N; ++n)
                {
                    int r = n / g.Cout, co = n % g.Cout;
                    int j = g.trS * p0 + r - g.trOff;
                    if (j < 0 || j >= g.Lout)
                        continue;
                    T t = v[(size_t)n];
                    if (g.act)
                        t = gelu(t);
                    i64 o = bb * g.yBatchStride + ((i64)p1 * g.Lout + j) * g.ldy + co;
                    if (g.res >= 0)
                        t += A[(size_t)(g.res + o)];
                    st(g.y + o, t);
                }
            }
            else if (planes)
            {
                // rows are tokens m = b kvT + t. EPI_KPL: columns below kvCol0 fp32 [row][n]; from kvCol0 on plane element
                // m (kvH kvHs) + n - kvCol0. EPI_VT (kvCol0 = 0): the V^T tile image of attention_split.hip, element
                // (((b kvH + head) nt + t / 64) kvHs + dim) 64 + 8 slot + 4 half + t % 4 with, for tt = t % 64,
                // slot = 4 (tt / 32) + (tt / 4) % 4, half = (tt / 16) % 2 (igemm_common.h igemm_epilogue)
                const int b = (int)(m / g.kvT), t = (int)(m % g.kvT), nt = g.kvT / 64;
                for (int n = 0; n < g.N; ++n)
                {
                    if (g.epi == EPI_KPL && n < g.kvCol0)
                    {
                        st(yrow + n, v[(size_t)n]);
                        continue;
                    }
                    i64 e;
                    if (g.epi == EPI_KPL)
                        e = m * (i64)(g.kvH * g.kvHs) + (n - g.kvCol0);
                    else
                    {
                        const int head = n / g.kvHs, dim = n % g.kvHs, tt = t & 63;
                        const int slot = 4 * (tt >> 5) + ((tt >> 2) & 3), half = (tt >> 4) & 1;
                        e = ((((i64)b * g.kvH + head) * nt + (t >> 6)) * g.kvHs + dim) * 64 + slot * 8 + half * 4 + (tt & 3);
                    }
                    unsigned short h[3];
                    split3((float)Tr<T>::val(v[(size_t)n]), h);
                    for (int q = 0; q < 3; ++q)
                        st_bf16(g.kv, q * kvPlane + e, h[q]);
                    if (precise)
                        kvR[(size_t)e] = Tr<T>::val(v[(size_t)n]), kvS[(size_t)e] = (float)Tr<T>::mag(v[(size_t)n]);
                }
            }
            if (g.rowstat >= 0)
                for (int nb = 0; nb < g.NB; ++nb)
                {
                    T s = 0.f, ss = 0.f;
                    for (int n = nb * BN; n < std::min(g.N, (nb + 1) * BN); ++n)
                    {
                        if (g.epi == EPI_STATS_FACT) // factorised statistics: roles of the columns, plan.h
                        {
                            if (n < g.Cout)
                                ss += v[(size_t)n] * v[(size_t)n];
                            else if (n == g.Cout)
                                s += v[(size_t)n];
                            else if (n == g.Cout + 1)
                                ss += 2.0f * v[(size_t)n];
                            continue;
                        }
                        s += v[(size_t)n];
                        ss += v[(size_t)n] * v[(size_t)n];
                    }
                    st(g.rowstat + (m * g.NB + nb) * 2, s);
                    st(g.rowstat + (m * g.NB + nb) * 2 + 1, ss);
                }
        }
    }

    template <class T>
    void run_reduce(const StatsReduce &s)
    {
        typedef typename Tr<T>::W Wd;
        int G = s.G0 > 1 ? s.G0 : 1;
        for (int b = 0; b < s.B; ++b)
            for (int gi = 0; gi < G; ++gi)
            {
                Wd sum = 0, sq = 0;
                for (int r = gi; r < s.R; r += G)
                    for (int nb = 0; nb < s.NB; ++nb)
                    {
                        const float *p = &A[(size_t)(s.rowstat + (((i64)b * s.R + r) * s.NB + nb) * 2)];
                        sum += p[0];
                        sq += p[1];
                    }
                Wd mean = sum / s.count;
                Wd var = (sq - s.count * mean * mean) / (s.count - 1.0);
                if (var < Wd(0))
                    var = 0;
                if (!std::is_same<T, float>::value)
                    census_stat(s.count, num(sum), num(sq), num(var), -1.0);
                const i64 o = s.out + ((i64)b * G + gi) * 4;
                st(o, Tr<T>::rf(mean));
                st(o + 2, Tr<T>::rf(sqrt_(var)));
                st(o + 1, s.mode == MODE_RSTD ? Tr<T>::rf(1.0 / sqrt_(var + (double)s.eps)) : Tr<T>::rf(1.0 / (sqrt_(var) + (double)s.eps)));
                st(o + 3, T(0.f));
            }
    }

    template <class T>
    void run_stft(const Stft &s)
    {
        typedef typename Tr<T>::W Wd;
        const float *win = &A[(size_t)s.window];
        for (int b = 0; b < s.B; ++b)
            for (int t = 0; t < s.T; ++t)
            {
                Wd sum = 0, sq = 0, sumT = 0, sqT = 0;
                for (int ch = 0; ch < 2; ++ch)
                {
                    std::vector<std::complex<double>> buf(4096);
                    double l1 = 0; // sum of the absolute values of the terms of every bin
                    for (int i = 0; i < 4096; ++i)
                    {
                        // model-level symmetric padding (Q2), model_inference.cpp:22-46; reference
                        // frame t+2 starts at padded sample t*1024 (see DESIGN.md STFT note)
                        i64 j = (i64)t * 1024 + i - s.pad;
                        if (j < 0)
                            j = -1 - j;
                        if (j >= s.seg)
                            j = 2 * (i64)s.seg - 1 - j;
                        T x = A[(size_t)(s.mix + ((i64)b * s.seg + j) * 2 + ch)];
                        buf[i] = Tr<T>::val(x * win[i]);
                        l1 += std::fabs(buf[i].real());
                    }
                    fft(buf, -1);
                    for (int f = 0; f < 2048; ++f)
                    {
                        T re = Tr<T>::mk(buf[f].real() / 64.0, l1 / 64.0), im = Tr<T>::mk(buf[f].imag() / 64.0, l1 / 64.0);
                        const i64 o = s.x + (((i64)b * s.T + t) * 2048 + f) * 4 + 2 * ch;
                        st(o, re), st(o + 1, im);
                        sum += re + im;
                        sq += Tr<T>::wd(re) * re + Tr<T>::wd(im) * im;
                    }
                    for (i64 j = (i64)t * 1024; j < std::min((i64)s.seg, (i64)(t + 1) * 1024); ++j)
                    {
                        T x = A[(size_t)(s.mix + ((i64)b * s.seg + j) * 2 + ch)];
                        sumT += x;
                        sqT += Tr<T>::wd(x) * x;
                    }
                }
                st(s.rowstat + ((i64)b * s.T + t) * 2, Tr<T>::rf(sum));
                st(s.rowstat + ((i64)b * s.T + t) * 2 + 1, Tr<T>::rf(sq));
                st(s.rowstatT + ((i64)b * s.T + t) * 2, Tr<T>::rf(sumT));
                st(s.rowstatT + ((i64)b * s.T + t) * 2 + 1, Tr<T>::rf(sqT));
            }
    }

    template <class T>
    void run_ln(const LayerNorm &l)
    {
        typedef typename Tr<T>::W Wd;
#pragma omp parallel for schedule(static)
        for (int r = 0; r < l.rows; ++r)
        {
            const float *x = &A[(size_t)(l.x + (i64)r * l.D)];
            Wd s = 0;
            for (int c = 0; c < l.D; ++c)
                s += x[c];
            T mean = Tr<T>::rf(s / l.D);
            Wd ss = 0;
            for (int c = 0; c < l.D; ++c)
                ss += (Tr<T>::wd(x[c]) - mean) * (Tr<T>::wd(x[c]) - mean);
            T rstd = Tr<T>::rf(1.0 / sqrt_(ss / (l.D - 1) + (double)l.eps));
            if (!std::is_same<T, float>::value)
                census_elements(x, l.D, 1, l.D, l.D, num(ss) / (l.D - 1));
            std::vector<T> tmp((size_t)l.D);
            for (int c = 0; c < l.D; ++c)
            {
                T v = (x[c] - mean) * rstd * W[l.w_w + c] + W[l.b_w + c];
                if (l.pe >= 0)
                    v += A[(size_t)(l.pe + (i64)(r % l.rowsPerBatch) * l.D + c)];
                tmp[(size_t)c] = v;
            }
            for (int c = 0; c < l.D; ++c)
                st(l.y + (i64)r * l.D + c, tmp[(size_t)c]);
        }
    }

    template <class T>
    void run_gn(const GnApply &g)
    {
        for (int b = 0; b < g.B; ++b)
            for (i64 i = 0; i < (i64)g.rows * g.C; ++i)
            {
                i64 o = (i64)b * g.rows * g.C + i;
                T v = A[(size_t)(g.x + o)];
                if (g.stats >= 0)
                {
                    const float *st4 = &A[(size_t)(g.stats + (i64)b * 4)];
                    int c = (int)(i % g.C);
                    v = (v - st4[0]) * st4[1] * W[g.w_w + c] + W[g.b_w + c];
                }
                if (g.res >= 0)
                    v += A[(size_t)(g.res + o)];
                st(g.y + o, v);
            }
    }

    // K / V as the attention kernel sees them: fp32 rows, or the sum of the three bf16 planes (= the projected fp32 value: the
    // split is exact; EPI_KPL / EPI_VT layouts as in run_igemm)
    float attn_k(const Attention &a, int b, int s, int c) const
    {
        if (a.kpl < 0)
            return A[(size_t)(a.k + b * a.kBatch + (i64)s * a.ldk + c)];
        const i64 plane = (i64)a.B * a.Tk * a.H * a.hs, e = ((i64)b * a.Tk + s) * (a.H * a.hs) + c;
        return ld_bf16(a.kpl, e) + ld_bf16(a.kpl, plane + e) + ld_bf16(a.kpl, 2 * plane + e);
    }
    float attn_v(const Attention &a, int b, int s, int c) const
    {
        if (a.vt < 0)
            return A[(size_t)(a.v + b * a.vBatch + (i64)s * a.ldv + c)];
        const i64 plane = (i64)a.B * a.Tk * a.H * a.hs;
        const int head = c / a.hs, dim = c % a.hs, tt = s & 63, nt = a.Tk / 64;
        const int slot = 4 * (tt >> 5) + ((tt >> 2) & 3), half = (tt >> 4) & 1;
        const i64 e = ((((i64)b * a.H + head) * nt + (s >> 6)) * a.hs + dim) * 64 + slot * 8 + half * 4 + (tt & 3);
        return ld_bf16(a.vt, e) + ld_bf16(a.vt, plane + e) + ld_bf16(a.vt, 2 * plane + e);
    }

    // interp_set_attention: operands given as dense [B][T][H * hs] fp32 arrays written where run_attention reads them - Q rows, fp32
    // K / V rows or, where the op reads operand planes, their exact three-term split in the layouts of run_igemm's EPI_KPL / EPI_VT
    // (the inverse of attn_k / attn_v). Keeps no record in mask: it is no step.
    void set_attention(const Attention &a, const float *q, const float *k, const float *v)
    {
        const int C = a.H * a.hs;
        const i64 plane = (i64)a.B * a.Tk * C;
        unsigned short *kp = a.kpl >= 0 ? reinterpret_cast<unsigned short *>(&A[(size_t)a.kpl]) : nullptr;
        unsigned short *vp = a.vt >= 0 ? reinterpret_cast<unsigned short *>(&A[(size_t)a.vt]) : nullptr;
        for (int b = 0; b < a.B; ++b)
        {
            for (int t = 0; t < a.Tq; ++t)
                for (int c = 0; c < C; ++c)
                    A[(size_t)(a.q + b * a.qBatch + (i64)t * a.ldq + c)] = q[((i64)b * a.Tq + t) * C + c];
            for (int s = 0; s < a.Tk; ++s)
                for (int c = 0; c < C; ++c)
                {
                    const i64 src = ((i64)b * a.Tk + s) * C + c;
                    unsigned short h[3];
                    if (!kp)
                        A[(size_t)(a.k + b * a.kBatch + (i64)s * a.ldk + c)] = k[src];
                    else
                    {
                        split3(k[src], h);
                        for (int p = 0; p < 3; ++p)
                            kp[p * plane + src] = h[p];
                    }
                    if (!vp)
                        A[(size_t)(a.v + b * a.vBatch + (i64)s * a.ldv + c)] = v[src];
                    else
                    {
                        const int head = c / a.hs, dim = c % a.hs, tt = s & 63, nt = a.Tk / 64;
                        const int slot = 4 * (tt >> 5) + ((tt >> 2) & 3), half = (tt >> 4) & 1;
                        const i64 e = ((((i64)b * a.H + head) * nt + (s >> 6)) * a.hs + dim) * 64 + slot * 8 + half * 4 + (tt & 3);
                        split3(v[src], h);
                        for (int p = 0; p < 3; ++p)
                            vp[p * plane + e] = h[p];
                    }
                }
        }
    }
    // LocalState: the [q | k | v | decay] row of qkvd as run_local_attn reads it; q / k / v dense [B][T][H], decay [B][T][16]
    // (4 heads x 4 terms: the logits before the sigmoid)
    void set_local_attn(const LocalAttn &a, const float *q, const float *k, const float *v, const float *decay)
    {
        for (i64 r = 0; r < (i64)a.B * a.T; ++r)
        {
            float *row = &A[(size_t)(a.qkvd + r * a.ld)];
            for (int c = 0; c < a.H; ++c)
                row[c] = q[r * a.H + c], row[a.H + c] = k[r * a.H + c], row[2 * a.H + c] = v[r * a.H + c];
            for (int c = 0; c < 16; ++c)
                row[3 * a.H + c] = decay[r * 16 + c];
        }
    }

    template <class T>
    void run_attention(const Attention &a)
    {
#pragma omp parallel for collapse(2) schedule(static)
        for (int b = 0; b < a.B; ++b)
            for (int h = 0; h < a.H; ++h)
            {
                std::vector<T> sc((size_t)a.Tk), o((size_t)a.hs);
                std::vector<float> kk((size_t)a.Tk * a.hs), vv((size_t)a.Tk * a.hs);
                for (int s = 0; s < a.Tk; ++s)
                    for (int j = 0; j < a.hs; ++j)
                        kk[(size_t)s * a.hs + j] = attn_k(a, b, s, h * a.hs + j), vv[(size_t)s * a.hs + j] = attn_v(a, b, s, h * a.hs + j);
                for (int t = 0; t < a.Tq; ++t)
                {
                    const float *q = &A[(size_t)(a.q + b * a.qBatch + (i64)t * a.ldq + h * a.hs)];
                    T mx = -INFINITY;
                    for (int s = 0; s < a.Tk; ++s)
                    {
                        const float *k = &kk[(size_t)s * a.hs];
                        T d = 0;
                        for (int j = 0; j < a.hs; ++j)
                            d += T(q[j]) * k[j];
                        sc[(size_t)s] = d * a.scale;
                        mx = max_(mx, sc[(size_t)s]);
                    }
                    T sum = 0;
                    for (int s = 0; s < a.Tk; ++s)
                    {
                        sc[(size_t)s] = exp_(sc[(size_t)s] - mx);
                        sum += sc[(size_t)s];
                    }
                    for (int j = 0; j < a.hs; ++j)
                        o[(size_t)j] = 0;
                    for (int s = 0; s < a.Tk; ++s)
                    {
                        const float *v = &vv[(size_t)s * a.hs];
                        T p = sc[(size_t)s] / sum;
                        for (int j = 0; j < a.hs; ++j)
                            o[(size_t)j] += p * v[j];
                    }
                    for (int j = 0; j < a.hs; ++j)
                        st(a.o + b * a.oBatch + (i64)t * a.ldo + h * a.hs + j, o[(size_t)j]);
                }
            }
    }

    template <class T>
    void run_istft(const Istft &s)
    {
        const float *win = &A[(size_t)s.window];
        const int CS = 4 * s.S;
        for (int b = 0; b < s.B; ++b)
        {
            const float *st4 = &A[(size_t)(s.stats + (i64)b * 4)];
            float mean = st4[0], stdv = st4[2];
            for (int src = 0; src < s.S; ++src)
                for (int ch = 0; ch < 2; ++ch)
                    for (int t = 0; t < s.T; ++t)
                    {
                        std::vector<std::complex<double>> buf(4096, {0, 0});
                        double l1 = 0;
                        for (int f = 0; f < 2048; ++f)
                        {
                            const float *x = &A[(size_t)(s.x + (((i64)b * s.T + t) * 2048 + f) * CS + src * 4 + 2 * ch)];
                            T re = T(stdv) * x[0] + mean, im = T(stdv) * x[1] + mean; // model_inference.cpp:380-393
                            buf[f] = std::complex<double>(Tr<T>::val(re * 64.0f), Tr<T>::val(im * 64.0f));
                            l1 += 2.0 * 64.0 * (Tr<T>::mag(re) + Tr<T>::mag(im));
                        }
                        buf[0] = {buf[0].real(), 0};
                        for (int f = 1; f < 2048; ++f)
                            buf[4096 - f] = std::conj(buf[f]);
                        fft(buf, +1);
                        const i64 o = s.frames + ((((i64)b * s.S + src) * 2 + ch) * s.T + t) * 4096;
                        for (int i = 0; i < 4096; ++i)
                            st(o + i, Tr<T>::rf(Tr<T>::mk(buf[i].real(), l1)) * win[i]);
                    }
        }
    }

    template <class T>
    T frame_at(i64 off) const
    {
        return A[(size_t)off];
    }

    template <class T>
    void run_ola(const Ola &o)
    {
        for (int b = 0; b < o.B; ++b)
        {
            const float *st4 = &A[(size_t)(o.statsT + (i64)b * 4)];
            for (int src = 0; src < o.S; ++src)
                for (int ch = 0; ch < 2; ++ch)
                    for (int i = 0; i < o.seg; ++i)
                    {
                        // sample n of the (T+4)-frame overlap-add buffer; reference frame f starts at f*1024;
                        // kept waveform drops 2048 (dsp.cpp:113-116) then `pad` (model_inference.cpp:454-455)
                        i64 n = 2048 + o.pad + i;
                        T acc = 0.f;
                        for (i64 f = n / 1024 - 3; f <= n / 1024; ++f)
                        {
                            i64 t = f - 2; // frames 0,1 and T+2,T+3 are zero (model_inference.cpp:439-444)
                            if (t < 0 || t >= o.T)
                                continue;
                            T yv = frame_at<T>(o.frames + ((((i64)b * o.S + src) * 2 + ch) * o.T + t) * 4096 + (n - f * 1024));
                            acc += yv * 1.0f / 4096.0f / (A[(size_t)(o.wss + n)] + 1e-8f);
                        }
                        T tb = T(st4[2]) * A[(size_t)(o.xt + ((i64)b * o.seg + i) * (2 * o.S) + src * 2 + ch)] + st4[0];
                        st(o.out + (((i64)b * o.S + src) * 2 + ch) * o.seg + i, acc + tb);
                    }
        }
    }

    // order: 0 = plan order. 1 / 2 = the most skewed interleavings two concurrent streams may produce
    // under the derived cross-stream waits (Op::waitOp): always advance stream (order-1) as far as its
    // waits allow before the other stream takes ONE step. If the derived waits were missing a
    // hazard, one of the two skews would reorder the conflicting ops and change the result.
    std::vector<int> schedule(int order) const
    {
        const int n = (int)pl.ops.size();
        std::vector<int> seq;
        if (order == 0)
        {
            for (int i = 0; i < n; ++i)
                seq.push_back(i);
            return seq;
        }
        std::vector<int> q[2];
        for (int i = 0; i < n; ++i)
            q[pl.ops[i].stream ? 1 : 0].push_back(i);
        size_t pos[2] = {0, 0};
        std::vector<char> done(n, 0);
        const int fav = order - 1;
        auto ready = [&](int s) {
            if (pos[s] >= q[s].size())
                return false;
            const int w = pl.ops[q[s][pos[s]]].waitOp;
            return w < 0 || done[w];
        };
        auto step = [&](int s) {
            const int i = q[s][pos[s]++];
            done[i] = 1;
            seq.push_back(i);
        };
        while (pos[0] < q[0].size() || pos[1] < q[1].size())
        {
            if (ready(fav))
                step(fav);
            else if (ready(1 - fav))
                step(1 - fav);
            else
                return std::vector<int>(); // deadlock: cannot happen (waits only point backwards)
        }
        return seq;
    }

    // ---- Demucs v3 ops (plan.h)
    template <class T>
    void run_group_stats(const GroupStats &g)
    {
        typedef typename Tr<T>::W Wd;
        const int gs = g.C / g.G;
        for (int b = 0; b < g.B; ++b)
            for (int gi = 0; gi < g.G; ++gi)
            {
                const double cnt = (double)g.rows * gs;
                Wd sum = 0;
                for (int r = 0; r < g.rows; ++r)
                    for (int c = gi * gs; c < (gi + 1) * gs; ++c)
                        sum += A[(size_t)(g.x + ((i64)b * g.rows + r) * g.C + c)];
                const T mean = Tr<T>::rf(sum / cnt);
                Wd ss = 0;
                for (int r = 0; r < g.rows; ++r)
                    for (int c = gi * gs; c < (gi + 1) * gs; ++c)
                    {
                        const Wd d = Tr<T>::wd(A[(size_t)(g.x + ((i64)b * g.rows + r) * g.C + c)]) - Tr<T>::wd(mean);
                        ss += d * d;
                    }
                const Wd var = ss / (cnt - 1.0);
                if (!std::is_same<T, float>::value)
                    census_elements(&A[(size_t)(g.x + (i64)b * g.rows * g.C + gi * gs)], gs, g.rows, g.C, cnt, num(var));
                const i64 o = g.out + ((i64)b * g.G + gi) * 4;
                st(o, mean);
                st(o + 1, Tr<T>::rf(1.0 / sqrt_(var + (double)g.eps)));
                st(o + 2, Tr<T>::rf(sqrt_(var)));
                st(o + 3, T(0.f));
            }
    }
    template <class T>
    void run_gn_act(const GnAct &g)
    {
        const int gs = g.C / g.G, Co = g.mode == 2 ? g.C / 2 : g.C;
        for (int b = 0; b < g.B; ++b)
            for (int r = 0; r < g.rowsOut; ++r)
            {
                const float *x = &A[(size_t)(g.x + ((i64)b * g.rowsIn + r + g.rowOff) * g.C)];
                auto gn = [&](int c) -> T {
                    const float *st4 = &A[(size_t)(g.stats + ((i64)b * g.G + c / gs) * 4)];
                    return (T(x[c]) - st4[0]) * st4[1] * W[g.w_w + c] + W[g.b_w + c];
                };
                std::vector<T> tmp((size_t)Co);
                for (int c = 0; c < Co; ++c)
                {
                    T v = gn(c);
                    if (g.mode == 1)
                        v = gelu(v);
                    else if (g.mode == 2)
                        v = v * sigmoidf(gn(c + Co));
                    if (g.scale_w >= 0)
                        v *= W[g.scale_w + c];
                    if (g.res >= 0)
                        v += A[(size_t)(g.res + ((i64)b * g.rowsOut + r) * Co + c)];
                    tmp[(size_t)c] = v;
                }
                for (int c = 0; c < Co; ++c)
                    st(g.y + ((i64)b * g.rowsOut + r) * Co + c, tmp[(size_t)c]);
            }
    }
    template <class T>
    void run_lstm(const Lstm &l)
    {
        const int H = l.H, Tn = l.T;
#pragma omp parallel for collapse(2) schedule(static)
        for (int b = 0; b < l.B; ++b)
            for (int dir = 0; dir < 2; ++dir)
            {
                std::vector<T> h((size_t)H, T(0.f)), c((size_t)H, T(0.f)), hn((size_t)H);
                const float *U = W + l.whh_w + (i64)dir * 4 * H * H;
                for (int step = 0; step < Tn; ++step)
                {
                    const int t = dir == 0 ? step : Tn - 1 - step;
                    const float *xp = &A[(size_t)(l.xproj + ((i64)b * Tn + t) * 8 * H + (i64)dir * 4 * H)];
                    for (int j = 0; j < H; ++j)
                    {
                        T gt[4];
                        for (int q = 0; q < 4; ++q)
                        {
                            const float *u = U + (i64)(4 * j + q) * H;
                            T acc = xp[4 * j + q]; // the MFMA accumulates onto the input projection, k ascending
                            for (int k = 0; k < H; ++k)
                                acc = fma_(T(u[k]), h[(size_t)k], acc);
                            gt[q] = acc;
                        }
                        const T ig = sigmoidf(gt[0]), fg = sigmoidf(gt[1]), gg = tanh_(gt[2]), og = sigmoidf(gt[3]);
                        const T cn = fg * c[(size_t)j] + ig * gg;
                        c[(size_t)j] = Tr<T>::rebase(cn);
                        if (!std::is_same<T, float>::value && std::fabs(num(Tr<T>::wd(cn))) >= 8.0)
                            census(CEN_C8);
                        hn[(size_t)j] = og * tanh_(cn);
                    }
                    // The magnitude of an output is that of ITS step from the state before it, the state taken as numbers of their
                    // own (rebase): the errors of earlier steps enter the bound as one allowance per step (op_reference.bound_c:
                    // c grows with T), not as magnitudes multiplied through the recurrence, which grow without bound
                    for (int j = 0; j < H; ++j)
                        st(l.out + ((i64)b * Tn + t) * 2 * H + (i64)dir * H + j, hn[(size_t)j]);
                    for (int j = 0; j < H; ++j)
                        h[(size_t)j] = Tr<T>::rebase(hn[(size_t)j]);
                }
            }
    }
    template <class T>
    void run_local_attn(const LocalAttn &a)
    {
        const int heads = 4, nd = 4, hd = a.H / heads, Tn = a.T;
        const float sq = std::sqrt((float)hd);
#pragma omp parallel for collapse(2) schedule(static)
        for (int b = 0; b < a.B; ++b)
            for (int h = 0; h < heads; ++h)
            {
                std::vector<T> w((size_t)Tn);
                for (int s = 0; s < Tn; ++s)
                {
                    const float *row = &A[(size_t)(a.qkvd + ((i64)b * Tn + s) * a.ld)];
                    const float *q = row + h * hd;
                    T dq[4];
                    for (int n = 0; n < nd; ++n)
                        dq[n] = 0.5f * sigmoidf(T(row[3 * a.H + h * nd + n]));
                    T mx = -INFINITY;
                    for (int t = 0; t < Tn; ++t)
                    {
                        const float *k = &A[(size_t)(a.qkvd + ((i64)b * Tn + t) * a.ld + a.H + h * hd)];
                        T dot = 0.f;
                        for (int c = 0; c < hd; ++c)
                            dot += T(q[c]) * k[c];
                        T v = dot / sq, decay = 0.f;
                        const float delta = (float)std::abs(t - s);
                        for (int n = 0; n < nd; ++n)
                            decay += (-(float)(n + 1) * delta / 2.0f) * dq[n];
                        w[(size_t)t] = t != s ? v + decay : T(-100.0f);
                        mx = max_(mx, w[(size_t)t]);
                    }
                    T sum = 0.f;
                    for (int t = 0; t < Tn; ++t)
                    {
                        w[(size_t)t] = exp_(w[(size_t)t] - mx);
                        sum += w[(size_t)t];
                    }
                    for (int t = 0; t < Tn; ++t)
                        w[(size_t)t] /= sum;
                    for (int c = 0; c < hd; ++c)
                    {
                        T acc = 0.f;
                        for (int t = 0; t < Tn; ++t)
                            acc += w[(size_t)t] * A[(size_t)(a.qkvd + ((i64)b * Tn + t) * a.ld + 2 * a.H + h * hd + c)];
                        st(a.out + ((i64)b * Tn + s) * a.H + h * hd + c, acc);
                    }
                }
            }
    }

    // OP_DCONV_ROW: the unfused definition (plan.h), statistics in double from the formed tensors (no factor)
    template <class T>
    void run_dconv_row(const DconvRow &r)
    {
        typedef typename Tr<T>::W Wd;
        const int Tn = r.T, F = r.F, C = r.C, H = r.hid;
#pragma omp parallel for schedule(static)
        for (i64 row = 0; row < (i64)r.B * F; ++row)
        {
            const int b = (int)(row / F), f = (int)(row % F);
            std::vector<T> xs((size_t)Tn * C); // the row, updated in place by both layers
            for (int t = 0; t < Tn; ++t)
                for (int c = 0; c < C; ++c)
                    xs[(size_t)t * C + c] = A[(size_t)(r.x + (((i64)b * Tn + t) * F + f) * C + c)];
            auto X = [&](int t, int c) -> T & { return xs[(size_t)t * C + c]; };
            std::vector<T> h((size_t)Tn * H), y((size_t)Tn * 2 * C);
            for (int j = 0; j < 2; ++j)
            {
                const int d = j + 1;
                const float *k1 = W + r.k1_w[j], *k1b = W + r.k1_b[j], *k2 = W + r.k2_w[j], *k2b = W + r.k2_b[j];
                Wd s = 0, q = 0;
                for (int t = 0; t < Tn; ++t)
                    for (int n = 0; n < H; ++n)
                    {
                        T acc = 0.f;
                        for (int tap = 0; tap < 3; ++tap)
                        {
                            const int ti = t + (tap - 1) * d;
                            if (ti < 0 || ti >= Tn)
                                continue;
                            for (int c = 0; c < C; ++c)
                                acc += X(ti, c) * k1[(i64)n * 3 * C + tap * C + c];
                        }
                        const T v = acc + k1b[n];
                        h[(size_t)t * H + n] = v;
                        s += v, q += Tr<T>::wd(v) * v;
                    }
                T m1, r1, m2, r2;
                inner_stats(s, q, (double)H * Tn, r.eps, m1, r1);
                for (int t = 0; t < Tn; ++t)
                    for (int n = 0; n < H; ++n)
                        h[(size_t)t * H + n] = gelu((h[(size_t)t * H + n] - m1) * r1 * W[r.gn1_w[j] + n] + W[r.gn1_b[j] + n]);
                s = q = 0;
                for (int t = 0; t < Tn; ++t)
                    for (int n = 0; n < 2 * C; ++n)
                    {
                        T acc = 0.f;
                        for (int k = 0; k < H; ++k)
                            acc += h[(size_t)t * H + k] * k2[(i64)n * 16 + k];
                        const T v = acc + k2b[n];
                        y[(size_t)t * 2 * C + n] = v;
                        s += v, q += Tr<T>::wd(v) * v;
                    }
                inner_stats(s, q, 2.0 * C * Tn, r.eps, m2, r2);
                for (int t = 0; t < Tn; ++t)
                    for (int c = 0; c < C; ++c)
                    {
                        const int na = (c / 16) * 32 + c % 16, ng = na + 16; // packed GLU pair (model_pack.cpp paired_row)
                        const T a = (y[(size_t)t * 2 * C + na] - m2) * r2 * W[r.gn2_w[j] + na] + W[r.gn2_b[j] + na];
                        const T g = (y[(size_t)t * 2 * C + ng] - m2) * r2 * W[r.gn2_w[j] + ng] + W[r.gn2_b[j] + ng];
                        X(t, c) += W[r.scale_w[j] + c] * (a * sigmoidf(g));
                    }
            }
            for (int t = 0; t < Tn; ++t)
                for (int c = 0; c < C; ++c)
                    st(r.x + (((i64)b * Tn + t) * F + f) * C + c, X(t, c));
        }
    }

    template <class T>
    void run_op(const Op &op)
    {
        switch (op.kind)
        {
        case OP_IGEMM: run_igemm<T>(op.g); break;
        case OP_STATS_REDUCE: run_reduce<T>(op.sr); break;
        case OP_STFT: run_stft<T>(op.stft); break;
        case OP_LAYERNORM: run_ln<T>(op.ln); break;
        case OP_GN_APPLY: run_gn<T>(op.gn); break;
        case OP_ATTENTION: run_attention<T>(op.at); break;
        case OP_ISTFT: run_istft<T>(op.istft); break;
        case OP_OLA: run_ola<T>(op.ola); break;
        case OP_GROUP_STATS: run_group_stats<T>(op.gs); break;
        case OP_GN_ACT: run_gn_act<T>(op.ga); break;
        case OP_LSTM: run_lstm<T>(op.lstm); break;
        case OP_LOCAL_ATTN: run_local_attn<T>(op.la); break;
        case OP_DCONV_ROW: run_dconv_row<T>(op.dr); break;
        default: break;
        }
    }

    void run(int order = 0)
    {
        for (int idx : schedule(order))
            run_op<float>(pl.ops[idx]);
    }
};

// the fused GPU kernel never rounds the frames: a chained precise OP_OLA takes them as the OP_ISTFT step left them
template <>
P Interp::frame_at<P>(i64 off) const
{
    return chained ? P(R[(size_t)off], (double)S[(size_t)off]) : P((double)A[(size_t)off]);
}
} // namespace

extern "C"
{
    void *interp_create(const char *model_path, int64_t seg, int B)
    {
        auto *it = new Interp();
        std::string err;
        if (!load_and_pack(model_path, it->pm, err))
        {
            fprintf(stderr, "%s\n", err.c_str());
            delete it;
            return nullptr;
        }
        build_plan(it->pm, seg, B, it->pl, plan_opts_from_env(GEMM_F32, false));
        it->A.assign((size_t)it->pl.arenaFloats, 0.f);
        std::copy(it->pl.constants.begin(), it->pl.constants.end(), it->A.begin());
        it->W = it->pm.blob.data();
        return it;
    }
    // the plan only (no arena): for tools and tests that look at the op list of big batches
    void *interp_create_plan(const char *model_path, int64_t seg, int B)
    {
        auto *it = new Interp();
        std::string err;
        if (!load_and_pack(model_path, it->pm, err))
        {
            fprintf(stderr, "%s\n", err.c_str());
            delete it;
            return nullptr;
        }
        int gemm = GEMM_F32;
        if (const char *e = getenv("DMX_INTERP_GEMM")) // tools/plan_dump.py: the tile choices of the split modes (host only)
            gemm = atoi(e);
        build_plan(it->pm, seg, B, it->pl, plan_opts_from_env(gemm, gemm != GEMM_F32));
        it->W = nullptr;
        return it;
    }
    void interp_free(void *h) { delete (Interp *)h; }
    int interp_n_ops(void *h) { return (int)((Interp *)h)->pl.ops.size(); }
    double interp_arena_mb(void *h) { return (double)((Interp *)h)->pl.arenaFloats * 4 / 1e6; }
    // mix [B][seg][2] interleaved -> out [B][S][2][seg]
    // number of cross-stream waits in the plan
    int interp_n_waits(void *h)
    {
        int c = 0;
        for (auto &op : ((Interp *)h)->pl.ops)
            c += op.waitOp >= 0;
        return c;
    }
    void interp_run_order(void *h, const float *mix, float *out, int order)
    {
        Interp *it = (Interp *)h;
        const Plan &pl = it->pl;
        std::memcpy(&it->A[(size_t)pl.mixOff], mix, sizeof(float) * (size_t)(pl.B * pl.geo.seg * 2));
        it->run(order);
        std::memcpy(out, &it->A[(size_t)pl.outOff], sizeof(float) * (size_t)((i64)pl.B * pl.S * 2 * pl.geo.seg));
    }
    void interp_run(void *h, const float *mix, float *out)
    {
        Interp *it = (Interp *)h;
        const Plan &pl = it->pl;
        std::memcpy(&it->A[(size_t)pl.mixOff], mix, sizeof(float) * (size_t)(pl.B * pl.geo.seg * 2));
        it->run();
        std::memcpy(out, &it->A[(size_t)pl.outOff], sizeof(float) * (size_t)((i64)pl.B * pl.S * 2 * pl.geo.seg));
    }
    // tap -> returns ndim, fills shape (batch first), copies data if dst != null
    int interp_tap(void *h, const char *name, int64_t *shape, float *dst)
    {
        Interp *it = (Interp *)h;
        for (auto &op : it->pl.ops)
            if (op.kind == OP_TAP && op.name == name)
            {
                int nd = 0;
                i64 per = 1;
                shape[nd++] = it->pl.B;
                for (int j = 0; j < 4 && op.tap.shape[j] > 0; ++j)
                {
                    shape[nd++] = op.tap.shape[j];
                    per *= op.tap.shape[j];
                }
                if (dst)
                    for (int b = 0; b < it->pl.B; ++b)
                        std::memcpy(dst + b * per, &it->A[(size_t)(op.tap.off + b * op.tap.batchStride)], sizeof(float) * (size_t)per);
                return nd;
            }
        return -1;
    }
}

// lists the (tile cfg, prologue, epilogue, act, rowstat) combinations a plan uses (build tooling)
extern "C" int interp_combos(void *h, int *out, int cap)
{
    Interp *it = (Interp *)h;
    int n = 0;
    for (auto &op : it->pl.ops)
        if (op.kind == OP_IGEMM && n + 5 <= cap)
        {
            out[n++] = op.g.cfg;
            out[n++] = op.g.pro;
            out[n++] = op.g.epi;
            out[n++] = op.g.act;
            out[n++] = op.g.rowstat >= 0;
        }
    return n / 5;
}

// one line per igemm op: name, tile cfg, M, N, K, number of tiles (tools: which tile a batch size gets)
extern "C" int interp_plan_dump(void *h, char *buf, int cap)
{
    Interp *it = (Interp *)h;
    std::string all;
    char line[256];
    for (auto &op : it->pl.ops)
        if (op.kind == OP_IGEMM)
        {
            const IGemm &g = op.g;
            const i64 M = (i64)g.B * g.P1 * g.P0;
            const i64 tiles = ((M + kTileCfgs[g.cfg].BM - 1) / kTileCfgs[g.cfg].BM) * g.NB;
            snprintf(line, sizeof(line), "%s %d %lld %d %d %lld %d %d %d\n", op.name.c_str(), g.cfg, (long long)M, g.N, g.K, (long long)tiles,
                     (int)(g.rowstat >= 0), g.hterms, g.epi);
            all += line;
        }
    if ((int)all.size() + 1 > cap)
        return -1;
    memcpy(buf, all.c_str(), all.size() + 1);
    return (int)all.size();
}

// ---- the kernel selection (csrc/gemm_select.cpp: host arithmetic), driven without a GPU by tests/test_gemm_select_cpu.py
static void print_choice(std::string &all, const std::string &name, const IGemm &g, const GemmChoice &c)
{
    char line[320];
    IGemm chosen = g;
    chosen.choice = c;
    snprintf(line, sizeof(line), "%s %d %d %d %d %d %d %s %d\n", name.c_str(), g.cfg, g.epi, g.hterms, c.family, c.arith, c.wnf, c.label ? c.label : "-",
             (int)gemm_kernel_exists(chosen));
    all += line;
}
static int copy_out(const std::string &all, char *buf, int cap)
{
    if ((int)all.size() + 1 > cap)
        return -1;
    memcpy(buf, all.c_str(), all.size() + 1);
    return (int)all.size();
}
// is x an fp16 number (subnormals included)? What dmx_model_upload lists for the fp16 plane
static bool is_fp16_number(float x)
{
    if (x == 0.f)
        return true;
    int e;
    (void)std::frexp(x, &e); // |x| in [2^(e-1), 2^e)
    if (!std::isfinite(x) || e > 16)
        return false;
    const float q = std::ldexp(x, -std::max(e - 11, -24)); // in units of the fp16 ulp at x
    return q == std::floor(q);
}

// The plan a context of GEMM mode `gemm` builds for the handle's model at segment length seg and batch B (gemm_select.h build_chosen_plan, as
// exec.cpp dmx_get_plan calls it), one line per OP_IGEMM: name, tile cfg, epilogue, hterms, family, arithmetic, wnf, label, the chosen kernel exists
// (gemm_select.h gemm_kernel_exists).
// Model facts: both kinds of weight planes exist; BOTH inexact lists hold the blob elements that are not fp16 numbers (the fp16 list
// of dmx_model_upload; every fp16 number is two-bf16-term exact, so it contains the bf16 list) plus all weights of the op named
// `inexact` ("" = none).
extern "C" int interp_select_dump(void *h, int64_t seg, int B, int gemm, int linMode, const char *inexact, char *buf, int cap)
{
    Interp *it = (Interp *)h;
    if (!it->scanned)
        for (size_t i = 0; i < it->pm.blob.size(); ++i)
            if (!is_fp16_number(it->pm.blob[i]))
                it->notFp16.push_back((i64)i);
    it->scanned = true;
    std::vector<i64> bad = it->notFp16;
    GemmModelFacts f;
    f.bf16Planes = f.fp16Plane = true;
    f.planeDelta = (i64)it->pm.blob.size() + 512;
    f.inexactW = f.inexactH = &bad;
    const bool kvPlanes = gemm != GEMM_F32 && it->pm.arch != 3;
    Plan pl;
    build_chosen_plan(it->pm, seg, B, gemm, kvPlanes, f, linMode, pl);
    if (inexact && *inexact)
    {
        bool found = false;
        for (const Op &op : pl.ops)
            if (op.kind == OP_IGEMM && op.name == inexact)
            {
                for (i64 i = 0; i < (i64)op.g.Np * op.g.Kp; ++i)
                    bad.push_back(op.g.w_w + i);
                found = true;
            }
        if (!found)
            return -2;
        std::sort(bad.begin(), bad.end());
        pl = Plan();
        build_chosen_plan(it->pm, seg, B, gemm, kvPlanes, f, linMode, pl);
    }
    std::string all;
    for (const Op &op : pl.ops)
        if (op.kind == OP_IGEMM)
        {
            print_choice(all, op.name, op.g, op.g.choice);
            const GemmChoice again = select_gemm(op.g, gemm, f, linMode); // (a second call gives the same choice)
            if (again != op.g.choice || again.label != op.g.choice.label)
                return -3;
        }
    return copy_out(all, buf, cap);
}

// The choice for a hand-made op: a copy of op `name` of the handle's plan with tile cfg, epilogue, N, Np, residual offset and
// row-statistics offset replaced (-2 keeps a field); every weight counts as exact. One line as interp_select_dump prints it.
extern "C" int interp_select_one(void *h, const char *name, int gemm, int linMode, int cfg, int epi, int N, int Np, int res, int rowstat, char *buf, int cap)
{
    Interp *it = (Interp *)h;
    GemmModelFacts f;
    f.bf16Planes = f.fp16Plane = true;
    f.planeDelta = (i64)it->pm.blob.size() + 512;
    for (const Op &op : it->pl.ops)
        if (op.kind == OP_IGEMM && op.name == name)
        {
            IGemm g = op.g;
            g.cfg = cfg != -2 ? cfg : g.cfg, g.epi = epi != -2 ? epi : g.epi, g.N = N != -2 ? N : g.N, g.Np = Np != -2 ? Np : g.Np;
            g.res = res != -2 ? res : g.res, g.rowstat = rowstat != -2 ? rowstat : g.rowstat;
            std::string all;
            print_choice(all, op.name, g, select_gemm(g, gemm, f, linMode));
            return copy_out(all, buf, cap);
        }
    return -2;
}

// The tile table (csrc/gemm_tiles.h), one line per tile cfg: cfg, BM, BN, waves along M, along N, row fragments, column fragments,
// K sub-steps, kind (TileKind), fp32 label, split label or "-"
extern "C" int interp_tiles(char *buf, int cap)
{
    std::string all;
    char line[256];
    for (int c = 0; c < kNumTileCfgs; ++c)
    {
        const TileCfg &t = kTileCfgs[c];
        snprintf(line, sizeof(line), "%d %d %d %d %d %d %d %d %d %s %s\n", c, t.BM, t.BN, t.WM, t.WN, t.MF, t.NF, t.KS, t.kind, t.label, t.splitLabel ? t.splitLabel : "-");
        all += line;
    }
    return copy_out(all, buf, cap);
}

// One list, two users: a hand-made op (N columns, S1 taps of seg0, prologue, epilogue, with or without a residual) of an fp32 plan.
// Returns bit 0: choose_tile sends it to the direct kernels; bit 1: gemm_kernel_exists says the direct kernel for it is compiled
extern "C" int interp_direct_probe(int N, int S1, int seg0, int pro, int epi, int res)
{
    IGemm g;
    std::memset((void *)&g, 0, sizeof(g));
    g.B = 1, g.P1 = 64, g.P0 = 1, g.L1 = 64, g.L0 = 1, g.Cin = seg0;
    g.S1 = S1, g.stride1 = 1, g.dil1 = 1, g.pad1 = S1 / 2, g.seg0 = seg0, g.stride0 = 1;
    g.K = S1 * seg0, g.Kp = rup(g.K, 16), g.N = N, g.Np = rup(N, 16), g.xBatchStride = (i64)g.L1 * g.L0 * g.Cin;
    g.pro = pro, g.epi = epi, g.G0 = 1, g.NB = 1;
    g.res = res ? 64 : -1, g.scale_w = g.rowstat = g.table_w = g.kv = -1;
    const bool routed = choose_tile(g, epi == EPI_GLU || epi == EPI_GN_GLU_SCALE_RES, false, GEMM_F32, GemmSwitches()).cfg == kDirectCfg;
    g.cfg = kDirectCfg;
    g.choice = GemmChoice{GF_DIRECT, 0, 0, kTileCfgs[kDirectCfg].label};
    return (routed ? 1 : 0) | (gemm_kernel_exists(g) ? 2 : 0);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The step interface: one op at a time on the interpreter's arena, in fp32 (mode 0: what interp_run does, op by op) or in double
// (mode 1; + 2: the op's GEMM runs on fp16 terms on the device, the magnitudes carry that mode's allowance; + 4: an OP_OLA takes
// the frames of the OP_ISTFT stepped just before it unrounded, as the fused GPU kernel does). tests/test_gpu_op_parity.py puts
// each HIP kernel next to it; tests/test_op_reference_cpu.py checks the harness itself.

// The plan a context of GEMM mode `gemm` builds (gemm_select.h build_chosen_plan, as exec.cpp dmx_get_plan calls it: every weight of
// the synthetic test models is an fp16 number, derived ones are listed as inexact), with an arena.
extern "C" void *interp_create_chosen(const char *model_path, int64_t seg, int B, int gemm, int kvPlanes)
{
    auto *it = new Interp();
    std::string err;
    if (!load_and_pack(model_path, it->pm, err))
    {
        fprintf(stderr, "%s\n", err.c_str());
        delete it;
        return nullptr;
    }
    for (size_t i = 0; i < it->pm.blob.size(); ++i)
        if (!is_fp16_number(it->pm.blob[i]))
            it->notFp16.push_back((i64)i);
    it->scanned = true;
    GemmModelFacts f;
    f.bf16Planes = f.fp16Plane = true;
    f.planeDelta = (i64)it->pm.blob.size() + 512;
    f.inexactW = f.inexactH = &it->notFp16;
    build_chosen_plan(it->pm, seg, B, gemm, kvPlanes != 0, f, 1, it->pl);
    it->A.assign((size_t)it->pl.arenaFloats, 0.f);
    std::copy(it->pl.constants.begin(), it->pl.constants.end(), it->A.begin());
    it->W = it->pm.blob.data();
    return it;
}

extern "C" int64_t interp_arena_floats(void *h) { return ((Interp *)h)->pl.arenaFloats; }
extern "C" int64_t interp_const_floats(void *h) { return (int64_t)((Interp *)h)->pl.constants.size(); }
extern "C" int64_t interp_mix_off(void *h) { return ((Interp *)h)->pl.mixOff; }
extern "C" int64_t interp_out_off(void *h) { return ((Interp *)h)->pl.outOff; }
extern "C" float *interp_arena(void *h) { return ((Interp *)h)->A.data(); }
// the packed weights (W space; the w_w= / bias_w= words of interp_op_info are offsets into it)
extern "C" const float *interp_weights(void *h) { return ((Interp *)h)->W; }
extern "C" int64_t interp_weight_floats(void *h) { return (int64_t)((Interp *)h)->pm.blob.size(); }
// valid after the first interp_step of the handle; precise / magnitude / planes after a step in double
extern "C" unsigned char *interp_mask(void *h) { return ((Interp *)h)->mask.data(); }
extern "C" double *interp_precise(void *h) { return ((Interp *)h)->R.data(); }
extern "C" float *interp_magnitude(void *h) { return ((Interp *)h)->S.data(); }
extern "C" int64_t interp_planes(void *h, double **r, float **s)
{
    Interp *it = (Interp *)h;
    *r = it->kvR.data(), *s = it->kvS.data();
    return (int64_t)it->kvR.size();
}

// op i in the words of dmx_debug_op_info (csrc/plan_describe.h): the two plans are compared as text
extern "C" int interp_op_info(void *h, int i, char *buf, int cap)
{
    Interp *it = (Interp *)h;
    if (i < 0 || i >= (int)it->pl.ops.size())
        return -1;
    const Op &op = it->pl.ops[(size_t)i];
    const std::string all = describe_op(op);
    return copy_out(all, buf, cap);
}

// Operands of attention op i (OP_ATTENTION, or OP_LOCAL_ATTN with its decay logits) written straight into the ranges the op reads:
// q [B][Tq][H hs], k / v [B][Tk][H hs] dense fp32; decay [B][T][16] for LocalState, null otherwise. -1: no such op or a decay
// array that does not go with the op's kind.
extern "C" int interp_set_attention(void *h, int i, const float *q, const float *k, const float *v, const float *decay)
{
    Interp *it = (Interp *)h;
    if (i < 0 || i >= (int)it->pl.ops.size() || !q || !k || !v)
        return -1;
    const Op &op = it->pl.ops[(size_t)i];
    if (op.kind == OP_ATTENTION && !decay)
        it->set_attention(op.at, q, k, v);
    else if (op.kind == OP_LOCAL_ATTN && decay)
        it->set_local_attn(op.la, q, k, v, decay);
    else
        return -1;
    return 0;
}

// the census of the last precise step (one per process: handles are stepped one at a time): CEN_N counters, see the enum
extern "C" int interp_census(long long *out, int cap)
{
    for (int k = 0; k < CEN_N && k < cap; ++k)
        out[k] = g_census[k].load();
    return CEN_N;
}

// Where op i reads each of its operands, by role, for tests that write crafted values there (tests/value_cases.py): words
// role=off:rows:cols:ld:batchStride:batches (floats; element (b, r, c) at off + b batchStride + r ld + c). Roles: act (the
// activation operand), prostats / epistats (the records {mean, scale, std, 0} a prologue / epilogue reads), res (the residual),
// rowstat (the partials of an OP_STATS_REDUCE), xproj (OP_LSTM), rowtensor (the in-place tensor of an OP_DCONV_ROW). Words W.name
// give a range of the packed weights in the same form; conv= a GEMM's gather geometry, rows= {rowOff, rowsOut, G} of an OP_GN_ACT,
// reduce= {G, count, mode, eps bits} of an OP_STATS_REDUCE
extern "C" int interp_operands(void *h, int i, char *buf, int cap)
{
    Interp *it = (Interp *)h;
    if (i < 0 || i >= (int)it->pl.ops.size())
        return -1;
    const Op &op = it->pl.ops[(size_t)i];
    std::string all;
    auto word = [&](const char *role, i64 off, i64 rows, i64 cols, i64 ld, i64 batch, i64 nb) {
        char t[192];
        snprintf(t, sizeof(t), "%s=%lld:%lld:%lld:%lld:%lld:%lld ", role, (long long)off, (long long)rows, (long long)cols, (long long)ld, (long long)batch, (long long)nb);
        all += t;
    };
    switch (op.kind)
    {
    case OP_IGEMM:
    {
        const IGemm &g = op.g;
        const int G = g.G0 > 1 ? g.G0 : 1;
        const int Nout = g.epi == EPI_GLU || g.epi == EPI_GN_GLU_SCALE_RES ? g.N / 2 : g.N;
        word("act", g.x, (i64)g.L1 * g.L0, g.Cin, g.Cin, g.xBatchStride, g.B);
        {
            // how output row (b, p1, p0) gathers its K = S1 seg0 operand elements: k = s1 seg0 + o is element o of the run starting
            // at (p0 stride0 - pad0) Cin of input row in1 = p1 stride1 + s1 dil1 - pad1 (plan.h IGemm)
            char t[256];
            snprintf(t, sizeof(t), "conv=%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d ", g.L1, g.L0, g.Cin, g.K / g.seg0, g.stride1, g.dil1, g.pad1, g.seg0, g.stride0, g.pad0,
                     g.P1, g.P0, G);
            all += t;
        }
        if (g.pro == PRO_AFFINE)
            word("prostats", g.proStats, g.B, 4, 4, 0, 1);
        if (g.pro == PRO_GN_GELU)
            word("prostats", g.proStats, (i64)g.B * G, 4, 4, 0, 1);
        if (g.epi == EPI_GN_GLU_SCALE_RES)
            word("epistats", g.epiStats, (i64)g.B * G, 4, 4, 0, 1);
        if (g.res >= 0 && g.epi != EPI_TRCONV)
            word("res", g.res, (i64)g.P1 * g.P0, Nout, g.ldy, g.yBatchStride, g.B);
        break;
    }
    case OP_STATS_REDUCE:
    {
        unsigned eb;
        std::memcpy(&eb, &op.sr.eps, 4);
        word("rowstat", op.sr.rowstat, op.sr.R, (i64)op.sr.NB * 2, (i64)op.sr.NB * 2, (i64)op.sr.R * op.sr.NB * 2, op.sr.B);
        word("reduce", op.sr.G0 > 1 ? op.sr.G0 : 1, (i64)op.sr.count, op.sr.mode, eb, 0, 1);
        break;
    }
    case OP_LAYERNORM: word("act", op.ln.x, op.ln.rows, op.ln.D, op.ln.D, 0, 1); break;
    case OP_GROUP_STATS: word("act", op.gs.x, op.gs.rows, op.gs.C, op.gs.C, (i64)op.gs.rows * op.gs.C, op.gs.B); break;
    case OP_GN_ACT:
        word("act", op.ga.x, op.ga.rowsIn, op.ga.C, op.ga.C, (i64)op.ga.rowsIn * op.ga.C, op.ga.B);
        word("epistats", op.ga.stats, (i64)op.ga.B * op.ga.G, 4, 4, 0, 1);
        word("W.w", op.ga.w_w, 1, op.ga.C, op.ga.C, 0, 1), word("W.b", op.ga.b_w, 1, op.ga.C, op.ga.C, 0, 1);
        if (op.ga.scale_w >= 0)
            word("W.scale", op.ga.scale_w, 1, op.ga.mode == 2 ? op.ga.C / 2 : op.ga.C, op.ga.C, 0, 1);
        word("rows", op.ga.rowOff, op.ga.rowsOut, op.ga.G, 0, 0, 1);
        if (op.ga.res >= 0)
        {
            const int Co = op.ga.mode == 2 ? op.ga.C / 2 : op.ga.C;
            word("res", op.ga.res, op.ga.rowsOut, Co, Co, (i64)op.ga.rowsOut * Co, op.ga.B);
        }
        break;
    case OP_LSTM:
        word("W.whh", op.lstm.whh_w, 2, 4 * (i64)op.lstm.H * op.lstm.H, 4 * (i64)op.lstm.H * op.lstm.H, 0, 1);
        word("xproj", op.lstm.xproj, op.lstm.T, 8 * (i64)op.lstm.H, 8 * (i64)op.lstm.H, (i64)op.lstm.T * 8 * op.lstm.H, op.lstm.B); break;
    case OP_DCONV_ROW:
        word("rowtensor", op.dr.x, (i64)op.dr.T * op.dr.F, op.dr.C, op.dr.C, (i64)op.dr.T * op.dr.F * op.dr.C, op.dr.B);
        break;
    default: break;
    }
    return copy_out(all, buf, cap);
}

extern "C" int interp_step(void *h, int i, int mode)
{
    Interp *it = (Interp *)h;
    if (i < 0 || i >= (int)it->pl.ops.size())
        return -1;
    const size_t n = (size_t)it->pl.arenaFloats;
    it->mask.assign(n, 0);
    it->kvR.clear(), it->kvS.clear();
    it->hterms = (mode & 2) != 0, it->chained = (mode & 4) != 0;
    if (mode & 1)
    {
        for (auto &c : g_census)
            c.store(0);
        if (it->R.size() != n)
            it->R.assign(n, 0.0), it->S.assign(n, 0.f);
        it->run_op<P>(it->pl.ops[(size_t)i]);
    }
    else
        it->run_op<float>(it->pl.ops[(size_t)i]);
    return 0;
}

