// kernels.h — launch interface of the hand-written gfx950 kernels (device pointers resolved).
// Semantics of every op are specified by plan.h and, executable, by tests/cpu_interp.cpp.
#pragma once
#include "gemm_select.h"
#include "loudness_plan.h"
#include "meters_plan.h"
#include "limiter_plan.h"
#include <hip/hip_runtime.h>
#include <cstdlib>

namespace dmx
{

struct FastDiv // n / d for n < 2^31: magic == 0 ? n >> shift : umulhi(n, magic) >> shift
{
    unsigned magic, shift;
};
inline FastDiv make_fastdiv(unsigned d)
{
    FastDiv f;
    f.magic = 0;
    f.shift = 0;
    if (d == 0)
        d = 1;
    if ((d & (d - 1)) == 0)
    {
        while ((1u << f.shift) < d)
            ++f.shift;
        return f;
    }
    unsigned s = 0;
    while ((1ull << s) < d)
        ++s;
    f.magic = (unsigned)((((unsigned long long)1 << (31 + s)) + d - 1) / d); // exact for n < 2^31
    f.shift = s - 1;
    return f;
}

struct GemmArgs
{
    const float *X;
    i64 xBS;
    int B, P1, P0, L1, L0, Cin;
    int S1, stride1, dil1, pad1, seg0, stride0, pad0, K, Kp;
    int pro;
    const float *proStats, *proW, *proB;
    int G0;
    const float *Wt, *bias;
    const unsigned short *Wb1, *Wb2; // bf16 planes of the weight blob (same element offsets as Wt), or null (igemm_split.hip)
    int N, Np;
    int epi, act;
    float *Y;
    i64 yBS;
    int ldy;
    const float *res, *scale, *epiStats, *epiW, *epiB;
    float *rowstat;
    int NB;
    const float *table;
    float tableScale;
    int Lout, Cout;
    int trS, trOff; // EPI_TRCONV: output position j = trS*p0 + r - trOff (plan.h)
    const float *rowScale; // fp16-term kernels (GEMM_FP16X3): [M][2] = {2^s, 2^-s} per A row (launch_rowscale), else null
    unsigned short *kvPl; // EPI_KPL / EPI_VT: three bf16 planes, kvPlane elements apart (plan.h IGemm::kv)
    i64 kvPlane;
    int kvCol0, kvT, kvH, kvHs;
    i64 M;
    const float *zero; // >= 16 B of zeros, 16-byte aligned: target of out-of-range staging loads
    // launch geometry (filled by launch_igemm): 1-D grid, workgroup id -> (row tile, column tile)
    unsigned tilesM, tilesN;
    FastDiv dP0, dP1; // row index m -> (b, p1, p0) without 64-bit divisions (M < 2^31 is checked by the launcher)
    int xcdMap; // 1: XCD-aware mapping (all column tiles of a row tile on ONE XCD, adjacent in dispatch order)
};

// direct (register-resident weights, no LDS) kernels for the HBM-bound layers; -1 if the shape is
// not in their table
int launch_dgemm(const GemmArgs &a, hipStream_t s);

// The frequency branch's whole DConv residual branch with the (C, T) row of one (segment, bin) resident on the CU
// (dconv_row.hip; plan.h OP_DCONV_ROW). Pointers of the two layers (dilation 1, 2) into the packed model.
struct DconvRowArgs
{
    float *x; // [B][T][F][C], in place
    int B, T, F, C, hid;
    const float *img[2]; // per layer (dilation 1, 2): the weight image in the kernel's LDS layout (plan.h DconvRowGeo)
    float eps;
    const float *zero;
    // filled by the launcher
    int rowsPerXcd;
    double n1, invN1, invN1m1, n2, invN2, invN2m1; // element counts of the two GroupNorms (hid T, 2C T) and the reciprocals of n, n - 1
};
// -1 when no kernel exists for the shape; dry = availability check only (needs B, T, F, C, hid)
int launch_dconv_row(const DconvRowArgs &a, hipStream_t s, bool dry = false);

// returns 0, or -1 when the (tile, prologue, epilogue) combination is not instantiated (gemm_select.h gemm_kernel_exists is the
// host-side answer)
int launch_igemm(int cfg, const GemmArgs &a, hipStream_t s);
// linear layers on a 256x128 tile with four waves of 128x64 (igemm_lin256.hip); -1 when the op is not a plain linear layer
int launch_igemm_lin256(const GemmArgs &a, hipStream_t s);
// the exact-split kernel family `ch` chose for the op (gemm_select.h; igemm_split.hip): bf16 terms on the two planes Wb1 / Wb2, or
// (GF_SPLIT_LINH) fp16 terms with Wb1 = the fp16 plane and rowScale set. -1: the family does not exist for the op's (tile,
// prologue, epilogue) - an internal error, the selection only names kernels that exist
int launch_igemm_split(const GemmChoice &ch, int cfg, const GemmArgs &a, hipStream_t s);
// per-row scales of a linear layer's A operand (rows of K contiguous floats, the addressing of `a`): out[m] = rowscale_of(max |a|)
void launch_rowscale(const GemmArgs &a, float *out, hipStream_t s);
// the fp16 three-term split applied to an array under ONE scale 2^sexp: planes [3][n] fp16 bit patterns (unit test of the split)
void launch_split3h_debug(const float *d_x, i64 n, int sexp, unsigned short *d_planes, hipStream_t s);
// the kernels' three-term activation split applied to an array: planes [3][n] bf16 bit patterns (unit test of the split)
void launch_split3_debug(const float *d_x, i64 n, unsigned short *d_planes, hipStream_t s);

struct ReduceArgs
{
    const float *rowstat;
    float *out;
    int B, R, NB, G0;
    double count;
    int mode;
    float eps;
    double *scratch;
    int nchunk;
};
void launch_stats_reduce(const ReduceArgs &a, hipStream_t s);

struct StftArgs
{
    const float *mix;
    float *x, *rowstat, *rowstatT;
    int B, T, seg, pad;
    const float *window, *twiddle;
};
void launch_stft(const StftArgs &a, hipStream_t s);

struct LnArgs
{
    const float *x;
    float *y;
    int rows, D, rowsPerBatch;
    const float *w, *b, *pe;
    float eps;
};
void launch_layernorm(const LnArgs &a, hipStream_t s);

struct GnArgs
{
    const float *x;
    float *y;
    const float *res;
    int B, rows, C;
    const float *stats, *w, *b;
};
void launch_gn_apply(const GnArgs &a, hipStream_t s);

struct AttnArgs
{
    const float *q, *k, *v;
    float *o;
    int ldq, ldk, ldv, ldo;
    i64 qB, kB, vB, oB;
    int B, Tq, Tk, H, hs;
    float scale;
    unsigned nQt; // query tiles per (batch, head) (filled by launch_attention)
    int xcdMap;   // 1: all query tiles of one (batch, head) on ONE XCD (its K/V stay in that XCD's L2)
    // LocalState attention of Demucs v3 (launch_attention_local): decay logits of query s, head h, term n at
    // decay[b * dB + s * ldd + 4 h + n]; null for the transformer's attention
    const float *decay;
    int ldd;
    i64 dB;
    // bf16 operand planes written by the K / V projections (plan.h Attention::kpl / vt), or null
    const unsigned short *kpl, *vt;
    i64 kvPlane; // elements per plane = B * Tk * H * hs
    int form;    // launch_attention / launch_attention_split: the AttentionForm (attention_select.h) the plan chose for this op
};

void launch_attention(const AttnArgs &a, hipStream_t s);
// GEMM_BF16X3 contexts: the same attention with both products on the bf16 matrix pipe through exact three-term operand
// splits (attention_split.hip); -1 = no kernel for this head dim. dry = availability check only
int launch_attention_split(const AttnArgs &a, hipStream_t s, bool dry = false);
// Demucs v3 LocalState (src/layers.cpp:533-721) on the same flash kernel: scores + decay penalty, diagonal = -100;
// head dims 48 / 96. Returns -1 for other shapes.
int launch_attention_local(const AttnArgs &a, hipStream_t s);

struct IstftArgs
{
    const float *x, *stats;
    float *frames;
    int B, T, S;
    const float *window, *twiddle;
};
void launch_istft(const IstftArgs &a, hipStream_t s);

struct OlaArgs
{
    const float *frames, *xt, *statsT, *wss;
    float *out;
    int B, T, S, seg, pad;
};
void launch_ola(const OlaArgs &a, hipStream_t s);
// ISTFT + overlap-add + time-branch sum in one kernel (the inverse frames stay in registers)
struct IstftOlaArgs
{
    const float *x, *stats, *xt, *statsT, *wss, *window, *twiddle;
    float *out;
    int B, T, S, seg, pad;
    int nch, fpc; // frame chunks per (batch, source) and frames per chunk (filled by the launcher)
    const float *rden; // (1 / 4096) / (wss + 1e-8), same indexing as wss (plan.h Ola::rden)
};
void launch_istft_ola(const IstftOlaArgs &a, hipStream_t s);

// ---- Demucs v3 (v3.hip; plan.h OP_GROUP_STATS / OP_GN_ACT / OP_LSTM / OP_LOCAL_ATTN)
struct GroupStatsArgs
{
    const float *x;
    float *out;
    double *partials; // [B][G][32 chunks][2]
    int B, rows, C, G;
    float eps;
};
void launch_group_stats(const GroupStatsArgs &a, hipStream_t s);
struct GnActArgs
{
    const float *x;
    float *y;
    const float *stats, *res, *w, *b, *scale;
    int B, rowsIn, C, G, mode, rowOff, rowsOut;
};
void launch_gn_act(const GnActArgs &a, hipStream_t s);
struct LstmArgs
{
    const float *xproj, *whh;
    float *out;
    void *gran;       // h exchange granules, lstm_sync_floats(B, H) floats; zeroed by the launcher
    unsigned *status; // raised when a bounded spin timed out (checked by dmx_ctx_synchronize)
    int B, T, H;
};
int launch_lstm(const LstmArgs &a, hipStream_t s); // -1: unsupported hidden size; -2: the grid of spinning workgroups cannot be co-resident on this device
struct LocalAttnArgs
{
    const float *qkvd;
    float *out;
    int B, T, H, ld;
};
int launch_local_attn(const LocalAttnArgs &a, hipStream_t s); // -1: unsupported shape

// ---- track level (model_apply.cpp:60-288) ----
// Every track-level kernel serves several tracks per launch (dmx_tracks_infer); one track is the T = 1 case. The per-track
// tables travel by value in the kernel arguments (no device table, no host synchronisation between launches); each stays
// well inside HIP's 4 KB kernel-argument limit.
struct TrackStatsTable
{
    static const int kMax = 32;
    const float *audio[kMax]; // interleaved [n][2]
    i64 n[kMax];
    float *stats[kMax];       // 2 floats: mean, std
};
// partial (sum, sumsq) of the mono reference (mean over channels) of tracks 0..T-1: grid (nblk, T), track t's block b covers
// samples [b*per, (b+1)*per), per = ceil(n_t / nblk); partials [T][nblk][2]
void launch_track_stats(const TrackStatsTable &t, int T, double *partials, int nblk, hipStream_t s);
// stats_t[0]=mean, stats_t[1]=std (unbiased) from partials, blocks summed in order
void launch_track_stats_final(const TrackStatsTable &t, int T, const double *partials, int nblk, hipStream_t s);
// one track (dmx_track_stats_device)
void launch_track_stats(const float *audio, i64 n, double *partials, int nblk, hipStream_t s);
void launch_track_stats_final(const double *partials, int nblk, i64 n, float *stats, hipStream_t s);
// chunk extraction: mixes[i] = segment `seg` of the normalised, shifted, zero-padded track of item i, centred in a zero
// segment (segment_inference, model_apply.cpp:250-288). The items of one launch may come from different tracks.
struct TrackSegItem
{
    const float *audio; // interleaved [n][2]
    const float *stats;
    i64 n;
    int shift;
    int seg; // segment index within the track
};
struct TrackSegIdx
{
    static const int kMax = 64; // = the largest max_batch (dmx_ctx_create)
    TrackSegItem v[kMax];
};
void launch_track_gather(const TrackSegItem *items, int nIdx, i64 seg, i64 stride, float *mixes, hipStream_t s);
// one track: segIdx is a HOST array
void launch_track_gather(const float *audio, i64 n, const float *stats, int shiftOffset, i64 seg, i64 stride,
                         i64 len, const int *segIdx, int nIdx, float *mixes, hipStream_t s);
// overlap-add of segment outputs [.][S][2][seg] into planes [planeBase, planeBase + nPlanes) (plane = stem*2 + channel) and
// samples [i0, i1) of out, per track of the table (grid z).
// layout 0: planar [S][2][n]; layout 1: Eigen column-major image (s + S*(c + 2*i))
// Segment g of a track is block blk = slot0 + (g - gBase) of segOut, less `ring` when blk >= ring (a ring of segment
// blocks shared by several tracks); every segment the samples [i0, i1) touch must be there.
struct TrackOlaEntry
{
    const float *segOut;
    const float *stats;
    float *out;
    i64 n, len, i0, i1; // len: shifted length (dmx_track_geometry)
    i64 gBase, slot0;
    int nSeg, shift;
};
struct TrackOlaTable
{
    static const int kMax = 32;
    TrackOlaEntry e[kMax];
};
void launch_track_ola(const TrackOlaEntry *entries, int T, int S, i64 seg, i64 stride, i64 ring, int layout, int planeBase,
                      int nPlanes, hipStream_t s);
// one track; gBase: segOut[0] is segment gBase (a device that holds only a stretch of the segments)
void launch_track_ola(const float *segOut, int nSeg, int S, i64 seg, i64 stride, i64 len, i64 n, int shiftOffset,
                      const float *stats, float *out, int layout, int planeBase, int nPlanes, i64 i0, i64 i1, hipStream_t s,
                      int gBase = 0);
// the shifts ensemble (dmx_tracks_infer_opts, N >= 2 copies): per output sample, the normalised overlap-add value of each copy
// k (track_ola_kernel's weights, order and skips, on copy k's own shifted geometry) is summed in increasing k, then
// (e / N) * std + mean. A track's segments are items dealt in (row g, copy k) order, copies with nseg_k <= g absent:
//   item(g, k) = sum_k' min(g, nseg_k') + #{k' < k : nseg_k' > g}   (= g N + k while g < min_k nseg_k).
// Item `it` of a piece's track is ring block slotLo + (it - itemLo), less `ring` when that is >= ring.
struct TrackEnsPiece
{
    const float *stats;
    float *out;
    i64 n, i0, i1;
    i64 itemLo, slotLo; // the lowest item the piece reads, and its ring block
    int nMin, nTail;    // rows g < nMin hold all N copies; rows [nMin, nMin + nTail) are the tail (nTail N <= kMaxTail)
};
struct TrackEnsCopy
{
    int shift, nseg;
};
struct TrackEnsTable
{
    static const int kMaxPieces = 16, kMaxCopies = 256; // a launch carries min(kMaxPieces, kMaxCopies / N) pieces
    // tail rows x copies of a piece's track, tabulated in LDS per block: nTail <= ceil(22049 / stride) + 1 <= 55 at the
    // smallest segment (4096) and overlap 0.9, times N <= 32
    static const int kMaxTail = 2048;
    TrackEnsPiece p[kMaxPieces];
    TrackEnsCopy c[kMaxCopies]; // piece z's copies: c[z N + k]
};
void launch_track_ola_ens(const TrackEnsPiece *pieces, const TrackEnsCopy *copies, int P, int N, const float *segOut, int S,
                          i64 seg, i64 stride, i64 ring, int layout, int planeBase, int nPlanes, hipStream_t s);
// a bag of Q models (dmx_tracks_infer_bag; specification: DESIGN.md section 2.9, restated in tests/bag_spec.py): per output
// sample of stem s, model q's value e_q is track_ola_ens_kernel's e / N on q's own copies (v_0 itself when N = 1), read from
// q's own ring of segment blocks; over the models with w[q][s] != 0 in increasing q, a = w e_q for the first and
// fmaf(w, e_q, a) after it, W the fp32 sum of those weights in the same order; out = (a / W) * std + mean. A model with
// w[q][s] == 0 is not read for stem s: the diagonal bag moves the bytes of a plain overlap-add.
// Model q's items of a piece's track follow launch_track_ola_ens's rule on q's copies c[(z Q + q) N + k]; item `it` is block
// slotLo + (it - itemLo) of ring q, less ringBlocks[q] when that is >= ringBlocks[q].
struct TrackBagPiece
{
    const float *stats;
    float *out;
    i64 n, i0, i1;
};
struct TrackBagModel // one model's view of a piece
{
    int itemLo, slotLo; // the lowest item of the model the piece reads, and its ring block
    int nMin, nTail;    // as TrackEnsPiece, over the model's own copies
};
struct TrackBagTable
{
    // a launch carries min(kMaxPieces, kMaxModels / Q, kMaxCopies / (Q N)) pieces
    static const int kMaxPieces = 8, kMaxModels = 32, kMaxCopies = 256, kMaxBag = 8, kMaxStems = 8;
    // tail rows x copies, tabulated in LDS per block for the models that contribute to the block's stem only; the launch
    // sizes the table (dynamic LDS) from its own pieces, so an ordinary bag (a few hundred entries) keeps full occupancy
    static const int kMaxTail = 12288; // 48 KB
    TrackBagPiece p[kMaxPieces];
    TrackBagModel m[kMaxModels]; // piece z's models: m[z Q + q]
    TrackEnsCopy c[kMaxCopies];  // piece z's copies: c[(z Q + q) N + k]
    float w[kMaxBag * kMaxStems]; // w[q S + s]
    const float *ring[kMaxBag];
    i64 ringBlocks[kMaxBag];
};
// LDS entries a launch over these pieces needs (the largest, over pieces and stems, of the contributing models' nTail N);
// -1: a cap of the kernel is exceeded (Q, S, Q N, a piece's tail). The host path checks this before any GPU work.
i64 track_ola_bag_tail_entries(const TrackBagModel *models, int P, int Q, int N, int S, const float *w);
// false: nothing was launched (a cap exceeded: see track_ola_bag_tail_entries)
bool launch_track_ola_bag(const TrackBagPiece *pieces, const TrackBagModel *models, const TrackEnsCopy *copies, int P, int Q, int N,
                          const float *w, const float *const *rings, const i64 *ringBlocks, int S, i64 seg, i64 stride, int layout,
                          int planeBase, int nPlanes, hipStream_t s);
// ---- the PCM output stage (pcm.hip; specification: DESIGN.md section 2.8, restated in tests/pcm_spec.py) ----
// S x 2 fp32 planes (plane p = stem*2 + channel at planes + p*planeStride) -> nOut outputs of interleaved stereo PCM.
// stem < 0: output o is stem o; else output 0 is stem `stem` and output 1 the sum of the other stems in increasing order.
// Output o's bytes start at pcm + o*outStride (outStride a multiple of 16, pcm 16-byte aligned: the kernel stores whole
// dwords only, and the last dword of an odd 24-bit track ends in two zero bytes of that padding). A piece is the frames
// [i0, i1) of one track: i0 a multiple of 4, i1 a multiple of 4 or n.
struct PcmPiece
{
    const float *planes;
    unsigned char *pcm;
    unsigned *peaks; // nOut bit patterns of non-negative floats, zeroed before the track's first piece
    i64 n, planeStride, outStride, i0, i1;
};
struct PcmTable
{
    static const int kMax = 32;
    PcmPiece p[kMax];
};
// peaks[o] = max(peaks[o], largest |x| of output o over the piece, NaN ignored), per piece of the table
void launch_pcm_peak(const PcmPiece *pieces, int P, int S, int stem, hipStream_t s);
// clip (DMX_CLIP_*; rescale reads peaks[o]: every piece of the track must have been through launch_pcm_peak) and
// quantisation (DMX_PCM_*) of the pieces' frames
void launch_pcm_encode(const PcmPiece *pieces, int P, int S, int stem, int encoding, int clip, hipStream_t s);
// the gain table of a remix (dmx_remix_spec, checked): output o = the sum over the sources with g[o][s] != 0, in increasing
// s, of g[o][s] * source s; sources 0..S-1 are the stems, source S the mixture. Passed in the kernel arguments.
struct PcmGains
{
    static const int kMaxOut = 8, kMaxSrc = 7; // DMX_MAX_OUTPUTS, and 6 stems + the mixture
    float g[kMaxOut][kMaxSrc];
    int nOut, S;
};
struct RemixPiece : PcmPiece
{
    const float *mix; // the track interleaved [n][2], any 4-byte alignment; may be NULL when no row uses the mixture
};
struct RemixTable
{
    static const int kMax = 32;
    RemixPiece p[kMax];
};
void launch_remix_peak(const RemixPiece *pieces, int P, const PcmGains &G, hipStream_t s);
void launch_remix_encode(const RemixPiece *pieces, int P, const PcmGains &G, int encoding, int clip, hipStream_t s);
// ---- the loudness stage (loudness.hip; specification: DESIGN.md section 2.14, restated in tests/loudness_spec.py) ----
struct LoudPiece : RemixPiece
{
    const float *gains; // G.nOut gains on the device (launch_loud_gain)
};
struct LoudTable
{
    static const int kMax = 32;
    LoudPiece p[kMax];
};
// launch_remix_encode with every gathered sample multiplied by its output's gain before clip (pcm.hip)
void launch_loud_encode(const LoudPiece *pieces, int P, const PcmGains &G, int encoding, int clip, hipStream_t s);
// (LoudPlan and the pure host functions: loudness_plan.h)
// measures the G.nOut outputs of the piece's frames [0, lp.n): signal o uses the workspace slot work + (slot0 + o) *
// loud_workspace_bytes(n) (16-byte aligned). Four launches on s. eOut: NULL, or G.nOut x 2 x H hop energies on the device;
// resOut: NULL, or G.nOut entries {int32 lufs_c, float 0, double L}. marks: NULL, or five events around the four launches.
void launch_loud_measure(const RemixPiece &pc, const PcmGains &G, const LoudPlan &lp, unsigned char *work, int slot0, double *eOut,
                         void *resOut, hipStream_t s, hipEvent_t *marks = nullptr);
// behind the measurement of nOut outputs (slots 0 .. nOut - 1) and the mixture (slot nOut) and behind the peak kernel: the gains
// (DMX_LOUD_*), peaks[o] *= gain, and the report of nOut + 1 entries; all on the device, one launch
void launch_loud_gain(const unsigned char *work, i64 slotBytes, int nOut, unsigned *peaks, int mode, int targetC, float maxPeak,
                      const float *table, float *gains, void *report, hipStream_t s);
// launch_loud_gain with the ceiling read from the true peaks tp[o] (launch_true_peak) in place of the sample peaks; peaks[o] still
// becomes the gained SAMPLE peak
void launch_loud_gain_tp(const unsigned char *work, i64 slotBytes, int nOut, unsigned *peaks, const unsigned *tp, int mode, int targetC,
                         float maxPeak, const float *table, float *gains, void *report, hipStream_t s);
// ---- the meters (meters.hip; specification: DESIGN.md section 2.15, restated in tests/meters_spec.py) ----
// (TpFilter and the pure host functions: meters_plan.h)
// peaks[o] of each piece = max(peaks[o], the true peak of output o over the frames the piece evaluates): the pieces' `peaks`
// point at the bit patterns of the TRUE peaks, zeroed before the track's first piece. All pieces are at the filter's rate.
void launch_true_peak(const RemixPiece *pieces, int P, const PcmGains &G, const TpFilter &f, hipStream_t s);
// behind launch_loud_measure of nSignals signals in the slots slot0 ..: out[o] = {tp[o], lra_c, max_momentary_c, max_short_c},
// nSignals entries of dmx_meters_result on the device. One launch.
void launch_meters(const unsigned char *work, int slot0, int nSignals, const LoudPlan &lp, const unsigned *tp, void *out, hipStream_t s);
// ---- the look-ahead peak limiter (limiter.hip; specification: DESIGN.md section 2.16, restated in tests/limiter_spec.py) ----
// (the tables, the slopes and the workspace: limiter_plan.h)
// one job: the envelopes over the G.nOut outputs of the piece's frames [0, pc.n), each output o under its gain (gains[o] on the
// device, or gainImm where gains is null). link: one envelope over all outputs (DMX_LOUD_MIXTURE), else one per output; envelope
// e uses the workspace work + e * lim_workspace_bytes(n). tables: the kLimTableWords words of lim_tables on the device. res:
// G.nOut entries of dmx_limit_result on the device, zeroed here. f.F > 1: the level takes the interpolated phases
// (DMX_LOUD_TRUE_PEAK) and res[o].true_peak_out is measured. Three launches, or four; marks: NULL, or five events around them.
struct LimJob
{
    RemixPiece pc;
    PcmGains G;
    const float *gains;
    float gainImm, ceiling;
    int qa, qr, link;
    unsigned char *work;
    const int32_t *tables;
    void *res;
};
void launch_limit(const LimJob &job, const TpFilter &f, bool truePeak, hipStream_t s, hipEvent_t *marks = nullptr);
// launch_loud_encode with every gained sample multiplied by its frame's limiter gain before clip (pcm.hip): output o reads the
// plane gplane + o * gplaneStride (fp32 per frame, 16-byte aligned; stride 0: the outputs share one plane)
struct LimitPiece : LoudPiece
{
    const float *gplane;
    i64 gplaneStride;
};
struct LimitTable
{
    static const int kMax = 32;
    LimitPiece p[kMax];
};
void launch_limit_encode(const LimitPiece *pieces, int P, const PcmGains &G, int encoding, int clip, hipStream_t s);
// ---- the track path's converter (resample.hip) ----
// outputs [k0, k1) of the conversion of `planes` planar planes (plane p = stem*2 + channel at src + p*n, n samples each):
// output k of plane p goes to dst + stem*dstStem + channel*dstChan + k*dstStep (planar [S][2][n_out]: 2 n_out, n_out, 1; the
// Eigen image s + S*(c + 2*k): 1, S, 2 S). The value of an output is dmx_resample_device's, whatever the cut into pieces.
struct ResamplePiece
{
    const float *src;
    float *dst;
    i64 n, dstStem, dstChan, dstStep, k0, k1;
};
struct ResampleTable
{
    static const int kMax = 32;
    ResamplePiece p[kMax];
    int blk0[kMax + 1]; // piece z owns the workgroups [blk0[z], blk0[z + 1]) of the grid's x
};
// pure host: DMX_OK when the filter of the ratio exists and a launch over `planes` planes fits the LDS, else the error
int resample_check(int rateIn, int rateOut, int planes);
// the device's copy of the filter, made on first use (a blocking upload): call it before the work that must not stall
int resample_prepare(int device, int rateIn, int rateOut);
// one launch per ResampleTable::kMax non-empty pieces, all of one ratio; DMX_OK or an error
int launch_resample_pieces(int device, const ResamplePiece *pieces, int P, int planes, int rateIn, int rateOut, hipStream_t s);
// ---- the FLAC input stage (flac_in.hip; specification: DESIGN.md section 2.12, restated in tests/flac_in_spec.py) ----
} // namespace dmx
struct dmx_flac_info;
namespace dmx
{
// 0 and *info, or -1 and a message (pure host)
int flac_in_probe(const void *file, int64_t bytes, dmx_flac_info *info, char *msg, size_t msgLen);
// -1: an info the kernels do not take
int64_t flac_in_workspace_bytes(const dmx_flac_info *info, int64_t bytes);
// five launches on s; out 16-byte aligned and padded to 16 bytes, status {DMX_FLAC_*, good}, work 16-byte aligned; -1 as above
// (marks: NULL, or six events recorded around the five launches)
int launch_flac_decode(const unsigned char *file, long long bytes, const dmx_flac_info *info, int encoding, void *out, long long *status,
                       void *work, hipStream_t s, hipEvent_t *marks = nullptr);

// ---- the FLAC output stage (flac.hip; specification: DESIGN.md section 2.11, restated in tests/flac_spec.py) ----
// an upper bound of the encoded stream of n frames of `bits` (16 | 24) bit stereo, a multiple of 16; -1: bad argument
i64 flac_bound(int bits, i64 n);
// the workspace ONE output needs (a multiple of 16): the table of frame lengths, their offsets, one bound-sized slot per frame
i64 flac_workspace_bytes(int bits, i64 n);
// nOut outputs of interleaved PCM as pcm.hip writes it (output o at pcm + o*pcmStride, 16-byte aligned) -> nOut .flac files
// (output o at out + o*outStride, any alignment), their byte counts in sizes[o]; work: nOut * flac_workspace_bytes, 16-byte
// aligned. Three launches on s, no host synchronisation. level 0 | 1 | 2: FIXED predictors alone, + LPC order 8, + LPC orders 8
// and 12 (tests/flac_lpc_spec.py). marks: null, or four events recorded around the three launches (tools/flac_bench.py).
void launch_flac_encode(const unsigned char *pcm, i64 pcmStride, int bits, i64 n, int rate, int nOut, unsigned char *out, i64 outStride,
                        long long *sizes, unsigned char *work, hipStream_t s, int level = 0, hipEvent_t *marks = nullptr);
// dst[r*dpitch + i] = src[r*spitch + i], r < rows, i < width (floats)
void launch_copy_rows(float *dst, i64 dpitch, const float *src, i64 spitch, i64 width, int rows, hipStream_t s);
// dst[i] = fp16 bit pattern of src[i], round to nearest even (the opt-in fp16 weight plane, api.cpp dmx_model_fp16_plane)
void launch_f32_to_f16(const float *src, unsigned short *dst, i64 n, hipStream_t s);
// interleaved <-> planar helpers
void launch_planar_to_interleaved(const float *src, float *dst, i64 n, hipStream_t s);


#ifdef __HIPCC__
// erf for the exact GELU 0.5 v (1 + erf(v / sqrt 2)) (/root/reference/src/layers.hpp:51-63, conv.hpp:203-204).
// Branch-free two-range minimax fit, max abs error 9.7e-8 (~1.6 ulp at 1) against scipy.special.erf over
// [-6, 6] in fp32 arithmetic (fit + check: DESIGN.md section 2.2): |x| < 0.92: x * A(x^2);
// else sign(x) * (1 - 2^B(min(|x|, 4))). 19 VALU instructions incl. one v_exp_f32; the ocml erff costs
// ~45 on a wave whose lanes straddle its two ranges, and a 128x128 GELU epilogue evaluates 64 per lane.
__device__ __forceinline__ float dmx_erff(float x)
{
    const float t = fminf(fabsf(x), 4.0f);
    const float s = x * x;
    float a = fmaf(-0.0005843715625815094f, s, 0.004958246368914843f);
    a = fmaf(a, s, -0.026736384257674217f);
    a = fmaf(a, s, 0.11280667781829834f);
    a = fmaf(a, s, -0.3761231601238251f);
    a = fmaf(a, s, 1.1283791065216064f);
    a *= x;
    float b = fmaf(0.0002812488819472492f, t, -0.004376694560050964f);
    b = fmaf(b, t, 0.03201308846473694f);
    b = fmaf(b, t, -0.149833083152771f);
    b = fmaf(b, t, -0.9193801283836365f);
    b = fmaf(b, t, -1.6268224716186523f);
    b = fmaf(b, t, -0.0002986486360896379f);
    const float r = copysignf(1.0f - __builtin_amdgcn_exp2f(b), x);
    return t < 0.92f ? a : r;
}
__device__ __forceinline__ float dmx_gelu(float v) { return 0.5f * v * (1.0f + dmx_erff(v * 0.70710678118654752440f)); }
#endif

} // namespace dmx
