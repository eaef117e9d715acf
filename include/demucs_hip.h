/* demucs_hip.h — C ABI of the MI355X-native HTDemucs inference path.
 *
 * This is the drop-in boundary for the hot path of sevagh/demucs.cpp (reference at
 * /root/reference, citations below are file:line in that tree). The reference has no
 * FFI/plugin registry: its boundary is the C++ API in namespace demucscpp
 * (src/model.hpp:649-666). Each entry point here replaces one of those functions; the
 * header-only C++ shim demucs_cpp_amd/host/demucscpp_hip.hpp restates the reference
 * signatures on top of this ABI, and INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions: plain C, opaque handles, int status (0 = DMX_OK), no exceptions or C++
 * types across the ABI, dmx_last_error() gives the message of the last failure on the
 * calling thread. All audio is fp32, 44.1 kHz, stereo. A context is NOT thread-safe;
 * create one context per host thread / stream, or use a dmx_engine, which serialises internally (the model handle is immutable after load
 * and may be shared, like the reference's `const demucs_model&`).
 *
 * There is NO CPU fallback: every entry point that computes fails with
 * DMX_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef DEMUCS_HIP_H
#define DEMUCS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C"
{
#endif

#define DMX_OK 0
#define DMX_ERR_IO 1          /* weight file cannot be opened / truncated            */
#define DMX_ERR_FORMAT 2      /* bad magic, unknown tensor, wrong element count       */
#define DMX_ERR_NO_DEVICE 3   /* no usable HIP device (there is no CPU fallback)      */
#define DMX_ERR_HIP 4         /* HIP runtime error                                    */
#define DMX_ERR_ARG 5         /* invalid argument                                     */
#define DMX_DEBUG_NO_KERNEL 6 /* dmx_debug_run_op_as: no such kernel, nothing launched */

#define DMX_SEGMENT_SAMPLES 343980 /* 7.8 s @ 44.1 kHz, src/model.hpp:652, :20        */
#define DMX_MAX_SHIFT 22050        /* 0.5 s, src/model.hpp:654                         */
#define DMX_MAX_SHIFTS 32          /* copies of the shifts ensemble (dmx_tracks_infer_opts) */
#define DMX_MAX_OVERLAP 0.9f       /* largest segment overlap (10 segments per sample)  */

/* Audio memory layouts at the boundary.
 * DMX_LAYOUT_EIGEN : the exact memory image of the reference's Eigen types
 *     input  Eigen::MatrixXf(2, N)  column-major  = interleaved stereo L0 R0 L1 R1 ...
 *     output Eigen::Tensor3dXf(S, 2, N) column-major: element (s,c,n) at s + S*(c + 2n)
 *     (src/model_apply.cpp:60-62; cli-apps/demucs.cpp:21-76,185-204)
 * DMX_LAYOUT_PLANAR: input [2][N], output [S][2][N] row-major (cf. the wasm glue's
 *     per-stem planar pointers, src_wasm/demucs.cpp:82-93). */
#define DMX_LAYOUT_EIGEN 0
#define DMX_LAYOUT_PLANAR 1

    typedef struct dmx_model dmx_model;
    typedef struct dmx_ctx dmx_ctx;

    /* progress callback, same meaning as demucscpp::ProgressCallback (src/model.hpp:17):
     * fraction in [0,1] and a message; invoked synchronously on the calling thread. */
    typedef void (*dmx_progress_fn)(float progress, const char *message, void *user);

    const char *dmx_last_error(void);
    int dmx_device_count(void);

    /* Replaces demucscpp::load_demucs_model (src/model.hpp:649-650, src/model_load.cpp:50) and
     * demucscpp_v3::load_demucs_v3_model (src/model.hpp:1396-1397, src/model_load.cpp:1302):
     * reads a dmc4 / dmc6 (HTDemucs v4) or dmc3 (Demucs v3 hdemucs_mmi) ggml-style fp16 weight file, repacks it
     * and uploads it to `device`; the magic selects the architecture. Same failure cases as the reference
     * (open failure, bad magic, unknown tensor name, element-count mismatch) plus "tensor missing". */
    int dmx_model_load(const char *model_file, int device, dmx_model **out);
    void dmx_model_free(dmx_model *m);
    /* the same weights on another device, without re-reading / re-packing the file (one replica per GPU) */
    int dmx_model_clone(const dmx_model *src, int device, dmx_model **out);
    int dmx_model_n_sources(const dmx_model *m); /* 4 or 6 (demucs_model::is_4sources) */
    int dmx_model_n_tensors(const dmx_model *m);
    /* 4: HTDemucs v4 (dmc4 / dmc6 file); 3: Demucs v3 hdemucs_mmi (dmc3 file). Every other entry point takes either. */
    int dmx_model_arch(const dmx_model *m);
    int dmx_model_device(const dmx_model *m);

    /* Execution context = the reference's demucs_segment_buffers + stft_buffers
     * (src/model.hpp:569-647, src/dsp.hpp:20-101) for `max_batch` segments in flight,
     * allocated once in HBM. segment_samples = 0 selects DMX_SEGMENT_SAMPLES. */
    int dmx_ctx_create(const dmx_model *m, int64_t segment_samples, int max_batch, dmx_ctx **out);
    /* How a context forms the fp32 products of its convolutions / linear layers (the reference does them in fp32 through
     * Eigen's GEMM, src/conv.hpp:71-524, src/layers.cpp:426-440). All modes take and return fp32 and keep every other
     * operation (normalisations, activations, FFTs, reductions) in fp32:
     *   DMX_GEMM_F32    v_mfma_f32_16x16x4_f32: each output is one k-ordered fp32 fmaf chain;
     *   DMX_GEMM_BF16X3 exact operand splits on the bf16 matrix pipe: an activation is the sum of three bf16 terms
     *                   (a = a1 + a2 + a3, round-to-nearest splits: exact for 2^-109 <= |a| <= 3.3895e38, within 2^-125 below,
     *                   non-finite above), a weight - an fp16
     *                   number in the file - of two (w = w1 + w2: exact), and a w is accumulated in fp32 from five exact
     *                   partial products; the dropped a3 w2 is <= 2^-24 |a w|. MI355X's bf16 MFMA
     *                   rate is 16x its fp32 MFMA rate. Ops whose weights are not fp16-exact stay on the fp32 kernels.
     *   DMX_GEMM_FP16X3 OPT-IN, never the default, reported separately by bench.py. As DMX_GEMM_BF16X3, except that the
     *                   transformer's linear layers take their weights - fp16 numbers in the model files - as ONE exact fp16
     *                   term and split each activation row, multiplied by a power of two chosen from the row's largest
     *                   magnitude (it lands in [2^14, 2^15): nothing can overflow), into three fp16 terms: three
     *                   v_mfma_f32_16x16x32_f16 per product term instead of five bf16 MFMAs. BOUNDED, not exact: an element
     *                   more than 2^15 times smaller than the largest of its row loses bits, at most 2^-39 of that largest
     *                   (the fp32 and bf16x3 modes have no such term); batch size and sharding still do not change a bit.
     * dmx_ctx_create uses the process default: DMX_GEMM_BF16X3 unless the environment says DMX_GEMM=f32 / fp16x3 (read once),
     * or what dmx_set_default_gemm set. A context keeps its mode for life; contexts of different modes may coexist on one
     * model. (No reference counterpart.) */
#define DMX_GEMM_F32 0
#define DMX_GEMM_BF16X3 1
#define DMX_GEMM_FP16X3 2
    int dmx_ctx_create_gemm(const dmx_model *m, int64_t segment_samples, int max_batch, int gemm, dmx_ctx **out);
    int dmx_ctx_gemm(const dmx_ctx *c);
    int dmx_default_gemm(void);
    int dmx_set_default_gemm(int gemm); /* also what dmx_engine_create gives its contexts */
    void dmx_ctx_free(dmx_ctx *c);
    int64_t dmx_ctx_segment_samples(const dmx_ctx *c);
    int dmx_ctx_max_batch(const dmx_ctx *c);
    int64_t dmx_ctx_arena_bytes(const dmx_ctx *c);
    int dmx_ctx_synchronize(dmx_ctx *c);
    /* Order the context's device work on a caller-owned HIP stream (a hipStream_t passed as void*,
     * e.g. the stream a framework issues its own kernels and RCCL collectives on): every *_device
     * entry point then enqueues behind / ahead of the caller's work on that stream and no host
     * synchronisation is needed around the calls. NULL returns to the context's own stream.
     * The context synchronises its current stream before switching. (No reference counterpart:
     * the Eigen path is synchronous host code.) */
    int dmx_ctx_set_stream(dmx_ctx *c, void *hip_stream);
    /* Rebind the context to another model of the same architecture on the same device (the arena and the
     * plan are shared; the four fine-tuned models of demucs_ft.cpp:136-184 run through one context). */
    int dmx_ctx_set_model(dmx_ctx *c, const dmx_model *m);

    /* Replaces demucscpp::model_inference (src/model.hpp:662-666,
     * src/model_inference.cpp:48): one full segment, host pointers.
     *   mix : 2 x segment_samples in `layout`; out : S x 2 x segment_samples in `layout`. */
    int dmx_segment_infer(dmx_ctx *c, const float *mix, float *out, int layout);

    /* Same on device memory, `batch` (<= max_batch) segments, asynchronous on the
     * context's stream (pair with dmx_ctx_synchronize). The kernels read d_mix and write d_out
     * directly (no staging copy): both must be 16-byte aligned and stay valid until the work completes:
     *   d_mix : [batch][segment_samples][2] interleaved, d_out : [batch][S][2][segment_samples] planar. */
    int dmx_segment_infer_device(dmx_ctx *c, const float *d_mix, float *d_out, int batch);

    /* Replaces demucscpp::demucs_inference (src/model.hpp:658-660,
     * src/model_apply.cpp:60-288): normalise, shift, overlapping-segment loop,
     * overlap-add, trim, de-normalise. shift_offset in [0, DMX_MAX_SHIFT) replaces the
     * reference's unseeded rand() % 22050 (src/model_apply.cpp:114); pass -1 to draw
     * rand() % 22050 like the reference.  audio : 2 x n, out : S x 2 x n, both `layout`. */
    int dmx_track_infer(dmx_ctx *c, const float *audio, int64_t n, int shift_offset, float *out, int layout,
                        dmx_progress_fn progress, void *user);

    /* Several tracks in one call (no reference counterpart: replaces a loop of demucs_inference calls, one per input file).
     * Track t: audio[t] 2 x n[t], out[t] S x 2 x n[t], both `layout`; shift_offsets NULL or -1 entries: rand() % 22050
     * drawn in track order, like successive dmx_track_infer calls. Every out[t] is bit-identical to
     * dmx_track_infer(c, audio[t], n[t], shift_offsets[t], out[t], layout, ...) on a context of the same max_batch.
     * The tracks' segments are laid end to end in track order and dealt in batches of max_batch (a batch may mix tracks);
     * every batch is enqueued without waiting on the one before, and each track - or each finished piece of a long one -
     * is overlap-added and copied out underneath later batches. A track is uploaded when its first batch is enqueued.
     * Device memory beyond the context's arena is bounded by max_batch and the longest track, whatever the number of tracks:
     *   2 max_batch segment outputs (S x 2 x segment_samples floats each) + 2 max_batch segment inputs, and at most
     *   2 max_batch track slots of (S x 2 + 4) x n_max floats (n_max = the longest track; 2 x n_max of it only for
     *   the planar layout), held from the batch of a track's first segment until its last copy-out has completed.
     * Arguments are checked before any GPU work (n_tracks >= 1, no null pointer, n[t] >= 2, shift in [-1, 22050)); the
     * error message names the track. Progress is the fraction of all segments done (non-decreasing, last value 1).
     * Copies into pageable memory block the calling thread, as in dmx_track_infer. dmx_track_infer is the n_tracks = 1 case. */
    int dmx_tracks_infer(dmx_ctx *c, int n_tracks, const float *const *audio, const int64_t *n, const int *shift_offsets,
                         float *const *out, int layout, dmx_progress_fn progress, void *user);

    /* dmx_tracks_infer with demucs's two inference-time quality options (apply_model(shifts=, overlap=); the reference fixes
     * shifts = 1 and overlap = 0.25). Each track is run as n_shifts copies, copy k shifted by shift_offsets[t*n_shifts + k]
     * (NULL or -1 entries: rand() % 22050, drawn in row-major (track, copy) order), each cut into segments at the stride
     * (int64)((1 - overlap) * segment_samples) evaluated in fp32. Per output sample, each copy's normalised overlap-add value
     * (the triangle-weighted sum over its segments in segment order, divided by the weight sum) is summed in fp32 in
     * increasing copy order, then out = (sum / n_shifts) * std + mean: demucs's `out += shifted_out; out /= shifts` before
     * de-normalisation. n_shifts = 1 and overlap = 0.25 give the bits of dmx_tracks_infer.
     *   1 <= n_shifts <= DMX_MAX_SHIFTS, 0 <= overlap <= DMX_MAX_OVERLAP (finite), shift_offsets in [-1, 22050).
     * Arguments are checked before any GPU work and nothing is written on error; the message names the track and the copy
     * ("track 2, shift 1: ..."). The (track, copy, segment) items are dealt in batches of max_batch in (track, segment,
     * copy) order, so the copies of one stretch of a track are adjacent and a piece of output is finished as soon as every
     * copy's segments covering it are done. Progress is the fraction of all items done (one report per batch, last value 1).
     * Device memory beyond the context's arena is bounded as for dmx_tracks_infer, except the ring of segment outputs:
     *   R segment outputs (S x 2 x segment_samples floats each), R = the longest reach of an overlap-add back from the end
     *   of its batch rounded up to a multiple of max_batch, at least 2 max_batch and at most the total number of items;
     *   about max_batch + n_shifts (ceil((segment_samples + 22050) / stride) + 1) - independent of the number and the
     *   length of the tracks. 2 max_batch at n_shifts = 1 and overlap 0.25, and while n_shifts stays below about
     *   max_batch / 3 at the production segment and overlap 0.25. */
    int dmx_tracks_infer_opts(dmx_ctx *c, int n_tracks, const float *const *audio, const int64_t *n, int n_shifts, float overlap,
                              const int *shift_offsets, float *const *out, int layout, dmx_progress_fn progress, void *user);

    /* ---- stems as WAV-ready PCM (csrc/pcm.hip; no reference counterpart: the reference writes float32 only,
     * cli-apps/demucs.cpp:100-102). demucs's --two-stems, --clip-mode and --int24 / --float32 applied on the GPU to the
     * finished fp32 track, so that what leaves the device is the exact content of a WAV `data` chunk: interleaved stereo
     * L0 R0 L1 R1 ..., little-endian. 24-bit output is PACKED, 3 bytes per sample, not padded to 4: a WAV writer fwrites it
     * as it is. Specification (restated in tests/pcm_spec.py), all fp32, v[s][c][i] = the value
     * dmx_tracks_infer_opts writes for stem s, channel c, frame i:
     *   outputs  stem = -1: the S stems. 0 <= stem < S (two-stems): output 0 = v[stem]; output 1 = the other stems added in
     *            increasing order, starting from the first of them (demucs's `other_stem += source`).
     *   peak     per output, the largest |x| over both channels and all frames, NaN ignored, 0 if there is none.
     *   clip     DMX_CLIP_NONE y = x; DMX_CLIP_CLAMP y = x < -0.99f ? -0.99f : x > 0.99f ? 0.99f : x (a NaN stays one);
     *            DMX_CLIP_RESCALE d = max(1.01f * peak, 1.0f), y = x / d, correctly rounded (demucs's prevent_clip).
     *   encode   DMX_PCM_F32 y; DMX_PCM_S16 rint(y * 32768.0f) saturated to [-32768, 32767]; DMX_PCM_S24
     *            rint(y * 8388608.0f) saturated to [-8388608, 8388607]; ties to even, NaN -> 0, +-inf saturates, no dither. */
#define DMX_PCM_F32 0
#define DMX_PCM_S16 1
#define DMX_PCM_S24 2
#define DMX_CLIP_NONE 0
#define DMX_CLIP_RESCALE 1
#define DMX_CLIP_CLAMP 2
    typedef struct dmx_output_spec
    {
        int encoding, clip, stem; /* DMX_PCM_*, DMX_CLIP_*, -1 (all stems) or the stem of two-stems */
    } dmx_output_spec;
    /* number of outputs of a model under a spec: its number of sources, or 2 in two-stems mode; -1: invalid argument */
    int dmx_output_count(const dmx_model *m, const dmx_output_spec *spec);
    /* bytes of ONE output of n frames: n * 2 * {4, 2, 3}; pure host function; -1: invalid argument */
    int64_t dmx_output_bytes(const dmx_output_spec *spec, int64_t n);
    /* dmx_tracks_infer_opts whose result is WAV data. out[t]: n_out = dmx_output_count() consecutive chunks of
     * dmx_output_bytes(spec, n[t]) bytes. peaks: NULL or the peaks (of the specification above, in every clip mode) of all
     * outputs, n_out floats per track in track order. audio[t] in `layout` as before. The fp32 track is the bits of
     * dmx_tracks_infer_opts with the same arguments, whatever max_batch and the other tracks of the call.
     * With DMX_CLIP_NONE / DMX_CLIP_CLAMP a piece of a track is encoded and copied out as soon as it is final (one contiguous
     * copy per output and piece); with DMX_CLIP_RESCALE the pieces' peaks accumulate and the track is encoded and copied out
     * when its last piece is done. Device memory: as dmx_tracks_infer_opts, plus per track slot the encoded outputs
     * (n_out x dmx_output_bytes(spec, n_max), each rounded up to 16 bytes: never more than the slot's fp32 result) and n_out
     * peaks. Arguments are checked before any GPU work and nothing is written on error; a message about the spec names the
     * field ("output spec: stem 7 of a 4-source model").
     * The engine (several GPUs, the fine-tuned bag) is out of scope: dmx_engine_track_infer returns fp32. */
    int dmx_tracks_infer_pcm(dmx_ctx *c, int n_tracks, const float *const *audio, const int64_t *n, int n_shifts, float overlap,
                             const int *shift_offsets, const dmx_output_spec *spec, void *const *out, float *peaks, int layout,
                             dmx_progress_fn progress, void *user);
    /* ---- bags of models on the track path (restated in tests/bag_spec.py; demucs's BagOfModels:
     * cli-apps/demucs_ft.cpp:136-184 is its one-hot case). Q models of the context's architecture, S stems each, a weight
     * w[q][s] >= 0 per (model, stem): the diagonal is the fine-tuned bag (stem i from model i), equal weights average the
     * models (an ensemble). Per output sample of stem s, all fp32: model q's value e_q is what dmx_tracks_infer_opts forms
     * before de-normalisation (each copy's normalised overlap-add value, summed in increasing copy order and divided by
     * n_shifts; the one copy's value itself at n_shifts = 1), on q's own shifts. Over the models with w[q][s] != 0 in
     * increasing q: a = w e_q for the first, a = fmaf(w, e_q, a) after it; W = the fp32 sum of those weights in the same
     * order; out = (a / W) * std + mean. A model with w[q][s] == 0 is not read for stem s. With one contributing model at
     * weight 1 - and with one model listed twice at equal weights and shifts - the bits are dmx_tracks_infer_opts's. */
#define DMX_MAX_BAG 8 /* and n_models * n_shifts <= 256 */
    /* validates a weight matrix (row-major n_models x n_sources) and gives the effective one: weights NULL needs
     * n_models == n_sources and means the diagonal. Pure host function. weights_out (n_models x n_sources) and sums_out
     * (n_sources: the fp32 column sums W above) may be NULL. Rejected: n_models outside [1, DMX_MAX_BAG], a negative or
     * non-finite weight, a stem without a model, a model without a non-zero weight. */
    int dmx_bag_weights(int n_models, int n_sources, const float *weights, float *weights_out, float *sums_out);
    /* dmx_tracks_infer_opts (spec NULL: out[t] is S x 2 x n[t] floats in `layout`, peaks unused) or dmx_tracks_infer_pcm
     * (spec given) through a bag. shift_offsets: n_tracks x n_models x n_shifts, the shift of track t, model q, copy k at
     * [(t * n_models + q) * n_shifts + k]; NULL or -1 entries are rand() % 22050 drawn in that row-major order, so one
     * track at one shift draws like dmx_engine_track_infer. The context may be bound to any model of the bag's
     * architecture; it is bound to that model again on return, on success and on error.
     * A track is uploaded once and its statistics are computed once. Model q's items are dmx_tracks_infer_opts's (track,
     * row, copy) sequence for its own shifts; a batch holds items of one model and the context is rebound between batches
     * (free when the models take the same exact-split decisions, as fine-tuned models do; otherwise the plans are rebuilt
     * at every rebind). The next batch always comes from the model that lags furthest behind in (track, row), so that a
     * piece of a track is final - overlap-added, encoded and copied out as for one model - as soon as every model's copies
     * have covered it; no host wait between batches. Device memory beyond the arena: the track slots of
     * dmx_tracks_infer (_pcm), and one ring of segment outputs PER MODEL, each sized by dmx_tracks_infer_opts's rule from the
     * reach of the overlap-adds into that model's items: at most about 2 max_batch + n_shifts (ceil((segment_samples +
     * 22050) / stride) + 1) blocks rounded up to a multiple of max_batch - independent of the number and the length of
     * the tracks.
     * Arguments are checked before any GPU work and nothing is written on error: "model 2: differs in architecture or
     * device from the context's", "weights: stem 1 has no model", "weights: model 3 has no non-zero weight", "track 2,
     * model 1, shift 0: ...". Progress is the fraction of all models' items done (one report per batch, last value 1). */
    int dmx_tracks_infer_bag(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                             const float *const *audio, const int64_t *n, int n_shifts, float overlap, const int *shift_offsets,
                             const dmx_output_spec *spec /* NULL: fp32 in `layout` */, void *const *out, float *peaks, int layout,
                             dmx_progress_fn progress, void *user);
    /* the stage alone on device memory (a building block, as dmx_resample_device): n_sources x 2 planes of n >= 1 floats,
     * plane p = stem * 2 + channel at d_planes + p * plane_stride (plane_stride >= n; any alignment of the planes is handled).
     * d_out: 16-byte aligned; output o starts at d_out + o * DMX_OUTPUT_STRIDE(dmx_output_bytes(spec, n)) - the kernels store
     * whole dwords, and up to 15 bytes behind an output are padding (written or not). d_peaks: n_out floats (required: the
     * rescale mode reads them back on the device). Enqueued on `stream` (hipStream_t, may be NULL). */
#define DMX_OUTPUT_STRIDE(bytes) (((bytes) + 15) / 16 * 16)
    int dmx_pcm_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                              const dmx_output_spec *spec, void *d_out, float *d_peaks, void *stream);
    /* host buffers: planes [n_sources][2][n]; out: n_out consecutive chunks of dmx_output_bytes(spec, n); peaks NULL or n_out */
    int dmx_pcm_encode(int device, const float *planes, int n_sources, int64_t n, const dmx_output_spec *spec, void *out,
                       float *peaks);

    /* ---- remixed outputs (csrc/pcm.hip; DESIGN.md section 2.10, restated in tests/remix_spec.py; no reference counterpart).
     * The output stage generalised from "a stem, or the sum of the others" to a gain matrix over the stems and the original
     * mixture: demucs's --other-method add | minus | none, and what a user mixes from the stems afterwards ("everything with
     * the vocals 12 dB down", "the residual the model left over"), formed on the GPU so that only the wanted bytes leave it.
     * Sources: src[0..S) the S stems exactly as dmx_tracks_infer_opts (dmx_tracks_infer_bag on the bag path) writes them;
     * src[S] the MIXTURE: the caller's track as passed in, frames [0, n), not normalised and not shifted. A spec has n_out
     * outputs and a row-major gain matrix g[n_out][S + 1] (last column: the mixture). Output o, channel c, frame i, all fp32:
     * the sources are visited in increasing index; a source with g[o][s] == 0 is skipped and NOT READ (a NaN in a stem nobody
     * asked for does not spread); the first visited source gives a = g * x, each later one p = g * x, a = a + p. Every product
     * and every sum is its own correctly rounded fp32 operation: there is NO fused multiply-add, so plain float32 arithmetic
     * restates it exactly. Peak, clip and encode of each output are then those of the specification above (peak over both
     * channels and all frames with NaN ignored, the rescale divisor from that output's own peak, ties to even).
     * Consequences: 0/1 gains give dmx_output_spec's outputs bit for bit (1 * x is exact); the row -1 on a stem, +1 on the
     * mixture gives exactly the fp32 mixture - stem. */
#define DMX_MAX_OUTPUTS 8
#define DMX_OTHER_ADD 0   /* two outputs: the stem, the other stems added (dmx_output_spec's two-stems) */
#define DMX_OTHER_MINUS 1 /* two outputs: the stem, mixture - stem                                    */
#define DMX_OTHER_NONE 2  /* one output: the stem                                                     */
    typedef struct dmx_remix_spec
    {
        int encoding, clip, n_out; /* DMX_PCM_*, DMX_CLIP_*, 1 .. DMX_MAX_OUTPUTS */
        const float *gains;        /* n_out x (n_sources + 1), row-major, last column = the mixture */
    } dmx_remix_spec;
    /* the matrices of demucs's three --other-method's for `stem` of an n_sources-source model (n_sources <= 6): gains_out
     * holds 2 x (n_sources + 1) floats, *n_out becomes 2 (add, minus) or 1 (none). Pure host function. */
    int dmx_remix_two_stems(int n_sources, int stem, int method, float *gains_out, int *n_out);
    /* validates a spec for a model of n_sources (1 .. 6) sources. Pure host function. Rejected, each with a message of its own
     * ("remix spec: output 2 has no non-zero gain"): n_out outside [1, DMX_MAX_OUTPUTS], a NULL gain matrix, a non-finite gain
     * (named by output and source), a row with no non-zero gain, a bad encoding, a bad clip mode. */
    int dmx_remix_check(int n_sources, const dmx_remix_spec *spec);
    /* dmx_tracks_infer_pcm under a remix spec. models == NULL and n_models == 0: the context's own model; the fp32 track
     * behind the gains is the bits of dmx_tracks_infer_opts. Otherwise a bag exactly as dmx_tracks_infer_bag (models, weights,
     * shift_offsets n_tracks x n_models x n_shifts, the context bound to its model again on return). out[t]: n_out consecutive
     * chunks of dmx_output_bytes() for the spec's encoding; peaks: NULL or n_out floats per track. Pieces are encoded and
     * copied out as soon as they are final under DMX_CLIP_NONE / DMX_CLIP_CLAMP and at the track's end under
     * DMX_CLIP_RESCALE, as dmx_tracks_infer_pcm does. The mixture column reads the track's one upload (interleaved on the
     * device for either `layout`): there is no second upload. The spec is checked before any GPU work and nothing is written
     * on error. Device memory: as dmx_tracks_infer_pcm with n_out from the spec - per track slot n_out x dmx_output_bytes(spec,
     * n_max), each rounded up to 16 bytes, and n_out peaks; with n_out > S at DMX_PCM_F32 the encoded outputs may exceed the
     * slot's fp32 result (8 float32 outputs of a 4-source model: twice it). The engine stays out of scope. */
    int dmx_tracks_infer_remix(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                               const float *const *audio, const int64_t *n, int n_shifts, float overlap, const int *shift_offsets,
                               const dmx_remix_spec *spec, void *const *out, float *peaks, int layout, dmx_progress_fn progress,
                               void *user);
    /* the stage alone on device memory, as dmx_pcm_encode_device: d_mix is the mixture interleaved [n][2] at any 4-byte
     * alignment; it may be NULL when the mixture column of the gains is all zero (an error, with a message, when it is NULL
     * and the column is not). d_out, the outputs' stride and d_peaks (n_out floats) as there. */
    int dmx_remix_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride, const float *d_mix,
                                const dmx_remix_spec *spec, void *d_out, float *d_peaks, void *stream);
    /* host buffers: planes [n_sources][2][n], mix [n][2] or NULL; out: n_out consecutive chunks; peaks NULL or n_out */
    int dmx_remix_encode(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                         void *out, float *peaks);

    /* ---- loudness (csrc/loudness.hip; DESIGN.md section 2.14, restated in tests/loudness_spec.py; no reference counterpart).
     * Integrated loudness after ITU-R BS.1770-4 / EBU R 128 of a stereo signal x[2][n] of fp32 samples at `rate` Hz, measured
     * on the GPU in binary64, and the gain that brings a track's outputs to a target.
     * Coefficients (host, libm, binary64): shelf f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196,
     * K = tan(pi f0 / rate), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2, b = [(Vh + Vb K/Q + K^2)/a0,
     * 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0], a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0]; high-pass f0 = 38.13547087602444,
     * Q = 0.5003270373238773, b = [1, -2, 1] (not normalised), a as above. At 48 kHz these are the BS.1770 table values.
     * Measurement: y = highpass(shelf(x)) per channel from zero state; hop h = (rate + 5) / 10 frames, H = n / h whole hops
     * (the tail is ignored); e[c][j] the sum of y^2 over hop j; block b in [0, H - 3): z[b] = (sum over both channels and hops
     * b .. b + 3 of e) / (4 h); l[b] = -0.691 + 10 log10 z[b]; a block with l[b] <= -70 is dropped (absolute gate), then one
     * with l[b] <= -0.691 + 10 log10(mean z of the remaining blocks) - 10 (relative gate); L = -0.691 + 10 log10(mean z of the
     * blocks past both gates). A NaN block passes the gates, so one NaN in the signal makes L NaN. UNMEASURABLE: H < 4, no
     * block left, or L not finite. The quantum lufs_c = rint(100 L), ties to even, an int32 in hundredths of a LU
     * (DMX_LUFS_UNMEASURABLE = INT32_MIN); everything downstream uses lufs_c, never L, so the gain and every output byte are
     * reproducible although the device sums in another order than a host would. The device's sums have a fixed order and
     * use no atomics: L is the same bits from run to run, whatever else a call holds.
     * Gain (fp32): target_c = rint(100 target_lufs); k = clamp(target_c - lufs_c, -6000, 6000); g = T[k + 6000] with the
     * host-made table T[i] = (float)pow(10.0, (i - 6000) / 2000.0); ceiling: with P the sample peak of the specification
     * above, if P > 0 and the fp32 product g * P exceeds max_peak then g = max_peak / P, correctly rounded (+inf: no
     * ceiling); unmeasurable: g = 1, no ceiling. Apply: y = g * x, one fp32 product per sample on the gathered output value
     * (behind the remix sum, in front of clip); clip and encode follow with the peak g * P, which is exactly the peak of
     * the gained samples (a positive factor and its rounding are monotone) and is the peak reported. g == 1 gives the bytes
     * of the entry point without loudness.
     * Modes: DMX_LOUD_MEASURE no gain, only the report; DMX_LOUD_MIXTURE one g for all outputs of a track, from the lufs_c
     * of the MIXTURE (the caller's track at its own rate) and the largest of the outputs' peaks - the outputs keep their
     * balance and none exceeds the ceiling; DMX_LOUD_EACH every output its own lufs_c, P and g.
     * The report of a track holds n_out + 1 entries, the outputs and then the mixture (whose gain is 0); lufs is the
     * unquantised L, NaN when unmeasurable. A mono file is measured as the dual-mono stereo it becomes.
     * True peak (4x oversampled), loudness range and the momentary and short-term maxima are the meters below, and
     * DMX_LOUD_TRUE_PEAK turns the ceiling into a true-peak one. Out of scope: ReplayGain tags (FLAC tags stay out of
     * scope), the engine. */
#define DMX_LOUD_MEASURE 0
#define DMX_LOUD_MIXTURE 1
#define DMX_LOUD_EACH 2
#define DMX_LUFS_UNMEASURABLE (-2147483647 - 1)
#define DMX_LOUD_MIN_RATE 4000 /* tan(pi f0 / rate) of the shelf needs rate > 2 * 1682 */
    typedef struct dmx_loudness_spec
    {
        int mode;          /* DMX_LOUD_* */
        float target_lufs; /* finite, in [-70, 0] */
        float max_peak;    /* > 0; +inf: no ceiling */
    } dmx_loudness_spec;
    typedef struct dmx_loudness_result
    {
        int32_t lufs_c; /* rint(100 L), or DMX_LUFS_UNMEASURABLE */
        float gain;     /* the gain applied (1 under DMX_LOUD_MEASURE; 0 in the mixture's entry and from the measuring calls) */
        double lufs;    /* L, NaN when unmeasurable */
    } dmx_loudness_result;
    /* the two stages' b0 b1 b2 a1 a2, ten doubles. Pure host function; DMX_ERR_ARG for rate < DMX_LOUD_MIN_RATE. */
    int dmx_loudness_coefficients(int rate, double *coef);
    /* the table T above, 12001 floats. Pure host function. */
    int dmx_loudness_gain_table(float *table);
    /* validates a spec for a signal at `rate`. Pure host function. Rejected, each with a message that names the field
     * ("loudness spec: target_lufs 3 is not in [-70, 0]"): a bad mode, a target_lufs that is not finite or outside [-70, 0],
     * a max_peak that is not above 0, a rate below DMX_LOUD_MIN_RATE. */
    int dmx_loudness_check(const dmx_loudness_spec *spec, int rate);
    /* bytes of device workspace for ONE measured signal of n frames, whatever the rate: 64 + 256 per tile of 4096 frames (64
     * bytes of states, 192 of hop partials sized for the smallest hop) + 16 per 400 frames (the hop energies, sized likewise) -
     * about n / 10. The design condition of at most one byte per frame holds from 320 frames on; below that the first tile's
     * 320 bytes are a constant that a shorter signal cannot be spared. Pure host function; -1 for n < 1. */
    int64_t dmx_loudness_workspace_bytes(int64_t n);
    /* measures one signal on device memory, asynchronous on `stream`, four launches: d_x is planar (channel c at d_x + c *
     * plane_stride, plane_stride >= n) or, with plane_stride == 0, interleaved [n][2]; any 4-byte alignment. d_result: one
     * entry ON THE DEVICE (gain 0); d_e: NULL or 2 x (n / h) doubles on the device, e[c][j]; d_work: 16-byte aligned,
     * the bytes above. 1 <= n < 2^36. */
    int dmx_loudness_device(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, dmx_loudness_result *d_result,
                            double *d_e, void *d_work, void *stream);
    /* measurement (tools/loudness_bench.py): the call above, synchronised, with the times of its four launches (states, scan,
     * energies, final) between HIP events in ms[0..4) and, in ms[4], the peak kernel's time on the same signal */
    int dmx_loudness_device_timed(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate,
                                  dmx_loudness_result *d_result, double *d_e, void *d_work, void *stream, float *ms);
    /* the same on host buffers: x planar [2][n] or (interleaved != 0) [n][2]; e NULL or 2 x (n / h) doubles */
    int dmx_loudness(int device, const float *x, int64_t n, int interleaved, int rate, dmx_loudness_result *result, double *e);
    /* dmx_remix_encode_device behind the loudness stage: measure the n_out outputs and the mixture, form the peaks and the
     * gains, encode - all enqueued on `stream`, no host round trip. d_mix is required (it is the signal DMX_LOUD_MIXTURE
     * measures, and the report's last entry). d_report: n_out + 1 entries on the device. d_work: 16-byte aligned,
     * (n_out + 1) x dmx_loudness_workspace_bytes(n) + 64 bytes. Under DMX_LOUD_MEASURE the bytes and peaks are
     * dmx_remix_encode_device's, from the kernels it launches. This call has no context to own the gain table: the first
     * call on a device uploads one copy (48 KB, a blocking copy) that stays for the life of the process.
     * An output spec (a stem, or the sum of the others) reaches the stage as its 0/1 gain matrix (dmx_remix_two_stems or
     * unit rows), whose bytes are the output spec's: the measuring kernels are instantiated for gain tables only. */
    int dmx_loud_encode_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride, const float *d_mix,
                               const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out, float *d_peaks,
                               dmx_loudness_result *d_report, void *d_work, void *stream);
    /* host buffers: planes [n_sources][2][n], mix [n][2]; out: n_out consecutive chunks; peaks NULL or n_out; report NULL or
     * n_out + 1 entries */
    int dmx_loud_encode(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                        const dmx_loudness_spec *loud, int rate, void *out, float *peaks, dmx_loudness_result *report);

    /* ---- meters (csrc/meters.hip; DESIGN.md section 2.15, restated in tests/meters_spec.py; no reference counterpart): what
     * EBU R 128 asks for beside integrated loudness, of the same signals, on the GPU.
     * True peak TP: the oversampling factor F is 4 for rate < 96000, 2 for rate < 192000, else 1 (TP is then the sample
     * peak). Taps h[k] = (float)(sinc((k - 6 F) / F) * 0.5 * (1 - cos(2 pi k / (12 F)))), k = 0 .. 12 F, sinc(t) =
     * sin(pi t) / (pi t), sinc(0) = 1, made on the host in binary64 and rounded once. Phase 0 is the sample itself; phase p
     * (0 < p < F) at frame i is y_p[i] = sum over j = 0 .. 11 of h[p + F j] * x[i + 6 - j], x = 0 outside [0, n), in fp32,
     * every product rounded and then added with a rounding of its own, j ascending. TP is the largest |y_p[i]| over the
     * channels, 0 <= i < n and the phases; NaN is ignored, nothing left gives 0. TP >= the sample peak, and TP is exact:
     * the same bits as the specification, whatever the cut into tiles and pieces.
     * Hop meters, from the hop energies e[c][j] and the hop h of the section on loudness, H = n / h: momentary blocks are
     * that section's l[b]; short-term blocks S[b] = -0.691 + 10 log10((sum over hops b .. b + 29, channel 0 then channel 1
     * of a hop, of e) / (30 h)), b in [0, H - 29). max_momentary_c = max rint(100 l[b]), max_short_c = max rint(100 S[b]),
     * int32 in hundredths of a LU; DMX_LUFS_UNMEASURABLE without a block or with a block that is not finite; a block of
     * zero energy is -inf and never wins (all zero: unmeasurable).
     * Loudness range after EBU Tech 3342 over an integer histogram: s_c[b] = min(rint(100 S[b]), 2000); the values above
     * -7000 are counted in bins k = s_c + 7000; mean = sum cnt[k] 10^((k - 7000) / 1000) / sum cnt[k] in binary64, k
     * ascending; r_c = floor(100 * 10 log10(mean)) - 2000; the bins with k - 7000 > r_c remain, m values; lra_c =
     * v[((m - 1) 95 + 50) / 100] - v[((m - 1) 10 + 50) / 100] in their ascending order. Unmeasurable: H < 30, a block that
     * is not finite, no bin past a gate.
     * DMX_LOUD_TRUE_PEAK, OR-ed into dmx_loudness_spec.mode, makes max_peak a true-peak ceiling: the gain rule above reads
     * TP where it reads P (under DMX_LOUD_MIXTURE the largest TP of the outputs). The peaks a call returns stay the gained
     * SAMPLE peaks g * P (what DMX_CLIP_RESCALE divides by). Without the flag every byte and every launch is unchanged. */
#define DMX_LOUD_TRUE_PEAK 0x100
    typedef struct dmx_meters_result
    {
        float true_peak;         /* TP of the signal as measured, linear; the TP that leaves is the fp32 product gain * true_peak */
        int32_t lra_c;           /* hundredths of a LU, or DMX_LUFS_UNMEASURABLE */
        int32_t max_momentary_c; /* idem */
        int32_t max_short_c;     /* idem */
    } dmx_meters_result;
    /* the factor F for `rate` and the 12 F + 1 taps (taps may be NULL). Pure host function; DMX_ERR_ARG for rate < 1. */
    int dmx_true_peak_filter(int rate, int *factor, float *taps);
    /* bytes of device workspace for ONE metered signal on top of dmx_loudness_workspace_bytes(n): 64 (the histogram lives in
     * LDS). Pure host function; -1 for n < 1. */
    int64_t dmx_meters_workspace_bytes(int64_t n);
    /* dmx_loudness_device plus the two new stages, asynchronous on `stream`: d_meters is one entry ON THE DEVICE; d_work:
     * 16-byte aligned, dmx_loudness_workspace_bytes(n) + dmx_meters_workspace_bytes(n) bytes. d_result receives what
     * dmx_loudness_device writes, from the same launches. */
    int dmx_meters_device(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, dmx_loudness_result *d_result,
                          double *d_e, void *d_work, void *stream, dmx_meters_result *d_meters);
    /* measurement (tools/meters_bench.py): the true-peak launch and the peak kernel on the same signal, synchronised, their
     * times between HIP events in ms[0] and ms[1], and the meters launch behind a measurement in ms[2]; d_work as above */
    int dmx_meters_device_timed(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, void *d_work, void *stream,
                                float *ms);
    /* the same on host buffers */
    int dmx_meters(int device, const float *x, int64_t n, int interleaved, int rate, dmx_loudness_result *result, double *e,
                   dmx_meters_result *meters);
    /* dmx_loud_encode_device plus a meters report of n_out + 1 entries on the device, the outputs and then the mixture, each
     * signal as measured (in front of the gain). Honours DMX_LOUD_TRUE_PEAK, as dmx_loud_encode_device does (which then
     * enqueues the true-peak launch over the outputs and the gain launch's true-peak form, and nothing else new). d_work:
     * (n_out + 1) x (dmx_loudness_workspace_bytes(n) + dmx_meters_workspace_bytes(n)) + 64 bytes. */
    int dmx_loud_encode_meters_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                      const float *d_mix, const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out,
                                      float *d_peaks, dmx_loudness_result *d_report, void *d_work, void *stream,
                                      dmx_meters_result *d_meters);
    /* host buffers, as dmx_loud_encode; meters NULL or n_out + 1 entries */
    int dmx_loud_encode_meters(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                               const dmx_loudness_spec *loud, int rate, void *out, float *peaks, dmx_loudness_result *report,
                               dmx_meters_result *meters);

    /* ---- look-ahead peak limiter (csrc/limiter.hip; DESIGN.md section 2.16, restated in tests/limiter_spec.py; no reference
     * counterpart): holds a stereo signal under a ceiling c by shaping its peaks, where the ceiling rule of the section on
     * loudness lowers the whole signal's gain. The stage is exact: the same bits as the specification, whatever the cut into
     * tiles. All that depends on time runs in integers in the log domain, one octave being U = 65536 units; only maxima
     * carry state, and a maximum has no order.
     * Tables, made on the host in binary64 with libm: LUT[k] = ceil(U log2(1 + (k + 1) / 4096)) + 2, k = 0 .. 4095 (int32: the
     * logarithm rounded up, with two units of slack for the fp32 roundings below); THI[a] = 2^(-a / 16), a = 0 .. 384, and
     * TLO[b] = 2^(-b / 65536), b = 0 .. 4095 (float), both rounded TOWARDS ZERO.
     * Gain of a reduction D (units, 0 <= D <= 24 U): G(D) = THI[D >> 12] * TLO[D & 4095], one fp32 product. G(0) == 1
     * exactly, and G is non-increasing (checked by exhaustion, tests/test_limiter_cpu.py).
     * Level: p[j] = max over the two channels of |g x[c][j]|, g x the fp32 product; a NaN sample is ignored by the detector
     * and stays NaN in the output. With true_peak, p[j] also takes |g y_p[j]| for the F - 1 interpolated phases y_p of the
     * section on meters at frame j: the same taps, the same order of operations, zeros outside [0, n).
     * Required reduction: where p[j] > c, M[j] = min(U e + LUT[m >> 11], 24 U), with e the unbiased exponent and m the 23
     * mantissa bits of the correctly rounded fp32 quotient p[j] / c; else M[j] = 0. p G(M) <= c for p / c < 2^24.
     * Envelope: D[i] = max(0, max over j <= i of M[j] - qr (i - j), max over j >= i of M[j] - qa (j - i)): a linear-in-dB
     * attack with unlimited look-ahead and a linear-in-dB release. Slopes: attack_ms and release_ms are the times in which
     * the reduction moves by 10 dB, q = clamp(rint(U log2(10^0.5) 1000 / (ms rate)), 1, 2^20) in binary64; both times finite
     * and in [0.1, 10000]; defaults 5 and 100.
     * Apply: y = (g x[c][j]) G(D[j]), two fp32 products in that order. Where D[j] == 0 the second factor is exactly 1: a
     * signal that never exceeds c leaves unchanged. For finite samples with p / c < 2^24, peak_out <= c holds exactly.
     * true_peak_out is the true peak of the limited signal; the gain moves from sample to sample and changes the inter-sample
     * crests, so true_peak_out is NOT guaranteed to stay under c (DESIGN.md section 2.16 gives the figures on the fixtures).
     * Behind the loudness stage: DMX_LOUD_LIMIT, OR-ed into dmx_loudness_spec.mode (the struct stays as it is), and the mode
     * DMX_LOUD_UNITY. With the flag the ceiling rule of the section on loudness no longer lowers g: g = T[k + 6000] always, and
     * g = 1 when unmeasurable; the limiter holds max_peak instead. DMX_LOUD_UNITY is the limiter without loudnorm: the outputs are
     * measured and reported as under DMX_LOUD_MEASURE, g = 1. Linking: stereo is always linked (the max over the channels);
     * DMX_LOUD_MIXTURE has one envelope for the call, from the largest p[j] over its outputs, so that the outputs keep their
     * balance at every instant; DMX_LOUD_EACH and DMX_LOUD_UNITY have one envelope per output. DMX_LOUD_TRUE_PEAK makes the
     * level the true-peak one. The peaks a call returns are then peak_out, the exact maximum over the limited samples, which
     * is what DMX_CLIP_RESCALE divides by. Every entry point that takes a loudness spec accepts the flag and the mode; those
     * of the sections above (`_loud`, `_meters`) are the `_limit` ones of this section with both new arguments NULL (the default
     * times, no limiter report), and without the flag they enqueue exactly what they enqueued. dmx_loudness_check alone keeps
     * the contract of the section on meters - it answers for the modes of that section and refuses 0x200 and 3 - and
     * dmx_limiter_check is the validator that knows the limiter; both run the same checks. Out of scope: the engine. */
#define DMX_LOUD_UNITY 3
#define DMX_LOUD_LIMIT 0x200
#define DMX_LIMIT_ATTACK_MS 5.0f
#define DMX_LIMIT_RELEASE_MS 100.0f
    typedef struct dmx_limiter_spec
    {
        float attack_ms;  /* finite, in [0.1, 10000] */
        float release_ms; /* idem */
    } dmx_limiter_spec;
    typedef struct dmx_limit_result
    {
        float peak_out;         /* the largest |y| of the limited samples, NaN ignored */
        float true_peak_out;    /* the true peak of the limited signal; 0 unless true_peak */
        int32_t max_reduction;  /* the largest D, in units */
        int64_t limited_frames; /* frames with D > 0 */
    } dmx_limit_result;
    /* LUT (4096 int32), THI (385 floats), TLO (4096 floats). Pure host function. */
    int dmx_limiter_tables(int32_t *lut, float *thi, float *tlo);
    /* the slopes qa and qr in units per frame. Pure host function; DMX_ERR_ARG, with a message that names the field, for
     * rate < 1 and for a time that is not finite or outside [0.1, 10000]. */
    int dmx_limiter_slopes(int rate, double attack_ms, double release_ms, int32_t *qa, int32_t *qr);
    /* bytes of device workspace for ONE envelope over n frames: 8 n4 + 64 per tile of 2048 frames, n4 = n rounded up to a
     * multiple of 4. M lies at byte 0 as int32 [n], the gain plane G(D) at byte 4 n4 as float [n], the tiles' aggregates
     * behind them. A multiple of 16. Pure host function; -1 for n < 1. */
    int64_t dmx_limiter_workspace_bytes(int64_t n);
    /* limits one signal on device memory under the gain `gain` and the ceiling max_peak (> 0, finite), asynchronous on
     * `stream`: three launches (detect, carry, envelope), and a fourth with true_peak != 0 (the limited signal's true peak). d_x
     * as dmx_loudness_device takes it; lim NULL: the default times. d_result: one entry ON THE DEVICE; d_work: 16-byte aligned,
     * the bytes above, and holds M and the gain plane afterwards. 1 <= n < 2^36. The first call on a device uploads one copy
     * of the tables (34 KB, a blocking copy) that stays for the life of the process. */
    int dmx_limit_device(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, float gain, float max_peak,
                         int true_peak, const dmx_limiter_spec *lim, dmx_limit_result *d_result, void *d_work, void *stream);
    /* measurement (tools/limiter_bench.py): the call above, synchronised, with the times of its launches between HIP events in
     * ms[0..4) (detect, carry, envelope, the true peak of the limited signal: 0 without true_peak) and, in ms[4], the peak
     * kernel's time on the same signal */
    int dmx_limit_device_timed(int device, const float *d_x, int64_t n, int64_t plane_stride, int rate, float gain, float max_peak,
                               int true_peak, const dmx_limiter_spec *lim, dmx_limit_result *d_result, void *d_work, void *stream,
                               float *ms);
    /* the same on host buffers: x planar [2][n] or (interleaved != 0) [n][2]; m NULL or n int32 (M); gain_plane NULL or n
     * floats (G(D)) */
    int dmx_limit(int device, const float *x, int64_t n, int interleaved, int rate, float gain, float max_peak, int true_peak,
                  const dmx_limiter_spec *lim, int32_t *m, float *gain_plane, dmx_limit_result *result);

    /* validates a loudness spec that may carry DMX_LOUD_LIMIT or be DMX_LOUD_UNITY, and the limiter's times (lim NULL: the
     * defaults), for a signal at `rate`. Pure host function. Rejected, each with a message that names the field: what
     * dmx_loudness_check rejects (the mode message lists the new values); DMX_LOUD_LIMIT with DMX_LOUD_MEASURE and
     * DMX_LOUD_UNITY without DMX_LOUD_LIMIT ("mode"); DMX_LOUD_LIMIT with max_peak = +inf ("max_peak"); a bad time
     * ("attack_ms", "release_ms"). */
    int dmx_limiter_check(const dmx_loudness_spec *spec, const dmx_limiter_spec *lim, int rate);
    /* dmx_loud_encode_meters_device plus the limiter: d_meters may be NULL here; lim NULL: the default times; d_limit NULL or
     * n_out entries on the device. Without DMX_LOUD_LIMIT in the mode the call enqueues exactly what
     * dmx_loud_encode_device resp. dmx_loud_encode_meters_device enqueues and d_limit is zeroed. With it: the measurements
     * (and meters) as before, the gain launch without a ceiling, the limiter's three or four launches over one envelope
     * (DMX_LOUD_MIXTURE) or n_out, and the encode launch that reads the gain plane; the peak kernel is not needed and not
     * launched. d_work: the bytes of the call without the limiter, rounded up to 64, plus n_out x
     * dmx_limiter_workspace_bytes(n) + 64 x n_out bytes. The first call on a device uploads the limiter's tables (34 KB). */
    int dmx_loud_encode_limit_device(int device, const float *d_planes, int n_sources, int64_t n, int64_t plane_stride,
                                     const float *d_mix, const dmx_remix_spec *spec, const dmx_loudness_spec *loud, int rate, void *d_out,
                                     float *d_peaks, dmx_loudness_result *d_report, void *d_work, void *stream,
                                     dmx_meters_result *d_meters, const dmx_limiter_spec *lim, dmx_limit_result *d_limit);
    /* host buffers, as dmx_loud_encode_meters; limit NULL or n_out entries */
    int dmx_loud_encode_limit(int device, const float *planes, int n_sources, int64_t n, const float *mix, const dmx_remix_spec *spec,
                              const dmx_loudness_spec *loud, int rate, void *out, float *peaks, dmx_loudness_result *report,
                              dmx_meters_result *meters, const dmx_limiter_spec *lim, dmx_limit_result *limit);

    /* dmx_tracks_infer_meters and dmx_tracks_infer_from_flac_meters (below) with the limiter: the `_meters` forms plus the
     * limiter's times (lim NULL: the defaults) and a report of n_tracks x n_out entries (limit NULL: none; zeroed without
     * DMX_LOUD_LIMIT). With the flag a track is a whole-track one (DMX_LOUD_UNITY too): behind its last piece its outputs are
     * measured, gained without a ceiling, limited at the track's own rate, encoded through the gain plane and copied out; the
     * peaks are peak_out, and the peak kernel is not launched. Device memory per track slot, on top of the call without the
     * limiter: dmx_limiter_workspace_bytes(n_max) per envelope - one under DMX_LOUD_MIXTURE, n_out under DMX_LOUD_EACH and
     * DMX_LOUD_UNITY - plus 64 x n_out bytes of results. */
    int dmx_tracks_infer_limit(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                               const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                               const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                               float *peaks, int layout, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud,
                               dmx_loudness_result *report, dmx_meters_result *meters, const dmx_limiter_spec *lim, dmx_limit_result *limit);
    int dmx_tracks_infer_from_flac_limit(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                         const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                         const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out,
                                         int64_t *sizes, float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user,
                                         const dmx_loudness_spec *loud, dmx_loudness_result *report, dmx_meters_result *meters,
                                         const dmx_limiter_spec *lim, dmx_limit_result *limit);

    /* ---- stems as FLAC (csrc/flac.hip; demucs's --flac; no reference counterpart: the reference holds no encoder).
     * Specification (restated in tests/flac_spec.py with an independent decoder): interleaved stereo
     * PCM as the stages above write it (16-bit pairs or packed 24 bit) -> a complete .flac file: "fLaC", one STREAMINFO block
     * (block size 4096, the stream's smallest / largest frame, 36-bit total samples, MD5 all zero = not computed), frames
     * of 4096 samples (the last: n mod 4096) with FIXED predictors of order 0..4, CONSTANT and VERBATIM subframes, partitioned
     * Rice coding (partition order <= 4, no escape code) and the four stereo decorrelations - every choice by exact bit
     * counts with stated tie-breaks, so the bytes are reproducible anywhere. sample_rate (1 .. 655350) is carried in the
     * headers only; rates other than 44100 / 48000 are written as "from STREAMINFO", which is legal but outside the
     * streamable subset. A compression LEVEL (tests/flac_lpc_spec.py) adds LPC candidates behind the FIXED orders: level 0
     * (the default everywhere) none, level 1 order 8, level 2 orders 8 and 12 - an integer Welch window, exact int64
     * autocorrelation, Levinson-Durbin in binary64 with a fixed operation order and no contraction, 12 / 15 bit coefficients
     * with error feedback, chosen by the same exact bit counts, so a frame never grows with the level and the bound and the
     * workspace stand unchanged. Out of scope: wasted-bits detection, MD5, orders above 12, escape-coded partitions, variable
     * block sizes, seek tables, tags, mono / multichannel. */
    /* an upper bound of the file for n frames of `bits` (16 | 24): 42 + 18 * ceil(n / 4096) + n * 2 * bits / 8, rounded up to
     * 16. Pure host function; -1 on a bad argument (bits, n < 1, n >= 2^36). */
    int64_t dmx_flac_bound(int bits, int64_t n);
    /* bytes of device workspace dmx_flac_encode_device needs for ONE stream (a table of frame lengths and offsets and one
     * bound-sized slot per frame: a little more than dmx_flac_bound). Pure host function; -1 on a bad argument. */
    int64_t dmx_flac_workspace_bytes(int bits, int64_t n);
    /* the stage alone on device memory, asynchronous on `stream`, three launches: d_pcm (16-byte aligned; n frames) ->
     * d_out (dmx_flac_bound bytes, any alignment), *d_size (an int64 ON THE DEVICE: the file's byte count), d_work
     * (dmx_flac_workspace_bytes, 16-byte aligned). */
    int dmx_flac_encode_device(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, void *d_out, int64_t *d_size,
                               void *d_work, void *stream);
    /* the same on host buffers: out holds dmx_flac_bound(bits, n) bytes, *size receives the file's byte count */
    int dmx_flac_encode(int device, const void *pcm, int bits, int64_t n, int sample_rate, void *out, int64_t *size);
    /* the two calls above at a compression level (0: their bytes; 1: + LPC order 8; 2: + LPC orders 8 and 12). A level
     * outside [0, 2] is DMX_ERR_ARG before any GPU work. */
    int dmx_flac_encode_device_level(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                                     int64_t *d_size, void *d_work, void *stream);
    int dmx_flac_encode_level(int device, const void *pcm, int bits, int64_t n, int sample_rate, int level, void *out, int64_t *size);
    /* measurement: dmx_flac_encode_device_level, synchronised, with the times of its three kernels (frames, scan, compact)
     * between HIP events in ms[0..3) */
    int dmx_flac_encode_device_timed(int device, const void *d_pcm, int bits, int64_t n, int sample_rate, int level, void *d_out,
                                     int64_t *d_size, void *d_work, void *stream, float *ms);
    /* the level that dmx_tracks_infer_flac and dmx_tracks_infer_from_flac with flac_out use on this context (default 0);
     * the getter returns -1 for a NULL context */
    int dmx_ctx_set_flac_level(dmx_ctx *c, int level);
    int dmx_ctx_flac_level(const dmx_ctx *c);
    /* dmx_tracks_infer_remix whose outputs leave as .flac files: the same arguments plus sample_rate and sizes. out[t]: n_out
     * chunks at a stride of dmx_flac_bound(bits, n[t]); sizes[t * n_out + o]: the byte count of track t's output o; the PCM
     * behind a file is the bytes dmx_tracks_infer_remix returns for the same arguments (bits 16 for DMX_PCM_S16, 24 for
     * DMX_PCM_S24; DMX_PCM_F32 is rejected before any GPU work, as is a NULL sizes or a sample_rate outside [1, 655350];
     * nothing is written on error). The PCM stage runs as there into the slot's buffer (piecewise under DMX_CLIP_NONE /
     * DMX_CLIP_CLAMP, whole-track under DMX_CLIP_RESCALE); the FLAC stage runs once per track behind its last piece, and only
     * FLAC bytes are copied out: one device-to-host copy per output of exactly its length, after the byte counts have reached
     * the host (a wait on the batch's event, taken when the next batch is already enqueued). Device memory: per track slot,
     * on top of dmx_tracks_infer_remix's, n_out x dmx_flac_bound(bits, n_max) bytes plus n_out x
     * dmx_flac_workspace_bytes(bits, n_max). dmx_output_spec users go through dmx_remix_two_stems or 0/1 gains. */
    int dmx_tracks_infer_flac(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                              const float *const *audio, const int64_t *n, int n_shifts, float overlap, const int *shift_offsets,
                              const dmx_remix_spec *spec, int sample_rate, void *const *out, int64_t *sizes, float *peaks, int layout,
                              dmx_progress_fn progress, void *user);

    /* ---- tracks as FLAC (csrc/flac_in.hip; DESIGN.md section 2.12, restated in tests/flac_in_spec.py): native FLAC streams
     * (RFC 9639) of 1 or 2 channels and 8, 12, 16, 20 or 24 bits, every subframe type (CONSTANT, VERBATIM, FIXED 0-4, LPC
     * 1-32), both Rice methods with escapes, wasted bits, the four channel assignments, fixed and variable blocking. CRC-8
     * and CRC-16 are verified on every frame; STREAMINFO's MD5 is NOT (it is serial over the whole stream). Out of scope,
     * each refused by the probe with its own message: Ogg FLAC, more than 2 channels, 32-bit samples, unknown length. */
    typedef struct dmx_flac_info
    {
        int sample_rate, channels, bits;
        int64_t total_samples;              /* per channel, >= 1 */
        int min_block, max_block;           /* STREAMINFO's block size range */
        int min_frame, max_frame;           /* STREAMINFO's frame byte range (0: unknown) */
        int variable_blocking;              /* the blocking strategy bit of the first frame */
        int64_t first_frame;                /* byte offset of the first frame */
    } dmx_flac_info;
#define DMX_FLAC_OK 0                   /* every sample was delivered                                         */
#define DMX_FLAC_BROKEN 1               /* the stream breaks at sample `good`: [good, n) is zero               */
#define DMX_FLAC_TOO_MANY_CANDIDATES 2  /* more header look-alikes than 2 * ceil(n / min_block) + 1024: good = 0 */
    /* pure host function, no GPU: skips an ID3v2 tag, checks "fLaC" and the metadata chain, reads STREAMINFO and locates the
     * first frame. Every failure returns DMX_ERR_FORMAT (DMX_ERR_ARG for a NULL pointer) with its own dmx_last_error text. */
    int dmx_flac_probe(const void *file, int64_t bytes, dmx_flac_info *info);
    /* bytes of device workspace one dmx_flac_decode_device call needs (candidate masks and tables, two int32 planes of
     * total_samples); -1 on an info the decoder does not take. Pure host function. */
    int64_t dmx_flac_decode_workspace_bytes(const dmx_flac_info *info, int64_t bytes);
    /* the file in device memory (d_file, `bytes` long, info from the probe) -> total_samples frames at d_out (16-byte
     * aligned, DMX_OUTPUT_STRIDE(total_samples * frame bytes) large): DMX_PCM_F32 interleaved stereo (float)v / 2^(bits-1)
     * with mono duplicated - the floats cli/wav.hpp gives for the same integers; DMX_PCM_S16 / DMX_PCM_S24 the bytes
     * csrc/pcm.hip writes, only for a stereo stream of exactly that depth. d_status: two int64 ON THE DEVICE, {DMX_FLAC_*,
     * good}: samples [0, good) are the stream's, [good, n) are zero. Asynchronous on `stream`, five launches, d_work
     * (dmx_flac_decode_workspace_bytes, 16-byte aligned) needs no initialisation. */
    int dmx_flac_decode_device(int device, const void *d_file, int64_t bytes, const dmx_flac_info *info, int encoding, void *d_out,
                               int64_t *d_status, void *d_work, void *stream);
    /* measurement aid: the same with HIP events around the five launches; synchronises `stream`; ms[0..5) receive the
     * milliseconds of candidates, scan, chain, decode, finish */
    int dmx_flac_decode_profile(int device, const void *d_file, int64_t bytes, const dmx_flac_info *info, int encoding, void *d_out,
                                int64_t *d_status, void *d_work, void *stream, float *ms);
    /* the same on host buffers: out holds total_samples * frame bytes, status two int64 */
    int dmx_flac_decode(int device, const void *file, int64_t bytes, const dmx_flac_info *info, int encoding, void *out, int64_t *status);
    /* dmx_tracks_infer_remix (flac_out == 0; sizes may be NULL) or dmx_tracks_infer_flac at 44100 Hz (flac_out != 0) on tracks
     * given as the images of .flac files: files[t] of file_bytes[t] bytes. Every file is probed before any GPU work; a probe
     * that fails, or a sample rate other than 44100, fails the call with a message that names the track, and nothing is
     * written. n[t] is the file's total_samples (>= 2), which sizes out[t] as there. The file's bytes go up on the upload
     * stream and are decoded in the track's slot (mono duplicated); the remix mixture is the decoded track. Damage inside
     * the frames is only known on the device: track_status[2 t], [2 t + 1] receive {DMX_FLAC_*, good} of track t, its samples
     * from `good` on are silence, every track runs to its end, and after all work has drained the call returns
     * DMX_ERR_FORMAT naming the first damaged track; the other tracks' outputs are complete and what a call without the
     * damaged track gives. Device memory: per track slot, on top of the output form's, the largest file and the largest
     * dmx_flac_decode_workspace_bytes. */
    int dmx_tracks_infer_from_flac(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                   const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                   const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                   float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user);

    /* ---- tracks at any sample rate. Track t has n[t] frames at rates[t] Hz. A track at 44100 Hz is
     * what the entry points above make of it, bit for bit. Any other track is the composition of the public calls:
     *   x44 = dmx_resample(x, rates[t] -> 44100), dmx_resample_length(n[t], rates[t], 44100) frames;
     *   the stems of x44 as dmx_tracks_infer_opts (models given: dmx_tracks_infer_bag) makes them: same shifts, overlap, rand() order;
     *   every stem plane v = dmx_resample(v44, 44100 -> rates[t]), cut to its first n[t] frames;
     *   spec NULL: fp32 stems S x 2 x n[t] in `layout` (sizes, peaks not used, flac_out must be 0); else the outputs of
     *   dmx_remix_encode on v with the CALLER's track (not the round trip) as the mixture and the peak over the n[t] native
     *   frames, as PCM (flac_out == 0) or as .flac files whose headers carry rates[t] (dmx_tracks_infer_flac's out / sizes).
     * Both conversions run in the track's slot: no stem crosses to the host at 44.1 kHz, and the pieces of a track leave as they
     * become final (a native-rate frame k is final once the 44.1 kHz frames below dmx_resample_ready's argument are). out[t],
     * dmx_output_bytes and dmx_flac_bound are sized by n[t]. Refused before any GPU work, naming the track, nothing written:
     * fewer than 2 frames at 44.1 kHz, a rate dmx_resample_filter refuses (or whose filter does not fit the kernel), FLAC
     * output above 655350 Hz. Device memory: as the entry point of the same output form on the lengths at 44.1 kHz, the encoded
     * outputs on n[t]; and, only in a call with a track that is not at 44100 Hz, per track slot 2 m_max floats (the track at
     * its rate) and n_sources x 2 x m_max floats (its stems at its rate), m_max the most frames of such a track. */
    int dmx_tracks_infer_rates(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                               const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                               const int *shift_offsets, const dmx_remix_spec *spec /* NULL: fp32 S x 2 x n[t] in layout */, int flac_out,
                               void *const *out, int64_t *sizes, float *peaks, int layout, dmx_progress_fn progress, void *user);
    /* dmx_tracks_infer_from_flac with every track at the rate of its file, as dmx_tracks_infer_rates runs it: the file is decoded
     * in the slot at its own rate (a damaged stream is silence from `good` on BEFORE the conversion; track_status is in the
     * file's frames). Device memory: both of the above. */
    int dmx_tracks_infer_from_flac_rates(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                         const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                         const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                         float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user);
    /* the two calls above behind the loudness stage (the section on loudness, above): the arguments of dmx_tracks_infer_rates
     * (rates == NULL: 44100 for all tracks) resp. dmx_tracks_infer_from_flac_rates, plus the loudness spec (required, as is
     * the remix spec) and the report, NULL or n_tracks x (n_out + 1) entries, per track its outputs and then its mixture.
     * DMX_LOUD_MIXTURE and DMX_LOUD_EACH make a track a whole-track one, as DMX_CLIP_RESCALE does: its outputs are measured,
     * gained, encoded and copied out behind its last piece. DMX_LOUD_MEASURE lets the pieces leave as without loudness, from
     * the kernels that run without it, and measures behind the last piece. The mixture is the caller's track at its own
     * rate (the slot's one upload); a damaged FLAC track is measured as it stands, silence from `good` on. The report leaves
     * with the peaks, which are those of the gained samples. Refused before any GPU work, naming the field and, for a rate
     * below DMX_LOUD_MIN_RATE, the track. Device memory: per track slot, on top of the call without loudness, (n_out + 1) x
     * dmx_loudness_workspace_bytes(n_max) + 64 + 16 (n_out + 1) bytes, and once per context the gain table (48 KB, built on
     * the host and uploaded by the context's first such call, freed with the context). */
    int dmx_tracks_infer_loud(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                              const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                              const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                              float *peaks, int layout, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud,
                              dmx_loudness_result *report);
    int dmx_tracks_infer_from_flac_loud(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                        const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                        const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out,
                                        int64_t *sizes, float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user,
                                        const dmx_loudness_spec *loud, dmx_loudness_result *report);
    /* the two calls above with a meters report (the section on meters, above): meters is NULL (the calls above) or n_tracks x
     * (n_out + 1) entries, per track the outputs and then the mixture, each signal as measured (in front of the gain). They
     * honour DMX_LOUD_TRUE_PEAK, as the calls above do: those then enqueue per track the true-peak launch over its outputs and
     * the gain launch's true-peak form, and nothing else new. Device memory: with the flag or a meters report, per track slot
     * another 64 + 16 (n_out + 1) bytes. */
    int dmx_tracks_infer_meters(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                const float *const *audio, const int64_t *n, const int *rates, int n_shifts, float overlap,
                                const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out, int64_t *sizes,
                                float *peaks, int layout, dmx_progress_fn progress, void *user, const dmx_loudness_spec *loud,
                                dmx_loudness_result *report, dmx_meters_result *meters);
    int dmx_tracks_infer_from_flac_meters(dmx_ctx *c, const dmx_model *const *models, int n_models, const float *weights, int n_tracks,
                                          const void *const *files, const int64_t *file_bytes, int n_shifts, float overlap,
                                          const int *shift_offsets, const dmx_remix_spec *spec, int flac_out, void *const *out,
                                          int64_t *sizes, float *peaks, int64_t *track_status, dmx_progress_fn progress, void *user,
                                          const dmx_loudness_spec *loud, dmx_loudness_result *report, dmx_meters_result *meters);
    /* pure host function: the outputs of a conversion of n_in -> n_out = dmx_resample_length frames that no longer change once
     * the inputs [0, n_in_final) are final: n_out when n_in_final == n_in, else min(n_out, max(0, ceil((n_in_final L - c) / M))),
     * the first output whose newest tap (c + k M) div L reaches n_in_final. -1: invalid argument */
    int64_t dmx_resample_ready(int64_t n_in_final, int64_t n_in, int rate_in, int rate_out, int64_t n_out);

    /* ---- building blocks of dmx_track_infer on device memory (segment sharding over
     * several GPUs: one process per GPU runs steps 2-3 on its share, results are gathered
     * (RCCL) to the root which runs step 4). All asynchronous on the context's stream.   */
    /* 0. geometry of the segment loop (src/model_apply.cpp:145-189) */
    int dmx_track_geometry(const dmx_ctx *c, int64_t n, int shift_offset, int64_t *shifted_len, int *n_segments,
                           int64_t *stride);
    /*    pure host function, no device: the segment-loop geometry for any overlap in [0, DMX_MAX_OVERLAP]
     *    (dmx_track_geometry is overlap = 0.25 on a context's segment) */
    int dmx_track_geometry_overlap(int64_t segment_samples, int64_t n, int shift_offset, float overlap, int64_t *shifted_len,
                                   int *n_segments, int64_t *stride);
    /* 1. mean / unbiased std of the mono reference (src/model_apply.cpp:72-78);
     *    d_audio interleaved [n][2]; d_stats: 2 floats */
    int dmx_track_stats_device(dmx_ctx *c, const float *d_audio, int64_t n, float *d_stats);
    /* 2. chunks seg_idx[0..n_idx) of the normalised, shifted, zero-padded track, each
     *    centred in a zero segment (src/model_apply.cpp:93-138,189-194,250-262)
     *    -> d_mix [n_idx][segment_samples][2]; seg_idx is a HOST array */
    int dmx_track_gather_device(dmx_ctx *c, const float *d_audio, int64_t n, const float *d_stats, int shift_offset,
                                const int *seg_idx, int n_idx, float *d_mix);
    /* 3. dmx_segment_infer_device on d_mix                                               */
    /* 4. triangle-weighted overlap-add of ALL n_segments outputs (segment order), divide
     *    by the weight sum, trim, de-normalise (src/model_apply.cpp:171-246,129-135,88);
     *    d_seg_out [n_segments][S][2][segment_samples]; d_out S x 2 x n in `layout`     */
    int dmx_track_overlap_add_device(dmx_ctx *c, const float *d_seg_out, int n_segments, int64_t n, int shift_offset,
                                     const float *d_stats, float *d_out, int layout);

    /* ---- several GPUs and / or a bag of models in ONE process (csrc/engine.cpp) ----------------------
     * Replaces the loop nest "for each model of the bag (cli-apps/demucs_ft.cpp:221-241): for each
     * overlapping segment (src/model_apply.cpp:189-235)": the (model, segment) work items are dealt in
     * contiguous, balanced ranges to the devices, every device runs its items on its own host thread and
     * stream, the per-item outputs are gathered to the root device over xGMI (RCCL send/recv, or SDMA
     * peer copies), and the root overlap-adds each model's segments in segment order - bit-identical to
     * dmx_track_infer on one device. n_models == 1: plain demucs_inference. n_models > 1 (= number of
     * sources): the fine-tuned bag, stem i of the result is stem i of model i (demucs_ft.cpp:238-241).
     *   devices / n_devices : HIP device ids (n_devices <= 0: all visible devices). The same id may be
     *                         listed more than once (several logical devices on one GPU; P2P transport only).
     *   transport           : DMX_TRANSPORT_AUTO = env DMX_GATHER ("rccl" / "p2p"), else RCCL when there
     *                         are >= 2 distinct devices, else P2P.
     * An engine serialises concurrent dmx_engine_track_infer calls internally (the reference's threaded
     * driver calls demucs_inference concurrently on one const model, threaded_inference.hpp:105-123).  */
#define DMX_TRANSPORT_AUTO 0
#define DMX_TRANSPORT_RCCL 1
#define DMX_TRANSPORT_P2P 2
    typedef struct dmx_engine dmx_engine;
    int dmx_engine_create(const char *const *model_files, int n_models, const int *devices, int n_devices, int max_batch,
                          int transport, dmx_engine **out);
    void dmx_engine_free(dmx_engine *e);
    int dmx_engine_n_devices(const dmx_engine *e);
    int dmx_engine_n_models(const dmx_engine *e);
    int dmx_engine_n_sources(const dmx_engine *e);
    int dmx_engine_arch(const dmx_engine *e); /* dmx_model_arch of its models */
    int dmx_engine_transport(const dmx_engine *e);
    /* where a track is finished (overlap-add, de-normalisation, copy-out). Same bits either way.
     *   DMX_FINISH_ROOT  (default): every device's segment blocks are gathered on the first device, which
     *                    overlap-adds the track - the reference's structure (model_apply.cpp:207-246) with
     *                    the gather SURVEY.md section 8e names;
     *   DMX_FINISH_OWNER (env DMX_FINISH=owner): the owner of segments [g0, g1) finishes the stretch
     *                    [g0*stride, g1*stride) itself; only the tail of segment g0-1 crosses the link
     *                    (2.75 MB instead of 11 MB per segment), and G devices copy out in parallel.
     *                    A bag in the Eigen layout is still finished on the root. */
#define DMX_FINISH_ROOT 0
#define DMX_FINISH_OWNER 1
    int dmx_engine_set_finish(dmx_engine *e, int finish);
    int dmx_engine_finish(const dmx_engine *e);
    /* the root device's context bound to model `model` (segment-level calls: dmx_segment_infer*) */
    dmx_ctx *dmx_engine_root_ctx(dmx_engine *e, int model);
    /* shift_offsets: one per model (NULL or -1 entries: rand() % 22050 drawn in model order, like the
     * reference's successive demucs_inference calls); audio 2 x n, out S x 2 x n, both `layout`. */
    int dmx_engine_track_infer(dmx_engine *e, const float *audio, int64_t n, const int *shift_offsets, float *out, int layout,
                               dmx_progress_fn progress, void *user);

    /* the dealing of (model, segment) items used by dmx_engine_track_infer (pure host function):
     * runs_out[(l*n_models + m)*2 + {0,1}] = segment range [g0, g1) of model m owned by device l */
    int dmx_engine_partition(const int *n_segments, int n_models, int n_devices, int *runs_out);

    /* ---- sample-rate conversion on the GPU (the step in front of the path; the role
     * libnyquist plays for the reference's CLIs, cli-apps/demucs.cpp:21-76). The reference itself rejects input that
     * is not 44.1 kHz (:30-36) and so do the drop-in CLIs unless DMX_RESAMPLE=1 is set; there is no reference
     * arithmetic to reproduce. Specification (csrc/resample.hip, restated in oracle/resample_oracle.py and pinned
     * there against scipy.signal.resample_poly): L/M = rate_out/rate_in in lowest terms, R = max(L, M), c = 16 R,
     * h[i] = sinc((i - c)/R) * kaiser(beta 8.6), i = 0..2c, sum(h) = L;  y[k] = sum_j x[j] h[c + k M - j L] for
     * k < ceil(n L / M), x = 0 outside [0, n); per output one fp32 fmaf chain in ascending tap order.          */
    int64_t dmx_resample_length(int64_t n_in, int rate_in, int rate_out); /* ceil(n_in L / M); -1: invalid argument */
    /* the filter (pure host function, no GPU): up = L, down = M, taps h[0 .. n_taps-1] (taps may be NULL) */
    int dmx_resample_filter(int rate_in, int rate_out, int *up, int *down, int *n_taps, float *taps, int cap);
    /* `planes` signals of n_in samples; element (plane, j) at plane*plane_stride + j*sample_stride (floats):
     * interleaved stereo = planes 2, strides 1 and 2; planar = strides n and 1. Device pointers on `device`,
     * enqueued on `stream` (hipStream_t, may be NULL).                                                        */
    int dmx_resample_device(int device, const float *d_in, int64_t n_in, int planes, int64_t in_plane_stride, int64_t in_sample_stride,
                            int rate_in, int rate_out, float *d_out, int64_t out_plane_stride, int64_t out_sample_stride, void *stream);
    /* host buffers; interleaved != 0: [n][planes], else [planes][n]; out holds dmx_resample_length() samples per plane */
    int dmx_resample(int device, const float *in, int64_t n_in, int planes, int interleaved, int rate_in, int rate_out, float *out);

    /* ---- debug taps (layer-level parity tests, cf. the reference's print-only layer tests
     * test/test_layers.cpp:1390-2157): copies a named intermediate activation of the last
     * dmx_segment_infer* call to the host. shape[0] is the batch. Returns ndim or -1.      */
    int dmx_debug_tap(dmx_ctx *c, const char *name, int64_t *shape, float *host_dst);
    int dmx_debug_n_ops(const dmx_ctx *c);
    /* per-op timing with HIP events on the context's stream (`reps` launches per op); fills
     * `report` with lines "name\tkernel\tms_per_launch\talgorithmic_flops\talgorithmic_bytes".
     * Returns the number of ops or -1. Leaves the activations undefined.                   */
    int dmx_debug_profile(dmx_ctx *c, int batch, int reps, char *report, int report_cap);
    /* ---- one op at a time (op-level parity tests). All act on the context's own plan for `batch` (1 .. max batch) and launch
     * on the context's stream; every launch is followed by a checked synchronisation and returns its error.
     * dmx_debug_plan_info: number of ops, floats of the context's arena, of the plan's part of it, and of its leading constants.
     * dmx_debug_op_info: one line of key=value words for op i: name kind stream reads= writes= scratch= (arena ranges lo:hi, ...
     *   as the plan's dependency analysis sees them; scratch: what the kernel may write beyond its results) launches= (0: a
     *   marker, or an inverse STFT that runs inside the following overlap-add) and, for a GEMM, K N M pro epi act res stat hterms
     *   y ldy Kp w_w bias_w kvCol0 cfg family arith wnf label BM BN NB (rowstat= kv= kvPlane=). Returns the length or -1.
     * dmx_debug_arena_fill: every float of the arena = the 32-bit pattern, then the plan's constants restored.
     * dmx_debug_arena_io: copies n floats at arena offset off from (write != 0) or to the host.
     * dmx_debug_run_op: launches op i alone.
     * dmx_debug_op_cfgs / dmx_debug_run_op_as: the tile configurations GEMM i may be asked to run on, and a run of a copy of it
     *   on one of them with the kernel the selection gives under lin_mode (DMX_SPLIT_LIN); DMX_DEBUG_NO_KERNEL, nothing
     *   launched, where that kernel does not exist; `choice` receives "cfg= family= arith= wnf= label= BM= BN= NB=".
     * dmx_debug_run_attention_as: a run of a copy of attention op i (the transformer's or v3's LocalState) in form 0 = 64-query
     *   workgroups, 1 = 128-query workgroups, 2 = paired (the form= word of dmx_debug_op_info names the plan's own);
     *   DMX_DEBUG_NO_KERNEL, nothing launched, where the form does not exist: paired without K / V operand planes, with keys that
     *   are no whole 64-key tiles or in a DMX_GEMM_F32 context; LocalState in anything but form 0.                          */
    int dmx_debug_plan_info(dmx_ctx *c, int batch, int *n_ops, int64_t *arena_floats, int64_t *plan_floats, int64_t *const_floats);
    int dmx_debug_op_info(dmx_ctx *c, int batch, int i, char *buf, int cap);
    int dmx_debug_arena_fill(dmx_ctx *c, int batch, unsigned pattern);
    int dmx_debug_arena_io(dmx_ctx *c, int64_t off, int64_t n, float *host, int write);
    int dmx_debug_run_op(dmx_ctx *c, int batch, int i);
    int dmx_debug_op_cfgs(dmx_ctx *c, int batch, int i, int *cfgs, int cap);
    int dmx_debug_run_op_as(dmx_ctx *c, int batch, int i, int cfg, int lin_mode, char *choice, int cap);
    int dmx_debug_run_attention_as(dmx_ctx *c, int batch, int i, int form);
    /* the operand splits of DMX_GEMM_BF16X3, exposed for their unit tests. Weights (pure host function): w[i] -> bf16 bit
     * patterns w1[i], w2[i]; returns the number of elements with w1 + w2 != w. Activations (runs the kernels' own device
     * function on `device`): x[i] -> planes[0..n), [n..2n), [2n..3n) = a1, a2, a3; host pointers. */
    int64_t dmx_debug_split_weights(const float *w, int64_t n, unsigned short *w1, unsigned short *w2);
    int dmx_debug_split_activations(int device, const float *x, int64_t n, unsigned short *planes);
    /* the fp16 three-term split of DMX_GEMM_FP16X3 applied to x[i] * 2^scale_exp (|scale_exp| <= 126): planes[0..n), [n..2n),
     * [2n..3n) = h1, h2, h3 as fp16 bit patterns; host pointers (unit test of the split and of its stated bound) */
    int dmx_debug_split_activations_fp16(int device, const float *x, int64_t n, int scale_exp, unsigned short *planes);

#ifdef __cplusplus
}
#endif
#endif /* DEMUCS_HIP_H */
