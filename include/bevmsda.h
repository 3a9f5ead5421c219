/* bevmsda — C ABI of the MI355X-native multi-scale deformable attention path.
 *
 * This header is the drop-in boundary for BEVFormer's BEV-encoder hot path.
 * The entry points replace the two functions the reference binds from
 * mmcv-full's `_ext` module
 *     ext_loader.load_ext('_ext', ['ms_deform_attn_backward', 'ms_deform_attn_forward'])
 *     (projects/mmdet3d_plugin/bevformer/modules/multi_scale_deformable_attn_function.py:10-12)
 * and are what `bevformer_amd/ext.py` (the `_ext`-shaped Python module) calls
 * through ctypes.  Plain pointers and sizes only: no torch types, no ownership
 * transfer, no allocation — the caller owns every buffer, exactly as in the
 * reference where Python allocates the gradient buffers
 * (multi_scale_deformable_attn_function.py:146-148).
 *
 * Conventions (identical to the reference op, ibid. :97-112):
 *   value          (N, S, M, D)        contiguous, S = sum_l H_l*W_l
 *   spatial_shapes (L, 2) int64        (H_l, W_l), DEVICE memory
 *   level_start    (L,)   int64        first row of level l in S, DEVICE memory
 *   loc            (N, Q, M, L, P, 2)  fp32 (x, y), normalised to [0,1]
 *   attn           (N, Q, M, L, P)     fp32
 *   out / grad_out (N, Q, M*D)
 * All device pointers must be 16-byte aligned (torch allocations are).
 * `stream` is a hipStream_t (NULL = the null stream).  Every function is
 * asynchronous with respect to the host, re-entrant, keeps no global state and
 * never throws; it returns BEVMSDA_OK or a negative error code.
 */
#ifndef BEVMSDA_H_
#define BEVMSDA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7: bevmsda_fused_desc.reserved narrowed (the retired sampling A/B knobs return BEVMSDA_ERR_BAD_OPTION: see the struct);
 * nothing else changed, entry points and layouts are those of version 6 */
#define BEVMSDA_ABI_VERSION 7

enum {
  BEVMSDA_OK = 0,
  BEVMSDA_ERR_NULL_POINTER = -1, /* a required pointer is NULL               */
  BEVMSDA_ERR_BAD_SHAPE = -2,    /* negative dim, or a dim of 0 where illegal */
  BEVMSDA_ERR_TOO_LARGE = -3,    /* S*M*D or Q*M*L*P*2 does not fit int32     */
  BEVMSDA_ERR_MISALIGNED = -4,   /* pointer not 16-byte aligned               */
  BEVMSDA_ERR_LAUNCH = -5,       /* hipLaunchKernel failed (see hipGetLastError) */
  BEVMSDA_ERR_BAD_OPTION = -6,   /* unknown tuning value                      */
  BEVMSDA_ERR_UNSUPPORTED = -7   /* shape not covered by this entry point: use the unfused one */
};

/* Optional launch tuning (benchmark sweeps).  Zero-initialise for defaults. */
typedef struct bevmsda_tuning {
  int32_t variant;   /* 0 = library default; 1 = generic lane-group kernels; 2 = one lane per
                        channel; 3/4/5 = D=32 forward sized for 4/8/2 waves per SIMD */
  int32_t qtile;     /* 0 = default; queries of one head handled by adjacent lane groups */
  int32_t xcd_remap; /* 0 = default, 1 = off, 2 = on: contiguous row ranges per XCD */
  int32_t reserved[5]; /* backward only: [0] = rows per workgroup of the grad_value sort kernel (0 = default; 64 / 128 /
                          256); [1], [2] = low / high word of a DEVICE address of 8 uint64 that receive the phase clocks
                          of that kernel (0 = off; tools/gvprof.py); [3] = 1: bf16 storage takes the 8-byte-lane gather
                          kernel instead of the 16-byte-lane one */
} bevmsda_tuning;

int bevmsda_abi_version(void);
const char *bevmsda_error_string(int code);

/* ms_deform_attn_forward (call site: multi_scale_deformable_attn_function.py:118-124).
 * Writes every element of `out`. */
int bevmsda_forward_f32(const float *value, const int64_t *spatial_shapes,
                        const int64_t *level_start, const float *loc, const float *attn,
                        int N, int S, int M, int D, int L, int Q, int P, float *out,
                        void *stream);

/* ms_deform_attn_backward (call site: ibid. :150-160).
 * grad_value is ACCUMULATED into (the caller zeroes it, ibid. :146);
 * grad_loc and grad_attn are fully overwritten. */
int bevmsda_backward_f32(const float *value, const int64_t *spatial_shapes,
                         const int64_t *level_start, const float *loc, const float *attn,
                         const float *grad_out, int N, int S, int M, int D, int L, int Q, int P,
                         float *grad_value, float *grad_loc, float *grad_attn, void *stream);

/* bf16 storage variants: value / out / grad_out are bfloat16 (uint16_t bit
 * patterns), sampling locations, attention weights and all arithmetic stay
 * fp32; grad_value is accumulated in fp32.  No reference semantics exist for
 * this (the reference always up-casts to fp32, ibid. :93) — tolerance is
 * stated against the fp32 oracle in tests/. */
int bevmsda_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                         const int64_t *level_start, const float *loc, const float *attn,
                         int N, int S, int M, int D, int L, int Q, int P, uint16_t *out,
                         void *stream);
int bevmsda_backward_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                          const int64_t *level_start, const float *loc, const float *attn,
                          const uint16_t *grad_out, int N, int S, int M, int D, int L, int Q,
                          int P, float *grad_value, float *grad_loc, float *grad_attn,
                          void *stream);

/* Ragged batches: R query rows in total, row r samples value[row_batch[r]]
 * (row_batch: int32, DEVICE memory, values in [0,N)); loc is (R, M, L, P, 2),
 * attn (R, M, L, P), out / grad_out (R, M*D).  This is how the encoder runs
 * SpatialCrossAttention without the reference's zero-padded per-camera
 * rebatch (spatial_cross_attention.py:143-153: rows beyond a camera's hit
 * count are computed and thrown away there) — same results, fewer rows. */
int bevmsda_forward_ragged_f32(const float *value, const int64_t *spatial_shapes,
                               const int64_t *level_start, const float *loc, const float *attn,
                               const int32_t *row_batch, int N, int S, int M, int D, int L,
                               int R, int P, float *out, void *stream);
int bevmsda_backward_ragged_f32(const float *value, const int64_t *spatial_shapes,
                                const int64_t *level_start, const float *loc, const float *attn,
                                const int32_t *row_batch, const float *grad_out, int N, int S,
                                int M, int D, int L, int R, int P, float *grad_value,
                                float *grad_loc, float *grad_attn, void *stream);
int bevmsda_forward_ragged_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                                const int64_t *level_start, const float *loc, const float *attn,
                                const int32_t *row_batch, int N, int S, int M, int D, int L,
                                int R, int P, uint16_t *out, void *stream);
int bevmsda_backward_ragged_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                                 const int64_t *level_start, const float *loc, const float *attn,
                                 const int32_t *row_batch, const uint16_t *grad_out, int N, int S,
                                 int M, int D, int L, int R, int P, float *grad_value,
                                 float *grad_loc, float *grad_attn, void *stream);

/* bevmsda_backward_ragged_* with the row count in DEVICE memory (`nrows`, read when the kernels run; csrc/frame_plan.h
 * writes it): R is the CAPACITY of the row arrays (loc, attn, row_batch, grad_out, grad_loc, grad_attn), rows
 * [0, min(*nrows, R)) are processed, the others neither read nor written — no host synchronisation between the frame
 * plan and the backward of multi_scale_deformable_attn_function.py:130-163, so a training step can be captured in a
 * HIP graph.  `grad_value_stride`: floats between two pixels of grad_value (0 = M * D, the dense (N, S, M, D) array;
 * larger, a multiple of 4: the pixel rows of a wider array — the gradients of the encoder layers' value projections of a
 * frame side by side, the operand of ONE input-gradient GEMM).
 * Second-generation kernels only: D = 32, P in {4, 8}, L <= 4, value < 2 GiB; else BEVMSDA_ERR_UNSUPPORTED. */
int bevmsda_backward_rows_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                              const float *loc, const float *attn, const int32_t *row_batch, const float *grad_out,
                              const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                              float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream);
int bevmsda_backward_rows_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                               const float *loc, const float *attn, const int32_t *row_batch, const uint16_t *grad_out,
                               const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                               float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream);

/* bevmsda_backward_rows_* WITHOUT the sampling locations as an operand (round 6): when the forward was
 * bevmsda_fused_forward_rows_save_* with save_loc = NULL, the backward kernels recompute every location from what that
 * forward read, with its own two operations (spatial_cross_attention.py:357-372: reference + offset / (W_l, H_l)):
 *   loc(r, m, l, p) = ref[(r * A + p % A) * 2 + c] + offs[row_src[r] * proj_row + m * off_head + (l * P + p) * 2 + c] / (W_l, H_l)[c]
 * (row_src NULL: row r itself; one queue entry, pillar-anchor references: the K = 1, ref_mode = 0 form of
 * bevmsda_fused_desc).  `attn` stays an operand (the forward's save_attn).  What multi_scale_deformable_attn_function.py
 * :94-128 keeps for backward shrinks from 12 to 4 bytes per sampling point (564 MB of a bevformer_base training step); the
 * step takes the same time — what the forward kernel gains without its location stores (32 us of 335 per layer) the backward
 * kernels spend on the row_src -> offset indirection (profiles/r6/r6t_fused_save_ab.txt, r6s_save_loc_cost.txt).
 * offs / ref 8-byte aligned, proj_row and off_head even; else as bevmsda_backward_rows_*. */
typedef struct bevmsda_loc_source {
  const float *offs;        /* sampling-offset projections (the fused forward's `offs`) */
  const float *ref;         /* reference points (R, A, 2), normalised (x, y) */
  const int32_t *row_src;   /* optional: projection row of operand row r */
  int64_t proj_row;         /* floats between two projection rows */
  int32_t off_head;         /* floats between two heads' offsets inside a row */
  int32_t A;                /* reference points per row: point p uses anchor p % A */
} bevmsda_loc_source;
int bevmsda_backward_rows_offs_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const bevmsda_loc_source *loc_source, const float *attn, const int32_t *row_batch,
                                   const float *grad_out, const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                                   float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream);
int bevmsda_backward_rows_offs_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                    const bevmsda_loc_source *loc_source, const float *attn, const int32_t *row_batch,
                                    const uint16_t *grad_out, const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                                    float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream);

/* bevmsda_backward_* whose N * Q operand rows SHARE `grad_rows` rows of grad_out: row r reads grad_scale *
 * grad_out[r % grad_rows] — TemporalSelfAttention averages its queue entries (temporal_self_attention.py:257-262), so the
 * N = 2 entries of a query receive the same output gradient times 1 / 2; no repeated, pre-scaled copy of it is formed.
 * `grad_value_stride`: as in bevmsda_backward_rows_*.  Second-generation kernels only (D = 32, P in {4, 8}, L <= 4). */
int bevmsda_backward_shared_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *loc,
                                const float *attn, const float *grad_out, int64_t grad_rows, float grad_scale, int N, int S, int M,
                                int D, int L, int Q, int P, float *grad_value, int64_t grad_value_stride, float *grad_loc,
                                float *grad_attn, void *stream);
int bevmsda_backward_shared_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *loc,
                                 const float *attn, const uint16_t *grad_out, int64_t grad_rows, float grad_scale, int N, int S,
                                 int M, int D, int L, int Q, int P, float *grad_value, int64_t grad_value_stride, float *grad_loc,
                                 float *grad_attn, void *stream);

/* Same as above with explicit tuning. */
int bevmsda_forward_f32_ex(const float *value, const int64_t *spatial_shapes,
                           const int64_t *level_start, const float *loc, const float *attn,
                           int N, int S, int M, int D, int L, int Q, int P, float *out,
                           void *stream, const bevmsda_tuning *tuning);
int bevmsda_backward_f32_ex(const float *value, const int64_t *spatial_shapes,
                            const int64_t *level_start, const float *loc, const float *attn,
                            const float *grad_out, int N, int S, int M, int D, int L, int Q,
                            int P, float *grad_value, float *grad_loc, float *grad_attn,
                            void *stream, const bevmsda_tuning *tuning);
int bevmsda_forward_bf16_ex(const uint16_t *value, const int64_t *spatial_shapes,
                            const int64_t *level_start, const float *loc, const float *attn,
                            int N, int S, int M, int D, int L, int Q, int P, uint16_t *out,
                            void *stream, const bevmsda_tuning *tuning);
int bevmsda_backward_bf16_ex(const uint16_t *value, const int64_t *spatial_shapes,
                             const int64_t *level_start, const float *loc, const float *attn,
                             const uint16_t *grad_out, int N, int S, int M, int D, int L, int Q,
                             int P, float *grad_value, float *grad_loc, float *grad_attn,
                             void *stream, const bevmsda_tuning *tuning);

/* Fused front end of the two attention modules (inference path).
 *
 * The reference computes, with separate elementwise launches per layer,
 *     attention_weights = softmax(logits over L*P)          spatial_cross_attention.py:340-348
 *                                                            temporal_self_attention.py:209-211
 *     sampling_locations = reference + offsets / (W_l, H_l)  spatial_cross_attention.py:357-372
 *                                                            temporal_self_attention.py:224-229
 * and, in TemporalSelfAttention, the mean over the two BEV-queue entries after the
 * operator (temporal_self_attention.py:257-262).  This entry point takes the raw
 * projection outputs and does all of it inside the sampling kernel.
 *
 *   offs    sampling-offset projections, element (r, m, q, l, p, c) at
 *           offs[r*proj_row + m*off_head + q*off_k + (l*P + p)*2 + c]
 *   logits  attention logits, element (r, m, q, l, p) at
 *           logits[r*proj_row + m*lg_head + q*lg_k + l*P + p]      (softmax over l, p)
 *   ref     (R, K, A, 2) fp32 normalised reference points; ref_mode 0: point p uses
 *           anchor p % A (the pillar anchors of MSDeformableAttention3D), ref_mode 1:
 *           level l uses ref l (A = L)
 *   row_batch  optional (R,) int32: value batch entry base of row r (else r / Q)
 *   row_src    optional (R,) int32: row of offs / logits used by output row r (else r) —
 *              SpatialCrossAttention projects every BEV query once and each camera that
 *              sees the query reads the same projection row
 *   value batch entry of (row r, queue entry q) = base * vmul + q * vadd
 *   out     (R, M*D) = (1/K) * sum_q sample(value[entry(r, q)], loc(r, q), softmax(r, q))
 * Supported: D = 32, P in {4, 8}, 1 <= L <= 4, K in {1, 2} with P*K <= 8, value < 2 GiB; anything else
 * returns BEVMSDA_ERR_UNSUPPORTED and the caller uses bevmsda_forward_*.  Forward only. */
typedef struct bevmsda_fused_desc {
  int64_t R;          /* output rows */
  int64_t proj_row;   /* row stride of offs / logits, in floats (even) */
  int32_t N, S, M, D, L, P, Q;
  int32_t K, A, ref_mode;
  int32_t off_head, off_k, lg_head, lg_k;
  int32_t vmul, vadd;
  int32_t reserved[6];   /* bf16 entry points only: [1] = 1 selects the 8-byte-lane kernel instead of the 16-byte-lane one,
                            [2] = 1 (16-byte-lane kernel) makes `out` an fp32 (R, M*D) matrix; [3]: the row-count hint of
                            the _rows_ entry points (below), 0 elsewhere; [5]: 0 = default, 1 = generic kernel bodies only
                            (fp32: TemporalSelfAttention's shape not on its body with compile-time head / level counts).
                            [0] and [4] are 0.  Anything else: BEVMSDA_ERR_BAD_OPTION, on every entry point, before any
                            launch (since ABI version 7; the knobs that lived here are in tools/experimental/) */
} bevmsda_fused_desc;

int bevmsda_fused_forward_f32(const float *value, const int64_t *spatial_shapes,
                              const int64_t *level_start, const float *offs, const float *logits,
                              const float *ref, const int32_t *row_batch, const int32_t *row_src,
                              const bevmsda_fused_desc *desc, float *out, void *stream);

/* bevmsda_fused_forward_f32 over a value of which only some row panels were projected
 * (bevmsda_linear_panel_rows2_masked_f32), with a device-side check instead of advance knowledge of the offsets:
 * need (need_len int32, DEVICE memory): entry e != 0 <=> cells [e << need_shift, (e + 1) << need_shift) of every value
 * batch entry hold projected rows; need_len << need_shift >= desc->S.  A tap of an output row with a non-zero BILINEAR
 * COEFFICIENT on a cell outside them ORs 1 into *halo_flag (int32, DEVICE memory; the caller clears it) — whatever its
 * attention weight: one that underflowed to 0 would still multiply whatever the unprojected row holds (0 x NaN):
 * the output is then not to be used.  Taps with a zero coefficient are issued as always (0 x NaN is NaN: the projection's
 * table must also cover max W + 1 rows around the needed ones) and do not raise the flag.  Same sums in the same order as
 * bevmsda_fused_forward_f32, for either value of desc->reserved[5].  Covered: K = 2, P = 4 (TemporalSelfAttention); else
 * BEVMSDA_ERR_UNSUPPORTED. */
int bevmsda_fused_forward_halo_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                   const int32_t *row_src, const bevmsda_fused_desc *desc, const int32_t *need,
                                   int need_shift, int64_t need_len, int32_t *halo_flag, float *out, void *stream);
int bevmsda_fused_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                               const int64_t *level_start, const float *offs,
                               const float *logits, const float *ref, const int32_t *row_batch,
                               const int32_t *row_src, const bevmsda_fused_desc *desc,
                               uint16_t *out, void *stream);

/* The same entry points with the ROW COUNT in device memory: desc->R is the capacity of the row
 * arrays (row_batch, row_src, ref, out), `nrows` points to the actual count (int32, DEVICE memory,
 * e.g. counters[0] of bevmsda_frame_plan_f32), read by the kernels when they run.
 * desc->reserved[3] = the caller's HINT of the count (0 = none): rows below the hint are covered by
 * a launch with one workgroup per block of rows like the fixed-count entry point, rows beyond it by
 * a small strided launch — any count <= desc->R is computed correctly, the hint only sizes the
 * grids.  The launch geometry depends on (capacity, hint) only, so one captured HIP graph serves
 * every frame. */
int bevmsda_fused_forward_rows_f32(const float *value, const int64_t *spatial_shapes,
                                   const int64_t *level_start, const float *offs, const float *logits,
                                   const float *ref, const int32_t *row_batch, const int32_t *row_src,
                                   const int32_t *nrows, const bevmsda_fused_desc *desc, float *out,
                                   void *stream);
int bevmsda_fused_forward_rows_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                                    const int64_t *level_start, const float *offs, const float *logits,
                                    const float *ref, const int32_t *row_batch, const int32_t *row_src,
                                    const int32_t *nrows, const bevmsda_fused_desc *desc, uint16_t *out,
                                    void *stream);

/* bevmsda_fused_forward_rows_* that also WRITE what the operator's backward reads (training forward of
 * SpatialCrossAttention's sampling: K = 1, P = 8, L >= 2; else BEVMSDA_ERR_UNSUPPORTED): save_loc (R, M, L, P, 2) = the
 * sampling locations reference + offset / (W_l, H_l) (spatial_cross_attention.py:357-372), save_attn (R, M, L, P) = the
 * softmax over the L * P logits of a head (:340-348) — the operands `sampling_locations` / `attention_weights` that
 * multi_scale_deformable_attn_function.py:94-128 saves for backward.  Rows [0, *nrows) are written.  The backward then
 * needs no bevmsda_frontend_expand_rows_f32 pass.  save_loc may be NULL: the locations are then not written and the
 * backward is bevmsda_backward_rows_offs_* (above), which recomputes them. */
int bevmsda_fused_forward_rows_save_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                        const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                        const int32_t *row_src, const int32_t *nrows, const bevmsda_fused_desc *desc, float *out,
                                        float *save_loc, float *save_attn, void *stream);
int bevmsda_fused_forward_rows_save_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                         const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                         const int32_t *row_src, const int32_t *nrows, const bevmsda_fused_desc *desc,
                                         uint16_t *out, float *save_loc, float *save_attn, void *stream);

/* Backward of bevmsda_fused_forward_f32 in three steps (the autograd path of the modules; reference statements:
 * bevformer/modules/spatial_cross_attention.py:340-372, temporal_self_attention.py:209-229, 257-262 — what
 * autograd records there as softmax / divide / add / view nodes):
 *   1. bevmsda_frontend_expand_f32: the raw projection rows -> sampling locations `loc` (K*R, M, L, P, 2),
 *      attention weights `attn` (K*R, M, L, P) and `row_batch_k` (K*R) = the value batch entry of every (queue entry,
 *      row), QUEUE-MAJOR (row q*R + r): the operands of bevmsda_backward_ragged_f32 (or, with one batch element and
 *      one value batch entry per queue entry, of bevmsda_backward_f32 with N = K, Q = R), recomputed instead of saved
 *      by the forward;
 *   2. the operator's backward over those K*R rows with grad_out[q*R + r] = grad_out[r] / K;
 *   3. bevmsda_frontend_chain_f32: its grad_loc / grad_attn -> the gradient of the raw projection rows (softmax
 *      backward over the L*P logits of a (row, head, queue entry); 1 / (W_l, H_l) on the offsets).  With `row_src`
 *      (several rows share a projection row) the results are ADDED to grad_offs / grad_logits with fp32 atomics — the
 *      caller zeroes them; without it they are stored.  grad_offs / grad_logits address the gradient matrix exactly as
 *      offs / logits address the projection matrix (same desc->proj_row, off_head, off_k, lg_head, lg_k).
 * Supported: P in {4, 8}, L <= 4, K in {1, 2}; else BEVMSDA_ERR_UNSUPPORTED. */
int bevmsda_frontend_expand_f32(const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                const int32_t *row_src, const int64_t *spatial_shapes, const bevmsda_fused_desc *desc,
                                float *loc, float *attn, int32_t *row_batch_k, void *stream);
/* Step 1 with the row count in device memory (K = 1): desc->R is the capacity, rows [0, min(*nrows, R)) are written. */
int bevmsda_frontend_expand_rows_f32(const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                     const int32_t *row_src, const int32_t *nrows, const int64_t *spatial_shapes,
                                     const bevmsda_fused_desc *desc, float *loc, float *attn, int32_t *row_batch_k,
                                     void *stream);
int bevmsda_frontend_chain_f32(const float *grad_loc, const float *grad_attn, const float *attn, const int32_t *row_src,
                               const int64_t *spatial_shapes, const bevmsda_fused_desc *desc, float *grad_offs,
                               float *grad_logits, void *stream);
/* Step 3 as a gather (K = 1, L in {1, 2, 4}): `q_rows` (slots, J) int32 lists the rows that read projection row
 * `slot` (-1 = none; the frame plan's table, spatial_cross_attention.py:136-153 inverted); every element of the
 * gradient matrix rows [0, slots) is STORED (no atomics, no zeroing by the caller, fixed summation order).
 * `n_extra` (device, may be NULL): the frame plan's count of slots with more than two rows; when it reads 0 only the
 * first two columns of the table are walked (rows fill the columns in order). */
int bevmsda_frontend_chain_gather_f32(const float *grad_loc, const float *grad_attn, const float *attn,
                                      const int32_t *q_rows, int64_t slots, int J, const int32_t *n_extra,
                                      const int64_t *spatial_shapes, const bevmsda_fused_desc *desc, float *grad_offs,
                                      float *grad_logits, void *stream);

/* Row-wise helpers of the encoder layer (csrc/rowops.h), fp32, forward only.
 *
 * out = LayerNorm(x + res) * gamma + beta over the last dimension C (res may be NULL):
 * the "+ identity" of every attention / FFN step followed by the layer's norm
 * (encoder.py:360-404; torch.nn.LayerNorm semantics: biased variance, eps inside the
 * square root).  C must be 256, 512 or 1024. */
int bevmsda_add_layernorm_f32(const float *x, const float *res, const float *gamma,
                              const float *beta, float eps, int64_t rows, int C, float *out,
                              void *stream);

/* Backward of bevmsda_add_layernorm_f32 (what autograd records for `dropout(x) + identity` followed by
 * torch.nn.LayerNorm, encoder.py:360-404): grad_x (rows, C) = the gradient of BOTH x and res (z = x + res is
 * recomputed, the forward saves nothing); grad_gamma_beta (2, C) = [sum_rows g * xhat ; sum_rows g], written (not
 * accumulated).  `scratch`: bevmsda_add_layernorm_backward_partials(rows) * 2 * C floats (per-workgroup partial
 * column sums, reduced by a second small launch).  C in {256, 512}. */
int64_t bevmsda_add_layernorm_backward_partials(int64_t rows);
int bevmsda_add_layernorm_backward_f32(const float *x, const float *res, const float *gamma, const float *grad_out,
                                       float eps, int64_t rows, int C, float *grad_x, float *scratch,
                                       float *grad_gamma_beta, void *stream);
/* The same with the incoming gradient given as TWO addends, grad_out + grad_out2 (grad_out2 may be NULL): a residual
 * branch's gradient and a projection's input gradient meet in front of a LayerNorm without a separate add pass. */
int bevmsda_add_layernorm_backward2_f32(const float *x, const float *res, const float *gamma, const float *grad_out,
                                        const float *grad_out2, float eps, int64_t rows, int C, float *grad_x,
                                        float *scratch, float *grad_gamma_beta, void *stream);
/* out[q, :] = scale[q] * sum_{j<J, idx[q,j]>=0} rows[idx[q,j], :] — the per-camera
 * scatter-add and division by the camera count of SpatialCrossAttention
 * (spatial_cross_attention.py:165-172) as a gather.  idx: (Q, J) int32, -1 = empty. */
int bevmsda_gather_mean_f32(const float *rows, const int32_t *idx, const float *scale, int64_t Q,
                            int J, int C, float *out, void *stream);

/* Backward of bevmsda_gather_mean_f32 w.r.t. `rows`: rows[r, :] = scale[s] * slots[s, :] with s = row_slot[r] (the
 * inverse of idx: the frame plan's row -> BEV query table), for r in [0, min(*nrows, R)) (`nrows`: device-side row
 * count, may be NULL = R); other rows are not touched.  C a multiple of 4. */
int bevmsda_rows_from_slots_f32(const float *slots, int64_t ld_slots, const float *scale, const int32_t *row_slot,
                                const int32_t *nrows, int64_t R, int C, float *rows, void *stream);

/* out[r, :] = bf16(scale * in[r, :]) (round to nearest even) for r in [0, min(*nrows, R)) (`nrows` device-side, may be
 * NULL = R): the incoming gradient rows of the sampling backward converted to the bf16 storage type of its kernels
 * without touching the unused capacity of a device-side plan.  Dense (R, C) matrices, C a multiple of 8. */
int bevmsda_cast_rows_bf16(const float *in, const int32_t *nrows, int64_t R, int C, float scale, uint16_t *out, void *stream);

/* Dense projection on the matrix cores (csrc/linear_mfma.h), fp32 in / fp32 out, forward only:
 *
 *     y[m, n] = act( sum_k A[m, k] * w[n, k] + bias[n] ),   A = [ x0 (+ a0) | x1 (+ a1) ]
 *
 * = torch.nn.functional.linear, the value / sampling_offsets / attention_weights /
 * output_proj Linear layers and the FFN of the encoder layer
 * (temporal_self_attention.py:198,206-211,267; spatial_cross_attention.py:173,334-348;
 * custom_base_transformer_layer.py:157-158).  The optional second source x1 concatenates
 * along K in place (TemporalSelfAttention's cat([value[:bs], query + query_pos], -1),
 * temporal_self_attention.py:186-197); a0 / a1 are optional element-wise addends (query_pos).
 * precision 0: every fp32 operand is split into two bf16 terms and each product is
 * accumulated in fp32 from three bf16 MFMAs (>= 16 mantissa bits per product); precision 1:
 * operands rounded to bf16 (one MFMA), fp32 accumulation.
 * Requirements: K0, K1 multiples of 32 (K1 may be 0 with x1 NULL), input row strides
 * multiples of 4 floats, input pointers 16-byte aligned (y: any float pointer / stride);
 * otherwise BEVMSDA_ERR_UNSUPPORTED / _MISALIGNED and
 * the caller uses the library GEMM. */
typedef struct bevmsda_linear_desc {
  int64_t M;                                  /* rows of A and y */
  int64_t ldx0, lda0, ldx1, lda1, ldw, ldy;   /* row strides in floats */
  int32_t N, K0, K1;
  int32_t relu;                               /* 1: y = max(y, 0) after the bias */
  int32_t precision;                          /* 0 = split-fp32 (3 products), 1 = bf16 inputs */
  int32_t variant;                            /* 0 = library default; 1 = first kernel over the fp32 weight
                                                 (bevmsda_linear_f32), 13 = first kernel over the packed weight
                                                 image, 131 = software-pipelined kernel (packed weight, no
                                                 addends; BEVMSDA_ERR_UNSUPPORTED when it does not cover the call) */
  int32_t group_cols;                         /* 0, or a multiple of 128 dividing N: output column n
                                                 is written to matrix n / group_cols of
                                                 N / group_cols consecutive (M, ldy) matrices at y,
                                                 column n % group_cols — several Linear layers that
                                                 share their input (the value projections of all
                                                 encoder layers) in one pass over that input */
  int32_t out_bf16;                           /* 1: y is a bf16 matrix (the fp32 result rounded to
                                                 nearest even; ldy / group layout in elements) — the
                                                 projected value of the bf16-storage sampling path;
                                                 float4-epilogue variants only, N and ldy % 4 == 0 */
  int32_t reserved[4];                        /* [0] = 1: y += result instead of y = result (fp32 y, N and ldy multiples of
                                                 4, 16-byte aligned y / bias; bevmsda_linear_f32 / _packed_f32 only): the
                                                 input gradients of several projections of one tensor summed in place;
                                                 [1] = 1: the default never picks the software-pipelined kernel;
                                                 [2]: panel shape of bevmsda_linear_panel_f32 */
} bevmsda_linear_desc;

int bevmsda_linear_f32(const float *x0, const float *a0, const float *x1, const float *a1,
                       const float *w, const float *bias, const bevmsda_linear_desc *desc,
                       float *y, void *stream);

/* The same projection with the weight pre-split once per weight version (inference: the
 * weights are constants): bevmsda_linear_pack_weight_f32 writes, for every 128-row tile and
 * 32-deep K chunk of w (N, K), the [hi | lo] bf16 planes in the padded row format the kernel
 * keeps in LDS, bevmsda_linear_packed_bytes(N, K) bytes in all (0 when K % 32 != 0); the kernel
 * then copies 20 KB chunks instead of loading and splitting fp32 weights in every block.
 * Caller-owned blob, 16-byte aligned.  desc->ldw is ignored. */
int64_t bevmsda_linear_packed_bytes(int N, int K);
int bevmsda_linear_pack_weight_f32(const float *w, int64_t ldw, int N, int K, uint16_t *blob,
                                   void *stream);
/* The same image of the (N, K) weight whose TRANSPOSE is what lies in memory: wt (K, ldwt), element (n, k) = wt[k * ldwt + n].
 * The input gradient of a Linear layer, g W, is the projection of g by W^T: its weight image is packed straight from the
 * layer's own weight — no contiguous transpose per training step.  wt 4-byte aligned, ldwt >= N. */
int bevmsda_linear_pack_weight_t_f32(const float *wt, int64_t ldwt, int N, int K, uint16_t *blob, void *stream);
int bevmsda_linear_packed_f32(const float *x0, const float *a0, const float *x1, const float *a1,
                              const uint16_t *wpack, const float *bias,
                              const bevmsda_linear_desc *desc, float *y, void *stream);
/* Input gradient of a Linear that sits behind a ReLU, with the ReLU's backward in the epilogue:
 *     y[m, n] = act[m, n] > 0 ? sum_k g[m, k] * w[n, k] : 0
 * g (M, desc->ldx0) = the gradient w.r.t. the Linear's output (desc->K0 columns), wpack = the packed image of the
 * TRANSPOSED weight (N = the Linear's in_features rows, K0 = out_features columns), act (M, ld_act) = the ReLU's output
 * saved by the forward (mmcv FFN: Linear -> ReLU -> Linear, custom_base_transformer_layer.py:157-158).  fp32 y with N,
 * ldy, ld_act multiples of 4 and 16-byte aligned pointers; no bias, no second source. */
int bevmsda_linear_relu_backward_packed_f32(const float *g, const uint16_t *wpack, const float *act, int64_t ld_act,
                                            float scale, const bevmsda_linear_desc *desc, float *y, void *stream);
/* scale: multiplies the passed elements (1 / (1 - p) when a Dropout sat between the ReLU and the Linear and `act` is
 * the activation AFTER that dropout: zero where dropped or not positive); 1 otherwise. */

/* The packed projection with bevmsda_gather_mean_f32 folded into its A-load:
 *     A[m, :] = scale[m] * sum_{j < 2, idx[m, j] >= 0} rows[idx[m, j], :]      (idx: (M, 2) int32)
 * — SpatialCrossAttention's per-camera scatter-add, camera-count division and output_proj
 * (spatial_cross_attention.py:165-173) in one kernel; same arithmetic as the two-step path
 * (bit-identical result).  desc->K1 must be 0, desc->ldx0 is replaced by ld_rows. */
int bevmsda_linear_gather_packed_f32(const float *rows, int64_t ld_rows, const int32_t *idx,
                                     const float *scale, const uint16_t *wpack, const float *bias,
                                     const bevmsda_linear_desc *desc, float *y, void *stream);

/* Per-frame geometry of the encoder on the device (csrc/frame_plan.h): camera projection of the
 * pillar anchors + visibility (BEVFormerEncoder.point_sampling, encoder.py:88-149), the visible
 * (camera, query) pairs of SpatialCrossAttention as a ragged row list (spatial_cross_attention.py:
 * 136-153, without its per-camera nonzero() host syncs) and 1 / max(#cameras seeing a query, 1)
 * (ibid. :169-172).  Three small launches, no host synchronisation; the row count stays on the device.
 *
 *   lidar2img (B, Nc, 4, 4) fp32;  ref_3d (B, D, Q, 3) normalised anchors (encoder.py:62-71);
 *   order (Q,) int32: position -> BEV query, the row order inside a camera
 * outputs (caller-owned, all DEVICE memory):
 *   ref_cam (Nc, B, Q, D, 2), bev_mask (Nc, B, Q, D) bytes 0/1, inv_count (B, Q),
 *   slot (Nc, Q) scratch bytes, block_scratch (bevmsda_frame_plan_scratch(Nc, Q) int32), row_query / row_batch (row_capacity,) int32 (tile-local slot
 *   j*Qt + q - q_lo with Qt = q_hi - q_lo; value batch entry j*Nc + cam), row_ref (row_capacity, D, 2),
 *   q_rows (B*Qt, Nc) / q_rows2 (B*Qt, 2) int32 rows of every slot (-1 = none),
 *   counters (bevmsda_frame_plan_counters(B, Nc) int32): [0] rows, [1] rows dropped because
 *   row_capacity was too small, [2] slots seen by more than two cameras, [3] rows of one batch
 *   element, [4 ...] first row of every (j, cam) run (+ the end).
 * As in the reference the visible set of a camera is taken from batch element 0.  Only queries in
 * [q_lo, q_hi) produce rows (BEV tiling over GPUs); ref_cam / bev_mask / inv_count cover all. */
typedef struct bevmsda_plan_desc {
  int32_t B, Nc, Q, D;
  double pc_range[6];
  float img_w, img_h;
  int32_t q_lo, q_hi;
  int32_t row_capacity;
  int32_t reserved[5];
} bevmsda_plan_desc;

int64_t bevmsda_frame_plan_counters(int B, int Nc);
int64_t bevmsda_frame_plan_scratch(int Nc, int Q);
int bevmsda_frame_plan_f32(const float *lidar2img, const float *ref_3d, const int32_t *order,
                           const bevmsda_plan_desc *desc, float *ref_cam, uint8_t *bev_mask,
                           float *inv_count, uint8_t *slot, int32_t *block_scratch,
                           int32_t *row_query, int32_t *row_batch,
                           float *row_ref, int32_t *q_rows, int32_t *q_rows2, int32_t *counters,
                           void *stream);
/* rows[q_rows[s, 0]] += sum_{j >= 2} rows[q_rows[s, j]] for slots seen by more than two cameras, so
 * that the two-row gather of bevmsda_linear_gather_packed_f32 sums over all of them; n_extra
 * (DEVICE, counters[2] above) = 0 makes the launch a no-op. */
int bevmsda_fold_extra_rows_f32(float *rows, int64_t ld_rows, const int32_t *q_rows, int64_t slots, int J,
                                int C, const int32_t *n_extra, void *stream);

/* Residual add + LayerNorm that follow a projection (`output_proj` / the FFN's second Linear, "+ identity" and
 * `norms[i]` of an encoder layer: temporal_self_attention.py:267-272, spatial_cross_attention.py:173-175,
 * encoder.py:376-404), as the epilogue descriptor of bevmsda_linear_panel_f32:
 *     y = LayerNorm(A w^T + bias + res) * gamma + beta         over the N = 256 columns of every row
 * torch.nn.LayerNorm semantics (biased variance, eps inside the square root). */
typedef struct bevmsda_layernorm_desc {
  const float *res;      /* (M, ldres) or NULL */
  int64_t ldres;
  const float *gamma;    /* (N) */
  const float *beta;     /* (N) */
  float eps;
  int32_t reserved[3];
} bevmsda_layernorm_desc;

/* Row-panel form of the projections (csrc/linear_panel.h): the same contract and arithmetic as
 * bevmsda_linear_packed_f32 / _gather_packed_f32 / _layernorm_packed_f32 behind one entry point, for the
 * layer shapes K0 + K1 in {256, 512} (K0 in {256, 512}, K1 in {0, 256}).  A workgroup fetches a panel of 64 or
 * 128 complete rows once (LDS-DMA), splits it once, and its wavefronts sweep the N columns without further
 * synchronisation, weight fragments coming straight from L2 in MFMA operand order.  The weight image is its own
 * format: bevmsda_linear_panel_pack_weight_f32 writes bevmsda_linear_panel_packed_bytes(N, K) bytes (0 when
 * K % 256 != 0).  idx / scale: optional two-row gather (then a0 / x1 must be NULL); ln: optional residual +
 * LayerNorm epilogue (N = 256).  desc->reserved[2]: 0 = panel shape by problem shape, 1 = 64-row panels (4
 * wavefronts, 64 x 64 tiles, two workgroups per CU), 2 = 128-row panels (8 wavefronts, 128 x 32 tiles), 3 = role-split
 * 64-row panels (csrc/linear_roles.h: 8 MFMA wavefronts of 64 x 32 tiles that hand finished tiles to 4 store wavefronts
 * through LDS; bit-identical to shapes 1 and 2) for the plain forms — one source, two row blocks (_rows2_f32) or row
 * segments (_segments_f32), K = 256, N % 32 == 0, fp32 or bf16 out, grouped or not; any other form takes the shape rule.
 * Shape 0 picks 3 for those forms from 65,536 rows and 1,024 columns on (the hoisted value projections).
 * K = 512 and ln need N <= 256; N % 4 == 0, group_cols % 64 == 0, all pointers 16-byte aligned, row strides
 * multiples of 4; anything else returns BEVMSDA_ERR_UNSUPPORTED / _MISALIGNED and the caller uses the entry
 * points above.  The k order inside an MFMA differs from the first kernel's: results agree to fp32 summation
 * order, not bit for bit.  The epilogue addresses one ROW PANEL (<= 128 rows x ldy) of an output group through a 32-bit
 * raw buffer with a 64-bit base: 128 * ldy * element size must stay below 2 GiB (BEVMSDA_ERR_TOO_LARGE otherwise).
 * desc->reserved[3] must be 0 for shapes 1 and 2 (BEVMSDA_ERR_BAD_OPTION otherwise; since ABI version 5 — the prefetch-depth,
 * epilogue, phase-skew and one-wavefront-per-SIMD knobs of earlier versions are retired).  With shape 3 it is a BENCHMARK knob
 * (0 in production): 1 = MFMA wavefronts at the store wavefronts' priority, 2 = non-temporal output stores, 3 = both,
 * 4 = neither (default-policy stores at the raised priority). */
int64_t bevmsda_linear_panel_packed_bytes(int N, int K);
int bevmsda_linear_panel_pack_weight_f32(const float *w, int64_t ldw, int N, int K, uint16_t *blob, void *stream);
/* ... of the (N, K) weight whose transpose lies in memory: wt (K, ldwt), element (n, k) = wt[k * ldwt + n] (backward GEMMs). */
int bevmsda_linear_panel_pack_weight_t_f32(const float *wt, int64_t ldwt, int N, int K, uint16_t *blob, void *stream);
/* Many weight images in ONE launch (round 6; the reference re-reads its nn.Linear weights on every call, e.g.
 * temporal_self_attention.py:197-211 — the images are this library's derived copies and a training step rebuilds all of
 * them from the weights' current values: 52 launches at bevformer_base, one with this entry).  `jobs`: DEVICE array, kept
 * alive and unchanged by the caller while a launch that reads it can run (graph replays included); kind bit 0 = the
 * source is the memory of the transpose (w[k * ldw + n]), bit 1 = row-panel image (bevmsda_linear_panel_pack_weight*),
 * else the first kernel's (bevmsda_linear_pack_weight*); first_block = sum of the block counts
 * (bevmsda_linear_pack_job_blocks) of the jobs before; `blocks` = the total.  Per-job shape / alignment rules are those
 * of the single-image entry points and are the caller's to check. */
typedef struct bevmsda_pack_job {
  const float *w;
  int64_t ldw;
  uint16_t *blob;
  int32_t N, K;
  int32_t kind;
  int32_t first_block;
} bevmsda_pack_job;
int64_t bevmsda_linear_pack_job_blocks(int N, int K, int kind);
int bevmsda_linear_pack_weights_multi_f32(const bevmsda_pack_job *jobs, int njobs, int64_t blocks, void *stream);

int bevmsda_linear_panel_f32(const float *x0, const float *a0, const float *x1, const float *a1, const int32_t *idx,
                             const float *scale, const uint16_t *wpanel, const float *bias,
                             const bevmsda_linear_desc *desc, const bevmsda_layernorm_desc *ln, float *y,
                             void *stream);

/* bevmsda_linear_panel_f32 whose A has TWO ROW BLOCKS in two tensors: rows [0, m_split) = x_lo, rows [m_split, desc->M) =
 * x_hi (row m - m_split; both with row stride desc->ldx0; K1 = 0, no addends / gather / LayerNorm).  The value tensor of
 * TemporalSelfAttention is torch.stack([prev_bev, bev_query]) (encoder.py:216-222 of the reference): its projection reads the
 * history BEV and the current queries where they lie instead of from a stacked copy (82 MB written and read per frame). */
int bevmsda_linear_panel_rows2_f32(const float *x_lo, const float *x_hi, int64_t m_split, const uint16_t *wpanel, const float *bias,
                                   const bevmsda_linear_desc *desc, float *y, void *stream);

/* bevmsda_linear_panel_rows2_f32 over a NEEDED-PANEL TABLE (BEV tiling with a halo: a rank's queries sample the history /
 * current BEV only near their own tile).  need (need_len int32, DEVICE memory, read when the kernel runs): entry e says
 * whether rows [e * need_rows, (e + 1) * need_rows) of EACH of the two row blocks (block-local row numbers) will be read;
 * need_len * need_rows covers the longer block.  A workgroup none of whose rows lies in a needed entry returns at once and
 * leaves its output rows unwritten; every row of a needed entry is computed, with the arithmetic of the unmasked launch
 * (bit-identical results).  Rows that share a workgroup's panel with a needed row are computed as well.  The table is the
 * caller's to widen by whatever its consumer touches beyond the needed rows (the sampling kernels' zero-coefficient taps:
 * max W + 1 rows).  K = 256, desc->reserved[3] = 0, no ReLU; anything else: BEVMSDA_ERR_UNSUPPORTED (run the unmasked launch).
 * No host synchronisation, graph-capturable. */
int bevmsda_linear_panel_rows2_masked_f32(const float *x_lo, const float *x_hi, int64_t m_split, const uint16_t *wpanel,
                                          const float *bias, const bevmsda_linear_desc *desc, const int32_t *need,
                                          int64_t need_rows, int64_t need_len, float *y, void *stream);

/* bevmsda_linear_panel_f32 over ROW SEGMENTS of which only some are needed (BEV tiling over GPUs, SURVEY.md §8e: the
 * camera-feature value projection is a replicated input, but a rank's queries see only some of the cameras): the rows
 * form ceil(M / seg_len) segments of seg_len rows (one per (batch entry, camera)); seg_start (segments + 1, int32, DEVICE
 * memory — the camera starts of bevmsda_frame_plan_f32's counters, read when the kernel runs) tells how many ragged
 * rows sample each segment.  The sampling kernels also ISSUE the taps whose bilinear coefficient is 0 (up to one image
 * row + 1 pixel before / after a level: rows of the neighbouring segment), and 0 x NaN is NaN, so the rows within
 * halo = max_l W_l + 1 of a used segment are computed too (level_shapes: (num_levels, 2) int64 [H, W], DEVICE memory,
 * the operator's spatial_shapes; NULL / 0 levels = no halo).  A workgroup all of whose rows (+- halo) lie in unused
 * segments returns at once and its output rows stay unwritten: nothing reads them.  No host synchronisation,
 * graph-capturable.  Single source, no addend. */
int bevmsda_linear_panel_segments_f32(const float *x0, const uint16_t *wpanel, const float *bias,
                                      const bevmsda_linear_desc *desc, const int32_t *seg_start, int64_t seg_len,
                                      const int64_t *level_shapes, int num_levels, float *y, void *stream);

/* The row-local tail of an encoder layer in one kernel (csrc/linear_chain.h):
 *     x = LayerNorm0(A w0^T + b0 + res)                          attention output projection, "+ identity", norm
 *     y = LayerNorm1(x + relu(x w1^T + b1) w2^T + b2)            FFN (C -> F -> C), "+ identity", norm
 * = SpatialCrossAttention's `output_proj` + residual (spatial_cross_attention.py:165-175; with idx / scale the
 * per-camera scatter-add and camera-count division as a two-row gather: A[m] = scale[m] * (rows[idx[m, 0]] +
 * rows[idx[m, 1]]), -1 = absent), `norms[1]`, the FFN and `norms[2]` of BEVFormerLayer's operation order
 * (encoder.py:376-404).  A workgroup owns 64 complete rows; x and the hidden layer never leave the chip.
 * w0p / w1p / w2p: bevmsda_linear_panel_pack_weight_f32 images of (C, C), (F, C), (C, F).  Supported: C = 256,
 * F = 512; row strides multiples of 4, every pointer 16-byte aligned; else BEVMSDA_ERR_UNSUPPORTED / _MISALIGNED and
 * the caller runs the three launches (bevmsda_linear_panel_f32 x 2 with LayerNorm descriptors + the first Linear).
 * Arithmetic as bevmsda_linear_panel_f32 (precision 0: three bf16 MFMAs per fp32 product; x and the hidden
 * activations are re-split from their fp32 values exactly as a separate launch would split them: same results as the
 * three-launch sequence to fp32 summation order). */
typedef struct bevmsda_chain_desc {
  int64_t M;                     /* rows of y */
  int64_t ld_rows, ld_res, ld_y; /* row strides in floats */
  int32_t C, F;                  /* embedding and hidden width */
  int32_t precision;             /* as bevmsda_linear_desc */
  float eps0, eps1;
  int32_t reserved[5];           /* [0]: bevmsda_proj_ln_proj_chain_f32: row stride of proj_out in floats; [1]: workgroup
                                    shape, 0 = default (by row count: 2, or 1 between 8,192 and 16,384 rows), 1 = 64-row panels (one workgroup per
                                    CU), 2 = 32-row panels (two), 3 = mixed: whole rounds of 256 x 64 rows on shape 1, the
                                    remaining rows on shape 2 (a second launch); [2]: bevmsda_proj_ffn_chain_f32 / _tail_f32: columns J of idx (0 = 2;
                                    2 < J <= 64: idx is (M, J), present rows first, and rows idx[m, 2..] >= 0 are added to
                                    row idx[m, 0]'s values, in column order, before the two-row sum — what
                                    bevmsda_fold_extra_rows_f32 does in a launch of its own) */
} bevmsda_chain_desc;

int bevmsda_proj_ffn_chain_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                               const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                               const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                               const bevmsda_chain_desc *desc, float *y, void *stream);

/* The same launch with the seam to the NEXT layer behind it (csrc/linear_chain.h TP): besides y the workgroup forms
 *     proj_out = [first | y + pos] w3^T + b3          (n3 columns, K = 512)
 * = the next BEVFormerLayer's TemporalSelfAttention `sampling_offsets` / `attention_weights` projection of
 * `cat([value[:bs], query + query_pos], -1)` (temporal_self_attention.py:197-211) with query = y, the rows this launch has
 * just produced: `first` (M, ld_first) = the history BEV's rows, `pos` (M, ld_pos) = the positional encoding or NULL,
 * w3p = the bevmsda_linear_panel_pack_weight_f32 image of the merged (n3, 512) weight, b3 (n3) or NULL.  Replaces one
 * bevmsda_linear_f32 two-source launch per layer (y is not re-read).  Supported: n3 a multiple of 64, <= 256; else
 * BEVMSDA_ERR_UNSUPPORTED and the caller runs the two launches.  Same arithmetic as that launch (split operands, fp32
 * accumulation); results agree to fp32 summation order. */
int bevmsda_proj_ffn_chain_tail_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                    const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                    const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                                    const bevmsda_chain_desc *desc, float *y, const float *first, int64_t ld_first,
                                    const float *pos, int64_t ld_pos, const uint16_t *w3p, const float *b3, int n3,
                                    float *proj_out, int64_t ld_proj, void *stream);

/* The same launch as the FORWARD of the autograd path: besides y it stores what the backward of the chain needs and the
 * inference launch keeps on chip — save_z0 (M, 256) = A w0^T + b0 + res (the input of LayerNorm0), save_x (M, 256) =
 * LayerNorm0(...), save_h (M, 512) = relu(x w1^T + b1), save_z1 (M, 256) = x + h w2^T + b2 (the input of LayerNorm1);
 * dense matrices, 16-byte aligned.  Same arithmetic, same y. */
int bevmsda_proj_ffn_chain_train_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                     const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p,
                                     const float *b1, const uint16_t *w2p, const float *b2, const float *gamma1,
                                     const float *beta1, const bevmsda_chain_desc *desc, float *y, float *save_z0,
                                     float *save_x, float *save_h, float *save_z1, const float *drop0, const float *droph,
                                     const float *drop1, void *stream);

/* The BACKWARD of that launch in one kernel (linear_chain.h MODE 2; the rows are complete in a workgroup, so both LayerNorm
 * backwards are row-local like the forward's LayerNorms): from grad_y (M, ld_grad_y) and the saved save_z0 / save_h / save_z1
 *     grad_z1 = LayerNorm1'(save_z1; grad_y)                     grad_gamma_beta1 (2, 256) += [sum g xhat | sum g]
 *     grad_h  = (grad_z1 w2) where save_h > 0                     (M, 512)
 *     grad_z0 = LayerNorm0'(save_z0; grad_h w1 + grad_z1)         grad_gamma_beta0 (2, 256) += ...      (= the residual's gradient)
 *     grad_in = grad_z0 w0                                        (M, 256): the gradient of the seam's (gathered) input rows
 * i.e. encoder.py:376-404 / the mmcv FFN / spatial_cross_attention.py:173-175 differentiated.  w0t_p / w1t_p / w2t_p: the
 * row-panel weight images (bevmsda_linear_panel_pack_weight_f32) of w0^T (256 x 256), w1^T (256 x 512), w2^T (512 x 256).
 * grad_z1 / grad_h / grad_z0 are outputs because the weight gradients read them (bevmsda_linear_wgrad_multi_f32).  The
 * caller zeroes grad_gamma_beta*.  train() mode (the forward ran with drop0 / droph / drop1): drop1 (M, 256) scales grad_z1 on
 * its way into the FFN (grad_z1 then holds the scaled gradient; x still receives the unscaled one), hidden_scale = 1 / (1 - p)
 * of the hidden dropout (save_h is zero where it dropped), drop0 (M, 256) scales grad_z0 on its way into the projection:
 * grad_zp (M, 256) = grad_z0 * drop0 is stored and grad_in = grad_zp w0.  NULL / 1.0 / NULL: no dropout. */
int bevmsda_proj_ffn_chain_backward_f32(const float *grad_y, int64_t ld_grad_y, const float *save_z0, const float *save_h,
                                        const float *save_z1, const float *gamma0, const float *gamma1, const uint16_t *w0t_p,
                                        const uint16_t *w1t_p, const uint16_t *w2t_p, const bevmsda_chain_desc *desc,
                                        float *grad_z1, float *grad_h, float *grad_z0, float *grad_in, float *grad_gamma_beta1,
                                        float *grad_gamma_beta0, const float *drop0, const float *drop1, float hidden_scale,
                                        float *grad_zp, void *stream);

/* The backward of bevmsda_proj_ln_proj_chain_train_f32 in one kernel (linear_chain.h MODE 3):
 *     grad_z0 = LayerNorm0'(save_z0; grad_proj w1 + grad_x)     grad_gamma_beta0 (2, 256) += [sum g xhat | sum g]
 *     grad_in = grad_z0 w0
 * grad_proj (M, ld_grad_proj) with desc->reserved[0] = N2 columns (a multiple of 256, <= 768: N2 / 256 panel passes), grad_x
 * (M, 256) or NULL: the gradient x received directly (it is the next attention's residual).  w0t_p / w1t_p: row-panel images
 * of w0^T (256 x 256) and w1^T (256 x N2).  temporal_self_attention.py:267-272 + the projections of
 * spatial_cross_attention.py:338-348 differentiated.  drop0 / grad_zp: as above (the attention's dropout of train() mode). */
int bevmsda_proj_ln_proj_chain_backward_f32(const float *grad_proj, int64_t ld_grad_proj, const float *grad_x, const float *save_z0,
                                            const float *gamma0, const uint16_t *w0t_p, const uint16_t *w1t_p,
                                            const bevmsda_chain_desc *desc, float *grad_z0, float *grad_in,
                                            float *grad_gamma_beta0, const float *drop0, float *grad_zp, void *stream);
/* drop0 (M, 256), droph (M, 512), drop1 (M, 256): dropout scale tensors (0 or 1 / (1 - p); NULL = inactive) of the three
 * nn.Dropout sites of the chain in train() mode — on the attention's projected output before "+ identity"
 * (spatial_cross_attention.py:175), on the FFN's hidden activations and on its output (mmcv FFN); save_h then holds the
 * hidden rows AFTER their dropout.  Gather form (idx) only when any is given. */

/* The attention-to-attention seam of a layer with the same machinery:
 *     x = LayerNorm0(A w0^T + b0 + res)        TemporalSelfAttention's output projection, "+ identity", norms[0]
 *     p = x w1^T + b1                           the next attention's projection of the same rows — SpatialCrossAttention's
 *                                               merged [sampling_offsets ; attention_weights] Linear (desc->F columns)
 * (temporal_self_attention.py:267-272, encoder.py:376-378, spatial_cross_attention.py:338-348).  x_out (M, ld_y) is stored
 * (it is the next attention's residual), p goes to proj_out (M, desc->reserved[0]); x is projected from its on-chip copy.
 * desc->F: a multiple of 32, at most 768; w1p: the panel image of (F, C).  Other requirements as above. */
int bevmsda_proj_ln_proj_chain_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                   const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                   const bevmsda_chain_desc *desc, float *x_out, float *proj_out, void *stream);

/* ... and as the forward of the autograd path (plain rows, no gather): save_z0 (M, 256) = the input of LayerNorm0. */
int bevmsda_proj_ln_proj_chain_train_f32(const float *rows, const uint16_t *w0p, const float *b0, const float *res,
                                         const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                         const bevmsda_chain_desc *desc, float *x_out, float *proj_out, float *save_z0,
                                         const float *drop0, void *stream);      /* drop0: as above (temporal_self_attention.py:272) */

/* Weight / bias gradient of a Linear layer (csrc/wgrad_mfma.h), the TN form of the projection:
 *     grad_w[n, k] += sum_m g[m, n] * x[m, k]          grad_b[n] += sum_m g[m, n]      (grad_b may be NULL)
 * g (M, ldg) = gradient w.r.t. the layer's output (N columns), x (M, ldx) = the layer's input (K columns).
 * ACCUMULATES (fp32 atomics over row slices): the caller zeroes grad_w / grad_b.  precision as for
 * bevmsda_linear_f32 (0: three bf16 MFMAs per product over split operands, 1: operands rounded to bf16).
 * N, K, ldg, ldx multiples of 4, g / x 16-byte aligned; otherwise BEVMSDA_ERR_UNSUPPORTED / _MISALIGNED. */
int bevmsda_linear_wgrad_f32(const float *g, int64_t ldg, const float *x, int64_t ldx, int64_t M, int N, int K,
                             float *grad_w, int64_t ldgw, float *grad_b, int precision, void *stream);

/* Several weight gradients over the SAME M rows in one launch (the backward of a layer seam needs two or three at
 * once): tiles of all problems share one round of workgroups — longer row slices, the epilogue atomics paid once
 * instead of once per Linear.  Up to 8 problems; each as bevmsda_linear_wgrad_f32 (accumulating; grad_b may be NULL). */
typedef struct bevmsda_wgrad_problem {
  const float *g;       /* (M, ldg): gradient w.r.t. the Linear's output, N columns */
  int64_t ldg;
  const float *x;       /* (M, ldx): the Linear's input, K columns */
  int64_t ldx;
  int32_t N, K;
  float *grad_w;        /* (N, ldgw), accumulated into */
  int64_t ldgw;
  float *grad_b;        /* (N) or NULL */
} bevmsda_wgrad_problem;
int bevmsda_linear_wgrad_multi_f32(const bevmsda_wgrad_problem *probs, int nprob, int64_t M, int precision, int workgroups,
                                   int variant, void *stream);
/* workgroups: 0 = the library's choice (benchmark sweeps: a target count); variant: 0 = operands split once to bf16 planes
 * in LDS, fragments by the transposing LDS read (csrc/wgrad_tr.h), 1 = the first kernel's gathered fragments. */

/* The encoder's caller, PerceptionTransformer.get_bev_features (modules/transformer.py:104-200).
 *
 * bevmsda_rotate_bev_f32: dst = rotate(src) of an (H, W) grid of C-float rows (row p at
 * ptr + p * ld) with nearest sampling and zero fill: torchvision.transforms.functional.rotate
 * as called on prev_bev at transformer.py:146-156.  theta = the 2 x 3 inverse affine matrix in
 * torchvision's normalised form (row 0 divided by W/2, row 1 by H/2: `rescaled_theta` of
 * _gen_affine_grid), computed by the caller from (angle, center).  C = 256 or 512; src != dst.
 *
 * bevmsda_flatten_feats_f32: one feature level feat (bs, Nc, C, hw) -> rows [s0, s0 + hw) of
 * out (Nc, S, bs, C), adding cams_embeds[cam] (Nc, C; may be NULL) and then level_embed (C; may
 * be NULL) — transformer.py:165-184.  C a multiple of 64. */
int bevmsda_rotate_bev_f32(const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int H, int W,
                           int C, const float *theta, void *stream);

/* The same with the six matrix values in DEVICE memory (`theta_dev`, fp32, read when the kernel runs): a captured
 * launch follows the ego pose of every replayed frame (detectors/bevformer.py:253-261 feeding transformer.py:146-156). */
int bevmsda_rotate_bev_dev_f32(const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int H, int W, int C,
                               const float *theta_dev, void *stream);
int bevmsda_flatten_feats_f32(const float *feat, const float *cams_embeds, const float *level_embed,
                              float *out, int bs, int Nc, int C, int hw, int S, int s0, void *stream);

/* bevmsda_flatten_feats_f32 for a level that is already channel-last (entry point ADDED to ABI version 7): rows
 * (bs * Nc * hw, C), row ((b * Nc + cam) * hw + p) at rows + row * ld_rows, -> rows [s0, s0 + hw) of out (Nc, S, bs, C) with
 * the same two adds in the same order, so both entry points write the same bits.  C a multiple of 4; ld_rows >= C and a
 * multiple of 4; pointers on 16 bytes. */
int bevmsda_flatten_rows_f32(const float *rows, int64_t ld_rows, const float *cams_embeds, const float *level_embed,
                             float *out, int bs, int Nc, int C, int hw, int S, int s0, void *stream);

/* The detection decoder's self-attention core (nn.MultiheadAttention between its input and output projections, reached
 * from the `self_attn` of the decoder layers, decoder.py:53-129 via mmcv's MultiheadAttention): per batch b and head h,
 *     out[t, b, 32 h .. 32 h + 32) = softmax_s(q[t, b, h] . k[s, b, h] * scale) v[s, b, h]
 * over all nk keys: no attention mask, no key-padding mask, no dropout.  q / k / v / out are matrices of fp32 rows in the
 * decoder's (sequence, batch) order — row t * bs + b at ptr + (t * bs + b) * ld, head h in columns [32 h, 32 h + 32) — so
 * q and k may be column blocks of one merged projection output (ld = its width).  Writes nq * bs rows of heads * 32
 * columns.  Both products are exact-fp32 MFMA whatever the GEMM mode of the caller (csrc/mha_d32.h).
 * D = 32 only, every ld a multiple of 4: else BEVMSDA_ERR_UNSUPPORTED and the caller runs its own attention; nq, bs or
 * heads = 0 is a no-op, nk = 0 with queries present BEVMSDA_ERR_BAD_SHAPE, ld < heads * 32 BEVMSDA_ERR_BAD_SHAPE,
 * heads or bs > 65535 BEVMSDA_ERR_TOO_LARGE. */
int bevmsda_mha_d32_f32(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, int nq, int nk,
                        int bs, int heads, int D, float scale, float *out, int64_t ldo, void *stream);

/* ---- Detection head (since ABI version 6; csrc/head_branch.h, csrc/head_decode.h).
 *
 * The branches of BEVFormerHead for every decoder layer in ONE launch (dense_heads/bevformer_head.py:118-213):
 *     reg   t = W3 relu(W2 relu(W1 x + b1) + b2) + b3                    256 -> 256 -> 256 -> code_size (8 or 10)
 *     cls   s = V3 relu(LN(V2 relu(LN(V1 x + c1)) + c2)) + c3            256 -> 256 -> 256 -> cls_out (1 .. 32)
 * x: rows in the decoder's order — layer l, query q, batch b at x + l * ld_layer + (q * bs + b) * ld_x, 256 fp32 each.
 * ref (L, bs, nq, 3): the reference point each layer CONSUMED.  A branch's weights are fragment-order images
 * (bevmsda_linear_panel_pack_weight_f32; the last one of the (code_size | cls_out, 256) matrix), biases and LayerNorm
 * parameters fp32 vectors.  `reg` / `cls`: HOST arrays of L entries (layer_stride 1), or of one entry shared by all
 * layers (layer_stride 0); they are copied into the launch.
 * BEVMSDA_HEAD_MODE_HEAD: out_box (L, bs, nq, code_size) with columns 0, 1, 4 = sigmoid(t + inverse_sigmoid(ref)) scaled
 * to pc_range (x, y, z), the others raw; out_cls (L, bs, nq, cls_out).
 * BEVMSDA_HEAD_MODE_REFINE (the decoder's refinement, modules/decoder.py:68-74; L = 1, reg only, cls / out_cls unused):
 * out_box (bs, nq, 3) = sigmoid(t[{0, 1, 4}] + inverse_sigmoid(ref)).
 * precision: 0 = split operands (three bf16 products), 1 = bf16.  Checked before any launch: unknown mode, precision or
 * layer_stride BEVMSDA_ERR_BAD_OPTION; negative dims, L > BEVMSDA_HEAD_MAX_LAYERS, code_size not 8 / 10, cls_out outside
 * 1 .. 32, ld_x < 256 BEVMSDA_ERR_BAD_SHAPE; row strides not multiples of 4 floats or x / images / vectors not 16-byte
 * aligned BEVMSDA_ERR_MISALIGNED; nq * bs > 2^24 rows BEVMSDA_ERR_TOO_LARGE; L, nq or bs = 0 is a no-op. */
#define BEVMSDA_HEAD_MAX_LAYERS 8
#define BEVMSDA_HEAD_MODE_HEAD 0
#define BEVMSDA_HEAD_MODE_REFINE 1
typedef struct bevmsda_head_branch {
  const uint16_t *w1, *w2, *w3;
  const float *b1, *b2, *b3;
  const float *gamma1, *beta1, *gamma2, *beta2; /* cls only */
  float eps1, eps2;                             /* cls only */
} bevmsda_head_branch;

typedef struct bevmsda_head_desc {
  int64_t ld_x, ld_layer;
  int32_t mode, L, nq, bs, code_size, cls_out, precision, layer_stride;
  double pc_range[6];
  int32_t reserved[4];
} bevmsda_head_desc;

int bevmsda_head_branches_f32(const float *x, const float *ref, const bevmsda_head_branch *reg, const bevmsda_head_branch *cls,
                              const bevmsda_head_desc *desc, float *out_box, float *out_cls, void *stream);

/* NMSFreeCoder.decode_single + denormalize_bbox for every batch entry (core/bbox/coders/nms_free_coder.py:40-100,
 * core/bbox/util.py:26-53), fixed-shape: cls (bs, nq, num_classes) logits and box (bs, nq, code_size) codes of the last
 * layer -> for rank r < max_num of the logits (descending, ties by the lower flat index q * num_classes + c):
 * scores (bs, max_num) = sigmoid(logit); labels (bs, max_num) int64; boxes (bs, max_num, code_size - 1) = (cx, cy, cz,
 * exp(w), exp(l), exp(h), atan2(sin, cos)[, vx, vy]); keep (bs, max_num) bytes = centre inside post_center_range (ends
 * inclusive) and the score test; count (bs) int32 = kept ranks.  ladder[0 .. n_ladder): the reference's thresholds (thr,
 * 0.9 thr, ... while >= 0.01): the first rung any score passes ('>' for rung 0, '>=' after) is the test, none: every
 * score passes; n_ladder = 0: no score test.  Nothing is read back by the host.
 * nq * num_classes <= 16384, max_num <= 1024, n_ladder <= 64, bs <= 65535: else BEVMSDA_ERR_TOO_LARGE; max_num >
 * nq * num_classes, a negative dim, code_size not 8 / 10: BEVMSDA_ERR_BAD_SHAPE; bs = 0 is a no-op. */
typedef struct bevmsda_decode_desc {
  int32_t bs, nq, num_classes, code_size, max_num, n_ladder;
  float post_center_range[6];
  float ladder[64];
  int32_t reserved[4];
} bevmsda_decode_desc;

int bevmsda_nms_free_decode_f32(const float *cls, const float *box, const bevmsda_decode_desc *desc, float *scores,
                                int64_t *labels, float *boxes, uint8_t *keep, int32_t *count, void *stream);

/* ---- Detection loss (csrc/det_cost.h, csrc/match_lsap.h, csrc/det_loss.h).  Three entry points ADDED to ABI version 6:
 * nothing that existed changed, so the version number stays 6 (a library without them fails the binding's symbol check).
 *
 * BEVFormerHead.loss (dense_heads/bevformer_head.py:214-480) without a host round trip: the match costs of
 * HungarianAssigner3D for every decoder layer and sample, a batched assignment solver, and the focal + L1 loss with its
 * gradients.  Ground truth is packed: gt (bs, gmax, code_size - 1) fp32 boxes in gravity-centre form (cx, cy, cz, w, l, h,
 * rot[, vx, vy]), label (bs, gmax) int32, count (bs) int32 in DEVICE memory (read by the kernels, clamped to [0, gmax]).
 * No entry point allocates or needs a workspace: every buffer is the caller's.
 * Checked before any launch, for the two descriptor calls: NULL descriptor BEVMSDA_ERR_NULL_POINTER; a negative dim,
 * code_size not 8 / 10, cls_out outside 1 .. 32 BEVMSDA_ERR_BAD_SHAPE; nq > 2048, gmax > 512 or L * bs > 65535
 * BEVMSDA_ERR_TOO_LARGE; then an empty problem (L, bs or nq = 0; gmax = 0 for the costs) is a no-op; then a NULL pointer
 * BEVMSDA_ERR_NULL_POINTER and a pointer off 4 bytes BEVMSDA_ERR_MISALIGNED.
 *
 * bevmsda_match_cost_f32: cost[l, b, g, q] (L, bs, gmax, nq) = cost_cls_weight * FocalLossCost(cls[l, b, q, label[b, g]]) +
 * cost_reg_weight * sum_{c < 8} |box[l, b, q, c] - normalize_bbox(gt[b, g])[c]| for g < count[b]; padded rows are not
 * written.  Evaluated in fp64, rounded once.
 *
 * bevmsda_lsap_f32: P rectangular assignment problems (shortest augmenting paths), problem p = rows [0, count[p]) of the
 * (gmax, nq) fp32 matrix at cost + p * gmax * nq, count[p] clamped to [0, min(gmax, nq)].  match (P, gmax): the column of
 * each row, -1 on padding; assigned (P, nq): the row of each column, -1 for none; status (P): 0 solved, 1 a non-finite cost
 * (nothing assigned), 2 step bound exhausted (nothing assigned; unreachable on finite costs).  The total of the result is
 * minimal; among equal totals the choice is the kernel's (deterministic), not scipy's.  P, gmax or nq negative
 * BEVMSDA_ERR_BAD_SHAPE; nq > 2048 or gmax > 512 BEVMSDA_ERR_TOO_LARGE; P = 0 is a no-op.  With the costs above: P = L * bs
 * and count repeated per layer.
 *
 * bevmsda_det_loss_f32: assigned (L, bs, nq) as written by bevmsda_lsap_f32, code_weights (code_size) and factors (2: the
 * classification averaging factor and the positive count, each >= 1) fp32 in DEVICE memory -> losses (L, 2) =
 * (loss_cls_weight * sum focal / factors[0], loss_box_weight * sum L1 / factors[1]) with nan_to_num, and their gradients
 * grad_cls (L, bs, nq, cls_out), grad_box (L, bs, nq, code_size), every element written.  fp64 evaluation, one rounding, a
 * fixed summation order: bit-reproducible. */
typedef struct bevmsda_loss_desc {
  int32_t L, bs, nq, cls_out, code_size, gmax;
  double cost_cls_weight, cost_reg_weight, cost_alpha, cost_gamma, cost_eps; /* FocalLossCost, BBox3DL1Cost */
  double loss_alpha, loss_gamma, loss_cls_weight, loss_box_weight;           /* FocalLoss, L1Loss */
  int32_t reserved[4];
} bevmsda_loss_desc;

int bevmsda_match_cost_f32(const float *cls, const float *box, const float *gt, const int32_t *label, const int32_t *count,
                           const bevmsda_loss_desc *desc, float *cost, void *stream);
int bevmsda_lsap_f32(const float *cost, const int32_t *count, int P, int gmax, int nq, int32_t *match, int32_t *assigned,
                     int32_t *status, void *stream);
int bevmsda_det_loss_f32(const float *cls, const float *box, const float *gt, const int32_t *label, const int32_t *count,
                         const int32_t *assigned, const float *code_weights, const float *factors,
                         const bevmsda_loss_desc *desc, float *losses, float *grad_cls, float *grad_box, void *stream);

/* ---- Detection loss of Group-DETR (csrc/det_cost.h, csrc/det_loss.h).  Two entry points ADDED to ABI version 7: nothing
 * that existed changed, so the version number stays 7 (a library without them fails the binding's symbol check).
 *
 * BEVFormerHead_GroupDETR.loss (dense_heads/bevformer_head.py:603-683): the head's num_query is groups * nq, query
 * g * nq + q of a sample is query q of group g, every group is matched against the sample's gt on its own and a layer's
 * loss is the mean over the groups.  Predictions stay as the head produces them: cls (L, bs, groups * nq, cls_out), box
 * (L, bs, groups * nq, code_size); problem p = (l * bs + b) * groups + g.  gt, label and count are as above (count[b] is
 * every group's of sample b).  The assignment is bevmsda_lsap_f32's with P = L * bs * groups and count[(p / groups) % bs]
 * for problem p; its assigned (P, nq) is (L, bs, groups * nq) in the predictions' row order.
 * Checked before any launch, in this order: NULL descriptor BEVMSDA_ERR_NULL_POINTER; a negative dim, groups < 1, code_size
 * not 8 / 10, cls_out outside 1 .. 32 BEVMSDA_ERR_BAD_SHAPE; nq > 2048, gmax > 512 or L * bs * groups > 65535 (the grid
 * limit) BEVMSDA_ERR_TOO_LARGE; then an empty problem (L, bs or nq = 0; gmax = 0 for the costs) is a no-op; then a NULL
 * pointer BEVMSDA_ERR_NULL_POINTER and a pointer off 4 bytes BEVMSDA_ERR_MISALIGNED.
 *
 * bevmsda_match_cost_grouped_f32: cost (L, bs, groups, gmax, nq), gt-major inside a problem; the values are
 * bevmsda_match_cost_f32's on the group's rows (fp64, one rounding), padded gt rows are not written.
 *
 * bevmsda_det_loss_grouped_f32: assigned (L, bs, groups * nq), code_weights, factors (2: per group, the same for every
 * group) as above -> group_losses (L, groups, 2), each bevmsda_det_loss_f32's pair on the group's rows; losses (L, 2), the
 * mean over the groups of those fp32 values, added in fp64 in group order and rounded once; grad_cls, grad_box: the
 * gradients of losses[l, 0] / losses[l, 1], the 1 / groups in the fp64 factor before the one rounding, every element
 * written.  Two launches (one workgroup per layer and group, then the means), no atomics: bit-reproducible.  groups = 1
 * gives bevmsda_det_loss_f32's bits. */
typedef struct bevmsda_group_loss_desc {
  int32_t L, bs, groups, nq, cls_out, code_size, gmax; /* nq: the queries of ONE group */
  int32_t pad;
  double cost_cls_weight, cost_reg_weight, cost_alpha, cost_gamma, cost_eps; /* FocalLossCost, BBox3DL1Cost */
  double loss_alpha, loss_gamma, loss_cls_weight, loss_box_weight;           /* FocalLoss, L1Loss */
  int32_t reserved[4];
} bevmsda_group_loss_desc;

int bevmsda_match_cost_grouped_f32(const float *cls, const float *box, const float *gt, const int32_t *label,
                                   const int32_t *count, const bevmsda_group_loss_desc *desc, float *cost, void *stream);
int bevmsda_det_loss_grouped_f32(const float *cls, const float *box, const float *gt, const int32_t *label,
                                 const int32_t *count, const int32_t *assigned, const float *code_weights,
                                 const float *factors, const bevmsda_group_loss_desc *desc, float *group_losses, float *losses,
                                 float *grad_cls, float *grad_box, void *stream);

/* ---- Optimizer step (csrc/optim.h).  Four entry points ADDED to ABI version 6: nothing that existed changed, so the
 * version number stays 6 (a library without them fails the binding's symbol check).
 *
 * torch.nn.utils.clip_grad_norm_(norm_type = 2) followed by torch.optim.AdamW's single-tensor update
 * (torch/optim/adamw.py: no amsgrad, no maximize) for fp32 parameters, in two launches over a DEVICE job table; every scalar
 * of the step lives in device memory, so both launches can be captured in a HIP graph.
 *
 * `jobs`: DEVICE array of `njobs` bevmsda_optim_job, one per parameter tensor that has a gradient this step, kept alive and
 * unchanged by the caller while a launch that reads it can run (graph replays included).  p, g, exp_avg, exp_avg_sq:
 * contiguous fp32 arrays of `numel` elements, 4-byte aligned (the 16-byte-lane path runs when all four are 16-byte aligned);
 * step: the parameter's step count, ONE fp32 in device memory; group: index into `groups`; first_block = sum of
 * bevmsda_optim_job_blocks(numel) of the jobs before; `blocks` = the total.  A job of 0 elements has no block and still
 * counts its step.  The table's contents are the caller's to check.
 * `groups`: DEVICE array of `ngroups` bevmsda_optim_group (doubles, as torch keeps them on the host).
 * `scalars`: 8 DEVICE 4-byte words the caller zeroes ONCE: [0] fp32 total_norm, [1] fp32 clip_coef, [2] int32 skip (this
 * step), [3] int32 steps skipped so far, [4] the norm kernel's ticket (0 between launches), [5 .. 7] reserved.
 * `workspace`: bevmsda_optim_workspace_bytes(blocks) bytes, 8-byte aligned, contents irrelevant.
 *
 * bevmsda_optim_grad_norm_f32: total_norm = sqrt(sum g^2) over all jobs (<= 16 squares per fp32 partial, then double, summed
 * in a fixed order: bit-reproducible); clip_coef = min(1, max_norm / (total_norm + 1e-6)) with flags bit 0 (clip), else 1;
 * skip = total_norm not finite and flags bit 1 (skip_nonfinite).  Then skipped += 1, or every job's step += 1.
 * bevmsda_optim_adamw_f32: does nothing when skip is set; else per job, with its group's numbers and t = its step:
 * p *= 1 - lr * weight_decay; exp_avg += (clip_coef * g - exp_avg) * (1 - beta1); exp_avg_sq = beta2 * exp_avg_sq +
 * (1 - beta2) * (clip_coef * g)^2; p -= lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps).  g is
 * not written.  Run it after bevmsda_optim_grad_norm_f32 on the same stream with the same table.
 *
 * Checked before any launch: njobs, ngroups or blocks negative (numel for _job_blocks: -1 is returned) BEVMSDA_ERR_BAD_SHAPE;
 * blocks >= 2^30 BEVMSDA_ERR_TOO_LARGE; unknown flags bits, or clipping with a max_norm that is negative or NaN
 * BEVMSDA_ERR_BAD_OPTION; then njobs = 0 is a no-op; then a NULL pointer BEVMSDA_ERR_NULL_POINTER (groups with ngroups = 0
 * too); jobs, groups or workspace off 8 bytes, scalars off 4 bytes BEVMSDA_ERR_MISALIGNED. */
#define BEVMSDA_OPTIM_CLIP 1
#define BEVMSDA_OPTIM_SKIP_NONFINITE 2
#define BEVMSDA_OPTIM_SCALAR_WORDS 8
typedef struct bevmsda_optim_job {
  float *p;
  const float *g;
  float *exp_avg;
  float *exp_avg_sq;
  float *step;
  int64_t numel;
  int32_t group;
  int32_t first_block;
} bevmsda_optim_job;
typedef struct bevmsda_optim_group {
  double lr, beta1, beta2, eps, weight_decay;
} bevmsda_optim_group;

int64_t bevmsda_optim_job_blocks(int64_t numel);
int64_t bevmsda_optim_workspace_bytes(int64_t blocks);
int bevmsda_optim_grad_norm_f32(const bevmsda_optim_job *jobs, int njobs, int64_t blocks, double max_norm, int flags,
                                void *workspace, void *scalars, void *stream);
int bevmsda_optim_adamw_f32(const bevmsda_optim_job *jobs, int njobs, int64_t blocks, const bevmsda_optim_group *groups,
                            int ngroups, const void *scalars, void *stream);

/* ---- 3 x 3 convolution over channel-last rows + inference BatchNorm (csrc/conv3x3.h).  Entry points ADDED to ABI version 7:
 * nothing that existed changed, so the version number stays 7 (a library without them fails the binding's symbol check).
 *
 * The blocks of ResNetFusion, BEVFormerV2's temporal fusion (modules/transformerV2.py:16-52), on (bs, H W, C) BEV rows:
 *     y[p, co] = act( bn_co( sum_{dy, dx in {-1, 0, 1}} sum_ci x[p + dy W + dx, ci] w[co, ci, dy + 1, dx + 1] ) + res[p, co] )
 * over the bs * H * W pixels p, (y, x) = ((p mod H W) div W, p mod W); a tap counts only where 0 <= y + dy < H and
 * 0 <= x + dx < W (zero padding 1, stride 1, dilation 1, groups 1, no conv bias).  bn_co(v) = v * scale + shift with
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale, computed in the kernel from the four c_out vectors.
 * x: the c_in = nseg * c_seg input channels lie in nseg (<= BEVMSDA_CONV_MAX_SEGMENTS) row matrices of c_seg columns each,
 * seg[s] with row stride ld_seg[s] floats (a pointer may be listed more than once).  res (optional) and y: (bs H W, c_out)
 * rows with strides ld_res / ld_y; y must not overlap x or res.  precision: 0 = split operands (three bf16 products),
 * 1 = bf16; fp32 accumulate.  The weight is the image bevmsda_conv3x3_pack_weight_f32 writes from the contiguous
 * (c_out, c_in, 3, 3) fp32 tensor: bevmsda_conv3x3_packed_bytes(c_out, c_in) bytes (0 when c_in is not a multiple of 32),
 * bevmsda_linear_pack_weight_f32's chunk format over the (c_out, 9 c_in) matrix with k = tap * c_in + ci.
 * Checked before any launch, in this order: NULL descriptor BEVMSDA_ERR_NULL_POINTER; precision not 0 / 1
 * BEVMSDA_ERR_BAD_OPTION; a negative size or nseg > BEVMSDA_CONV_MAX_SEGMENTS BEVMSDA_ERR_BAD_SHAPE; more than 2^24 rows, more
 * than 65536 channels BEVMSDA_ERR_TOO_LARGE; then an empty problem (bs, H, W or c_out = 0) is a no-op; nseg or c_seg = 0
 * BEVMSDA_ERR_BAD_SHAPE; c_seg or c_out not a multiple of 32 BEVMSDA_ERR_UNSUPPORTED; a NULL pointer (res excepted)
 * BEVMSDA_ERR_NULL_POINTER; a row stride below its width BEVMSDA_ERR_BAD_SHAPE; a row stride that is no multiple of 4 floats
 * or a pointer off 16 bytes BEVMSDA_ERR_MISALIGNED. */
#define BEVMSDA_CONV_MAX_SEGMENTS 8
typedef struct bevmsda_conv3x3_desc {
  const float *seg[BEVMSDA_CONV_MAX_SEGMENTS];
  int64_t ld_seg[BEVMSDA_CONV_MAX_SEGMENTS];
  const float *res;
  int64_t ld_res, ld_y;
  const float *gamma, *beta, *mean, *var;
  int32_t bs, H, W, nseg, c_seg, c_out, relu, precision;
  float eps;
  int32_t reserved[3];
} bevmsda_conv3x3_desc;

int64_t bevmsda_conv3x3_packed_bytes(int c_out, int c_in);
int bevmsda_conv3x3_pack_weight_f32(const float *w, int c_out, int c_in, uint16_t *blob, void *stream);
int bevmsda_conv3x3_bn_f32(const bevmsda_conv3x3_desc *desc, const uint16_t *wpack, float *y, void *stream);

/* ---- convolution over channel-last rows for an image neck (csrc/conv_rows.h).  Entry point ADDED to ABI version 7: nothing
 * that existed changed, so the version number stays 7.
 *
 * The convolutions of mmdet's FPN (necks/fpn.py as published; bevformer_base.py:54-61) on (n_img H W, c_in) rows:
 *     y[q, co] = bias[co] + sum_taps sum_ci relu_in?(x[row(q, dy, dx), ci]) w[co, ci, dy + 1, dx + 1]  (+ res[rrow(q), co])
 * over the n_img * Ho * Wo output pixels q = (img, oy, ox), Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
 * row(q, dy, dx) = img H W + (stride oy + dy) W + (stride ox + dx), a tap counting only inside the input image.
 * taps: 9 = 3 x 3 with zero padding 1 (stride 1 or 2), 1 = 1 x 1 with padding 0 (stride 1; dy = dx = 0).  relu_in != 0:
 * max(x, 0) on the input before the products (NaN stays NaN).  bias: (c_out) or NULL.  res_mode: BEVMSDA_CONV_RES_NONE,
 * BEVMSDA_CONV_RES_SAME (res is (n_img Ho Wo, c_out) rows) or BEVMSDA_CONV_RES_UP2 (res is the coarser map
 * (n_img Hc Wc, c_out) with Ho = 2 Hc, Wo = 2 Wc; output pixel (oy, ox) adds row img Hc Wc + (oy >> 1) Wc + (ox >> 1): nearest
 * upsampling by exactly 2); res is ignored with BEVMSDA_CONV_RES_NONE.  Row strides ld_x, ld_res, ld_y in floats.
 * precision: 0 = split operands (three bf16 products), 1 = bf16; fp32 accumulate.  wpack: for 9 taps the image of
 * bevmsda_conv3x3_pack_weight_f32, for 1 tap the image of bevmsda_linear_pack_weight_f32 over the (c_out, c_in) matrix.
 * Checked before any launch, in this order: a NULL descriptor BEVMSDA_ERR_NULL_POINTER; taps not 1 / 9, stride not 1 / 2,
 * stride 2 with 1 tap, res_mode or precision out of range BEVMSDA_ERR_BAD_OPTION; a negative size BEVMSDA_ERR_BAD_SHAPE; more
 * than 2^24 input or output rows, more than 65536 channels BEVMSDA_ERR_TOO_LARGE; then an empty problem (n_img, H, W or
 * c_out = 0) is a no-op; c_in = 0 BEVMSDA_ERR_BAD_SHAPE; c_in or c_out not a multiple of 32 BEVMSDA_ERR_UNSUPPORTED;
 * BEVMSDA_CONV_RES_UP2 with an odd output height or width BEVMSDA_ERR_BAD_SHAPE; x, wpack, y or (with a res_mode) res NULL
 * BEVMSDA_ERR_NULL_POINTER; a row stride below its width BEVMSDA_ERR_BAD_SHAPE; a row stride that is no multiple of 4 floats
 * or a pointer off 16 bytes BEVMSDA_ERR_MISALIGNED; y overlapping x or res BEVMSDA_ERR_BAD_OPTION. */
#define BEVMSDA_CONV_RES_NONE 0
#define BEVMSDA_CONV_RES_SAME 1
#define BEVMSDA_CONV_RES_UP2 2
typedef struct bevmsda_conv_rows_desc {
  const float *x;
  int64_t ld_x;
  const float *bias;
  const float *res;
  int64_t ld_res;
  int32_t n_img, H, W, c_in, c_out, taps, stride, relu_in, res_mode, precision;
  int32_t reserved[4];
} bevmsda_conv_rows_desc;

int bevmsda_conv_rows_f32(const bevmsda_conv_rows_desc *desc, const uint16_t *wpack, float *y, int64_t ld_y, void *stream);

/* ---- modulated deformable 3 x 3 convolution over channel-last rows (csrc/deform_conv.h).  Entry point ADDED to ABI version 7:
 * nothing that existed changed, so the version number stays 7.
 *
 * mmcv 1.4.0's ModulatedDeformConv2dPack (DCNv2) as published — restated, not pinned against its source —, the conv2 of the
 * stage-3 / stage-4 bottlenecks of the reference's backbone (bevformer_base.py:43-53), on (n_img H W, c_in) rows:
 *     y[q, co] = act( ep( sum_{k = 3 i + j} sigmoid(logit_k(q)) sum_ci w[co, ci, i, j]
 *                         bilin(x[img, :, :, ci], stride oy - 1 + i + dy_k(q), stride ox - 1 + j + dx_k(q)) ) )
 * over the n_img * Ho * Wo output pixels q = (img, oy, ox), Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1; 3 x 3, padding
 * 1, dilation 1, groups 1, deform_groups 1, stride 1 or 2.  bilin: bilinear interpolation in pixel coordinates, a corner
 * outside [0, H) x [0, W) counting zero; a position that is not finite or outside (-1, H) x (-1, W) counts exactly zero and
 * addresses nothing.  offs: (n_img Ho Wo, 32) rows with row stride ld_offs >= 32 floats, the raw output of the pack's
 * conv_offset at q: column 2 k = dy_k, 2 k + 1 = dx_k, 18 + k = the mask logit, columns 27 .. 31 padding (never read).
 * ep: + bias[co] (bias given), or bn[0] .. bn[3] = gamma, beta, running mean, running variance of an inference BatchNorm
 * (v * scale + shift, scale = gamma / sqrt(var + eps), shift = beta - mean * scale, computed in the kernel), or nothing;
 * act: max(v, 0) when relu != 0 (NaN stays NaN).  Row strides ld_x, ld_offs, ld_y in floats.  precision: 0 = split operands
 * (three bf16 products), 1 = bf16; fp32 accumulate; the positions, the coefficients and the blend are fp32 in both.  wpack:
 * the image of bevmsda_conv3x3_pack_weight_f32.
 * Checked before any launch, in this order: a NULL descriptor BEVMSDA_ERR_NULL_POINTER; stride not 1 / 2, precision not
 * 0 / 1, some but not all of bn[], bias and bn[] both given BEVMSDA_ERR_BAD_OPTION; a negative size BEVMSDA_ERR_BAD_SHAPE; more
 * than 2^24 input rows, more than 65536 channels BEVMSDA_ERR_TOO_LARGE; then an empty problem (n_img, H, W or c_out = 0) is a
 * no-op; c_in = 0 BEVMSDA_ERR_BAD_SHAPE; c_in or c_out not a multiple of 32 BEVMSDA_ERR_UNSUPPORTED; x, offs, wpack or y NULL
 * BEVMSDA_ERR_NULL_POINTER; ld_x < c_in, ld_y < c_out or ld_offs < 32 BEVMSDA_ERR_BAD_SHAPE; a row stride that is no multiple of
 * 4 floats or a pointer off 16 bytes BEVMSDA_ERR_MISALIGNED; y overlapping x or offs BEVMSDA_ERR_BAD_OPTION. */
typedef struct bevmsda_deform_conv_desc {
  const float *x;
  int64_t ld_x;
  const float *offs;
  int64_t ld_offs;
  const float *bias;
  const float *bn[4];
  float eps;
  int32_t n_img, H, W, c_in, c_out, stride, relu, precision;
  int32_t reserved[3];
} bevmsda_deform_conv_desc;

int bevmsda_deform_conv_f32(const bevmsda_deform_conv_desc *desc, const uint16_t *wpack, float *y, int64_t ld_y, void *stream);

/* ---- convolution over channel-last rows + inference BatchNorm (+ residual) (+ ReLU) for a backbone's bottlenecks
 * (csrc/conv_bn_rows.h).  Entry point ADDED to ABI version 7: nothing that existed changed, so the version number stays 7.
 *
 * The plain convolutions of mmdet's ResNet bottleneck (conv1, conv2, conv3, downsample; bevformer_base.py:43-53) with the norm
 * after each, the residual sum and the ReLU, on (n_img H W, c_in) rows:
 *     y[q, co] = act( bn_co( sum_taps sum_ci x[row(q, dy, dx), ci] w[co, ci, dy + 1, dx + 1] ) + res[q, co] )
 * over the n_img * Ho * Wo output pixels q = (img, oy, ox), Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
 * row(q, dy, dx) = img H W + (stride oy + dy) W + (stride ox + dx), a tap counting only inside the input image.
 * taps: 9 = 3 x 3 with zero padding 1, 1 = 1 x 1 with padding 0 (dy = dx = 0); stride 1 or 2 for both.  No conv bias.
 * bn[0] .. bn[3] = gamma, beta, running mean, running variance (c_out each): bn_co(v) = v * scale + shift with
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale, computed in the kernel.  res: NULL or (n_img Ho Wo, c_out) rows,
 * added after the norm.  act: max(v, 0) when relu != 0 (NaN stays NaN).  Row strides ld_x, ld_res, ld_y in floats.
 * precision: 0 = split operands (three bf16 products), 1 = bf16; fp32 accumulate.  wpack: for 9 taps the image of
 * bevmsda_conv3x3_pack_weight_f32, for 1 tap the image of bevmsda_linear_pack_weight_f32 over the (c_out, c_in) matrix.
 * Checked before any launch, in this order: a NULL descriptor BEVMSDA_ERR_NULL_POINTER; taps not 1 / 9, stride not 1 / 2 or
 * precision not 0 / 1 BEVMSDA_ERR_BAD_OPTION; a negative size BEVMSDA_ERR_BAD_SHAPE; more than 2^24 input rows, more than 65536
 * channels BEVMSDA_ERR_TOO_LARGE; then an empty problem (n_img, H, W or c_out = 0) is a no-op, whatever the pointers; c_in = 0
 * BEVMSDA_ERR_BAD_SHAPE; c_in or c_out not a multiple of 32 BEVMSDA_ERR_UNSUPPORTED; x, wpack, y or any of bn[] NULL
 * BEVMSDA_ERR_NULL_POINTER; a row stride below its width BEVMSDA_ERR_BAD_SHAPE; a row stride that is no multiple of 4 floats or a
 * pointer off 16 bytes (bn[] and res included) BEVMSDA_ERR_MISALIGNED; y overlapping x or res BEVMSDA_ERR_BAD_OPTION. */
typedef struct bevmsda_conv_bn_rows_desc {
  const float *x;
  int64_t ld_x;
  const float *res;
  int64_t ld_res;
  const float *bn[4];
  float eps;
  int32_t n_img, H, W, c_in, c_out, taps, stride, relu, precision;
  int32_t reserved[2];
} bevmsda_conv_bn_rows_desc;

int bevmsda_conv_bn_rows_f32(const bevmsda_conv_bn_rows_desc *desc, const uint16_t *wpack, float *y, int64_t ld_y, void *stream);

/* ---- the backbone's stem in one launch: 7 x 7 stride-2 convolution + inference BatchNorm + ReLU + 3 x 3 stride-2 max pooling
 * of an NCHW image batch, written as channel-last rows (csrc/stem_conv.h).  Entry points ADDED to ABI version 7: nothing that
 * existed changed, so the version number stays 7.
 *
 * mmdet's ResNet stem (conv1, bn1, relu, maxpool; bevformer_base.py:43-53) on an (n_img, 3, H, W) fp32 batch:
 *     c[img, oy, ox, co] = relu( bn_co( sum_ci sum_{i < 7} sum_{j < 7} x[img, ci, 2 oy - 3 + i, 2 ox - 3 + j] w[co, ci, i, j] ) )
 *     y[img, py, px, co] = max over the 3 x 3 window { c[img, 2 py - 1 + a, 2 px - 1 + b, co] }
 * with Hc = (H - 1) / 2 + 1, Wc likewise, Hp = (Hc - 1) / 2 + 1, Wp likewise.  An input tap outside the image counts zero and
 * addresses nothing; a window tap outside the conv map is left out.  bn[0] .. bn[3] = gamma, beta, running mean, running variance
 * (64 each): bn_co(v) = v * scale + shift, scale = gamma / sqrt(var + eps), shift = beta - mean * scale, computed in the kernel,
 * BEFORE the maximum.  ReLU keeps NaN; the maximum propagates NaN as torch.max_pool2d does.  No conv bias.
 * x: element strides ld_img, ld_ch, ld_row of the images, channels and rows, unit column stride.  y: pool = 1 the
 * (n_img Hp Wp, 64) pooled rows, pool = 0 the (n_img Hc Wc, 64) rows of c; row stride ld_y in floats, columns beyond 64 untouched.
 * precision: 0 = split operands (three bf16 products), 1 = bf16; fp32 accumulate; norm, ReLU and maximum in fp32.
 * wpack: the image of bevmsda_stem_pack_weight_f32 from the contiguous (64, 3, 7, 7) weight, bevmsda_stem_packed_bytes(64, 3) =
 * 2 * 11 * 64 * 16 * 2 bytes ([hi | lo plane][11 k-steps][64 columns][16 k] bf16; K = (ci, i) x j, j padded to 8 with zeros);
 * any other channel counts: 0 bytes, BEVMSDA_ERR_UNSUPPORTED.
 * Checked before any launch, in this order: a NULL descriptor BEVMSDA_ERR_NULL_POINTER; pool or precision not 0 / 1
 * BEVMSDA_ERR_BAD_OPTION; a negative size BEVMSDA_ERR_BAD_SHAPE; more than 2^24 conv pixels (n_img Hc Wc) BEVMSDA_ERR_TOO_LARGE;
 * then an empty problem (n_img, H, W or c_out = 0) is a no-op, whatever the pointers; c_in != 3 or c_out != 64
 * BEVMSDA_ERR_UNSUPPORTED; x, wpack, y or any of bn[] NULL BEVMSDA_ERR_NULL_POINTER; ld_row < W, ld_ch < (H - 1) ld_row + W,
 * ld_img < 2 ld_ch + (H - 1) ld_row + W (rows, channels or images that overlap) or ld_y < 64 BEVMSDA_ERR_BAD_SHAPE; ld_y no
 * multiple of 4 floats, y, wpack or any of bn[] off 16 bytes, x off 4 bytes BEVMSDA_ERR_MISALIGNED; y overlapping x
 * BEVMSDA_ERR_BAD_OPTION. */
typedef struct bevmsda_stem_desc {
  const float *x;
  int64_t ld_img, ld_ch, ld_row;
  const float *bn[4];
  float eps;
  int32_t n_img, H, W, c_in, c_out, pool, precision;
  int32_t reserved[2];
} bevmsda_stem_desc;

int64_t bevmsda_stem_packed_bytes(int32_t c_out, int32_t c_in);
int bevmsda_stem_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, uint16_t *out, void *stream);
int bevmsda_stem_f32(const bevmsda_stem_desc *desc, const uint16_t *wpack, float *y, int64_t ld_y, void *stream);

/* ---- backward of bevmsda_conv_bn_rows_f32 with a frozen (inference) BatchNorm: input gradient and weight gradient over
 * channel-last rows (csrc/conv_bwd_rows.h).  Entry points ADDED to ABI version 7: nothing that existed changed, so the version
 * number stays 7.
 *
 * With y = act(scale * conv(x, w) + shift + res), scale = gamma / sqrt(var + eps), and g the gradient w.r.t. y:
 *     gz[q, co] = g[q, co] * (y[q, co] > 0 ? 1 : 0) * scale[co]
 * over the n_img Ho Wo output pixels q (bevmsda_conv_bn_rows_f32's geometry: taps 1 / 9, stride 1 / 2, Ho = (H - 1) / stride + 1).
 * Both gradient entry points read gz through (g, y, gamma, var, eps): y NULL leaves the mask out (no ReLU, or g is masked
 * already), gamma and var both NULL the scale (g is a finished gz); one of gamma / var alone is BEVMSDA_ERR_BAD_OPTION.  The mask
 * is a product with 0 or 1: a NaN in g stays NaN.  precision: 0 = split operands (three bf16 products), 1 = bf16; fp32 accumulate.
 *
 * bevmsda_conv_gz_rows_f32: gz as (M, C) rows of their own (row strides in floats; gz may be g itself with the same stride).
 * Checked in this order: one of gamma / var alone BEVMSDA_ERR_BAD_OPTION; M or C negative BEVMSDA_ERR_BAD_SHAPE; M over 2^24 or C
 * over 65536 BEVMSDA_ERR_TOO_LARGE; M or C zero a no-op; C no multiple of 32 BEVMSDA_ERR_UNSUPPORTED; g or gz NULL
 * BEVMSDA_ERR_NULL_POINTER; a row stride below C BEVMSDA_ERR_BAD_SHAPE; a row stride no multiple of 4 or a pointer off 16 bytes
 * BEVMSDA_ERR_MISALIGNED; gz overlapping y, or g other than exactly, BEVMSDA_ERR_BAD_OPTION.
 *
 * bevmsda_conv_dgrad_rows_f32: over the n_img H W INPUT pixels p,
 *     dx[p, ci] = sum_taps sum_co gz[q(p, tap), co] w[co, ci, tap]  (+ add[p, ci]),  then  * (next_mask[p, ci] > 0 ? 1 : 0) * next_scale[ci]
 * q(p, tap) the output pixel whose tap reads p (a tap counting only where that pixel exists: inside the output map and, at stride
 * 2, at even distances).  add: NULL or (n_img H W, c_in) rows, which may be dx itself with the same stride.  next_mask: NULL or the
 * saved output of the convolution that produced x, with next_gamma / next_var / next_eps its norm (both NULL: scale 1; a scale
 * without a mask, or one vector alone, is BEVMSDA_ERR_BAD_OPTION): dx is then that convolution's gz.  wpack: the image of
 * bevmsda_conv_dgrad_pack_weight_f32 from the contiguous (c_out, c_in, k, k) weight — the (c_in, taps c_out) matrix, taps mirrored
 * — of bevmsda_conv_dgrad_packed_bytes(c_out, c_in, taps) bytes (0: channel counts off the granularity or taps not 1 / 9).
 *
 * bevmsda_conv_wgrad_rows_f32:  dw[co, ci, tap] += sum_q gz[q, co] x[row(q, tap), ci]  with fp32 atomics into the contiguous
 * (c_out, c_in, k, k) array dw, which the caller zero-fills (or seeds); a tap outside the input image contributes nothing.
 *
 * Both check before any launch, in this order: a NULL descriptor BEVMSDA_ERR_NULL_POINTER; taps not 1 / 9, stride not 1 / 2,
 * precision not 0 / 1, an unpaired scale vector BEVMSDA_ERR_BAD_OPTION; a negative size BEVMSDA_ERR_BAD_SHAPE; more than 2^24
 * input rows or more than 65536 channels BEVMSDA_ERR_TOO_LARGE; then an empty problem (n_img, H, W or c_in = 0; for the weight
 * gradient also c_out = 0) is a no-op, whatever the pointers; for the input gradient c_out = 0 BEVMSDA_ERR_BAD_SHAPE; c_in or c_out
 * no multiple of 32 BEVMSDA_ERR_UNSUPPORTED; g, wpack / x, dx / dw NULL BEVMSDA_ERR_NULL_POINTER; a row stride below its width
 * BEVMSDA_ERR_BAD_SHAPE; a row stride that is no multiple of 4 floats or a pointer off 16 bytes (dw: off 4 bytes)
 * BEVMSDA_ERR_MISALIGNED; dx overlapping g, y, next_mask or (other than exactly) add, dw overlapping g, y or x
 * BEVMSDA_ERR_BAD_OPTION.
 *
 * Options in the descriptors' former reserved words (sizes and every other offset unchanged; all zero: the behaviour above).
 * Input gradient: add_mode = BEVMSDA_CONV_ADD_POOL2 takes add as the rows of the (2H, 2W) map and adds, per pixel (iy, ix),
 *     ((a[2iy, 2ix] + a[2iy, 2ix + 1]) + (a[2iy + 1, 2ix] + a[2iy + 1, 2ix + 1]))
 * in this order: the transpose of BEVMSDA_CONV_RES_UP2; add may then not overlap dx at all.  add_after_mask = 1 applies
 * * (next_mask > 0) * next_scale to the convolution path first and adds afterwards: dx = masked conv_transpose + add.
 * Weight gradient: relu_x = 1 reads max(x, 0) in place of x (a NaN stays NaN): the forward's relu_in.  dbias not NULL:
 *     dbias[co] += sum_q gz[q, co]
 * with fp32 atomics, one per column per workgroup of the centre tap and the first c_in tile; the caller zero-fills (or seeds) it.
 * Their checks, where the list above has them: add_mode, add_after_mask or relu_x not 0 / 1, add_mode = 1 or add_after_mask = 1
 * with add NULL, add_after_mask = 1 with next_mask NULL BEVMSDA_ERR_BAD_OPTION (after the unpaired scale vector); POOL2 with
 * 4 n_img H W over 2^24 BEVMSDA_ERR_TOO_LARGE (after the row and channel bounds); dbias off 4 bytes BEVMSDA_ERR_MISALIGNED
 * (with dw); POOL2's add overlapping dx, dbias overlapping g, y, x or dw BEVMSDA_ERR_BAD_OPTION (with the other overlaps). */
#define BEVMSDA_CONV_ADD_SAME 0
#define BEVMSDA_CONV_ADD_POOL2 1

typedef struct bevmsda_conv_dgrad_rows_desc {
  const float *g;
  int64_t ld_g;
  const float *y;
  int64_t ld_y;
  const float *gamma, *var;
  const float *add;
  int64_t ld_add;
  const float *next_mask;
  int64_t ld_next_mask;
  const float *next_gamma, *next_var;
  float eps, next_eps;
  int32_t n_img, H, W, c_in, c_out, taps, stride, precision;
  int32_t add_mode;                     /* BEVMSDA_CONV_ADD_SAME / BEVMSDA_CONV_ADD_POOL2 (formerly reserved[0]) */
  int32_t add_after_mask;               /* 0: + add, then mask and scale; 1: mask and scale, then + add (formerly reserved[1]) */
} bevmsda_conv_dgrad_rows_desc;

typedef struct bevmsda_conv_wgrad_rows_desc {
  const float *g;
  int64_t ld_g;
  const float *y;
  int64_t ld_y;
  const float *gamma, *var;
  const float *x;
  int64_t ld_x;
  float eps;
  int32_t n_img, H, W, c_in, c_out, taps, stride, precision;
  int32_t relu_x;                       /* offset 100 (formerly reserved[0]): 1 reads max(x, 0) in place of x */
  float *dbias;                         /* offset 104 (formerly reserved[1..2]): NULL or (c_out) floats accumulated into */
} bevmsda_conv_wgrad_rows_desc;

int64_t bevmsda_conv_dgrad_packed_bytes(int32_t c_out, int32_t c_in, int32_t taps);
int bevmsda_conv_dgrad_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, int32_t taps, uint16_t *blob, void *stream);
int bevmsda_conv_gz_rows_f32(const float *g, int64_t ld_g, const float *y, int64_t ld_y, const float *gamma, const float *var,
                             float eps, int64_t M, int32_t C, float *gz, int64_t ld_gz, void *stream);
int bevmsda_conv_dgrad_rows_f32(const bevmsda_conv_dgrad_rows_desc *desc, const uint16_t *wpack, float *dx, int64_t ld_dx,
                                void *stream);
int bevmsda_conv_wgrad_rows_f32(const bevmsda_conv_wgrad_rows_desc *desc, float *dw, void *stream);

/* ---- backward of bevmsda_deform_conv_f32 with a frozen (inference) BatchNorm: the gradient with respect to the input rows, the
 * offsets and mask logits, and the weight (csrc/deform_conv_bwd.h).  Entry points ADDED to ABI version 7: nothing that existed
 * changed, so the version number stays 7.
 *
 * In bevmsda_deform_conv_f32's notation, with m_k the sigmoid of the mask logit, b_c the four bilinear coefficients of
 * ly, lx, hy = 1 - ly, hx = 1 - lx, v_c = x[row_c, ci] (0 for a corner outside the image), gz read through (g, y, gamma, var, eps)
 * exactly as by bevmsda_conv_dgrad_rows_f32, and dcol[q, k, ci] = sum_co gz[q, co] w[co, ci, k]:
 *     dx[row_c, ci]      += m_k b_c dcol[q, k, ci]                                 (corners inside the image only)
 *     doffs[q, 18 + k]   += m_k (1 - m_k) sum_ci dcol sum_c b_c v_c
 *     doffs[q, 2 k]      += m_k sum_ci dcol ((v10 - v00) hx + (v11 - v01) lx)
 *     doffs[q, 2 k + 1]  += m_k sum_ci dcol ((v01 - v00) hy + (v11 - v10) ly)
 *     dw[co, ci, k]      += sum_q gz[q, co] m_k sum_c b_c v_c
 * floor has zero slope (at an integer position: the slope of the cell floor selects).  A position that is not finite or outside
 * (-1, H) x (-1, W) adds exactly nothing and addresses nothing; m (1 - m) is formed from m (a logit of -inf gives 0).  All sums
 * are fp32 atomics: the caller zero-fills (or seeds) dx, doffs and dw; run-to-run bit equality is not promised.  doffs is an
 * (n_img Ho Wo, ld_doffs >= 32) row matrix in offs's layout whose columns 27 .. 31 are never written.
 *
 * bevmsda_deform_conv_dgrad_f32: dx and doffs in one launch; need_dx = 0 / need_doffs = 0 leaves that part out (its pointer is
 * then not looked at); both 0 is a no-op.  wpack: the image of bevmsda_deform_dgrad_pack_weight_f32 from the contiguous
 * (c_out, c_in, 3, 3) weight — the (9 c_in, c_out) matrix whose row k c_in + ci is w[:, ci, k] — of
 * bevmsda_deform_dgrad_packed_bytes(c_out, c_in) bytes (0: channel counts off the granularity).
 * bevmsda_deform_conv_wgrad_f32: dw, the contiguous (c_out, c_in, 3, 3) array.
 *
 * Both check before any launch, in this order: a NULL descriptor BEVMSDA_ERR_NULL_POINTER; stride not 1 / 2, precision not 0 / 1,
 * an unpaired scale vector BEVMSDA_ERR_BAD_OPTION; a negative size BEVMSDA_ERR_BAD_SHAPE; more than 2^24 input rows or more than
 * 65536 channels BEVMSDA_ERR_TOO_LARGE; then an empty problem (n_img, H, W, c_in or c_out = 0; for the input gradient also
 * need_dx = need_doffs = 0) is a no-op, whatever the pointers; c_in or c_out no multiple of 32 BEVMSDA_ERR_UNSUPPORTED; g, x, offs,
 * wpack / dw, a needed dx or doffs NULL BEVMSDA_ERR_NULL_POINTER; a row stride below its width (ld_offs, ld_doffs < 32)
 * BEVMSDA_ERR_BAD_SHAPE; a row stride that is no multiple of 4 floats or a pointer off 16 bytes (dw: off 4 bytes)
 * BEVMSDA_ERR_MISALIGNED; dx, doffs or dw overlapping g, y, x, offs or one another BEVMSDA_ERR_BAD_OPTION. */
typedef struct bevmsda_deform_conv_dgrad_desc {
  const float *g;
  int64_t ld_g;
  const float *y;
  int64_t ld_y;
  const float *gamma, *var;
  const float *x;
  int64_t ld_x;
  const float *offs;
  int64_t ld_offs;
  float *dx;
  int64_t ld_dx;
  float *doffs;
  int64_t ld_doffs;
  float eps;
  int32_t n_img, H, W, c_in, c_out, stride, precision, need_dx, need_doffs;
  int32_t reserved[2];
} bevmsda_deform_conv_dgrad_desc;

typedef struct bevmsda_deform_conv_wgrad_desc {
  const float *g;
  int64_t ld_g;
  const float *y;
  int64_t ld_y;
  const float *gamma, *var;
  const float *x;
  int64_t ld_x;
  const float *offs;
  int64_t ld_offs;
  float eps;
  int32_t n_img, H, W, c_in, c_out, stride, precision;
  int32_t reserved[2];
} bevmsda_deform_conv_wgrad_desc;

int64_t bevmsda_deform_dgrad_packed_bytes(int32_t c_out, int32_t c_in);
int bevmsda_deform_dgrad_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, uint16_t *blob, void *stream);
int bevmsda_deform_conv_dgrad_f32(const bevmsda_deform_conv_dgrad_desc *desc, const uint16_t *wpack, void *stream);
int bevmsda_deform_conv_wgrad_f32(const bevmsda_deform_conv_wgrad_desc *desc, float *dw, void *stream);

/* ---- BatchNorm with BATCH statistics over channel-last rows, forward and backward (csrc/batchnorm_rows.h): what a bottleneck
 * whose norms are in train() mode runs around its raw convolutions.  Entry points ADDED to ABI version 7: nothing that existed
 * changed, so the version number stays 7.
 *
 * Rows are (M, C) fp32 with unit column stride and a row stride ld >= C in floats; C a multiple of 32, 2 <= M <= 2^24.  All
 * arithmetic is fp32.  With invstd = 1 / sqrtf(var + eps) and xhat = (z - mean) * invstd, both formed in the kernels:
 *
 * bevmsda_bn_stats_rows_f32: mean[c] = sum_m z[m, c] / M and the BIASED var[c] = sum_m (z[m, c] - mean[c])^2 / M.  The variance is
 * never formed as E[z^2] - E[z]^2: per-thread shifted sums become (count, mean, M2) triples that are merged with Chan's formula,
 * inside a workgroup and, through `workspace`, across workgroups by a second kernel of the same call in a fixed order — no
 * floating-point atomics, two calls on the same input give the same bits; a constant column gives var = 0 exactly, no column a
 * negative value.  running_mean / running_var (both or neither; NULL: left alone) are updated in place,
 *     running_mean = (1 - momentum) running_mean + momentum mean,  running_var = (1 - momentum) running_var + momentum var M / (M - 1),
 * and num_batches_tracked (NULL: left alone) is incremented by one.
 * workspace: bevmsda_bn_rows_workspace_bytes(M, C) bytes the caller owns (0: M or C not covered); the library allocates nothing.
 *
 * bevmsda_bn_apply_rows_f32:  y = act(xhat * gamma + beta + res),  res NULL or (M, C) rows, act the ReLU when relu = 1 (a NaN
 * stays NaN).  y may be z itself with the same stride.
 *
 * bevmsda_bn_bwd_reduce_rows_f32: with gy = g * (y > 0 ? 1 : 0) (y NULL: gy = g; a product, a NaN in g stays NaN),
 *     sums[c] = S1 = sum_m gy[m, c]   (the gradient of beta),      sums[C + c] = S2 = sum_m gy[m, c] xhat[m, c]   (of gamma),
 * through the same workspace and the same fixed-order merge: deterministic.
 *
 * bevmsda_bn_bwd_apply_rows_f32:  dz = gamma * invstd * (gy - S1 / M - xhat * S2 / M)  from the sums of the call above, and gy
 * itself into `gy` when that is not NULL (the gradient of the residual branch).  dz may be g itself with the same stride.
 *
 * Each checks before any launch, in this order: its options — running_mean / running_var unpaired, momentum outside [0, 1] with
 * running statistics, relu not 0 / 1 — BEVMSDA_ERR_BAD_OPTION; M or C negative BEVMSDA_ERR_BAD_SHAPE; M over 2^24 or C over 65536
 * BEVMSDA_ERR_TOO_LARGE; M < 2 or C no multiple of 32 BEVMSDA_ERR_UNSUPPORTED; then C = 0 is a no-op; a required pointer NULL (all
 * but running_mean, running_var, num_batches_tracked, res, y of the backward calls, gy) BEVMSDA_ERR_NULL_POINTER; a row stride
 * below C BEVMSDA_ERR_BAD_SHAPE; a row stride that is no multiple of 4 floats or a pointer off 16 bytes (num_batches_tracked: off
 * 8 bytes) BEVMSDA_ERR_MISALIGNED; something written overlapping something read, other than the two exact aliases above,
 * BEVMSDA_ERR_BAD_OPTION. */
int64_t bevmsda_bn_rows_workspace_bytes(int64_t M, int32_t C);
int bevmsda_bn_stats_rows_f32(const float *z, int64_t ld_z, int64_t M, int32_t C, float *mean, float *var, float *running_mean,
                              float *running_var, int64_t *num_batches_tracked, float momentum, float *workspace, void *stream);
int bevmsda_bn_apply_rows_f32(const float *z, int64_t ld_z, const float *mean, const float *var, const float *gamma, const float *beta,
                              float eps, const float *res, int64_t ld_res, int32_t relu, int64_t M, int32_t C, float *y, int64_t ld_y,
                              void *stream);
int bevmsda_bn_bwd_reduce_rows_f32(const float *g, int64_t ld_g, const float *y, int64_t ld_y, const float *z, int64_t ld_z,
                                   const float *mean, const float *var, float eps, int64_t M, int32_t C, float *sums, float *workspace,
                                   void *stream);
int bevmsda_bn_bwd_apply_rows_f32(const float *g, int64_t ld_g, const float *y, int64_t ld_y, const float *z, int64_t ld_z,
                                  const float *mean, const float *var, const float *gamma, float eps, const float *sums, int64_t M,
                                  int32_t C, float *dz, int64_t ld_dz, float *gy, int64_t ld_gy, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVMSDA_H_ */
