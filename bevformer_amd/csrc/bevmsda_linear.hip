// C ABI of libbevmsda.so, dense projections and their weight images (linear_mfma.h, linear_pipe.h, linear_panel.h, linear_roles.h,
// linear_pack_multi.h): bevmsda_linear_*_f32, bevmsda_linear_pack_*, bevmsda_linear_panel_*.  No torch, no allocation, no global state.
#include "capi_checks.h"
#include "linear_mfma.h"
#include "linear_pipe.h"
#include "linear_panel.h"
#include "linear_roles.h"
#include "linear_pack_multi.h"

namespace {
constexpr bool kLinearPipeDefault = false;       // linear_pipe.h (software-pipelined) as the default where it applies
constexpr long long kLinearPipeMaxRows = 8192;   // ... and always for M <= this

// one launch of linear_panel_kernel: shape 1 = 64-row panels (4 wavefronts of 64 x 64 tiles), 2 = 128-row panels (8 wavefronts
// of 128 x 32 tiles); pre = what the split pass adds (0 nothing, 1 an addend matrix, 2 gather mode)
template <int NPROD, bool LN, int PRE, bool MASKED>
void panel_dispatch(int shape, dim3 grid, hipStream_t st, const bevmsda::PanelArgs &a) {
  if (shape == 1) hipLaunchKernelGGL((bevmsda::linear_panel_kernel<NPROD, 2, 2, 4, LN, PRE, 0, 0, MASKED>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::linear_panel_kernel<NPROD, 4, 1, 8, LN, PRE, 0, 0, MASKED>), grid, dim3(512), 0, st, a);
}
template <int NPROD, bool LN>
void panel_dispatch(int shape, int pre, bool masked, dim3 grid, hipStream_t st, const bevmsda::PanelArgs &a) {
  if constexpr (!LN) {
    if (masked) return panel_dispatch<NPROD, false, 0, true>(shape, grid, st, a);      // (plain projections only: checked by the caller)
  }
  if (pre == 2) panel_dispatch<NPROD, LN, 2, false>(shape, grid, st, a);
  else if (pre == 1) panel_dispatch<NPROD, LN, 1, false>(shape, grid, st, a);
  else panel_dispatch<NPROD, LN, 0, false>(shape, grid, st, a);
}
}  // namespace

extern "C" {

static int linear_launch(const float *x0, const float *a0, const float *x1, const float *a1, const float *w,
                         const uint16_t *wpack, const float *bias, const bevmsda_linear_desc *d, float *y,
                         void *stream, const int32_t *gidx = nullptr, const float *gscale = nullptr,
                         const float *mask = nullptr, long ldmask = 0, float mask_scale = 1.0f) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->M < 0 || d->N < 0 || d->K0 < 0 || d->K1 < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->M == 0 || d->N == 0) return BEVMSDA_OK;
  if (d->K0 == 0 || d->K0 % bevmsda::kLinKGran != 0 || d->K1 % bevmsda::kLinKGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!x0 || (!w && !wpack) || !y || (d->K1 > 0 && !x1)) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ldx0 % 4 != 0 || (w && d->ldw % 4 != 0) || (a0 && d->lda0 % 4 != 0) ||
      (d->K1 > 0 && (d->ldx1 % 4 != 0 || (a1 && d->lda1 % 4 != 0))))
    return BEVMSDA_ERR_UNSUPPORTED;
  const int gcols = d->group_cols;
  if (gcols < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (gcols > 0 && (gcols % bevmsda::kLinBN != 0 || d->N % gcols != 0)) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->ldx0 < d->K0 || (w && d->ldw < d->K0 + d->K1) || d->ldy < (gcols > 0 ? gcols : d->N) ||
      (d->K1 > 0 && d->ldx1 < d->K1))
    return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(x0) || (w && misaligned(w)) || (wpack && misaligned(wpack)) ||
      off4(y) || (a0 && misaligned(a0)) ||
      (d->K1 > 0 && (misaligned(x1) || (a1 && misaligned(a1)))))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::LinArgs a;
  a.x0 = x0; a.a0 = a0; a.x1 = d->K1 > 0 ? x1 : nullptr; a.a1 = d->K1 > 0 ? a1 : nullptr;
  a.ldx0 = d->ldx0; a.lda0 = d->lda0; a.ldx1 = d->ldx1; a.lda1 = d->lda1;
  a.w = w; a.ldw = d->ldw; a.wpack = wpack; a.bias = bias; a.y = y; a.ldy = d->ldy;
  a.gidx = gidx; a.gscale = gscale;
  a.M = d->M; a.N = d->N; a.K0 = d->K0; a.K1 = d->K1; a.relu = d->relu ? 1 : 0;
  a.group_cols = gcols;
  a.out_bf16 = d->out_bf16 ? 1 : 0;
  // desc->reserved[0] = 1: y += result (first kernel, float4 epilogue: fp32 y, N and ldy multiples of 4, aligned y / bias)
  a.accum = d->reserved[0] == 1 ? 1 : 0;
  if (d->reserved[0] != 0 && d->reserved[0] != 1) return BEVMSDA_ERR_BAD_OPTION;
  a.mask = mask; a.ldmask = ldmask; a.mask_scale = mask_scale;
  if (mask && (gcols != 0 || d->out_bf16 || d->N % 4 != 0 || d->ldy % 4 != 0 || ldmask % 4 != 0 || ldmask < d->N ||
               misaligned(y) || misaligned(mask) || (bias && misaligned(bias)) || d->variant == 131))
    return BEVMSDA_ERR_UNSUPPORTED;
  if (a.accum && (d->out_bf16 || d->N % 4 != 0 || d->ldy % 4 != 0 || gcols % 4 != 0 || misaligned(y) || (bias && misaligned(bias)) ||
                  d->variant == 131))
    return BEVMSDA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool add = a.a0 != nullptr || a.a1 != nullptr || gidx != nullptr;
  // the launch grid over bm x bn output tiles (capi_checks.h: xcd_grid), the tile counts into the kernel's arguments
  unsigned grid = 0;
  auto tile_grid = [&](int bm, int bn) {
    const long long nbm = (d->M + bm - 1) / bm, nbn = (d->N + bn - 1) / bn;
    a.nblk_m = static_cast<int>(nbm);
    a.nblk_n = static_cast<int>(nbn);
    return xcd_grid(nbm, nbn, &grid);
  };
  // desc->variant: 0 = library default; 1 = the first kernel over the fp32 weight matrix, 13 = over the packed weight
  // image (LDS-DMA into a single W area); 131 = the software-pipelined kernel (BEVMSDA_ERR_UNSUPPORTED when it does not
  // cover the call).  desc->reserved[1] = 1 keeps the default off the software-pipelined kernel.
  if (d->variant != 0 && d->variant != 1 && d->variant != 13 && d->variant != 131 && d->variant != 17) return BEVMSDA_ERR_BAD_OPTION;
  // desc->variant = 17 (round 6): 64-row x 256-column tiles of the first kernel over the packed weight image — for
  // 128 < N <= 256 every input row is staged ONCE (the 128 x 128 default stages it once per column tile) and the
  // 64-row workgroups (3 per CU) cover a 40,000-row call in one round
  if (d->variant == 17) {
    if (!wpack || a.accum || mask || d->N <= 128 || d->N % 4 != 0 || d->ldy % 4 != 0 || misaligned(y) || (bias && misaligned(bias)))
      return BEVMSDA_ERR_UNSUPPORTED;
    if (const int rc = tile_grid(64, 256); rc != BEVMSDA_OK) return rc;
    const dim3 g(grid), b(256);
    if (d->precision == 0) {
      if (add) hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<3, true, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
      else hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<3, false, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
    } else {
      if (add) hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<1, true, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
      else hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<1, false, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
    }
    return launch_status();
  }
  // software-pipelined kernel (linear_pipe.h)
  {
    const int nch = (d->K0 + d->K1) / 32;
    const bool covered = wpack && !add && !a.accum && !mask && (d->N % 4) == 0 && (d->ldy % 4) == 0 && (gcols % 4) == 0 && !misaligned(y) &&
                         (!bias || !misaligned(bias)) && (!d->out_bf16 || !off8(y)) && (nch == 8 || nch == 16);
    if (d->variant == 131 && !covered) return BEVMSDA_ERR_UNSUPPORTED;
    // default for tile-sized row counts (a rank's share of a BEV-tiled frame: one workgroup per CU, where its two-chunk
    // lead is worth 8-13 %: profiles/r2/r2_gemm_small_m.txt); at base size the first kernel's 4 workgroups per CU win
    if (covered && (d->variant == 131 || (d->variant == 0 && d->reserved[1] == 0 && (kLinearPipeDefault || d->M <= kLinearPipeMaxRows)))) {
      if (const int rc = tile_grid(128, 128); rc != BEVMSDA_OK) return rc;
#define BEVMSDA_PIPE(NP_, NCH_)                                                                                       \
  do {                                                                                                                \
    auto kern = bevmsda::linear_pipe_kernel<NP_, NCH_>;                                                               \
    const int dyn = 2 * ((NP_) == 3 ? 2 : 1) * bevmsda::kPipePlane * 2;                                               \
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, dyn) != \
        hipSuccess) return BEVMSDA_ERR_LAUNCH;                                                                        \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), dyn, st, a);                                                      \
  } while (0)
      if (d->precision == 0) { if (nch == 8) BEVMSDA_PIPE(3, 8); else BEVMSDA_PIPE(3, 16); }
      else { if (nch == 8) BEVMSDA_PIPE(1, 8); else BEVMSDA_PIPE(1, 16); }
#undef BEVMSDA_PIPE
      return launch_status();
    }
  }
  if ((d->variant == 1 && wpack) || (d->variant == 13 && !wpack)) return BEVMSDA_ERR_BAD_OPTION;
  if (const int rc = tile_grid(bevmsda::kLinBM, bevmsda::kLinBN); rc != BEVMSDA_OK) return rc;
  const dim3 g(grid), b(256);
  // bf16 output: the transposed-tile epilogue packs 4 consecutive columns per lane
  if (d->out_bf16 && (d->N % 4 != 0 || d->ldy % 4 != 0 || (gcols % 4) != 0 || off8(y) || (bias && misaligned(bias))))
    return BEVMSDA_ERR_UNSUPPORTED;
#define BEVMSDA_LIN(NP_, WM_)                                                                                     \
  do {                                                                                                            \
    if (add) hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<NP_, true, 32, true, WM_>), g, b, 0, st, a);    \
    else hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<NP_, false, 32, true, WM_>), g, b, 0, st, a);       \
  } while (0)
  if (d->precision == 0) { if (wpack) BEVMSDA_LIN(3, 3); else BEVMSDA_LIN(3, 0); }
  else { if (wpack) BEVMSDA_LIN(1, 3); else BEVMSDA_LIN(1, 0); }
#undef BEVMSDA_LIN
  return launch_status();
}

int bevmsda_linear_f32(const float *x0, const float *a0, const float *x1, const float *a1, const float *w,
                       const float *bias, const bevmsda_linear_desc *d, float *y, void *stream) {
  if (!w) return BEVMSDA_ERR_NULL_POINTER;
  return linear_launch(x0, a0, x1, a1, w, nullptr, bias, d, y, stream);
}

int bevmsda_linear_packed_f32(const float *x0, const float *a0, const float *x1, const float *a1,
                              const uint16_t *wpack, const float *bias, const bevmsda_linear_desc *d, float *y,
                              void *stream) {
  if (!wpack) return BEVMSDA_ERR_NULL_POINTER;
  return linear_launch(x0, a0, x1, a1, nullptr, wpack, bias, d, y, stream);
}

int bevmsda_linear_relu_backward_packed_f32(const float *g, const uint16_t *wpack, const float *act, int64_t ld_act,
                                            float scale, const bevmsda_linear_desc *d, float *y, void *stream) {
  if (!wpack || !act) return BEVMSDA_ERR_NULL_POINTER;
  if (d && (d->K1 != 0 || d->relu)) return BEVMSDA_ERR_BAD_SHAPE;
  return linear_launch(g, nullptr, nullptr, nullptr, nullptr, wpack, nullptr, d, y, stream, nullptr, nullptr, act,
                       static_cast<long>(ld_act), scale);
}

int bevmsda_linear_gather_packed_f32(const float *rows, int64_t ld_rows, const int32_t *idx, const float *scale,
                                     const uint16_t *wpack, const float *bias, const bevmsda_linear_desc *d,
                                     float *y, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (!wpack || !idx || !scale) return BEVMSDA_ERR_NULL_POINTER;
  if (d->K1 != 0) return BEVMSDA_ERR_BAD_SHAPE;
  bevmsda_linear_desc dd = *d;
  dd.ldx0 = ld_rows;
  return linear_launch(rows, nullptr, nullptr, nullptr, nullptr, wpack, bias, &dd, y, stream, idx, scale);
}

int64_t bevmsda_linear_packed_bytes(int N, int K) {
  if (N <= 0 || K <= 0 || K % 32 != 0) return 0;
  return static_cast<int64_t>((N + 127) / 128) * (K / 32) * 2 * 128 * 40 * 2;
}

int bevmsda_linear_pack_weight_f32(const float *w, int64_t ldw, int N, int K, uint16_t *blob, void *stream) {
  if (N <= 0 || K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (K % 32 != 0 || ldw % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ldw < K) return BEVMSDA_ERR_BAD_SHAPE;
  if (!w || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(w) || misaligned(blob)) return BEVMSDA_ERR_MISALIGNED;
  const long long threads = static_cast<long long>((N + 127) / 128) * 128 * (K / 8);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::lin_pack_weight_kernel<false>, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, static_cast<long>(ldw), N, K, blob);
  return launch_status();
}

int bevmsda_linear_pack_weight_t_f32(const float *wt, int64_t ldwt, int N, int K, uint16_t *blob, void *stream) {
  if (N <= 0 || K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (K % 32 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ldwt < N) return BEVMSDA_ERR_BAD_SHAPE;
  if (!wt || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(blob) || off4(wt)) return BEVMSDA_ERR_MISALIGNED;
  const long long threads = static_cast<long long>((N + 127) / 128) * 128 * (K / 8);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::lin_pack_weight_kernel<true>, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), wt, static_cast<long>(ldwt), N, K, blob);
  return launch_status();
}

// ---- row-panel projection (linear_panel.h)
int64_t bevmsda_linear_panel_packed_bytes(int N, int K) {
  if (N <= 0 || K <= 0 || K % bevmsda::kPanelK != 0) return 0;
  return static_cast<int64_t>((N + 63) / 64) * 2 * (K / 16) * 2 * 1024;
}

int bevmsda_linear_panel_pack_weight_f32(const float *w, int64_t ldw, int N, int K, uint16_t *blob, void *stream) {
  if (N <= 0 || K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (K % bevmsda::kPanelK != 0 || ldw % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ldw < K) return BEVMSDA_ERR_BAD_SHAPE;
  if (!w || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(w) || misaligned(blob)) return BEVMSDA_ERR_MISALIGNED;
  const int tiles32 = ((N + 63) / 64) * 2;
  const long long threads = 1LL * tiles32 * (K / 16) * 64;
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::lin_panel_pack_weight_kernel<false>, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, static_cast<long>(ldw), N, K, tiles32, blob);
  return launch_status();
}

int bevmsda_linear_panel_pack_weight_t_f32(const float *wt, int64_t ldwt, int N, int K, uint16_t *blob, void *stream) {
  if (N <= 0 || K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (K % bevmsda::kPanelK != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ldwt < N) return BEVMSDA_ERR_BAD_SHAPE;
  if (!wt || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(blob) || off4(wt)) return BEVMSDA_ERR_MISALIGNED;
  const int tiles32 = ((N + 63) / 64) * 2;
  const long long threads = 1LL * tiles32 * (K / 16) * 64;
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::lin_panel_pack_weight_kernel<true>, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), wt, static_cast<long>(ldwt), N, K, tiles32, blob);
  return launch_status();
}

// Many weight images in one launch (linear_pack_multi.h).  `jobs` is a DEVICE array of `njobs`
// bevmsda_pack_job (the caller keeps it alive and unchanged while launches that read it — graph replays included — can
// run); `blocks` = the total number of 256-thread blocks = first_block of a job past the last (bevmsda_linear_pack_job_blocks
// gives a job's block count).  Jobs are validated by the caller against the single-image entry points' rules.
int64_t bevmsda_linear_pack_job_blocks(int N, int K, int kind) {
  if (N <= 0 || K <= 0 || kind < 0 || kind > 3) return 0;
  if (kind & 2) {
    if (K % bevmsda::kPanelK != 0) return 0;
    const long long threads = 1LL * ((N + 63) / 64) * 2 * (K / 16) * 64;
    return (threads + 255) / 256;
  }
  if (K % 32 != 0) return 0;
  const long long threads = static_cast<long long>((N + 127) / 128) * 128 * (K / 8);
  return (threads + 255) / 256;
}

int bevmsda_linear_pack_weights_multi_f32(const bevmsda_pack_job *jobs, int njobs, int64_t blocks, void *stream) {
  static_assert(sizeof(bevmsda_pack_job) == sizeof(bevmsda::PackJob), "bevmsda_pack_job layout");
  if (njobs < 0 || blocks < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (njobs == 0 || blocks == 0) return BEVMSDA_OK;
  if (!jobs) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(jobs)) return BEVMSDA_ERR_MISALIGNED;
  if (blocks >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::lin_pack_weights_multi_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const bevmsda::PackJob *>(jobs), njobs);
  return launch_status();
}

// shape 3 (linear_roles.h: MFMA wavefronts that never store, C tiles drained by store wavefronts) by default for the plain
// projections with at least this many rows and kPanelRolesMinCols columns (the hoisted value projections)
static constexpr long kPanelRolesMinRows = 65536;
static constexpr int kPanelRolesMinCols = 1024;
// output stores of shape 3 by default: non-temporal (true) or the default policy (false)
static constexpr bool kPanelRolesNtStores = true;

static int panel_launch(const float *x0, const float *a0, const float *x1, const float *a1, const int32_t *idx,
                        const float *scale, const uint16_t *wpanel, const float *bias,
                        const bevmsda_linear_desc *d, const bevmsda_layernorm_desc *ln, float *y, void *stream,
                        const int32_t *seg_start, int64_t seg_len, const int64_t *level_shapes, int num_levels,
                        const float *xb = nullptr, int64_t m_split = 0, const int32_t *need = nullptr,
                        int64_t need_rows = 0, int64_t need_len = 0) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->M < 0 || d->N < 0 || d->K0 < 0 || d->K1 < 0 || d->group_cols < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (xb && (m_split < 0 || m_split > d->M)) return BEVMSDA_ERR_BAD_SHAPE;
  if (xb && (d->K1 != 0 || a0 || idx || ln || seg_start)) return BEVMSDA_ERR_UNSUPPORTED;
  if (xb && misaligned(xb)) return BEVMSDA_ERR_MISALIGNED;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->M == 0 || d->N == 0) return BEVMSDA_OK;
  const int K = d->K0 + d->K1;
  if ((K != 256 && K != 512) || (d->K0 != 256 && d->K0 != 512) || (d->K1 != 0 && d->K1 != 256)) return BEVMSDA_ERR_UNSUPPORTED;
  if (!x0 || !wpanel || !y || (d->K1 > 0 && !x1)) return BEVMSDA_ERR_NULL_POINTER;
  if ((idx == nullptr) != (scale == nullptr)) return BEVMSDA_ERR_NULL_POINTER;
  if (idx && (d->K1 != 0 || a0)) return BEVMSDA_ERR_BAD_SHAPE;
  const int gcols = d->group_cols;
  if (d->N % 4 != 0 || d->ldy % 4 != 0 || d->ldx0 % 4 != 0 || (a0 && d->lda0 % 4 != 0) ||
      (d->K1 > 0 && (d->ldx1 % 4 != 0 || (a1 && d->lda1 % 4 != 0))) || (gcols > 0 && (gcols % 64 != 0 || d->N % gcols != 0)))
    return BEVMSDA_ERR_UNSUPPORTED;
  if (d->ldx0 < d->K0 || d->ldy < (gcols > 0 ? gcols : d->N) || (d->K1 > 0 && d->ldx1 < d->K1)) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(x0) || misaligned(wpanel) || misaligned(y) || (bias && misaligned(bias)) || (a0 && misaligned(a0)) ||
      (d->K1 > 0 && (misaligned(x1) || (a1 && misaligned(a1)))))
    return BEVMSDA_ERR_MISALIGNED;
  const int64_t wbytes = bevmsda_linear_panel_packed_bytes(d->N, K);
  if (wbytes >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  // (the epilogue's raw buffer covers ONE row panel of one output group — 64-bit base, 32-bit record count and offsets
  // inside it: at most 128 rows x ldy elements of 2 or 4 bytes have to fit)
  if (!ln && 128LL * d->ldy * (d->out_bf16 ? 2 : 4) >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::PanelArgs a;
  a.x0 = x0; a.a0 = a0; a.x1 = d->K1 > 0 ? x1 : nullptr; a.a1 = d->K1 > 0 ? a1 : nullptr;
  a.ldx0 = d->ldx0; a.lda0 = d->lda0; a.ldx1 = d->ldx1; a.lda1 = d->lda1;
  a.gidx = idx; a.gscale = scale;
  a.wp = wpanel; a.wp_bytes = static_cast<unsigned>(wbytes);
  a.bias = bias; a.y = y; a.ldy = d->ldy; a.M = d->M; a.N = d->N; a.K0 = d->K0; a.K1 = d->K1;
  a.relu = d->relu ? 1 : 0; a.group_cols = gcols; a.out_bf16 = d->out_bf16 ? 1 : 0;
  a.res = nullptr; a.ldres = 0; a.gamma = a.beta = nullptr; a.eps = 0.f;
  a.xb = xb; a.m_split = m_split;
  a.need = need; a.need_rows = need_rows;
  a.skew = 0;
  if (need) {
    // needed-panel table (bevmsda_linear_panel_rows2_masked_f32): two row blocks, the default kernel of each shape
    if (!xb || d->relu || K != 256) return BEVMSDA_ERR_UNSUPPORTED;
    if (need_rows <= 0 || need_len <= 0) return BEVMSDA_ERR_BAD_SHAPE;
    const int64_t longest = m_split > d->M - m_split ? m_split : d->M - m_split;
    if ((longest + need_rows - 1) / need_rows > need_len) return BEVMSDA_ERR_BAD_SHAPE;    // (the table covers both blocks)
    if (off4(need)) return BEVMSDA_ERR_MISALIGNED;
    if (d->reserved[3] != 0) return BEVMSDA_ERR_UNSUPPORTED;                               // (role-split knobs: unmasked launches only)
  }
  a.seg_start = seg_start; a.seg_len = seg_len; a.level_shapes = level_shapes; a.num_levels = level_shapes ? num_levels : 0;
  if (seg_start && (seg_len <= 0 || num_levels < 0)) return BEVMSDA_ERR_BAD_SHAPE;
  if (ln) {
    if (d->N != 256 || gcols != 0 || d->relu || d->out_bf16) return BEVMSDA_ERR_UNSUPPORTED;
    if (!ln->gamma || !ln->beta) return BEVMSDA_ERR_NULL_POINTER;
    if (misaligned(ln->gamma) || misaligned(ln->beta) || (ln->res && (misaligned(ln->res) || ln->ldres % 4 != 0 || ln->ldres < d->N)))
      return BEVMSDA_ERR_MISALIGNED;
    a.res = ln->res; a.ldres = ln->ldres; a.gamma = ln->gamma; a.beta = ln->beta; a.eps = ln->eps;
  }
  // workgroup shape (desc->reserved[2]): 1 = 64-row panels, 4 wavefronts of 64 x 64 tiles, two workgroups per CU;
  // 2 = 128-row panels, 8 wavefronts of 128 x 32 tiles, one workgroup per CU (half the weight traffic per MFMA);
  // 0 = by shape.  Two panel passes (K = 512) and the LayerNorm epilogue need one column tile per wavefront: N <= 256
  // 3 = the role-split form (linear_roles.h: 64-row panels, 8 MFMA wavefronts that never store + 4 store wavefronts, one
  // workgroup per CU) for the plain projections — one source, two row blocks (rows2) or row segments, K = 256, N % 32 == 0,
  // fp32 or bf16 out, grouped or not; any other form takes the shape rule below.  desc->reserved[3] with shape 3 (benchmark
  // knobs): 0 = default (MFMA wavefronts at priority 1, stores by kPanelRolesNtStores); 1 = MFMA wavefronts at priority 0,
  // 2 = non-temporal stores, 3 = both; 4 = priority 1 with default-policy stores.  Shapes 1 and 2 have no knobs:
  // desc->reserved[3] must be 0
  int shape = d->reserved[2];
  if (shape < 0 || shape > 3) return BEVMSDA_ERR_BAD_OPTION;
  if ((K == 512 || ln) && d->N > 256) return BEVMSDA_ERR_UNSUPPORTED;
  const bool roles_form = !idx && !a.a0 && !a.a1 && !ln && K == 256 && d->N % 32 == 0;
  if (shape == 0 && roles_form && d->N >= kPanelRolesMinCols && d->M >= kPanelRolesMinRows) shape = 3;
  bevmsda_linear_desc d_rule;
  if (shape == 3 && !roles_form) {             // (the role-split knobs of reserved[3] mean nothing to the other shapes)
    d_rule = *d;
    d_rule.reserved[2] = 0;
    d_rule.reserved[3] = 0;
    d = &d_rule;
    shape = 0;
  }
  if (shape == 3) {
    if (d->reserved[3] < 0 || d->reserved[3] > 4) return BEVMSDA_ERR_BAD_OPTION;
    const int knob = d->reserved[3] == 0 ? (kPanelRolesNtStores ? 2 : 0) : d->reserved[3] & 3;
    const long long nb3 = (d->M + 63) / 64;
    if (nb3 >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
    const dim3 g3(static_cast<unsigned>(nb3)), b3(bevmsda::kRolesThreads);
    hipStream_t st3 = static_cast<hipStream_t>(stream);
    if (need) {
      if (d->precision == 0) hipLaunchKernelGGL((bevmsda::linear_roles_kernel<3, kPanelRolesNtStores ? 2 : 0, true, true>), g3, b3, 0, st3, a);
      else hipLaunchKernelGGL((bevmsda::linear_roles_kernel<1, kPanelRolesNtStores ? 2 : 0, true, true>), g3, b3, 0, st3, a);
      return launch_status();
    }
#define BEVMSDA_ROLES(NP_)                                                                                                \
    do {                                                                                                                  \
      switch (knob) {                                                                                                     \
        case 0: hipLaunchKernelGGL((bevmsda::linear_roles_kernel<NP_, 0, true>), g3, b3, 0, st3, a); break;               \
        case 1: hipLaunchKernelGGL((bevmsda::linear_roles_kernel<NP_, 0, false>), g3, b3, 0, st3, a); break;              \
        case 2: hipLaunchKernelGGL((bevmsda::linear_roles_kernel<NP_, 2, true>), g3, b3, 0, st3, a); break;               \
        default: hipLaunchKernelGGL((bevmsda::linear_roles_kernel<NP_, 2, false>), g3, b3, 0, st3, a); break;             \
      }                                                                                                                   \
    } while (0)
    if (d->precision == 0) BEVMSDA_ROLES(3); else BEVMSDA_ROLES(1);
#undef BEVMSDA_ROLES
    return launch_status();
  }
  if (d->reserved[3] != 0) return BEVMSDA_ERR_BAD_OPTION;
  if (shape == 0) shape = d->N >= 1024 && d->M >= 65536 ? 2 : 1;
  const int bm = shape == 1 ? 64 : 128;
  const long long nb = (d->M + bm - 1) / bm;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // one workgroup per row panel (a persistent grid was measured in round 5 and changed nothing: linear_panel.h)
  const dim3 grid(static_cast<unsigned>(nb));
  const int pre = idx ? 2 : (a.a0 || a.a1) ? 1 : 0;
  const bool masked = need != nullptr;         // (plain, one pass: checked above)
  if (d->precision == 0) {
    if (ln) panel_dispatch<3, true>(shape, pre, masked, grid, st, a); else panel_dispatch<3, false>(shape, pre, masked, grid, st, a);
  } else {
    if (ln) panel_dispatch<1, true>(shape, pre, masked, grid, st, a); else panel_dispatch<1, false>(shape, pre, masked, grid, st, a);
  }
  return launch_status();
}

int bevmsda_linear_panel_f32(const float *x0, const float *a0, const float *x1, const float *a1, const int32_t *idx,
                             const float *scale, const uint16_t *wpanel, const float *bias,
                             const bevmsda_linear_desc *d, const bevmsda_layernorm_desc *ln, float *y, void *stream) {
  return panel_launch(x0, a0, x1, a1, idx, scale, wpanel, bias, d, ln, y, stream, nullptr, 0, nullptr, 0);
}

int bevmsda_linear_panel_segments_f32(const float *x0, const uint16_t *wpanel, const float *bias, const bevmsda_linear_desc *d,
                                      const int32_t *seg_start, int64_t seg_len, const int64_t *level_shapes,
                                      int num_levels, float *y, void *stream) {
  if (!seg_start) return BEVMSDA_ERR_NULL_POINTER;
  return panel_launch(x0, nullptr, nullptr, nullptr, nullptr, nullptr, wpanel, bias, d, nullptr, y, stream, seg_start, seg_len,
                      level_shapes, num_levels);
}

int bevmsda_linear_panel_rows2_f32(const float *x_lo, const float *x_hi, int64_t m_split, const uint16_t *wpanel, const float *bias,
                                   const bevmsda_linear_desc *d, float *y, void *stream) {
  if (!x_hi) return BEVMSDA_ERR_NULL_POINTER;
  return panel_launch(x_lo, nullptr, nullptr, nullptr, nullptr, nullptr, wpanel, bias, d, nullptr, y, stream, nullptr, 0, nullptr, 0,
                      x_hi, m_split);
}

int bevmsda_linear_panel_rows2_masked_f32(const float *x_lo, const float *x_hi, int64_t m_split, const uint16_t *wpanel,
                                          const float *bias, const bevmsda_linear_desc *d, const int32_t *need, int64_t need_rows,
                                          int64_t need_len, float *y, void *stream) {
  if (!x_hi || !need) return BEVMSDA_ERR_NULL_POINTER;
  return panel_launch(x_lo, nullptr, nullptr, nullptr, nullptr, nullptr, wpanel, bias, d, nullptr, y, stream, nullptr, 0, nullptr, 0,
                      x_hi, m_split, need, need_rows, need_len);
}

}  // extern "C"
