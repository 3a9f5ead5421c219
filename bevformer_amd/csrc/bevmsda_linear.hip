// C ABI of libbevmsda.so, dense projections (declared in include/bevmsda.h): argument checks and
// launches of the MFMA projection kernels (linear_mfma.h, linear_pipe.h, linear_panel.h, wgrad_mfma.h), of the decoder's self-attention core (mha_d32.h) and of the detection head (head_branch.h, head_decode.h) and its loss (det_cost.h, match_lsap.h, det_loss.h), of the optimizer step (optim.h) and of the channel-last convolutions (conv3x3.h, conv_rows.h, deform_conv.h over conv_mfma.h).  No torch, no allocation, no global state.
#include "../../include/bevmsda.h"
#include "linear_mfma.h"
#include "linear_pipe.h"
#include "linear_panel.h"
#include "linear_roles.h"
#include "linear_chain.h"
#include "wgrad_mfma.h"
#include "wgrad_tr.h"
#include "mha_d32.h"
#include "head_branch.h"
#include "head_decode.h"
#include "det_cost.h"
#include "match_lsap.h"
#include "det_loss.h"
#include "optim.h"
#include "conv3x3.h"
#include "conv_rows.h"
#include "deform_conv.h"

namespace {
constexpr bool kLinearPipeDefault = false;       // linear_pipe.h (software-pipelined) as the default where it applies
constexpr long long kLinearPipeMaxRows = 8192;   // ... and always for M <= this
// linear_chain.h workgroup shape by measurement (tools/chain_small_m.py, profiles/r3): 32-row panels up to this many
// rows (a rank's tile of a BEV-tiled frame: 5,000 rows 20 vs 28 us), 64-row panels above (40,000 rows: 103 vs 103-110 us,
// half the weight traffic from L2)
constexpr long long kChainSmallRows = 8192;
inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

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
      (reinterpret_cast<uintptr_t>(y) & 3u) != 0 || (a0 && misaligned(a0)) ||
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
    const long long nbm = (d->M + 63) / 64, nbn = (d->N + 255) / 256;
    const long long grid = ((nbm + 7) / 8) * 8 * nbn;
    if (grid >= (1LL << 31) || nbm >= (1LL << 28)) return BEVMSDA_ERR_TOO_LARGE;
    a.nblk_m = static_cast<int>(nbm);
    a.nblk_n = static_cast<int>(nbn);
    const dim3 g(static_cast<unsigned>(grid)), b(256);
    if (d->precision == 0) {
      if (add) hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<3, true, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
      else hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<3, false, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
    } else {
      if (add) hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<1, true, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
      else hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<1, false, 32, true, 3, 256, false, 64>), g, b, 0, st, a);
    }
    return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
  }
  // software-pipelined kernel (linear_pipe.h)
  {
    const int nch = (d->K0 + d->K1) / 32;
    const bool covered = wpack && !add && !a.accum && !mask && (d->N % 4) == 0 && (d->ldy % 4) == 0 && (gcols % 4) == 0 && !misaligned(y) &&
                         (!bias || !misaligned(bias)) && (!d->out_bf16 || (reinterpret_cast<uintptr_t>(y) & 7u) == 0) &&
                         (nch == 8 || nch == 16);
    if (d->variant == 131 && !covered) return BEVMSDA_ERR_UNSUPPORTED;
    // default for tile-sized row counts (a rank's share of a BEV-tiled frame: one workgroup per CU, where its two-chunk
    // lead is worth 8-13 %: profiles/r2/r2_gemm_small_m.txt); at base size the first kernel's 4 workgroups per CU win
    if (covered && (d->variant == 131 || (d->variant == 0 && d->reserved[1] == 0 && (kLinearPipeDefault || d->M <= kLinearPipeMaxRows)))) {
      const long long nbm = (d->M + 127) / 128, nbn = (d->N + 127) / 128;
      const long long grid = ((nbm + 7) / 8) * 8 * nbn;
      if (grid >= (1LL << 31) || nbm >= (1LL << 28)) return BEVMSDA_ERR_TOO_LARGE;
      a.nblk_m = static_cast<int>(nbm);
      a.nblk_n = static_cast<int>(nbn);
#define BEVMSDA_PIPE(NP_, NCH_)                                                                                       \
  do {                                                                                                                \
    auto kern = bevmsda::linear_pipe_kernel<NP_, NCH_>;                                                               \
    const int dyn = 2 * ((NP_) == 3 ? 2 : 1) * bevmsda::kPipePlane * 2;                                               \
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, dyn) != \
        hipSuccess) return BEVMSDA_ERR_LAUNCH;                                                                        \
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(256), dyn, st, a);                               \
  } while (0)
      if (d->precision == 0) { if (nch == 8) BEVMSDA_PIPE(3, 8); else BEVMSDA_PIPE(3, 16); }
      else { if (nch == 8) BEVMSDA_PIPE(1, 8); else BEVMSDA_PIPE(1, 16); }
#undef BEVMSDA_PIPE
      return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
    }
  }
  if ((d->variant == 1 && wpack) || (d->variant == 13 && !wpack)) return BEVMSDA_ERR_BAD_OPTION;
  const long long nbm = (d->M + bevmsda::kLinBM - 1) / bevmsda::kLinBM;
  const long long nbn = (d->N + bevmsda::kLinBN - 1) / bevmsda::kLinBN;
  const long long grid = ((nbm + 7) / 8) * 8 * nbn;
  if (grid >= (1LL << 31) || nbm >= (1LL << 28)) return BEVMSDA_ERR_TOO_LARGE;
  a.nblk_m = static_cast<int>(nbm);
  a.nblk_n = static_cast<int>(nbn);
  const dim3 g(static_cast<unsigned>(grid)), b(256);
  // bf16 output: the transposed-tile epilogue packs 4 consecutive columns per lane
  if (d->out_bf16 && (d->N % 4 != 0 || d->ldy % 4 != 0 || (gcols % 4) != 0 ||
                      (reinterpret_cast<uintptr_t>(y) & 7u) != 0 || (bias && misaligned(bias))))
    return BEVMSDA_ERR_UNSUPPORTED;
#define BEVMSDA_LIN(NP_, WM_)                                                                                     \
  do {                                                                                                            \
    if (add) hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<NP_, true, 32, true, WM_>), g, b, 0, st, a);    \
    else hipLaunchKernelGGL((bevmsda::linear_splitbf16_kernel<NP_, false, 32, true, WM_>), g, b, 0, st, a);       \
  } while (0)
  if (d->precision == 0) { if (wpack) BEVMSDA_LIN(3, 3); else BEVMSDA_LIN(3, 0); }
  else { if (wpack) BEVMSDA_LIN(1, 3); else BEVMSDA_LIN(1, 0); }
#undef BEVMSDA_LIN
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
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

int bevmsda_linear_wgrad_f32(const float *g, int64_t ldg, const float *x, int64_t ldx, int64_t M, int N, int K,
                             float *grad_w, int64_t ldgw, float *grad_b, int precision, void *stream) {
  if (M < 0 || N <= 0 || K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (precision != 0 && precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (N % 4 != 0 || K % 4 != 0 || ldg % 4 != 0 || ldx % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ldg < N || ldx < K || ldgw < K) return BEVMSDA_ERR_BAD_SHAPE;
  if (M == 0) return BEVMSDA_OK;
  if (!g || !x || !grad_w) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(g) || misaligned(x) || (reinterpret_cast<uintptr_t>(grad_w) & 3u) != 0) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::WgradArgs a;
  a.g = g; a.x = x; a.ldg = ldg; a.ldx = ldx; a.gw = grad_w; a.ldgw = ldgw; a.gb = grad_b; a.M = M; a.N = N; a.K = K;
  a.tiles_n = (N + 127) / 128;
  a.tiles_k = (K + 127) / 128;
  // row slices: as many workgroups as are resident at once (2 per CU), at least 128 rows each
  const long long tiles = 1LL * a.tiles_n * a.tiles_k;
  // measured (tools/wgrad_ref.py): one round of workgroups (2 per CU -> 512) beats 1.5 rounds by 6-15 % for the
  // shapes with <= 8 output tiles; the 12-tile shape (768 x 256) is 20 % faster with 768 workgroups
  long long slices = tiles >= 12 ? (768 + tiles - 1) / tiles : 512 / tiles;
  long long rows = (M + slices - 1) / slices;
  rows = ((rows + 31) / 32) * 32;
  if (rows < 128) rows = 128;
  a.rows_per_block = static_cast<int>(rows);
  slices = (M + rows - 1) / rows;
  const long long slices8 = ((slices + 7) / 8) * 8;        // the kernel deals slices to XCDs: slice = 8 i + xcd
  if (tiles * slices8 >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  const dim3 grid(static_cast<unsigned>(tiles * slices8)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (precision == 0) hipLaunchKernelGGL((bevmsda::wgrad_splitbf16_kernel<3>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((bevmsda::wgrad_splitbf16_kernel<1>), grid, block, 0, st, a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_linear_wgrad_multi_f32(const bevmsda_wgrad_problem *probs, int nprob, int64_t M, int precision, int workgroups,
                                   int variant, void *stream) {
  if (variant != 0 && variant != 1 && variant != 2) return BEVMSDA_ERR_BAD_OPTION;
  if (nprob < 0 || nprob > bevmsda::kWgMaxProblems || M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (precision != 0 && precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (nprob == 0 || M == 0) return BEVMSDA_OK;
  if (!probs) return BEVMSDA_ERR_NULL_POINTER;
  if (variant == 2 && workgroups == 0) {
    // the 256 x 128 shape runs ONE 512-thread workgroup per CU, slices dealt to the XCDs in eights: it is taken when
    // tiles x 8 k workgroups fill at least 208 of the 256 CUs in one round (the grouped value projections, 12 tiles ->
    // 192 workgroups, stay on the 128 x 128 shape: 553 vs 538 us)
    long long t2 = 0;
    for (int i = 0; i < nprob; ++i) t2 += 1LL * ((probs[i].N + 255) / 256) * ((probs[i].K + 127) / 128);
    const long long s2 = t2 > 0 ? (256 / t2 / 8) * 8 : 0;
    if (s2 < 8 || t2 * s2 < 208) variant = 0;
  }
  bevmsda::WgradMultiArgs a{};
  long long tiles = 0;
  for (int i = 0; i < nprob; ++i) {
    const bevmsda_wgrad_problem &q = probs[i];
    if (q.N <= 0 || q.K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
    if (q.N % 4 != 0 || q.K % 4 != 0 || q.ldg % 4 != 0 || q.ldx % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
    if (q.ldg < q.N || q.ldx < q.K || q.ldgw < q.K) return BEVMSDA_ERR_BAD_SHAPE;
    if (!q.g || !q.x || !q.grad_w) return BEVMSDA_ERR_NULL_POINTER;
    if (misaligned(q.g) || misaligned(q.x) || (reinterpret_cast<uintptr_t>(q.grad_w) & 3u) != 0) return BEVMSDA_ERR_MISALIGNED;
    bevmsda::WgradArgs &w = a.p[i];
    w.g = q.g; w.x = q.x; w.ldg = q.ldg; w.ldx = q.ldx; w.gw = q.grad_w; w.ldgw = q.ldgw; w.gb = q.grad_b; w.M = M;
    // variant 2 (wgrad_tr.h, third shape): 256 x 128 output tiles
    w.N = q.N; w.K = q.K; w.tiles_n = (q.N + (variant == 2 ? 255 : 127)) / (variant == 2 ? 256 : 128); w.tiles_k = (q.K + 127) / 128;
    a.tile0[i] = static_cast<int>(tiles);
    tiles += 1LL * w.tiles_n * w.tiles_k;
  }
  if (tiles >= (1LL << 20)) return BEVMSDA_ERR_TOO_LARGE;
  a.tile0[nprob] = static_cast<int>(tiles);
  a.nprob = nprob;
  // one round of workgroups (2 per CU) over all tiles; 1.5 rounds from 12 tiles on (the single-problem policy);
  // `workgroups` > 0: the caller's target instead (benchmark sweeps)
  if (workgroups < 0 || workgroups > (1 << 20)) return BEVMSDA_ERR_BAD_OPTION;
  long long slices = workgroups > 0 ? workgroups / tiles : (tiles >= 12 ? (768 + tiles - 1) / tiles : 512 / tiles);
  if (variant == 2 && workgroups == 0) {
    // one 512-thread workgroup per CU and slices dealt to the XCDs in eights: the largest grid of tiles x 8 k workgroups
    // that still fits ONE round of 256 (a 257th workgroup costs a whole second round: 2.85 ms per step at 192 workgroups
    // against 3.81 at "256" = 288 launched, profiles/r6/r6e_wgrad_256x128_sweep.txt)
    slices = (256 / tiles / 8) * 8;
    if (slices < 8) slices = 8;
  }
  if (slices < 1) slices = 1;
  long long rows = (M + slices - 1) / slices;
  rows = ((rows + 31) / 32) * 32;
  if (rows < 128) rows = 128;
  slices = (M + rows - 1) / rows;
  for (int i = 0; i < nprob; ++i) a.p[i].rows_per_block = static_cast<int>(rows);
  const long long slices8 = ((slices + 7) / 8) * 8;
  if (tiles * slices8 >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  const dim3 grid(static_cast<unsigned>(tiles * slices8)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // variant 0: bf16 planes + transposing LDS reads (wgrad_tr.h); 1: fp32 tiles + gathered fragments (wgrad_mfma.h);
  // 2: 256 x 128 tiles, eight wavefronts, two LDS stages (wgrad_tr.h)
  if (variant == 2) {
    if (precision == 0) hipLaunchKernelGGL((bevmsda::wgrad_tr2_multi_kernel<3>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((bevmsda::wgrad_tr2_multi_kernel<1>), grid, dim3(512), 0, st, a);
  } else if (variant == 0) {
    if (precision == 0) hipLaunchKernelGGL((bevmsda::wgrad_tr_multi_kernel<3>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::wgrad_tr_multi_kernel<1>), grid, block, 0, st, a);
  } else {
    if (precision == 0) hipLaunchKernelGGL((bevmsda::wgrad_multi_kernel<3>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::wgrad_multi_kernel<1>), grid, block, 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
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
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_linear_pack_weight_t_f32(const float *wt, int64_t ldwt, int N, int K, uint16_t *blob, void *stream) {
  if (N <= 0 || K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (K % 32 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ldwt < N) return BEVMSDA_ERR_BAD_SHAPE;
  if (!wt || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(blob) || (reinterpret_cast<uintptr_t>(wt) & 3u)) return BEVMSDA_ERR_MISALIGNED;
  const long long threads = static_cast<long long>((N + 127) / 128) * 128 * (K / 8);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::lin_pack_weight_kernel<true>, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), wt, static_cast<long>(ldwt), N, K, blob);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
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
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_linear_panel_pack_weight_t_f32(const float *wt, int64_t ldwt, int N, int K, uint16_t *blob, void *stream) {
  if (N <= 0 || K <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (K % bevmsda::kPanelK != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ldwt < N) return BEVMSDA_ERR_BAD_SHAPE;
  if (!wt || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(blob) || (reinterpret_cast<uintptr_t>(wt) & 3u)) return BEVMSDA_ERR_MISALIGNED;
  const int tiles32 = ((N + 63) / 64) * 2;
  const long long threads = 1LL * tiles32 * (K / 16) * 64;
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::lin_panel_pack_weight_kernel<true>, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), wt, static_cast<long>(ldwt), N, K, tiles32, blob);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// Many weight images in one launch (linear_panel.h: lin_pack_weights_multi_kernel).  `jobs` is a DEVICE array of `njobs`
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
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
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
    if ((reinterpret_cast<uintptr_t>(need) & 3u) != 0) return BEVMSDA_ERR_MISALIGNED;
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
      return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
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
    return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
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
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
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

// ---- row-local tail of an encoder layer in one kernel (linear_chain.h)
// the next layer's [first | y + pos] projection behind y (linear_chain.h TP; bevmsda_proj_ffn_chain_tail_f32)
struct ChainTail {
  const float *first; long long ld_first;
  const float *pos; long long ld_pos;
  const uint16_t *w3p; const float *b3;
  float *proj; long long ld_proj;
  int n3;
};

static int ffn_chain_launch(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                            const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                            const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                            const bevmsda_chain_desc *d, float *y, void *stream, bool save, float *sv_z0, float *sv_x,
                            float *sv_h, float *sv_z1, const float *dk0 = nullptr, const float *dkh = nullptr,
                            const float *dk1 = nullptr, const ChainTail *tp = nullptr) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  const bool drop = dk0 || dkh || dk1;
  if (tp) {
    if (save || drop) return BEVMSDA_ERR_BAD_OPTION;
    if (tp->n3 <= 0 || tp->n3 > 256 || tp->n3 % 64 != 0) return BEVMSDA_ERR_UNSUPPORTED;      // (whole tiles of both workgroup shapes)
    if (d->M > 0 && (!tp->first || !tp->w3p || !tp->proj)) return BEVMSDA_ERR_NULL_POINTER;
    if (tp->ld_first % 4 != 0 || tp->ld_proj % 4 != 0 || (tp->pos && tp->ld_pos % 4 != 0)) return BEVMSDA_ERR_UNSUPPORTED;
    if (tp->ld_first < 256 || tp->ld_proj < tp->n3 || (tp->pos && tp->ld_pos < 256)) return BEVMSDA_ERR_BAD_SHAPE;
    if (misaligned(tp->first) || misaligned(tp->w3p) || misaligned(tp->proj) || (tp->pos && misaligned(tp->pos)) ||
        (tp->b3 && misaligned(tp->b3)))
      return BEVMSDA_ERR_MISALIGNED;
  }
  if (drop && !save) return BEVMSDA_ERR_BAD_OPTION;
  if ((dk0 && misaligned(dk0)) || (dkh && misaligned(dkh)) || (dk1 && misaligned(dk1))) return BEVMSDA_ERR_MISALIGNED;
  if (save && d->M > 0 && (!sv_z0 || !sv_x || !sv_h || !sv_z1)) return BEVMSDA_ERR_NULL_POINTER;
  if (save && (misaligned(sv_z0) || misaligned(sv_x) || misaligned(sv_h) || misaligned(sv_z1))) return BEVMSDA_ERR_MISALIGNED;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->C != bevmsda::kChainC || d->F != bevmsda::kChainF) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!rows || !w0p || !w1p || !w2p || !gamma0 || !beta0 || !gamma1 || !beta1 || !y) return BEVMSDA_ERR_NULL_POINTER;
  if ((idx == nullptr) != (scale == nullptr)) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_rows % 4 != 0 || d->ld_y % 4 != 0 || (res && d->ld_res % 4 != 0)) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->ld_rows < d->C || d->ld_y < d->C || (res && d->ld_res < d->C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(rows) || misaligned(w0p) || misaligned(w1p) || misaligned(w2p) || misaligned(y) || (res && misaligned(res)) ||
      (b0 && misaligned(b0)) || (b1 && misaligned(b1)) || (b2 && misaligned(b2)) || misaligned(gamma0) || misaligned(beta0) ||
      misaligned(gamma1) || misaligned(beta1))
    return BEVMSDA_ERR_MISALIGNED;
  // workgroup shape (desc->reserved[1]): 1 = 64-row panels (8 wavefronts, one workgroup per CU), 2 = 32-row panels
  // (4 wavefronts, two workgroups per CU); 0 = default
  int shape = d->reserved[1];
  if (shape < 0 || shape > 3) return BEVMSDA_ERR_BAD_OPTION;
  // desc->reserved[2]: columns of idx (0 = 2; J > 2: rows idx[m, 2..] >= 0 are added to the first row's — inference launches only)
  const int gst = d->reserved[2] == 0 ? 2 : d->reserved[2];
  if (gst < 2 || gst > 64 || (gst > 2 && (!idx || save))) return BEVMSDA_ERR_BAD_OPTION;
  // default: 32-row panels up to kChainSmallRows rows, mixed from one whole round of 64-row panels on (measured at 40,000
  // rows, interleaved runs on one box: 103.2-103.6 vs 106.6-107.2 us; profiles/r4/r4f_chain_mixed_shape_ab.txt)
  // (with the next layer's projection behind it the 32-row shape wins at every row count: two workgroups per CU cover each
  // other's fetch / split / barrier phases of the extra stage — 127 vs 140 us at 40,000 rows, base frame 4.09 vs 4.20 ms;
  // profiles/r6/r6u_seam_ab.txt)
  // (round 6, last day — at FRAME level, in a replayed graph, the inference launches are fastest as ONE launch of 32-row panels at
  // every row count: the mixed shape's isolated 3 us per launch do not pay for its second launch and the round of one workgroup
  // per CU — base frame 4.00 against 4.03 ms, bf16 2.78 against 2.81, first frame 3.94 against 4.03, small4 1.29 against 1.32,
  // queue 17.02 against 17.27; the training step too, by less: small4 bf16 4.96-4.97 against 4.98-5.00 ms, base 18.65-18.73 against
  // 18.70-18.76; profiles/r6z/r6zz_chain_shape_frame_ab.txt)
  // (between 8,192 and 16,384 rows — a tile of four ranks — one partial round of 64-row panels stays ahead: rank 1 of 4 1.61
  // against 1.66 ms)
  if (shape == 0) shape = (tp || d->M <= kChainSmallRows) ? 2 : (d->M >= 256LL * 64 ? 2 : 1);
  if (shape == 3) {
    // mixed (round 4): whole rounds of the 64-row shape (one workgroup per CU: 256 x 64 rows per round)
    // and the remainder — a partial round that would leave most CUs idle behind a few 64-row workgroups — on the 32-row
    // shape at two workgroups per CU, as a second launch over the tail rows
    const long long round64 = 256LL * 64;
    const long long head = (d->M / round64) * round64;
    const long long tail = d->M - head;
    if (head == 0 || tail == 0 || tail > 256LL * 2 * 32) {
      bevmsda_chain_desc one = *d;
      one.reserved[1] = (head == 0) ? 2 : 1;
      return ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, &one, y, stream,
                              save, sv_z0, sv_x, sv_h, sv_z1, dk0, dkh, dk1, tp);
    }
    bevmsda_chain_desc dh = *d, dt = *d;
    dh.M = head; dh.reserved[1] = 1;
    dt.M = tail; dt.reserved[1] = 2;
    int rc = ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, &dh, y, stream,
                              save, sv_z0, sv_x, sv_h, sv_z1, dk0, dkh, dk1, tp);
    if (rc != BEVMSDA_OK) return rc;
    const long long o = head;
    ChainTail tt{};
    if (tp) {
      tt = *tp;
      tt.first += o * tp->ld_first;
      if (tt.pos) tt.pos += o * tp->ld_pos;
      tt.proj += o * tp->ld_proj;
    }
    return ffn_chain_launch(idx ? rows : rows + o * d->ld_rows, idx ? idx + o * gst : nullptr, scale ? scale + o : nullptr, w0p, b0,
                            res ? res + o * d->ld_res : nullptr, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, &dt,
                            y + o * d->ld_y, stream, save, save ? sv_z0 + o * 256 : nullptr, save ? sv_x + o * 256 : nullptr,
                            save ? sv_h + o * 512 : nullptr, save ? sv_z1 + o * 256 : nullptr, dk0 ? dk0 + o * 256 : nullptr,
                            dkh ? dkh + o * 512 : nullptr, dk1 ? dk1 + o * 256 : nullptr, tp ? &tt : nullptr);
  }
  const int bm = shape == 1 ? 64 : 32;
  const long long nb = (d->M + bm - 1) / bm;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  a.rows = rows; a.ld_rows = d->ld_rows; a.gidx = idx; a.gscale = scale; a.gstride = gst;
  a.w0 = w0p; a.w1 = w1p; a.w2 = w2p; a.b0 = b0; a.b1 = b1; a.b2 = b2;
  a.res = res; a.ld_res = d->ld_res; a.gamma0 = gamma0; a.beta0 = beta0; a.gamma1 = gamma1; a.beta1 = beta1;
  a.eps0 = d->eps0; a.eps1 = d->eps1; a.y = y; a.ld_y = d->ld_y; a.M = d->M;
  a.sv_z0 = sv_z0; a.sv_x = sv_x; a.sv_h = sv_h; a.sv_z1 = sv_z1;
  a.dk0 = dk0; a.dkh = dkh; a.dk1 = dk1;
  if (tp) {
    a.tp_first = tp->first; a.ld_tp_first = tp->ld_first; a.tp_pos = tp->pos; a.ld_tp_pos = tp->ld_pos;
    a.w3 = tp->w3p; a.b3 = tp->b3; a.y3 = tp->proj; a.ld_y3 = tp->ld_proj; a.N3 = tp->n3;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
#define BEVMSDA_CHAIN_TP(NP_, PRE_)                                                                                               \
  do {                                                                                                                            \
    if (shape == 1) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 2, 1, 8, false, false, true>), grid, dim3(512), 0, st, a); \
    else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 1, 2, 4, false, false, true>), grid, dim3(256), 0, st, a);            \
  } while (0)
  if (tp) {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN_TP(3, 2); else BEVMSDA_CHAIN_TP(3, 0); }
    else { if (idx) BEVMSDA_CHAIN_TP(1, 2); else BEVMSDA_CHAIN_TP(1, 0); }
    return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
  }
#undef BEVMSDA_CHAIN_TP
#define BEVMSDA_CHAIN(NP_, PRE_, SV_, DR_)                                                                                        \
  do {                                                                                                                            \
    if (shape == 1) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 2, 1, 8, SV_, DR_>), grid, dim3(512), 0, st, a); \
    else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 1, 2, 4, SV_, DR_>), grid, dim3(256), 0, st, a);            \
  } while (0)
  if (drop) {                                  // (train() mode with active dropout: the gather form only)
    if (!idx) return BEVMSDA_ERR_UNSUPPORTED;
    if (d->precision == 0) BEVMSDA_CHAIN(3, 2, true, true); else BEVMSDA_CHAIN(1, 2, true, true);
  } else if (save) {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN(3, 2, true, false); else BEVMSDA_CHAIN(3, 0, true, false); }
    else { if (idx) BEVMSDA_CHAIN(1, 2, true, false); else BEVMSDA_CHAIN(1, 0, true, false); }
  } else {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN(3, 2, false, false); else BEVMSDA_CHAIN(3, 0, false, false); }
    else { if (idx) BEVMSDA_CHAIN(1, 2, false, false); else BEVMSDA_CHAIN(1, 0, false, false); }
  }
#undef BEVMSDA_CHAIN
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_proj_ffn_chain_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                               const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                               const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                               const bevmsda_chain_desc *d, float *y, void *stream) {
  return ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, d, y, stream, false,
                          nullptr, nullptr, nullptr, nullptr);
}

int bevmsda_proj_ffn_chain_tail_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                    const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                    const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                                    const bevmsda_chain_desc *d, float *y, const float *first, int64_t ld_first,
                                    const float *pos, int64_t ld_pos, const uint16_t *w3p, const float *b3, int n3,
                                    float *proj_out, int64_t ld_proj, void *stream) {
  const ChainTail tp{first, ld_first, pos, ld_pos, w3p, b3, proj_out, ld_proj, n3};
  return ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, d, y, stream, false,
                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &tp);
}

int bevmsda_proj_ffn_chain_train_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                     const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p,
                                     const float *b1, const uint16_t *w2p, const float *b2, const float *gamma1,
                                     const float *beta1, const bevmsda_chain_desc *d, float *y, float *save_z0, float *save_x,
                                     float *save_h, float *save_z1, const float *drop0, const float *droph,
                                     const float *drop1, void *stream) {
  return ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, d, y, stream, true,
                          save_z0, save_x, save_h, save_z1, drop0, droph, drop1);
}

// ---- backward of the projection + FFN chain (linear_chain.h, MODE 2)
int bevmsda_proj_ffn_chain_backward_f32(const float *grad_y, int64_t ld_grad_y, const float *save_z0, const float *save_h,
                                        const float *save_z1, const float *gamma0, const float *gamma1, const uint16_t *w0t_p,
                                        const uint16_t *w1t_p, const uint16_t *w2t_p, const bevmsda_chain_desc *d, float *grad_z1,
                                        float *grad_h, float *grad_z0, float *grad_in, float *grad_gamma_beta1,
                                        float *grad_gamma_beta0, const float *drop0, const float *drop1, float hidden_scale,
                                        float *grad_zp, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->C != bevmsda::kChainC || d->F != bevmsda::kChainF) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!grad_y || !save_z0 || !save_h || !save_z1 || !gamma0 || !gamma1 || !w0t_p || !w1t_p || !w2t_p || !grad_z1 || !grad_h ||
      !grad_z0 || !grad_in || !grad_gamma_beta1 || !grad_gamma_beta0)
    return BEVMSDA_ERR_NULL_POINTER;
  if (ld_grad_y % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ld_grad_y < d->C) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(grad_y) || misaligned(save_z0) || misaligned(save_h) || misaligned(save_z1) || misaligned(gamma0) ||
      misaligned(gamma1) || misaligned(w0t_p) || misaligned(w1t_p) || misaligned(w2t_p) || misaligned(grad_z1) ||
      misaligned(grad_h) || misaligned(grad_z0) || misaligned(grad_in) || (reinterpret_cast<uintptr_t>(grad_gamma_beta1) & 3u) ||
      (reinterpret_cast<uintptr_t>(grad_gamma_beta0) & 3u))
    return BEVMSDA_ERR_MISALIGNED;
  const long long nb = (d->M + 31) / 32;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  // the three GEMMs of the backward read the images of the TRANSPOSED weights in the slots of the forward's: stage "0" =
  // gz0 W0 (256 x 256), stage "1" = gz1 W2 (512 columns, K = 256), stage "2" = gh W1 (256 columns, K = 512)
  a.w0 = w0t_p; a.w1 = w2t_p; a.w2 = w1t_p;
  a.gamma0 = gamma0; a.gamma1 = gamma1; a.eps0 = d->eps0; a.eps1 = d->eps1; a.M = d->M;
  a.bw_gy = grad_y; a.bw_ld_gy = ld_grad_y; a.bw_z1 = save_z1; a.bw_h = save_h; a.bw_z0 = save_z0;
  a.bw_gz1 = grad_z1; a.bw_gh = grad_h; a.bw_gz0 = grad_z0; a.bw_din = grad_in;
  a.bw_dgb1 = grad_gamma_beta1; a.bw_dgb0 = grad_gamma_beta0;
  if (drop0 && !grad_zp) return BEVMSDA_ERR_NULL_POINTER;
  if ((drop0 && misaligned(drop0)) || (drop1 && misaligned(drop1)) || (grad_zp && misaligned(grad_zp))) return BEVMSDA_ERR_MISALIGNED;
  a.dk0 = drop0; a.dk1 = drop1; a.bw_hscale = hidden_scale; a.bw_gzp = grad_zp;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
  if (d->precision == 0) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<3, 0, 2, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<1, 0, 2, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- backward of the projection + LayerNorm + projection chain (linear_chain.h, MODE 3)
int bevmsda_proj_ln_proj_chain_backward_f32(const float *grad_proj, int64_t ld_grad_proj, const float *grad_x, const float *save_z0,
                                            const float *gamma0, const uint16_t *w0t_p, const uint16_t *w1t_p,
                                            const bevmsda_chain_desc *d, float *grad_z0, float *grad_in, float *grad_gamma_beta0,
                                            const float *drop0, float *grad_zp, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  const int N2 = d->reserved[0];
  if (d->C != bevmsda::kChainC || N2 <= 0 || N2 % 256 != 0 || N2 > bevmsda::kChainMaxN2) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!grad_proj || !save_z0 || !gamma0 || !w0t_p || !w1t_p || !grad_z0 || !grad_in || !grad_gamma_beta0) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_grad_proj % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ld_grad_proj < N2) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(grad_proj) || (grad_x && misaligned(grad_x)) || misaligned(save_z0) || misaligned(gamma0) || misaligned(w0t_p) ||
      misaligned(w1t_p) || misaligned(grad_z0) || misaligned(grad_in) || (reinterpret_cast<uintptr_t>(grad_gamma_beta0) & 3u))
    return BEVMSDA_ERR_MISALIGNED;
  const long long nb = (d->M + 31) / 32;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  a.w0 = w0t_p; a.w1 = w1t_p; a.N2 = N2;
  a.gamma0 = gamma0; a.eps0 = d->eps0; a.M = d->M;
  a.bw_gy = grad_proj; a.bw_ld_gy = ld_grad_proj; a.bw_z1 = grad_x; a.bw_z0 = save_z0;
  a.bw_gz0 = grad_z0; a.bw_din = grad_in; a.bw_dgb0 = grad_gamma_beta0;
  if (drop0 && !grad_zp) return BEVMSDA_ERR_NULL_POINTER;
  if ((drop0 && misaligned(drop0)) || (grad_zp && misaligned(grad_zp))) return BEVMSDA_ERR_MISALIGNED;
  a.dk0 = drop0; a.bw_gzp = grad_zp; a.bw_hscale = 1.f;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
  if (d->precision == 0) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<3, 0, 3, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<1, 0, 3, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

static int ln_proj_chain_launch(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                const bevmsda_chain_desc *d, float *x_out, float *proj_out, void *stream, bool save,
                                float *sv_z0, const float *dk0 = nullptr) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (dk0 && (!save || misaligned(dk0))) return BEVMSDA_ERR_BAD_OPTION;
  if (save && d->M > 0 && !sv_z0) return BEVMSDA_ERR_NULL_POINTER;
  if (save && misaligned(sv_z0)) return BEVMSDA_ERR_MISALIGNED;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  const long ld_y2 = d->reserved[0];
  if (d->C != bevmsda::kChainC || d->F <= 0 || d->F % 32 != 0 || d->F > bevmsda::kChainMaxN2) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!rows || !w0p || !w1p || !gamma0 || !beta0 || !x_out || !proj_out) return BEVMSDA_ERR_NULL_POINTER;
  if ((idx == nullptr) != (scale == nullptr)) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_rows % 4 != 0 || d->ld_y % 4 != 0 || ld_y2 % 4 != 0 || (res && d->ld_res % 4 != 0)) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->ld_rows < d->C || d->ld_y < d->C || ld_y2 < d->F || (res && d->ld_res < d->C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(rows) || misaligned(w0p) || misaligned(w1p) || misaligned(x_out) || misaligned(proj_out) || (res && misaligned(res)) ||
      (b0 && misaligned(b0)) || (b1 && misaligned(b1)) || misaligned(gamma0) || misaligned(beta0))
    return BEVMSDA_ERR_MISALIGNED;
  int shape = d->reserved[1];
  if (shape < 0 || shape > 3) return BEVMSDA_ERR_BAD_OPTION;
  // (isolated: mixed 100.4-101.5 vs 103.8-105.7 us at 40,000 rows; in the frame one launch of 32-row panels wins — see ffn_chain_launch)
  if (shape == 0) shape = d->M <= kChainSmallRows ? 2 : (d->M >= 256LL * 64 ? 2 : 1);
  if (d->F % 64 != 0) shape = 1;               // the 32-row shape walks 64-column tiles
  if (shape == 3) {                            // mixed: whole rounds on the 64-row shape, the tail on the 32-row shape
    const long long round64 = 256LL * 64;
    const long long head = (d->M / round64) * round64;
    const long long tail = d->M - head;
    bevmsda_chain_desc dh = *d, dt = *d;
    if (head == 0 || tail == 0 || tail > 256LL * 2 * 32) {
      dh.reserved[1] = (head == 0) ? 2 : 1;
      return ln_proj_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, &dh, x_out, proj_out, stream, save, sv_z0,
                                  dk0);
    }
    dh.M = head; dh.reserved[1] = 1;
    dt.M = tail; dt.reserved[1] = 2;
    int rc = ln_proj_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, &dh, x_out, proj_out, stream, save, sv_z0,
                                  dk0);
    if (rc != BEVMSDA_OK) return rc;
    const long long o = head;
    return ln_proj_chain_launch(idx ? rows : rows + o * d->ld_rows, idx ? idx + o * 2 : nullptr, scale ? scale + o : nullptr, w0p,
                                b0, res ? res + o * d->ld_res : nullptr, gamma0, beta0, w1p, b1, &dt, x_out + o * d->ld_y,
                                proj_out + o * ld_y2, stream, save, save ? sv_z0 + o * 256 : nullptr,
                                dk0 ? dk0 + o * 256 : nullptr);
  }
  const int bm = shape == 1 ? 64 : 32;
  const long long nb = (d->M + bm - 1) / bm;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  a.rows = rows; a.ld_rows = d->ld_rows; a.gidx = idx; a.gscale = scale;
  a.w0 = w0p; a.w1 = w1p; a.w2 = nullptr; a.b0 = b0; a.b1 = b1; a.b2 = nullptr;
  a.res = res; a.ld_res = d->ld_res; a.gamma0 = gamma0; a.beta0 = beta0; a.gamma1 = a.beta1 = nullptr;
  a.eps0 = d->eps0; a.eps1 = 0.f; a.y = x_out; a.ld_y = d->ld_y; a.M = d->M; a.y2 = proj_out; a.ld_y2 = ld_y2; a.N2 = d->F;
  a.sv_z0 = sv_z0;
  a.dk0 = dk0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
#define BEVMSDA_CHAIN(NP_, PRE_, SV_, DR_)                                                                                        \
  do {                                                                                                                            \
    if (shape == 1) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 1, 2, 1, 8, SV_, DR_>), grid, dim3(512), 0, st, a); \
    else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 1, 1, 2, 4, SV_, DR_>), grid, dim3(256), 0, st, a);            \
  } while (0)
  if (save) {                                  // (the autograd path's forward has no gather prepass: plain rows only)
    if (idx) return BEVMSDA_ERR_UNSUPPORTED;
    if (dk0) { if (d->precision == 0) BEVMSDA_CHAIN(3, 0, true, true); else BEVMSDA_CHAIN(1, 0, true, true); }
    else { if (d->precision == 0) BEVMSDA_CHAIN(3, 0, true, false); else BEVMSDA_CHAIN(1, 0, true, false); }
  } else {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN(3, 2, false, false); else BEVMSDA_CHAIN(3, 0, false, false); }
    else { if (idx) BEVMSDA_CHAIN(1, 2, false, false); else BEVMSDA_CHAIN(1, 0, false, false); }
  }
#undef BEVMSDA_CHAIN
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_proj_ln_proj_chain_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                   const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                   const bevmsda_chain_desc *d, float *x_out, float *proj_out, void *stream) {
  return ln_proj_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, d, x_out, proj_out, stream, false, nullptr);
}

int bevmsda_proj_ln_proj_chain_train_f32(const float *rows, const uint16_t *w0p, const float *b0, const float *res,
                                         const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                         const bevmsda_chain_desc *d, float *x_out, float *proj_out, float *save_z0,
                                         const float *drop0, void *stream) {
  return ln_proj_chain_launch(rows, nullptr, nullptr, w0p, b0, res, gamma0, beta0, w1p, b1, d, x_out, proj_out, stream, true,
                              save_z0, drop0);
}

int bevmsda_mha_d32_f32(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, int nq, int nk,
                        int bs, int heads, int D, float scale, float *out, int64_t ldo, void *stream) {
  if (nq < 0 || nk < 0 || bs < 0 || heads < 0 || D < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (D != bevmsda::kMhaD) return BEVMSDA_ERR_UNSUPPORTED;
  if (nq == 0 || bs == 0 || heads == 0) return BEVMSDA_OK;
  if (nk == 0) return BEVMSDA_ERR_BAD_SHAPE;                     // a softmax over no keys
  if (!q || !k || !v || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (ldq % 4 != 0 || ldk % 4 != 0 || ldv % 4 != 0 || ldo % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  const int64_t width = static_cast<int64_t>(heads) * bevmsda::kMhaD;
  if (ldq < width || ldk < width || ldv < width || ldo < width) return BEVMSDA_ERR_BAD_SHAPE;
  if (heads > 65535 || bs > 65535) return BEVMSDA_ERR_TOO_LARGE;  // grid y / z
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(out)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::MhaArgs a;
  a.q = q; a.k = k; a.v = v; a.o = out;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.nq = nq; a.nk = nk; a.bs = bs; a.scale = scale;
  const dim3 grid((nq + bevmsda::kMhaBQ - 1) / bevmsda::kMhaBQ, heads, bs), block(bevmsda::kMhaWaves * 64);
  hipLaunchKernelGGL(bevmsda::mha_d32_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- detection head (head_branch.h, head_decode.h): argument checks and launches

static int head_branch_table(const bevmsda_head_branch *src, int n, bool norms, bevmsda::HeadBranchW *dst) {
  for (int l = 0; l < n; ++l) {
    const bevmsda_head_branch &s = src[l];
    if (!s.w1 || !s.w2 || !s.w3 || !s.b1 || !s.b2 || !s.b3) return BEVMSDA_ERR_NULL_POINTER;
    if (norms && (!s.gamma1 || !s.beta1 || !s.gamma2 || !s.beta2)) return BEVMSDA_ERR_NULL_POINTER;
    if (misaligned(s.w1) || misaligned(s.w2) || misaligned(s.w3) || misaligned(s.b1) || misaligned(s.b2) ||
        (reinterpret_cast<uintptr_t>(s.b3) & 3u))
      return BEVMSDA_ERR_MISALIGNED;
    if (norms && (misaligned(s.gamma1) || misaligned(s.beta1) || misaligned(s.gamma2) || misaligned(s.beta2)))
      return BEVMSDA_ERR_MISALIGNED;
    bevmsda::HeadBranchW &d = dst[l];
    d.w1 = s.w1; d.w2 = s.w2; d.w3 = s.w3;
    d.b1 = s.b1; d.b2 = s.b2; d.b3 = s.b3;
    d.g1 = s.gamma1; d.be1 = s.beta1; d.g2 = s.gamma2; d.be2 = s.beta2;
    d.eps1 = s.eps1; d.eps2 = s.eps2;
  }
  return BEVMSDA_OK;
}

int bevmsda_head_branches_f32(const float *x, const float *ref, const bevmsda_head_branch *reg, const bevmsda_head_branch *cls,
                              const bevmsda_head_desc *d, float *out_box, float *out_cls, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->mode != BEVMSDA_HEAD_MODE_HEAD && d->mode != BEVMSDA_HEAD_MODE_REFINE) return BEVMSDA_ERR_BAD_OPTION;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->layer_stride != 0 && d->layer_stride != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->L < 0 || d->nq < 0 || d->bs < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->L > BEVMSDA_HEAD_MAX_LAYERS || (d->mode == BEVMSDA_HEAD_MODE_REFINE && d->L > 1)) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  const bool with_cls = d->mode == BEVMSDA_HEAD_MODE_HEAD;
  if (with_cls && (d->cls_out < 1 || d->cls_out > 32)) return BEVMSDA_ERR_BAD_SHAPE;
  const long long M = 1LL * d->nq * d->bs;
  if (M > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;
  if (d->L == 0 || M == 0) return BEVMSDA_OK;
  if (!x || !ref || !reg || !out_box || (with_cls && (!cls || !out_cls))) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_x < 256 || (d->L > 1 && d->ld_layer < M * d->ld_x)) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_x % 4 != 0 || d->ld_layer % 4 != 0) return BEVMSDA_ERR_MISALIGNED;       // rows must start on 16 bytes (LDS-DMA)
  if (misaligned(x) || (reinterpret_cast<uintptr_t>(ref) & 3u) || (reinterpret_cast<uintptr_t>(out_box) & 3u) ||
      (with_cls && (reinterpret_cast<uintptr_t>(out_cls) & 3u)))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::HeadArgs a = {};
  const int ntab = d->layer_stride == 0 ? 1 : d->L;
  int rc = head_branch_table(reg, ntab, false, a.reg);
  if (rc != BEVMSDA_OK) return rc;
  if (with_cls) {
    rc = head_branch_table(cls, ntab, true, a.cls);
    if (rc != BEVMSDA_OK) return rc;
  }
  a.x = x; a.ld_x = d->ld_x; a.ld_layer = d->ld_layer;
  a.ref = ref; a.out_box = out_box; a.out_cls = out_cls;
  a.nq = d->nq; a.bs = d->bs; a.code_size = d->code_size; a.cls_out = with_cls ? d->cls_out : 0;
  a.mode = d->mode; a.layer_stride = d->layer_stride;
  for (int i = 0; i < 3; ++i) {
    // the reference scales by the Python (double) difference pc_range[3 + i] - pc_range[i], rounded to fp32 by the multiply
    a.pc[i] = static_cast<float>(d->pc_range[i]);
    a.pc[3 + i] = static_cast<float>(d->pc_range[3 + i] - d->pc_range[i]);
  }
  const dim3 grid(static_cast<unsigned>((M + 31) / 32), d->L, with_cls ? 2 : 1), block(256);
  if (d->precision == 0) hipLaunchKernelGGL(bevmsda::head_branch_kernel<3>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(bevmsda::head_branch_kernel<1>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_nms_free_decode_f32(const float *cls, const float *box, const bevmsda_decode_desc *d,
                                float *scores, int64_t *labels, float *boxes, uint8_t *keep, int32_t *count, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->bs < 0 || d->nq < 0 || d->num_classes < 0 || d->max_num < 0 || d->n_ladder < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->bs > 65535) return BEVMSDA_ERR_TOO_LARGE;
  const long long n = 1LL * d->nq * d->num_classes;
  if (n > bevmsda::kDecodeMaxScores || d->max_num > bevmsda::kDecodeMaxNum || d->n_ladder > bevmsda::kDecodeMaxLadder)
    return BEVMSDA_ERR_TOO_LARGE;
  if (d->max_num > n) return BEVMSDA_ERR_BAD_SHAPE;               // as torch.topk: k out of range
  if (d->bs == 0) return BEVMSDA_OK;
  if (!count) return BEVMSDA_ERR_NULL_POINTER;
  if (d->max_num > 0 && (!cls || !box || !scores || !labels || !boxes || !keep)) return BEVMSDA_ERR_NULL_POINTER;
  if ((reinterpret_cast<uintptr_t>(cls) & 3u) || (reinterpret_cast<uintptr_t>(box) & 3u) || (reinterpret_cast<uintptr_t>(scores) & 3u) ||
      (reinterpret_cast<uintptr_t>(labels) & 7u) || (reinterpret_cast<uintptr_t>(boxes) & 3u) ||
      (reinterpret_cast<uintptr_t>(count) & 3u))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DecodeArgs a = {};
  a.cls = cls; a.box = box; a.n_ladder = d->n_ladder;
  for (int i = 0; i < d->n_ladder; ++i) a.ladder[i] = d->ladder[i];
  a.nq = d->nq; a.C = d->num_classes; a.code_size = d->code_size; a.max_num = d->max_num;
  for (int i = 0; i < 6; ++i) a.range[i] = d->post_center_range[i];
  a.scores = scores; a.labels = reinterpret_cast<long long *>(labels); a.boxes = boxes; a.keep = keep; a.count = count;
  const dim3 grid(d->bs);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n <= 2048) hipLaunchKernelGGL((bevmsda::nms_free_decode_kernel<2048, 256>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::nms_free_decode_kernel<16384, 1024>), grid, dim3(1024), 0, st, a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- detection loss (det_cost.h, match_lsap.h, det_loss.h): argument checks and launches

static inline bool off4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

static int loss_desc_check(const bevmsda_loss_desc *d) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->L < 0 || d->bs < 0 || d->nq < 0 || d->gmax < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->cls_out < 1 || d->cls_out > bevmsda::kLossMaxCls) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->nq > bevmsda::kLossMaxQueries || d->gmax > bevmsda::kLossMaxGt) return BEVMSDA_ERR_TOO_LARGE;
  if (1LL * d->L * d->bs > 65535) return BEVMSDA_ERR_TOO_LARGE;
  return BEVMSDA_OK;
}

int bevmsda_match_cost_f32(const float *cls, const float *box, const float *gt, const int32_t *label, const int32_t *count,
                           const bevmsda_loss_desc *d, float *cost, void *stream) {
  const int rc = loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0 || d->gmax == 0) return BEVMSDA_OK;
  if (!cls || !box || !gt || !label || !count || !cost) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(cost)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetCostArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.cost = cost;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.cls_weight = d->cost_cls_weight; a.reg_weight = d->cost_reg_weight;
  a.alpha = d->cost_alpha; a.gamma = d->cost_gamma; a.eps = d->cost_eps;
  const dim3 grid((d->nq + 255) / 256, d->gmax, d->L * d->bs);
  hipLaunchKernelGGL(bevmsda::det_cost_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_lsap_f32(const float *cost, const int32_t *count, int P, int gmax, int nq, int32_t *match, int32_t *assigned,
                     int32_t *status, void *stream) {
  if (P < 0 || gmax < 0 || nq < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (nq > bevmsda::kLossMaxQueries || gmax > bevmsda::kLossMaxGt) return BEVMSDA_ERR_TOO_LARGE;
  if (P == 0) return BEVMSDA_OK;
  if (!count || !status || (gmax > 0 && !match) || (nq > 0 && !assigned) || (gmax > 0 && nq > 0 && !cost))
    return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cost) || off4(count) || off4(match) || off4(assigned) || off4(status)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::LsapArgs a = {};
  a.cost = cost; a.count = count; a.match = match; a.assigned = assigned; a.status = status;
  a.gmax = gmax; a.nq = nq;
  hipLaunchKernelGGL(bevmsda::lsap_kernel, dim3(P), dim3(bevmsda::kLsapThreads), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_det_loss_f32(const float *cls, const float *box, const float *gt, const int32_t *label, const int32_t *count,
                         const int32_t *assigned, const float *code_weights, const float *factors,
                         const bevmsda_loss_desc *d, float *losses, float *grad_cls, float *grad_box, void *stream) {
  const int rc = loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0) return BEVMSDA_OK;
  if (!cls || !box || !count || !assigned || !code_weights || !factors || !losses || !grad_cls || !grad_box)
    return BEVMSDA_ERR_NULL_POINTER;
  if (d->gmax > 0 && (!gt || !label)) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(assigned) || off4(code_weights) ||
      off4(factors) || off4(losses) || off4(grad_cls) || off4(grad_box))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetLossArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.assigned = assigned;
  a.code_weights = code_weights; a.factors = factors; a.losses = losses; a.grad_cls = grad_cls; a.grad_box = grad_box;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.alpha = d->loss_alpha; a.gamma = d->loss_gamma; a.cls_weight = d->loss_cls_weight; a.box_weight = d->loss_box_weight;
  hipLaunchKernelGGL(bevmsda::det_loss_kernel, dim3(d->L), dim3(bevmsda::kDetLossThreads), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- Group-DETR form of the detection loss: `groups` blocks of nq queries per sample, problem (l * bs + b) * groups + g

static int group_loss_desc_check(const bevmsda_group_loss_desc *d) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->L < 0 || d->bs < 0 || d->nq < 0 || d->gmax < 0 || d->groups < 1) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->cls_out < 1 || d->cls_out > bevmsda::kLossMaxCls) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->nq > bevmsda::kLossMaxQueries || d->gmax > bevmsda::kLossMaxGt) return BEVMSDA_ERR_TOO_LARGE;
  if (1LL * d->L * d->bs * d->groups > 65535) return BEVMSDA_ERR_TOO_LARGE;     // (the problems ride on gridDim.z)
  return BEVMSDA_OK;
}

int bevmsda_match_cost_grouped_f32(const float *cls, const float *box, const float *gt, const int32_t *label,
                                   const int32_t *count, const bevmsda_group_loss_desc *d, float *cost, void *stream) {
  const int rc = group_loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0 || d->gmax == 0) return BEVMSDA_OK;
  if (!cls || !box || !gt || !label || !count || !cost) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(cost)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetCostArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.cost = cost;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.cls_weight = d->cost_cls_weight; a.reg_weight = d->cost_reg_weight;
  a.alpha = d->cost_alpha; a.gamma = d->cost_gamma; a.eps = d->cost_eps;
  const dim3 grid((d->nq + 255) / 256, d->gmax, d->L * d->bs * d->groups);
  hipLaunchKernelGGL(bevmsda::det_cost_grouped_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a, d->groups);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_det_loss_grouped_f32(const float *cls, const float *box, const float *gt, const int32_t *label,
                                 const int32_t *count, const int32_t *assigned, const float *code_weights,
                                 const float *factors, const bevmsda_group_loss_desc *d, float *group_losses, float *losses,
                                 float *grad_cls, float *grad_box, void *stream) {
  const int rc = group_loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0) return BEVMSDA_OK;
  if (!cls || !box || !count || !assigned || !code_weights || !factors || !group_losses || !losses || !grad_cls || !grad_box)
    return BEVMSDA_ERR_NULL_POINTER;
  if (d->gmax > 0 && (!gt || !label)) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(assigned) || off4(code_weights) ||
      off4(factors) || off4(group_losses) || off4(losses) || off4(grad_cls) || off4(grad_box))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetLossArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.assigned = assigned;
  a.code_weights = code_weights; a.factors = factors; a.losses = losses; a.grad_cls = grad_cls; a.grad_box = grad_box;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.alpha = d->loss_alpha; a.gamma = d->loss_gamma; a.cls_weight = d->loss_cls_weight; a.box_weight = d->loss_box_weight;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bevmsda::det_loss_grouped_kernel, dim3(d->groups, d->L), dim3(bevmsda::kDetLossThreads), 0, st, a,
                     group_losses);
  if (hipGetLastError() != hipSuccess) return BEVMSDA_ERR_LAUNCH;
  hipLaunchKernelGGL(bevmsda::det_loss_group_mean_kernel, dim3((2 * d->L + 63) / 64), dim3(64), 0, st, group_losses, losses,
                     d->L, d->groups);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- optimizer step (optim.h): argument checks and launches

static inline bool off8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

int64_t bevmsda_optim_job_blocks(int64_t numel) {
  if (numel < 0) return -1;
  return (numel + bevmsda::kOptimBlockElems - 1) / bevmsda::kOptimBlockElems;
}

// one double per block of the norm kernel (which runs one block when there is none)
int64_t bevmsda_optim_workspace_bytes(int64_t blocks) {
  if (blocks < 0) return -1;
  return (blocks > 0 ? blocks : 1) * static_cast<int64_t>(sizeof(double));
}

int bevmsda_optim_grad_norm_f32(const bevmsda_optim_job *jobs, int njobs, int64_t blocks, double max_norm, int flags,
                                void *workspace, void *scalars, void *stream) {
  static_assert(sizeof(bevmsda_optim_job) == sizeof(bevmsda::OptimJob) && sizeof(bevmsda_optim_job) == 56, "bevmsda_optim_job layout");
  static_assert(sizeof(bevmsda::OptimScalars) == 4 * BEVMSDA_OPTIM_SCALAR_WORDS, "scalars layout");
  if (njobs < 0 || blocks < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (blocks >= (1LL << 30)) return BEVMSDA_ERR_TOO_LARGE;
  if (flags & ~(BEVMSDA_OPTIM_CLIP | BEVMSDA_OPTIM_SKIP_NONFINITE)) return BEVMSDA_ERR_BAD_OPTION;
  if ((flags & BEVMSDA_OPTIM_CLIP) && !(max_norm >= 0.0)) return BEVMSDA_ERR_BAD_OPTION;
  if (njobs == 0) return BEVMSDA_OK;
  if (!jobs || !workspace || !scalars) return BEVMSDA_ERR_NULL_POINTER;
  if (off8(jobs) || off8(workspace) || off4(scalars)) return BEVMSDA_ERR_MISALIGNED;
  hipLaunchKernelGGL(bevmsda::optim_grad_norm_kernel, dim3(static_cast<unsigned>(blocks > 0 ? blocks : 1)),
                     dim3(bevmsda::kOptimThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const bevmsda::OptimJob *>(jobs), njobs, static_cast<int>(blocks), max_norm, flags,
                     static_cast<double *>(workspace), static_cast<bevmsda::OptimScalars *>(scalars));
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

int bevmsda_optim_adamw_f32(const bevmsda_optim_job *jobs, int njobs, int64_t blocks, const bevmsda_optim_group *groups,
                            int ngroups, const void *scalars, void *stream) {
  static_assert(sizeof(bevmsda_optim_group) == sizeof(bevmsda::OptimGroup) && sizeof(bevmsda_optim_group) == 40, "bevmsda_optim_group layout");
  if (njobs < 0 || blocks < 0 || ngroups < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (blocks >= (1LL << 30)) return BEVMSDA_ERR_TOO_LARGE;
  if (njobs == 0) return BEVMSDA_OK;
  if (!jobs || !groups || ngroups == 0 || !scalars) return BEVMSDA_ERR_NULL_POINTER;
  if (off8(jobs) || off8(groups) || off4(scalars)) return BEVMSDA_ERR_MISALIGNED;
  if (blocks == 0) return BEVMSDA_OK;             // (every job is empty: the steps were counted by the norm launch)
  hipLaunchKernelGGL(bevmsda::optim_adamw_kernel, dim3(static_cast<unsigned>(blocks)), dim3(bevmsda::kOptimThreads), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const bevmsda::OptimJob *>(jobs), njobs,
                     reinterpret_cast<const bevmsda::OptimGroup *>(groups), static_cast<const bevmsda::OptimScalars *>(scalars));
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- 3 x 3 convolution over channel-last rows + inference BatchNorm (conv3x3.h): argument checks and launches
int64_t bevmsda_conv3x3_packed_bytes(int c_out, int c_in) {
  if (c_out <= 0 || c_in <= 0 || c_in % bevmsda::kConvGran != 0) return 0;
  return static_cast<int64_t>((c_out + 127) / 128) * (9 * static_cast<int64_t>(c_in) / 32) * 2 * 128 * 40 * 2;
}

int bevmsda_conv3x3_pack_weight_f32(const float *w, int c_out, int c_in, uint16_t *blob, void *stream) {
  if (c_out < 0 || c_in < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (c_out == 0 || c_in == 0) return BEVMSDA_OK;
  if (c_in % bevmsda::kConvGran != 0 || c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!w || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if ((reinterpret_cast<uintptr_t>(w) & 3u) || misaligned(blob)) return BEVMSDA_ERR_MISALIGNED;
  const long long threads = static_cast<long long>((c_out + 127) / 128) * 128 * (9LL * c_in / 8);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::conv3x3_pack_weight_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, c_out, c_in, blob);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// the launch grid both convolution kernels share (conv_mfma.h): 128 x 128 tiles, row tiles rounded up to the 8 XCDs
static dim3 conv_grid(long long M, int c_out, int *nblk_m, int *nblk_n) {
  const long long nbm = (M + 127) / 128, nbn = (c_out + 127) / 128;
  *nblk_m = static_cast<int>(nbm);
  *nblk_n = static_cast<int>(nbn);
  return dim3(static_cast<unsigned>(((nbm + 7) / 8) * 8 * nbn));
}

int bevmsda_conv3x3_bn_f32(const bevmsda_conv3x3_desc *d, const uint16_t *wpack, float *y, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->bs < 0 || d->H < 0 || d->W < 0 || d->nseg < 0 || d->c_seg < 0 || d->c_out < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->nseg > BEVMSDA_CONV_MAX_SEGMENTS) return BEVMSDA_ERR_BAD_SHAPE;
  const long long HW = 1LL * d->H * d->W;
  if (HW > (1LL << 24) || HW * d->bs > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;
  if (1LL * d->nseg * d->c_seg > 65536 || d->c_out > 65536) return BEVMSDA_ERR_TOO_LARGE;
  const long long M = HW * d->bs;
  if (M == 0 || d->c_out == 0) return BEVMSDA_OK;
  if (d->nseg == 0 || d->c_seg == 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->c_seg % bevmsda::kConvGran != 0 || d->c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!wpack || !y || !d->gamma || !d->beta || !d->mean || !d->var) return BEVMSDA_ERR_NULL_POINTER;
  for (int s = 0; s < d->nseg; ++s)
    if (!d->seg[s]) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_y < d->c_out || (d->res && d->ld_res < d->c_out)) return BEVMSDA_ERR_BAD_SHAPE;
  for (int s = 0; s < d->nseg; ++s)
    if (d->ld_seg[s] < d->c_seg) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_y % 4 != 0 || (d->res && d->ld_res % 4 != 0)) return BEVMSDA_ERR_MISALIGNED;      // rows start on 16 bytes
  for (int s = 0; s < d->nseg; ++s)
    if (d->ld_seg[s] % 4 != 0 || misaligned(d->seg[s])) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(wpack) || misaligned(y) || (d->res && misaligned(d->res)) || misaligned(d->gamma) || misaligned(d->beta) ||
      misaligned(d->mean) || misaligned(d->var))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::Conv3x3Args a = {};
  for (int s = 0; s < d->nseg; ++s) {
    a.seg[s] = d->seg[s];
    a.ldseg[s] = d->ld_seg[s];
  }
  a.nseg = d->nseg; a.cseg = d->c_seg;
  a.wpack = wpack;
  a.gamma = d->gamma; a.beta = d->beta; a.mean = d->mean; a.var = d->var; a.eps = d->eps;
  a.res = d->res; a.ldres = d->ld_res;
  a.y = y; a.ldy = d->ld_y;
  a.M = M; a.H = d->H; a.W = d->W; a.N = d->c_out;
  a.relu = d->relu ? 1 : 0;
  const dim3 grid = conv_grid(M, d->c_out, &a.nblk_m, &a.nblk_n), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (d->precision == 0) hipLaunchKernelGGL(bevmsda::conv3x3_bn_kernel<3>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(bevmsda::conv3x3_bn_kernel<1>, grid, block, 0, st, a);
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- convolution over channel-last rows for an image neck (conv_rows.h): argument checks and launches
int bevmsda_conv_rows_f32(const bevmsda_conv_rows_desc *d, const uint16_t *wpack, float *y, int64_t ld_y, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->taps != 1 && d->taps != 9) return BEVMSDA_ERR_BAD_OPTION;
  if (d->stride != 1 && d->stride != 2) return BEVMSDA_ERR_BAD_OPTION;
  if (d->stride == 2 && d->taps == 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->res_mode < BEVMSDA_CONV_RES_NONE || d->res_mode > BEVMSDA_CONV_RES_UP2) return BEVMSDA_ERR_BAD_OPTION;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->n_img < 0 || d->H < 0 || d->W < 0 || d->c_in < 0 || d->c_out < 0) return BEVMSDA_ERR_BAD_SHAPE;
  const long long HW = 1LL * d->H * d->W;
  if (HW > (1LL << 24) || HW * d->n_img > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;
  if (d->c_in > 65536 || d->c_out > 65536) return BEVMSDA_ERR_TOO_LARGE;
  if (HW * d->n_img == 0 || d->c_out == 0) return BEVMSDA_OK;
  if (d->c_in == 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->c_in % bevmsda::kConvGran != 0 || d->c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  const int Ho = (d->H - 1) / d->stride + 1, Wo = (d->W - 1) / d->stride + 1;
  const long long M = 1LL * d->n_img * Ho * Wo;          // <= n_img H W <= 2^24
  if (d->res_mode == BEVMSDA_CONV_RES_UP2 && (Ho % 2 != 0 || Wo % 2 != 0)) return BEVMSDA_ERR_BAD_SHAPE;
  if (!d->x || !wpack || !y || (d->res_mode && !d->res)) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_x < d->c_in || ld_y < d->c_out || (d->res_mode && d->ld_res < d->c_out)) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_x % 4 != 0 || ld_y % 4 != 0 || (d->res_mode && d->ld_res % 4 != 0)) return BEVMSDA_ERR_MISALIGNED;   // rows start on 16 bytes
  if (misaligned(d->x) || misaligned(wpack) || misaligned(y) || (d->res_mode && misaligned(d->res)) ||
      (d->bias && misaligned(d->bias)))
    return BEVMSDA_ERR_MISALIGNED;
  {   // y must not overlap what the launch reads: its tiles are written while others still load
    auto overlap = [](const float *p, long long n, const float *q, long long m) { return p < q + m && q < p + n; };
    const long long ny = (M - 1) * ld_y + d->c_out;
    const long long nx = (HW * d->n_img - 1) * d->ld_x + d->c_in;
    const long long rrows = d->res_mode == BEVMSDA_CONV_RES_UP2 ? M / 4 : M;
    if (overlap(y, ny, d->x, nx)) return BEVMSDA_ERR_BAD_OPTION;
    if (d->res_mode && overlap(y, ny, d->res, (rrows - 1) * d->ld_res + d->c_out)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::ConvRowsArgs a = {};
  a.x = d->x; a.ldx = d->ld_x;
  a.wpack = wpack;
  a.bias = d->bias;
  a.res = d->res_mode ? d->res : nullptr; a.ldres = d->ld_res; a.res_mode = d->res_mode;
  a.y = y; a.ldy = ld_y;
  a.M = M; a.H = d->H; a.W = d->W; a.Ho = Ho; a.Wo = Wo; a.C = d->c_in; a.N = d->c_out;
  a.relu_in = d->relu_in ? 1 : 0;
  const dim3 grid = conv_grid(M, d->c_out, &a.nblk_m, &a.nblk_n), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool split = d->precision == 0;
  if (d->taps == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_rows_kernel<3, 1, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_rows_kernel<1, 1, 1>), grid, block, 0, st, a);
  } else if (d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_rows_kernel<3, 9, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_rows_kernel<1, 9, 1>), grid, block, 0, st, a);
  } else {
    if (split) hipLaunchKernelGGL((bevmsda::conv_rows_kernel<3, 9, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_rows_kernel<1, 9, 2>), grid, block, 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

// ---- modulated deformable 3 x 3 convolution over channel-last rows (deform_conv.h): argument checks and launches
int bevmsda_deform_conv_f32(const bevmsda_deform_conv_desc *d, const uint16_t *wpack, float *y, int64_t ld_y, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->stride != 1 && d->stride != 2) return BEVMSDA_ERR_BAD_OPTION;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  const int nbn = (d->bn[0] ? 1 : 0) + (d->bn[1] ? 1 : 0) + (d->bn[2] ? 1 : 0) + (d->bn[3] ? 1 : 0);
  if (nbn != 0 && nbn != 4) return BEVMSDA_ERR_BAD_OPTION;               // BatchNorm: all four vectors or none
  if (d->bias && nbn) return BEVMSDA_ERR_BAD_OPTION;                     // one epilogue
  if (d->n_img < 0 || d->H < 0 || d->W < 0 || d->c_in < 0 || d->c_out < 0) return BEVMSDA_ERR_BAD_SHAPE;
  const long long HW = 1LL * d->H * d->W;
  if (HW > (1LL << 24) || HW * d->n_img > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;
  if (d->c_in > 65536 || d->c_out > 65536) return BEVMSDA_ERR_TOO_LARGE;
  if (HW * d->n_img == 0 || d->c_out == 0) return BEVMSDA_OK;
  if (d->c_in == 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->c_in % bevmsda::kConvGran != 0 || d->c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  const int Ho = (d->H - 1) / d->stride + 1, Wo = (d->W - 1) / d->stride + 1;
  const long long M = 1LL * d->n_img * Ho * Wo;          // <= n_img H W <= 2^24
  if (!d->x || !d->offs || !wpack || !y) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_x < d->c_in || ld_y < d->c_out || d->ld_offs < 32) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_x % 4 != 0 || ld_y % 4 != 0 || d->ld_offs % 4 != 0) return BEVMSDA_ERR_MISALIGNED;   // rows start on 16 bytes
  if (misaligned(d->x) || misaligned(d->offs) || misaligned(wpack) || misaligned(y) || (d->bias && misaligned(d->bias)) ||
      (nbn && (misaligned(d->bn[0]) || misaligned(d->bn[1]) || misaligned(d->bn[2]) || misaligned(d->bn[3]))))
    return BEVMSDA_ERR_MISALIGNED;
  {   // y must not overlap what the launch reads: its tiles are written while others still load
    auto overlap = [](const float *p, long long n, const float *q, long long m) { return p < q + m && q < p + n; };
    const long long ny = (M - 1) * ld_y + d->c_out;
    if (overlap(y, ny, d->x, (HW * d->n_img - 1) * d->ld_x + d->c_in)) return BEVMSDA_ERR_BAD_OPTION;
    if (overlap(y, ny, d->offs, (M - 1) * d->ld_offs + 32)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::DeformConvArgs a = {};
  a.x = d->x; a.ldx = d->ld_x;
  a.offs = d->offs; a.ldoffs = d->ld_offs;
  a.wpack = wpack;
  a.bias = d->bias;
  a.gamma = d->bn[0]; a.beta = d->bn[1]; a.mean = d->bn[2]; a.var = d->bn[3]; a.eps = d->eps;
  a.y = y; a.ldy = ld_y;
  a.M = M; a.H = d->H; a.W = d->W; a.Ho = Ho; a.Wo = Wo; a.C = d->c_in; a.N = d->c_out;
  a.relu = d->relu ? 1 : 0;
  const dim3 grid = conv_grid(M, d->c_out, &a.nblk_m, &a.nblk_n), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool split = d->precision == 0;
  if (d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::deform_conv_rows_kernel<3, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::deform_conv_rows_kernel<1, 1>), grid, block, 0, st, a);
  } else {
    if (split) hipLaunchKernelGGL((bevmsda::deform_conv_rows_kernel<3, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::deform_conv_rows_kernel<1, 2>), grid, block, 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
}

}  // extern "C"
