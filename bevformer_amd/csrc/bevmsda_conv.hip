// C ABI of libbevmsda.so, channel-last convolutions (conv3x3.h, conv_rows.h, deform_conv.h, conv_bn_rows.h over conv_mfma.h), the
// backbone's stem (stem_conv.h) and the backward of the backbone's row convolutions (conv_bwd_rows.h, deform_conv_bwd.h):
// bevmsda_conv3x3_*, bevmsda_conv_rows_f32, bevmsda_deform_conv_f32, bevmsda_conv_bn_rows_f32, bevmsda_stem_*, bevmsda_conv_dgrad_*,
// bevmsda_conv_wgrad_rows_f32, bevmsda_conv_gz_rows_f32, bevmsda_deform_conv_dgrad_f32, bevmsda_deform_conv_wgrad_f32,
// bevmsda_deform_dgrad_*; and BatchNorm with batch statistics over channel-last rows for a backbone whose norms train
// (batchnorm_rows.h): bevmsda_bn_rows_workspace_bytes, bevmsda_bn_stats_rows_f32, bevmsda_bn_apply_rows_f32,
// bevmsda_bn_bwd_reduce_rows_f32, bevmsda_bn_bwd_apply_rows_f32.
#include "capi_checks.h"
#include "batchnorm_rows.h"
#include "conv3x3.h"
#include "conv_bn_rows.h"
#include "conv_bwd_rows.h"
#include "conv_rows.h"
#include "deform_conv.h"
#include "deform_conv_bwd.h"
#include "stem_conv.h"

extern "C" {

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
  if (off4(w) || misaligned(blob)) return BEVMSDA_ERR_MISALIGNED;
  const long long threads = static_cast<long long>((c_out + 127) / 128) * 128 * (9LL * c_in / 8);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::conv3x3_pack_weight_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, c_out, c_in, blob);
  return launch_status();
}

// the launch grid all convolution kernels share (conv_mfma.h): 128 x 128 tiles, row tiles rounded up to the 8 XCDs.  The
// callers bound M by 2^24 and c_out by 2^16 first: at most 2^17 x 2^9 tiles, so xcd_grid cannot refuse
static dim3 conv_grid(long long M, int c_out, int *nblk_m, int *nblk_n) {
  const long long nbm = (M + 127) / 128, nbn = (c_out + 127) / 128;
  *nblk_m = static_cast<int>(nbm);
  *nblk_n = static_cast<int>(nbn);
  unsigned grid = 0;
  xcd_grid(nbm, nbn, &grid);
  return dim3(grid);
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
  return launch_status();
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
  return launch_status();
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
  return launch_status();
}

// ---- convolution over channel-last rows + inference BatchNorm for a backbone's bottlenecks (conv_bn_rows.h): argument checks
// and launches
int bevmsda_conv_bn_rows_f32(const bevmsda_conv_bn_rows_desc *d, const uint16_t *wpack, float *y, int64_t ld_y, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->taps != 1 && d->taps != 9) return BEVMSDA_ERR_BAD_OPTION;
  if (d->stride != 1 && d->stride != 2) return BEVMSDA_ERR_BAD_OPTION;
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
  if (!d->x || !wpack || !y || !d->bn[0] || !d->bn[1] || !d->bn[2] || !d->bn[3]) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_x < d->c_in || ld_y < d->c_out || (d->res && d->ld_res < d->c_out)) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_x % 4 != 0 || ld_y % 4 != 0 || (d->res && d->ld_res % 4 != 0)) return BEVMSDA_ERR_MISALIGNED;   // rows start on 16 bytes
  if (misaligned(d->x) || misaligned(wpack) || misaligned(y) || misaligned(d->res) || misaligned(d->bn[0]) ||
      misaligned(d->bn[1]) || misaligned(d->bn[2]) || misaligned(d->bn[3]))
    return BEVMSDA_ERR_MISALIGNED;
  {   // y must not overlap what the launch reads: its tiles are written while others still load
    auto overlap = [](const float *p, long long n, const float *q, long long m) { return p < q + m && q < p + n; };
    const long long ny = (M - 1) * ld_y + d->c_out;
    if (overlap(y, ny, d->x, (HW * d->n_img - 1) * d->ld_x + d->c_in)) return BEVMSDA_ERR_BAD_OPTION;
    if (d->res && overlap(y, ny, d->res, (M - 1) * d->ld_res + d->c_out)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::ConvBnRowsArgs a = {};
  a.x = d->x; a.ldx = d->ld_x;
  a.wpack = wpack;
  a.gamma = d->bn[0]; a.beta = d->bn[1]; a.mean = d->bn[2]; a.var = d->bn[3]; a.eps = d->eps;
  a.res = d->res; a.ldres = d->ld_res;
  a.y = y; a.ldy = ld_y;
  a.M = M; a.H = d->H; a.W = d->W; a.Ho = Ho; a.Wo = Wo; a.C = d->c_in; a.N = d->c_out;
  a.relu = d->relu ? 1 : 0;
  const dim3 grid = conv_grid(M, d->c_out, &a.nblk_m, &a.nblk_n), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool split = d->precision == 0;
  if (d->taps == 1 && d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<3, 1, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<1, 1, 1>), grid, block, 0, st, a);
  } else if (d->taps == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<3, 1, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<1, 1, 2>), grid, block, 0, st, a);
  } else if (d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<3, 9, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<1, 9, 1>), grid, block, 0, st, a);
  } else {
    if (split) hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<3, 9, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_bn_rows_kernel<1, 9, 2>), grid, block, 0, st, a);
  }
  return launch_status();
}

// ---- the backbone's stem in one launch on an NCHW image batch (stem_conv.h): weight image, argument checks and launch
int64_t bevmsda_stem_packed_bytes(int32_t c_out, int32_t c_in) {
  if (c_out != bevmsda::kStemCout || c_in != bevmsda::kStemCin) return 0;
  return 2LL * bevmsda::kStemKSteps * bevmsda::kStemCout * 16 * 2;      // planes x k-steps x columns x 16 k x 2 bytes
}

int bevmsda_stem_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, uint16_t *out, void *stream) {
  if (c_out < 0 || c_in < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (c_out == 0 || c_in == 0) return BEVMSDA_OK;
  if (c_out != bevmsda::kStemCout || c_in != bevmsda::kStemCin) return BEVMSDA_ERR_UNSUPPORTED;
  if (!w || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(w) || misaligned(out)) return BEVMSDA_ERR_MISALIGNED;
  hipLaunchKernelGGL(bevmsda::stem_pack_weight_kernel, dim3((bevmsda::kStemPlane16 + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, out);
  return launch_status();
}

int bevmsda_stem_f32(const bevmsda_stem_desc *d, const uint16_t *wpack, float *y, int64_t ld_y, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if ((d->pool != 0 && d->pool != 1) || (d->precision != 0 && d->precision != 1)) return BEVMSDA_ERR_BAD_OPTION;
  if (d->n_img < 0 || d->H < 0 || d->W < 0 || d->c_in < 0 || d->c_out < 0) return BEVMSDA_ERR_BAD_SHAPE;
  const long long Hc = d->H > 0 ? (d->H - 1) / 2 + 1 : 0, Wc = d->W > 0 ? (d->W - 1) / 2 + 1 : 0;
  if (Hc * Wc > (1LL << 24) || Hc * Wc * d->n_img > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;
  if (Hc * Wc * d->n_img == 0 || d->c_out == 0) return BEVMSDA_OK;
  if (d->c_in != bevmsda::kStemCin || d->c_out != bevmsda::kStemCout) return BEVMSDA_ERR_UNSUPPORTED;
  if (!d->x || !wpack || !y || !d->bn[0] || !d->bn[1] || !d->bn[2] || !d->bn[3]) return BEVMSDA_ERR_NULL_POINTER;
  // rows inside channels inside images, none overlapping the next (Hc Wc <= 2^24: H, W <= 2^25 and the products fit)
  const long long row_ext = d->W, ch_ext = (d->H - 1LL) * d->ld_row + row_ext;
  if (d->ld_row < row_ext || d->ld_ch < ch_ext || ld_y < d->c_out) return BEVMSDA_ERR_BAD_SHAPE;
  const long long img_ext = (d->c_in - 1LL) * d->ld_ch + ch_ext;
  if (d->ld_img < img_ext) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_y % 4 != 0 || misaligned(y) || misaligned(wpack) || misaligned(d->bn[0]) || misaligned(d->bn[1]) ||
      misaligned(d->bn[2]) || misaligned(d->bn[3]) || off4(d->x))
    return BEVMSDA_ERR_MISALIGNED;
  const long long Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;
  const long long M = d->n_img * (d->pool ? Hp * Wp : Hc * Wc);
  {   // y must not overlap x: tiles are written while others still load
    auto overlap = [](const float *p, long long n, const float *q, long long m) { return p < q + m && q < p + n; };
    if (overlap(y, (M - 1) * ld_y + d->c_out, d->x, (d->n_img - 1LL) * d->ld_img + img_ext)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::StemArgs a = {};
  a.x = d->x; a.ld_img = d->ld_img; a.ld_ch = d->ld_ch; a.ld_row = d->ld_row;
  a.wpack = wpack;
  a.gamma = d->bn[0]; a.beta = d->bn[1]; a.mean = d->bn[2]; a.var = d->bn[3]; a.eps = d->eps;
  a.y = y; a.ldy = ld_y;
  a.H = d->H; a.W = d->W; a.Hc = static_cast<int>(Hc); a.Wc = static_cast<int>(Wc); a.Hp = static_cast<int>(Hp); a.Wp = static_cast<int>(Wp);
  a.tiles_y = static_cast<int>((Hp + bevmsda::kStemPH - 1) / bevmsda::kStemPH);
  a.tiles_x = static_cast<int>((Wp + bevmsda::kStemPW - 1) / bevmsda::kStemPW);
  a.pool = d->pool;
  // at most n_img Hp Wp <= 2^24 tiles
  const dim3 grid(static_cast<unsigned>(1LL * d->n_img * a.tiles_y * a.tiles_x)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (d->precision == 0) hipLaunchKernelGGL(bevmsda::stem_kernel<3>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(bevmsda::stem_kernel<1>, grid, block, 0, st, a);
  return launch_status();
}

}  // extern "C"

// ---- backward of the backbone's row convolutions (conv_bwd_rows.h)
namespace {

bool overlap(const float *p, long long n, const float *q, long long m) { return p < q + m && q < p + n; }

// the checks the two gradient entry points share on their common fields, in the documented order up to the empty problem; the
// row counts and the output size are handed back
struct Shape {
  long long HW, M_in, M_out;
  int Ho, Wo;
};

int common_options(int taps, int stride, int precision, const float *gamma, const float *var) {
  if (taps != 1 && taps != 9) return BEVMSDA_ERR_BAD_OPTION;
  if (stride != 1 && stride != 2) return BEVMSDA_ERR_BAD_OPTION;
  if (precision != 0 && precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if ((gamma == nullptr) != (var == nullptr)) return BEVMSDA_ERR_BAD_OPTION;         // the scale: both vectors or none
  return BEVMSDA_OK;
}

int common_shape(int n_img, int H, int W, int c_in, int c_out, int stride, Shape *s) {
  if (n_img < 0 || H < 0 || W < 0 || c_in < 0 || c_out < 0) return BEVMSDA_ERR_BAD_SHAPE;
  s->HW = 1LL * H * W;
  if (s->HW > (1LL << 24) || s->HW * n_img > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;
  if (c_in > 65536 || c_out > 65536) return BEVMSDA_ERR_TOO_LARGE;
  s->M_in = s->HW * n_img;
  s->Ho = H > 0 ? (H - 1) / stride + 1 : 0;
  s->Wo = W > 0 ? (W - 1) / stride + 1 : 0;
  s->M_out = 1LL * n_img * s->Ho * s->Wo;          // <= n_img H W <= 2^24
  return BEVMSDA_OK;
}

}  // namespace

extern "C" {

// ---- the input gradient's weight image (conv_bwd_rows.h)
int64_t bevmsda_conv_dgrad_packed_bytes(int32_t c_out, int32_t c_in, int32_t taps) {
  if (c_out <= 0 || c_in <= 0 || (taps != 1 && taps != 9) || c_out % bevmsda::kConvGran != 0) return 0;
  return static_cast<int64_t>((c_in + 127) / 128) * (static_cast<int64_t>(taps) * c_out / 32) * 2 * 128 * 40 * 2;
}

int bevmsda_conv_dgrad_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, int32_t taps, uint16_t *blob, void *stream) {
  if (taps != 1 && taps != 9) return BEVMSDA_ERR_BAD_OPTION;
  if (c_out < 0 || c_in < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (c_out > 65536 || c_in > 65536) return BEVMSDA_ERR_TOO_LARGE;
  if (c_out == 0 || c_in == 0) return BEVMSDA_OK;
  if (c_in % bevmsda::kConvGran != 0 || c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!w || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(w) || misaligned(blob)) return BEVMSDA_ERR_MISALIGNED;
  const long long threads = static_cast<long long>((c_in + 127) / 128) * 128 * (1LL * taps * c_out / 8);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::conv_dgrad_pack_weight_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, c_out, c_in, taps, blob);
  return launch_status();
}

// ---- gz rows of their own: argument checks and launch
int bevmsda_conv_gz_rows_f32(const float *g, int64_t ld_g, const float *y, int64_t ld_y, const float *gamma, const float *var,
                             float eps, int64_t M, int32_t C, float *gz, int64_t ld_gz, void *stream) {
  if ((gamma == nullptr) != (var == nullptr)) return BEVMSDA_ERR_BAD_OPTION;
  if (M < 0 || C < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (M > (1LL << 24) || C > 65536) return BEVMSDA_ERR_TOO_LARGE;
  if (M == 0 || C == 0) return BEVMSDA_OK;
  if (C % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!g || !gz) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_g < C || ld_gz < C || (y && ld_y < C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_g % 4 != 0 || ld_gz % 4 != 0 || (y && ld_y % 4 != 0)) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(g) || misaligned(gz) || misaligned(y) || misaligned(gamma) || misaligned(var)) return BEVMSDA_ERR_MISALIGNED;
  {   // gz may BE g (every element is read and then written by one thread), else it overlaps nothing the launch reads
    const long long ngz = (M - 1) * ld_gz + C;
    if (!(gz == g && ld_gz == ld_g) && overlap(gz, ngz, g, (M - 1) * ld_g + C)) return BEVMSDA_ERR_BAD_OPTION;
    if (y && overlap(gz, ngz, y, (M - 1) * ld_y + C)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::ConvGzArgs a = {};
  a.s.g = g; a.s.ldg = ld_g; a.s.y = y; a.s.ldy = ld_y; a.s.gamma = gamma; a.s.var = var; a.s.eps = eps;
  a.gz = gz; a.ldgz = ld_gz; a.M = M; a.N = C;
  const long long nb = (M * (C / 4) + 255) / 256;          // <= 2^24 * 2^14 / 2^8
  hipLaunchKernelGGL(bevmsda::conv_gz_rows_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

// ---- the input gradient: argument checks and launches
int bevmsda_conv_dgrad_rows_f32(const bevmsda_conv_dgrad_rows_desc *d, const uint16_t *wpack, float *dx, int64_t ld_dx, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  int rc = common_options(d->taps, d->stride, d->precision, d->gamma, d->var);
  if (rc != BEVMSDA_OK) return rc;
  if ((d->next_gamma == nullptr) != (d->next_var == nullptr)) return BEVMSDA_ERR_BAD_OPTION;
  if (d->next_gamma && !d->next_mask) return BEVMSDA_ERR_BAD_OPTION;              // a scale comes with its mask
  if ((d->add_mode != 0 && d->add_mode != 1) || (d->add_after_mask != 0 && d->add_after_mask != 1)) return BEVMSDA_ERR_BAD_OPTION;
  if ((d->add_mode == 1 || d->add_after_mask == 1) && !d->add) return BEVMSDA_ERR_BAD_OPTION;         // an order or a shape of nothing
  if (d->add_after_mask == 1 && !d->next_mask) return BEVMSDA_ERR_BAD_OPTION;
  const bool pool2 = d->add_mode == 1;
  Shape s;
  rc = common_shape(d->n_img, d->H, d->W, d->c_in, d->c_out, d->stride, &s);
  if (rc != BEVMSDA_OK) return rc;
  if (pool2 && 4 * s.M_in > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;            // the rows of the (2H, 2W) map
  if (s.M_in == 0 || d->c_in == 0) return BEVMSDA_OK;
  if (d->c_out == 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->c_in % bevmsda::kConvGran != 0 || d->c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!d->g || !wpack || !dx) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_g < d->c_out || (d->y && d->ld_y < d->c_out) || ld_dx < d->c_in || (d->add && d->ld_add < d->c_in) ||
      (d->next_mask && d->ld_next_mask < d->c_in))
    return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_g % 4 != 0 || (d->y && d->ld_y % 4 != 0) || ld_dx % 4 != 0 || (d->add && d->ld_add % 4 != 0) ||
      (d->next_mask && d->ld_next_mask % 4 != 0))
    return BEVMSDA_ERR_MISALIGNED;                                                // rows start on 16 bytes
  if (misaligned(d->g) || misaligned(d->y) || misaligned(d->gamma) || misaligned(d->var) || misaligned(wpack) || misaligned(dx) ||
      misaligned(d->add) || misaligned(d->next_mask) || misaligned(d->next_gamma) || misaligned(d->next_var))
    return BEVMSDA_ERR_MISALIGNED;
  {   // dx must not overlap what other tiles still read; add may BE dx (read and written by the thread that owns the element)
    const long long ndx = (s.M_in - 1) * ld_dx + d->c_in;
    if (overlap(dx, ndx, d->g, (s.M_out - 1) * d->ld_g + d->c_out)) return BEVMSDA_ERR_BAD_OPTION;
    if (d->y && overlap(dx, ndx, d->y, (s.M_out - 1) * d->ld_y + d->c_out)) return BEVMSDA_ERR_BAD_OPTION;
    // (POOL2: a thread reads four fine rows of add, which other threads' pixels of dx would cover: no overlap at all)
    if (d->add && !(!pool2 && d->add == dx && d->ld_add == ld_dx) &&
        overlap(dx, ndx, d->add, ((pool2 ? 4 : 1) * s.M_in - 1) * d->ld_add + d->c_in))
      return BEVMSDA_ERR_BAD_OPTION;
    if (d->next_mask && overlap(dx, ndx, d->next_mask, (s.M_in - 1) * d->ld_next_mask + d->c_in)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::ConvDgradArgs a = {};
  a.s.g = d->g; a.s.ldg = d->ld_g; a.s.y = d->y; a.s.ldy = d->ld_y; a.s.gamma = d->gamma; a.s.var = d->var; a.s.eps = d->eps;
  a.wpack = wpack;
  a.add = d->add; a.ldadd = d->ld_add; a.add_pool2 = pool2; a.add_after_mask = d->add_after_mask;
  a.nmask = d->next_mask; a.ldnmask = d->ld_next_mask; a.ngamma = d->next_gamma; a.nvar = d->next_var; a.neps = d->next_eps;
  a.dx = dx; a.lddx = ld_dx;
  a.M = s.M_in; a.H = d->H; a.W = d->W; a.Ho = s.Ho; a.Wo = s.Wo; a.C = d->c_out; a.N = d->c_in;
  // conv_mfma.h's grid: 128 x 128 tiles, row tiles rounded up to the 8 XCDs (M <= 2^24, c_in <= 2^16: xcd_grid cannot refuse)
  const long long nbm = (s.M_in + 127) / 128, nbn = (d->c_in + 127) / 128;
  a.nblk_m = static_cast<int>(nbm);
  a.nblk_n = static_cast<int>(nbn);
  unsigned g1 = 0;
  xcd_grid(nbm, nbn, &g1);
  const dim3 grid(g1), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool split = d->precision == 0;
  if (d->taps == 1 && d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<3, 1, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<1, 1, 1>), grid, block, 0, st, a);
  } else if (d->taps == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<3, 1, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<1, 1, 2>), grid, block, 0, st, a);
  } else if (d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<3, 9, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<1, 9, 1>), grid, block, 0, st, a);
  } else {
    if (split) hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<3, 9, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_dgrad_rows_kernel<1, 9, 2>), grid, block, 0, st, a);
  }
  return launch_status();
}

// ---- the weight gradient: argument checks and launches
int bevmsda_conv_wgrad_rows_f32(const bevmsda_conv_wgrad_rows_desc *d, float *dw, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  int rc = common_options(d->taps, d->stride, d->precision, d->gamma, d->var);
  if (rc != BEVMSDA_OK) return rc;
  if (d->relu_x != 0 && d->relu_x != 1) return BEVMSDA_ERR_BAD_OPTION;
  Shape s;
  rc = common_shape(d->n_img, d->H, d->W, d->c_in, d->c_out, d->stride, &s);
  if (rc != BEVMSDA_OK) return rc;
  if (s.M_in == 0 || d->c_in == 0 || d->c_out == 0) return BEVMSDA_OK;            // nothing to add
  if (d->c_in % bevmsda::kConvGran != 0 || d->c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!d->g || !d->x || !dw) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_g < d->c_out || (d->y && d->ld_y < d->c_out) || d->ld_x < d->c_in) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_g % 4 != 0 || (d->y && d->ld_y % 4 != 0) || d->ld_x % 4 != 0) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(d->g) || misaligned(d->y) || misaligned(d->gamma) || misaligned(d->var) || misaligned(d->x) || off4(dw) ||
      off4(d->dbias))
    return BEVMSDA_ERR_MISALIGNED;
  {   // dw and dbias are accumulated into while other workgroups still read
    const long long ndw = 1LL * d->c_out * d->c_in * d->taps;
    const long long ng = (s.M_out - 1) * d->ld_g + d->c_out, nx = (s.M_in - 1) * d->ld_x + d->c_in;
    if (overlap(dw, ndw, d->g, ng) || overlap(dw, ndw, d->x, nx) || (d->y && overlap(dw, ndw, d->y, (s.M_out - 1) * d->ld_y + d->c_out)))
      return BEVMSDA_ERR_BAD_OPTION;
    if (d->dbias && (overlap(d->dbias, d->c_out, d->g, ng) || overlap(d->dbias, d->c_out, d->x, nx) ||
                     (d->y && overlap(d->dbias, d->c_out, d->y, (s.M_out - 1) * d->ld_y + d->c_out)) ||
                     overlap(d->dbias, d->c_out, dw, ndw)))
      return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::ConvWgradArgs a = {};
  a.s.g = d->g; a.s.ldg = d->ld_g; a.s.y = d->y; a.s.ldy = d->ld_y; a.s.gamma = d->gamma; a.s.var = d->var; a.s.eps = d->eps;
  a.x = d->x; a.ldx = d->ld_x;
  a.dw = dw; a.dbias = d->dbias; a.relu_x = d->relu_x;
  a.M = s.M_out; a.H = d->H; a.W = d->W; a.Ho = s.Ho; a.Wo = s.Wo; a.C = d->c_in; a.N = d->c_out;
  a.tiles_n = (d->c_out + 127) / 128;
  a.tiles_k = (d->c_in + 127) / 128;
  // row slices as bevmsda_linear_wgrad_f32 picks them: about one round of resident workgroups (2 per CU), at least 128 rows each
  const long long tiles = 1LL * a.tiles_n * a.tiles_k * d->taps;                  // <= 2^9 * 2^9 * 9
  long long slices = tiles >= 512 ? 1 : 512 / tiles;
  long long rows = (s.M_out + slices - 1) / slices;
  rows = ((rows + 31) / 32) * 32;
  if (rows < 128) rows = 128;
  a.rows_per_block = static_cast<int>(rows);
  slices = (s.M_out + rows - 1) / rows;
  const long long slices8 = ((slices + 7) / 8) * 8;        // the kernel deals slices to XCDs: slice = 8 i + xcd
  if (tiles * slices8 >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  const dim3 grid(static_cast<unsigned>(tiles * slices8)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool split = d->precision == 0;
  if (d->taps == 1 && d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<3, 1, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<1, 1, 1>), grid, block, 0, st, a);
  } else if (d->taps == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<3, 1, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<1, 1, 2>), grid, block, 0, st, a);
  } else if (d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<3, 9, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<1, 9, 1>), grid, block, 0, st, a);
  } else {
    if (split) hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<3, 9, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::conv_wgrad_rows_kernel<1, 9, 2>), grid, block, 0, st, a);
  }
  return launch_status();
}

// ---- backward of the deformable convolution (deform_conv_bwd.h): the input gradient's weight image
int64_t bevmsda_deform_dgrad_packed_bytes(int32_t c_out, int32_t c_in) {
  if (c_out <= 0 || c_in <= 0 || c_out % bevmsda::kConvGran != 0 || c_in % bevmsda::kConvGran != 0) return 0;
  return static_cast<int64_t>((9LL * c_in + 127) / 128) * (c_out / 32) * 2 * 128 * 40 * 2;
}

int bevmsda_deform_dgrad_pack_weight_f32(const float *w, int32_t c_out, int32_t c_in, uint16_t *blob, void *stream) {
  if (c_out < 0 || c_in < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (c_out > 65536 || c_in > 65536) return BEVMSDA_ERR_TOO_LARGE;
  if (c_out == 0 || c_in == 0) return BEVMSDA_OK;
  if (c_in % bevmsda::kConvGran != 0 || c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!w || !blob) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(w) || misaligned(blob)) return BEVMSDA_ERR_MISALIGNED;
  const long long threads = ((9LL * c_in + 127) / 128) * 128 * (c_out / 8);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::deform_dgrad_pack_weight_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, c_out, c_in, blob);
  return launch_status();
}

// ---- the deformable input and offset gradient: argument checks and launches
int bevmsda_deform_conv_dgrad_f32(const bevmsda_deform_conv_dgrad_desc *d, const uint16_t *wpack, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  int rc = common_options(9, d->stride, d->precision, d->gamma, d->var);
  if (rc != BEVMSDA_OK) return rc;
  Shape s;
  rc = common_shape(d->n_img, d->H, d->W, d->c_in, d->c_out, d->stride, &s);
  if (rc != BEVMSDA_OK) return rc;
  if (s.M_in == 0 || d->c_in == 0 || d->c_out == 0 || (!d->need_dx && !d->need_doffs)) return BEVMSDA_OK;     // nothing to add
  if (d->c_in % bevmsda::kConvGran != 0 || d->c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  float *dx = d->need_dx ? d->dx : nullptr, *doffs = d->need_doffs ? d->doffs : nullptr;
  if (!d->g || !d->x || !d->offs || !wpack || (d->need_dx && !dx) || (d->need_doffs && !doffs)) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_g < d->c_out || (d->y && d->ld_y < d->c_out) || d->ld_x < d->c_in || d->ld_offs < 32 || (dx && d->ld_dx < d->c_in) ||
      (doffs && d->ld_doffs < 32))
    return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_g % 4 != 0 || (d->y && d->ld_y % 4 != 0) || d->ld_x % 4 != 0 || d->ld_offs % 4 != 0 || (dx && d->ld_dx % 4 != 0) ||
      (doffs && d->ld_doffs % 4 != 0))
    return BEVMSDA_ERR_MISALIGNED;                                                // rows start on 16 bytes
  if (misaligned(d->g) || misaligned(d->y) || misaligned(d->gamma) || misaligned(d->var) || misaligned(d->x) || misaligned(d->offs) ||
      misaligned(wpack) || misaligned(dx) || misaligned(doffs))
    return BEVMSDA_ERR_MISALIGNED;
  {   // dx and doffs are accumulated into while other workgroups still read
    const long long ng = (s.M_out - 1) * d->ld_g + d->c_out, ny = d->y ? (s.M_out - 1) * d->ld_y + d->c_out : 0;
    const long long nx = (s.M_in - 1) * d->ld_x + d->c_in, no = (s.M_out - 1) * d->ld_offs + 32;
    const long long ndx = (s.M_in - 1) * d->ld_dx + d->c_in, ndo = (s.M_out - 1) * d->ld_doffs + 32;
    const float *outs[2] = {dx, doffs};
    const long long nouts[2] = {ndx, ndo};
    for (int i = 0; i < 2; ++i) {
      if (!outs[i]) continue;
      if (overlap(outs[i], nouts[i], d->g, ng) || (d->y && overlap(outs[i], nouts[i], d->y, ny)) || overlap(outs[i], nouts[i], d->x, nx) ||
          overlap(outs[i], nouts[i], d->offs, no))
        return BEVMSDA_ERR_BAD_OPTION;
    }
    if (dx && doffs && overlap(dx, ndx, doffs, ndo)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::DeformDgradArgs a = {};
  a.s.g = d->g; a.s.ldg = d->ld_g; a.s.y = d->y; a.s.ldy = d->ld_y; a.s.gamma = d->gamma; a.s.var = d->var; a.s.eps = d->eps;
  a.wpack = wpack;
  a.x = d->x; a.ldx = d->ld_x;
  a.offs = d->offs; a.ldoffs = d->ld_offs;
  a.dx = dx; a.lddx = d->ld_dx;
  a.doffs = doffs; a.lddoffs = d->ld_doffs;
  a.M = s.M_out; a.H = d->H; a.W = d->W; a.Ho = s.Ho; a.Wo = s.Wo; a.C = d->c_in; a.N = d->c_out;
  // conv_mfma.h's grid over the (M, 9 c_in) dcol matrix (M <= 2^24, 9 c_in <= 9 * 2^16: at most 2^17 x 4608 tiles)
  const long long nbm = (s.M_out + 127) / 128, nbn = (9LL * d->c_in + 127) / 128;
  a.nblk_m = static_cast<int>(nbm);
  a.nblk_n = static_cast<int>(nbn);
  unsigned g1 = 0;
  rc = xcd_grid(nbm, nbn, &g1);
  if (rc != BEVMSDA_OK) return rc;
  const dim3 grid(g1), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool split = d->precision == 0;
  if (d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::deform_conv_dgrad_rows_kernel<3, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::deform_conv_dgrad_rows_kernel<1, 1>), grid, block, 0, st, a);
  } else {
    if (split) hipLaunchKernelGGL((bevmsda::deform_conv_dgrad_rows_kernel<3, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::deform_conv_dgrad_rows_kernel<1, 2>), grid, block, 0, st, a);
  }
  return launch_status();
}

// ---- the deformable weight gradient: argument checks and launches
int bevmsda_deform_conv_wgrad_f32(const bevmsda_deform_conv_wgrad_desc *d, float *dw, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  int rc = common_options(9, d->stride, d->precision, d->gamma, d->var);
  if (rc != BEVMSDA_OK) return rc;
  Shape s;
  rc = common_shape(d->n_img, d->H, d->W, d->c_in, d->c_out, d->stride, &s);
  if (rc != BEVMSDA_OK) return rc;
  if (s.M_in == 0 || d->c_in == 0 || d->c_out == 0) return BEVMSDA_OK;            // nothing to add
  if (d->c_in % bevmsda::kConvGran != 0 || d->c_out % bevmsda::kConvGran != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (!d->g || !d->x || !d->offs || !dw) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_g < d->c_out || (d->y && d->ld_y < d->c_out) || d->ld_x < d->c_in || d->ld_offs < 32) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_g % 4 != 0 || (d->y && d->ld_y % 4 != 0) || d->ld_x % 4 != 0 || d->ld_offs % 4 != 0) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(d->g) || misaligned(d->y) || misaligned(d->gamma) || misaligned(d->var) || misaligned(d->x) || misaligned(d->offs) ||
      off4(dw))
    return BEVMSDA_ERR_MISALIGNED;
  {   // dw is accumulated into while other workgroups still read
    const long long ndw = 9LL * d->c_out * d->c_in;
    if (overlap(dw, ndw, d->g, (s.M_out - 1) * d->ld_g + d->c_out) || overlap(dw, ndw, d->x, (s.M_in - 1) * d->ld_x + d->c_in) ||
        overlap(dw, ndw, d->offs, (s.M_out - 1) * d->ld_offs + 32) || (d->y && overlap(dw, ndw, d->y, (s.M_out - 1) * d->ld_y + d->c_out)))
      return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::DeformWgradArgs a = {};
  a.s.g = d->g; a.s.ldg = d->ld_g; a.s.y = d->y; a.s.ldy = d->ld_y; a.s.gamma = d->gamma; a.s.var = d->var; a.s.eps = d->eps;
  a.x = d->x; a.ldx = d->ld_x;
  a.offs = d->offs; a.ldoffs = d->ld_offs;
  a.dw = dw;
  a.M = s.M_out; a.H = d->H; a.W = d->W; a.Ho = s.Ho; a.Wo = s.Wo; a.C = d->c_in; a.N = d->c_out;
  a.tiles_n = (d->c_out + 127) / 128;
  a.tiles_k = (d->c_in + 127) / 128;
  // row slices as bevmsda_conv_wgrad_rows_f32 picks them: about one round of resident workgroups, at least 128 rows each
  const long long tiles = 9LL * a.tiles_n * a.tiles_k;                            // <= 2^9 * 2^9 * 9
  long long slices = tiles >= 512 ? 1 : 512 / tiles;
  long long rows = (s.M_out + slices - 1) / slices;
  rows = ((rows + 31) / 32) * 32;
  if (rows < 128) rows = 128;
  a.rows_per_block = static_cast<int>(rows);
  slices = (s.M_out + rows - 1) / rows;
  const long long slices8 = ((slices + 7) / 8) * 8;        // the kernel deals slices to XCDs: slice = 8 i + xcd
  if (tiles * slices8 >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  const dim3 grid(static_cast<unsigned>(tiles * slices8)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool split = d->precision == 0;
  if (d->stride == 1) {
    if (split) hipLaunchKernelGGL((bevmsda::deform_conv_wgrad_rows_kernel<3, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::deform_conv_wgrad_rows_kernel<1, 1>), grid, block, 0, st, a);
  } else {
    if (split) hipLaunchKernelGGL((bevmsda::deform_conv_wgrad_rows_kernel<3, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bevmsda::deform_conv_wgrad_rows_kernel<1, 2>), grid, block, 0, st, a);
  }
  return launch_status();
}

}  // extern "C"

// ---- BatchNorm with batch statistics over channel-last rows (batchnorm_rows.h)
namespace {

// the size checks every entry point starts with (after its own options), in the documented order; *empty: C = 0, a no-op
int bn_shape(int64_t M, int32_t C, bool *empty) {
  *empty = false;
  if (M < 0 || C < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (M > (1LL << 24) || C > 65536) return BEVMSDA_ERR_TOO_LARGE;
  if (M < 2 || C % 32 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  *empty = C == 0;
  return BEVMSDA_OK;
}

long long extent(int64_t M, int64_t ld, int32_t C) { return (M - 1) * ld + C; }

template <int LX> struct BnStatsK {
  static void launch(dim3 g, dim3 b, hipStream_t st, const bevmsda::BnRowsArgs &a) {
    hipLaunchKernelGGL(bevmsda::bn_stats_partial_kernel<LX>, g, b, 0, st, a);
  }
};
template <int LX> struct BnBwdK {
  static void launch(dim3 g, dim3 b, hipStream_t st, const bevmsda::BnRowsArgs &a) {
    hipLaunchKernelGGL(bevmsda::bn_bwd_partial_kernel<LX>, g, b, 0, st, a);
  }
};
template <int LX> struct BnApplyK {
  static void launch(dim3 g, dim3 b, hipStream_t st, const bevmsda::BnRowsArgs &a) {
    hipLaunchKernelGGL(bevmsda::bn_apply_kernel<LX>, g, b, 0, st, a);
  }
};
template <int LX> struct BnBwdApplyK {
  static void launch(dim3 g, dim3 b, hipStream_t st, const bevmsda::BnRowsArgs &a) {
    hipLaunchKernelGGL(bevmsda::bn_bwd_apply_kernel<LX>, g, b, 0, st, a);
  }
};

// launch one of the geometry's kernels: column tiles x row chunks (at most 2^11 x 2^11 workgroups)
template <template <int> class K>
void bn_launch_tiles(const bevmsda::BnRowsArgs &a, hipStream_t st) {
  const int lx = bevmsda::bn_lanes_x(a.C);
  const dim3 grid(static_cast<unsigned>(a.C / (4 * lx)), static_cast<unsigned>(bevmsda::bn_num_chunks(a.M))), block(bevmsda::kBnThreads);
  if (lx == 32) K<32>::launch(grid, block, st, a);
  else if (lx == 16) K<16>::launch(grid, block, st, a);
  else K<8>::launch(grid, block, st, a);
}

void bn_launch_final(const bevmsda::BnFinalArgs &f, hipStream_t st) {
  hipLaunchKernelGGL(bevmsda::bn_final_kernel, dim3(static_cast<unsigned>(f.C / 32)), dim3(bevmsda::kBnThreads), 0, st, f);
}

}  // namespace

extern "C" {

int64_t bevmsda_bn_rows_workspace_bytes(int64_t M, int32_t C) {
  if (M < 2 || M > (1LL << 24) || C <= 0 || C > 65536 || C % 32 != 0) return 0;
  return static_cast<int64_t>(bevmsda::bn_num_chunks(M)) * 2 * C * static_cast<int64_t>(sizeof(float));
}

int bevmsda_bn_stats_rows_f32(const float *z, int64_t ld_z, int64_t M, int32_t C, float *mean, float *var, float *running_mean,
                              float *running_var, int64_t *num_batches_tracked, float momentum, float *workspace, void *stream) {
  if ((running_mean == nullptr) != (running_var == nullptr)) return BEVMSDA_ERR_BAD_OPTION;     // both running vectors or none
  if (running_mean && !(momentum >= 0.f && momentum <= 1.f)) return BEVMSDA_ERR_BAD_OPTION;
  bool empty;
  const int rc = bn_shape(M, C, &empty);
  if (rc != BEVMSDA_OK) return rc;
  if (empty) return BEVMSDA_OK;
  if (!z || !mean || !var || !workspace) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_z < C) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_z % 4 != 0) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(z) || misaligned(mean) || misaligned(var) || misaligned(running_mean) || misaligned(running_var) ||
      misaligned(workspace) || off8(num_batches_tracked))
    return BEVMSDA_ERR_MISALIGNED;
  {   // nothing written may overlap z
    const long long nz = extent(M, ld_z, C), nws = bevmsda::bn_num_chunks(M) * 2LL * C;
    if (overlap(workspace, nws, z, nz) || overlap(mean, C, z, nz) || overlap(var, C, z, nz) ||
        (running_mean && (overlap(running_mean, C, z, nz) || overlap(running_var, C, z, nz))))
      return BEVMSDA_ERR_BAD_OPTION;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  bevmsda::BnRowsArgs a = {};
  a.z = z; a.ldz = ld_z; a.slab = workspace; a.M = M; a.chunk = bevmsda::bn_chunk_rows(M); a.C = C;
  bn_launch_tiles<BnStatsK>(a, st);
  bevmsda::BnFinalArgs f = {};
  f.slab = workspace; f.M = M; f.chunk = a.chunk; f.nchunks = static_cast<int>(bevmsda::bn_num_chunks(M)); f.C = C; f.welford = 1;
  f.shift = z;
  f.out0 = mean; f.out1 = var; f.running_mean = running_mean; f.running_var = running_var;
  f.num_batches_tracked = reinterpret_cast<long long *>(num_batches_tracked); f.momentum = momentum;
  bn_launch_final(f, st);
  return launch_status();
}

int bevmsda_bn_apply_rows_f32(const float *z, int64_t ld_z, const float *mean, const float *var, const float *gamma, const float *beta,
                              float eps, const float *res, int64_t ld_res, int32_t relu, int64_t M, int32_t C, float *y, int64_t ld_y,
                              void *stream) {
  if (relu != 0 && relu != 1) return BEVMSDA_ERR_BAD_OPTION;
  bool empty;
  const int rc = bn_shape(M, C, &empty);
  if (rc != BEVMSDA_OK) return rc;
  if (empty) return BEVMSDA_OK;
  if (!z || !mean || !var || !gamma || !beta || !y) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_z < C || ld_y < C || (res && ld_res < C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_z % 4 != 0 || ld_y % 4 != 0 || (res && ld_res % 4 != 0)) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(z) || misaligned(mean) || misaligned(var) || misaligned(gamma) || misaligned(beta) || misaligned(res) || misaligned(y))
    return BEVMSDA_ERR_MISALIGNED;
  {   // y may BE z (an element is read and then written by one thread), else it overlaps nothing the launch reads
    const long long ny = extent(M, ld_y, C);
    if (!(y == z && ld_y == ld_z) && overlap(y, ny, z, extent(M, ld_z, C))) return BEVMSDA_ERR_BAD_OPTION;
    if (res && overlap(y, ny, res, extent(M, ld_res, C))) return BEVMSDA_ERR_BAD_OPTION;
    if (overlap(y, ny, mean, C) || overlap(y, ny, var, C) || overlap(y, ny, gamma, C) || overlap(y, ny, beta, C)) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::BnRowsArgs a = {};
  a.z = z; a.ldz = ld_z; a.mean = mean; a.var = var; a.gamma = gamma; a.beta = beta; a.eps = eps;
  a.res = res; a.ldres = ld_res; a.y = y; a.ldy = ld_y; a.relu = relu;
  a.M = M; a.chunk = bevmsda::bn_chunk_rows(M); a.C = C;
  bn_launch_tiles<BnApplyK>(a, static_cast<hipStream_t>(stream));
  return launch_status();
}

int bevmsda_bn_bwd_reduce_rows_f32(const float *g, int64_t ld_g, const float *y, int64_t ld_y, const float *z, int64_t ld_z,
                                   const float *mean, const float *var, float eps, int64_t M, int32_t C, float *sums, float *workspace,
                                   void *stream) {
  bool empty;
  const int rc = bn_shape(M, C, &empty);
  if (rc != BEVMSDA_OK) return rc;
  if (empty) return BEVMSDA_OK;
  if (!g || !z || !mean || !var || !sums || !workspace) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_g < C || ld_z < C || (y && ld_y < C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_g % 4 != 0 || ld_z % 4 != 0 || (y && ld_y % 4 != 0)) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(g) || misaligned(y) || misaligned(z) || misaligned(mean) || misaligned(var) || misaligned(sums) || misaligned(workspace))
    return BEVMSDA_ERR_MISALIGNED;
  {   // nothing written may overlap what the launches read
    const long long nws = bevmsda::bn_num_chunks(M) * 2LL * C;
    const float *outs[2] = {sums, workspace};
    const long long nouts[2] = {2LL * C, nws};
    for (int i = 0; i < 2; ++i) {
      if (overlap(outs[i], nouts[i], g, extent(M, ld_g, C)) || overlap(outs[i], nouts[i], z, extent(M, ld_z, C)) ||
          (y && overlap(outs[i], nouts[i], y, extent(M, ld_y, C))) || overlap(outs[i], nouts[i], mean, C) ||
          overlap(outs[i], nouts[i], var, C))
        return BEVMSDA_ERR_BAD_OPTION;
    }
    if (overlap(sums, 2LL * C, workspace, nws)) return BEVMSDA_ERR_BAD_OPTION;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  bevmsda::BnRowsArgs a = {};
  a.g = g; a.ldg = ld_g; a.mask = y; a.ldmask = ld_y; a.z = z; a.ldz = ld_z; a.mean = mean; a.var = var; a.eps = eps;
  a.slab = workspace; a.M = M; a.chunk = bevmsda::bn_chunk_rows(M); a.C = C;
  bn_launch_tiles<BnBwdK>(a, st);
  bevmsda::BnFinalArgs f = {};
  f.slab = workspace; f.M = M; f.chunk = a.chunk; f.nchunks = static_cast<int>(bevmsda::bn_num_chunks(M)); f.C = C; f.welford = 0;
  f.out0 = sums; f.out1 = sums + C;
  bn_launch_final(f, st);
  return launch_status();
}

int bevmsda_bn_bwd_apply_rows_f32(const float *g, int64_t ld_g, const float *y, int64_t ld_y, const float *z, int64_t ld_z,
                                  const float *mean, const float *var, const float *gamma, float eps, const float *sums, int64_t M,
                                  int32_t C, float *dz, int64_t ld_dz, float *gy, int64_t ld_gy, void *stream) {
  bool empty;
  const int rc = bn_shape(M, C, &empty);
  if (rc != BEVMSDA_OK) return rc;
  if (empty) return BEVMSDA_OK;
  if (!g || !z || !mean || !var || !gamma || !sums || !dz) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_g < C || ld_z < C || ld_dz < C || (y && ld_y < C) || (gy && ld_gy < C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_g % 4 != 0 || ld_z % 4 != 0 || ld_dz % 4 != 0 || (y && ld_y % 4 != 0) || (gy && ld_gy % 4 != 0)) return BEVMSDA_ERR_MISALIGNED;
  if (misaligned(g) || misaligned(y) || misaligned(z) || misaligned(mean) || misaligned(var) || misaligned(gamma) || misaligned(sums) ||
      misaligned(dz) || misaligned(gy))
    return BEVMSDA_ERR_MISALIGNED;
  {   // dz may BE g (an element is read and then written by one thread); else dz and gy overlap nothing read, nor one another
    const long long ng = extent(M, ld_g, C), nz = extent(M, ld_z, C), ny = y ? extent(M, ld_y, C) : 0;
    float *outs[2] = {dz, gy};
    const long long nouts[2] = {extent(M, ld_dz, C), gy ? extent(M, ld_gy, C) : 0};
    for (int i = 0; i < 2; ++i) {
      if (!outs[i]) continue;
      if (!(i == 0 && dz == g && ld_dz == ld_g) && overlap(outs[i], nouts[i], g, ng)) return BEVMSDA_ERR_BAD_OPTION;
      if (overlap(outs[i], nouts[i], z, nz) || (y && overlap(outs[i], nouts[i], y, ny)) || overlap(outs[i], nouts[i], mean, C) ||
          overlap(outs[i], nouts[i], var, C) || overlap(outs[i], nouts[i], gamma, C) || overlap(outs[i], nouts[i], sums, 2LL * C))
        return BEVMSDA_ERR_BAD_OPTION;
    }
    if (gy && overlap(dz, nouts[0], gy, nouts[1])) return BEVMSDA_ERR_BAD_OPTION;
  }
  bevmsda::BnRowsArgs a = {};
  a.g = g; a.ldg = ld_g; a.mask = y; a.ldmask = ld_y; a.z = z; a.ldz = ld_z; a.mean = mean; a.var = var; a.gamma = gamma; a.eps = eps;
  a.sums = sums; a.dz = dz; a.lddz = ld_dz; a.gy = gy; a.ldgy = ld_gy;
  a.M = M; a.chunk = bevmsda::bn_chunk_rows(M); a.C = C;
  bn_launch_tiles<BnBwdApplyK>(a, static_cast<hipStream_t>(stream));
  return launch_status();
}

}  // extern "C"
