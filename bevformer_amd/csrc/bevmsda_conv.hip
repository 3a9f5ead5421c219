// C ABI of libbevmsda.so, channel-last convolutions (conv3x3.h, conv_rows.h, deform_conv.h, conv_bn_rows.h over conv_mfma.h) and the
// backbone's stem (stem_conv.h): bevmsda_conv3x3_*, bevmsda_conv_rows_f32, bevmsda_deform_conv_f32, bevmsda_conv_bn_rows_f32,
// bevmsda_stem_*.
#include "capi_checks.h"
#include "conv3x3.h"
#include "conv_bn_rows.h"
#include "conv_rows.h"
#include "deform_conv.h"
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
