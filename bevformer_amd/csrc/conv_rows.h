// Convolution over channel-last rows on the CDNA4 matrix cores, the shapes of an image neck (mmdet's FPN as the reference
// configs build it, bevformer_base.py:54-61): 1 x 1 lateral convolutions, 3 x 3 output convolutions, 3 x 3 stride-2 extra
// levels, bias, and the top-down "+ 2 x nearest upsampled coarser level" in the epilogue.
//
//   y[q, co] = bias[co] + sum_{taps (dy, dx)} sum_ci relu?(x[row(q, dy, dx), ci]) * w[co, ci, dy + 1, dx + 1]  (+ res[rrow(q), co])
//
// q runs over the n_img * Ho * Wo OUTPUT pixels, (img, oy, ox) = (q div Ho Wo, (q mod Ho Wo) div Wo, q mod Wo); the input
// row is computed per image: row(q, dy, dx) = img H W + (S oy + dy) W + (S ox + dx), S the stride (1 or 2), and a tap is
// live only where 0 <= S oy + dy < H and 0 <= S ox + dx < W (zero padding 1 for the 9-tap form; the 1-tap form is the
// 1 x 1 convolution, dy = dx = 0, padding 0, stride 1).  Ho = (H - 1) div S + 1, Wo = (W - 1) div S + 1.
//
// The GEMM is conv_mfma.h's, shared with conv3x3_bn_kernel (conv3x3.h): its main loop over K = taps * C_in chunks of 32 and its
// epilogue walk.  This header supplies what is this kernel's own: one source matrix, the tap count and the stride as
// template parameters, the input row index through (img, oy, ox) in the fetch, an optional ReLU on the A operand before the
// split (relu_before_extra_convs; NaN stays NaN), and the epilogue: + bias, then + res, where res is a same-shape row matrix
// (mode 1) or the 2 x nearest upsampling of a coarser map (mode 2): rrow(q) = img Hc Wc + (oy >> 1) Wc + (ox >> 1) with
// Ho = 2 Hc, Wo = 2 Wc — F.interpolate(size=, mode='nearest') for an exact factor of 2.
//
// Memory safety: a row of x is addressed only under its tap's predicate (output pixel inside the problem AND the tap
// inside the input image), a row of res and of y only for an output pixel inside the problem; masked lanes load nothing
// and stage zeros.  The weight image is lin_pack_weight_kernel's over the (C_out, taps * C_in) matrix with
// k = tap * C_in + ci: conv3x3_pack_weight_kernel's for 9 taps, the linear pack of the (C_out, C_in) matrix for 1.
#pragma once
#include "conv_mfma.h"

namespace bevmsda {

struct ConvRowsArgs {
  const float *x;                       // (n_img * H * W, ldx) input rows
  long ldx;
  const uint16_t *wpack;
  const float *bias;                    // (N) or nullptr
  const float *res;                     // mode 1: (M, ldres); mode 2: (n_img * (Ho / 2) * (Wo / 2), ldres)
  long ldres;
  int res_mode;                         // 0 none, 1 same shape, 2 nearest 2 x upsampled
  float *y;
  long ldy;
  long M;                               // n_img * Ho * Wo
  int H, W, Ho, Wo;
  int C, N;                             // C_in, C_out: multiples of kConvGran
  int relu_in;
  int nblk_m, nblk_n;
};

template <int NPROD, int TAPS, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) conv_rows_kernel(const ConvRowsArgs a) {
  static_assert((TAPS == 9 && (STRIDE == 1 || STRIDE == 2)) || (TAPS == 1 && STRIDE == 1), "3 x 3 stride 1 / 2, or 1 x 1");
  __shared__ __attribute__((aligned(16))) uint16_t lds[conv_lds_elems<NPROD>()];
  int mt, nt;
  if (!conv_tile(a.nblk_m, a.nblk_n, mt, nt)) return;

  const int tid = threadIdx.x;
  const int skq = (tid & 3) * 8;
  const int KC = a.C / kConvBK;             // channel chunks per tap

  // the staged output pixels of this thread: the input row under the centre tap and which taps lie inside the input image
  long gx[kConvNP];
  unsigned live[kConvNP];
  const int HWo = a.Ho * a.Wo;
  const long HW = static_cast<long>(a.H) * a.W;
#pragma unroll
  for (int p = 0; p < kConvNP; ++p) {
    const long m = static_cast<long>(mt) * kConvBM + p * kConvRPP + (tid >> 2);
    gx[p] = 0;
    live[p] = 0;
    if (m < a.M) {
      const long img = m / HWo;
      const int r = static_cast<int>(m - img * HWo);
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      const int cy = STRIDE * oy, cx = STRIDE * ox;       // inside the image: cy <= H - 1, cx <= W - 1
      gx[p] = img * HW + static_cast<long>(cy) * a.W + cx;
      live[p] = conv_live_taps<TAPS>(cy, cx, a.H, a.W);
    }
  }

  auto fetch = [&](int c, int p, float4 &v0, float4 &v1) {
    const int tap = TAPS == 1 ? 0 : c / KC;
    const int ch = (c - tap * KC) * kConvBK;    // first input channel of the chunk
    const float *base = a.x + ch + skq;
    const long shift = TAPS == 1 ? 0 : static_cast<long>(tap / 3 - 1) * a.W + (tap % 3 - 1);
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((live[p] >> tap) & 1u) {            // the only place a row of x is addressed
      const float4 *src = reinterpret_cast<const float4 *>(base + (gx[p] + shift) * a.ldx);
      v0 = src[0];
      v1 = src[1];
    }
  };

  lin_f32x16 acc[2][2];
  conv_mainloop<NPROD>(lds, a.wpack, nt, TAPS * KC, a.relu_in, fetch, acc);

  long rrow[2];               // the row of res an output row adds (addressed only where m < M)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = conv_out_row(mt, i);
    rrow[i] = m;
    if (a.res_mode == 2 && m < a.M) {
      const long img = m / HWo;
      const int r = static_cast<int>(m - img * HWo);
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      const int Wc = a.Wo >> 1;
      rrow[i] = img * (HWo >> 2) + static_cast<long>(oy >> 1) * Wc + (ox >> 1);
    }
  }
  conv_epilogue(acc, mt, nt, a.M, a.N,
      [&](int n) { return a.bias ? *reinterpret_cast<const float4 *>(a.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f); },
      [&](const float4 &b, int i, long m, int n, float4 v) {
        if (a.bias) v = lin_add4(v, b);
        if (a.res_mode) v = lin_add4(v, *reinterpret_cast<const float4 *>(a.res + rrow[i] * a.ldres + n));
        *reinterpret_cast<float4 *>(a.y + m * a.ldy + n) = v;
      });
}

}  // namespace bevmsda
