// Convolution over channel-last rows + inference BatchNorm (+ residual) (+ ReLU) on the CDNA4 matrix cores: the plain
// convolutions of a ResNet bottleneck (mmdet's backbone as the reference configs build it, bevformer_base.py:43-53) — conv1
// and conv3 (1 x 1), the plain conv2 (3 x 3), the downsample (1 x 1), each at stride 1 or 2 — with the norm that follows
// each, the block's residual sum and its ReLU in the epilogue.
//
//   y[q, co] = act( bn_co( sum_{taps (dy, dx)} sum_ci x[row(q, dy, dx), ci] * w[co, ci, dy + 1, dx + 1] ) + res[q, co] )
//
// q runs over the n_img * Ho * Wo OUTPUT pixels, (img, oy, ox) as in conv_rows.h: row(q, dy, dx) = img H W + (S oy + dy) W +
// (S ox + dx), S the stride, Ho = (H - 1) div S + 1, Wo = (W - 1) div S + 1.  The 9-tap form has zero padding 1 (a tap is live
// only inside the input image); the 1-tap form is the 1 x 1 convolution, dy = dx = 0, padding 0 — at stride 2 (caffe-style
// conv1, every downsample) its only tap reads input pixel (2 oy, 2 ox), which always lies inside the image.
//
// The GEMM is conv_mfma.h's, unchanged.  This header combines what two kernels already have: conv_rows_kernel's fetch (tap
// count and stride as template parameters, the input row through (img, oy, ox)) and conv3x3_bn_kernel's epilogue, with the
// same expressions — scale = gamma / sqrt(var + eps), shift = beta - mean * scale from the module's four vectors in the
// kernel, y = acc * scale + shift, + res (16-byte reads), ReLU (NaN stays NaN) — so that it gives that kernel's bits on that
// kernel's problem.
//
// Memory safety: a row of x is addressed only under its tap's predicate (output pixel inside the problem AND the tap inside
// the input image), a row of res and of y only for an output pixel inside the problem; masked lanes load nothing and stage
// zeros.  The weight image is conv3x3_pack_weight_kernel's for 9 taps, the linear pack of the (C_out, C_in) matrix for 1.
#pragma once
#include "conv_mfma.h"

namespace bevmsda {

struct ConvBnRowsArgs {
  const float *x;                       // (n_img * H * W, ldx) input rows
  long ldx;
  const uint16_t *wpack;
  const float *gamma, *beta, *mean, *var;       // (N) each
  float eps;
  const float *res;                     // (M, ldres) or nullptr
  long ldres;
  float *y;
  long ldy;
  long M;                               // n_img * Ho * Wo
  int H, W, Ho, Wo;
  int C, N;                             // C_in, C_out: multiples of kConvGran
  int relu;
  int nblk_m, nblk_n;
};

template <int NPROD, int TAPS, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) conv_bn_rows_kernel(const ConvBnRowsArgs a) {
  static_assert((TAPS == 9 || TAPS == 1) && (STRIDE == 1 || STRIDE == 2), "3 x 3 or 1 x 1, stride 1 / 2");
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
      if (TAPS == 1 && STRIDE == 1) {       // output pixel q is input pixel q
        gx[p] = m;
        live[p] = 1u;
      } else {
        const long img = m / HWo;
        const int r = static_cast<int>(m - img * HWo);
        const int oy = r / a.Wo, ox = r - oy * a.Wo;
        const int cy = STRIDE * oy, cx = STRIDE * ox;     // inside the image: cy <= H - 1, cx <= W - 1
        gx[p] = img * HW + static_cast<long>(cy) * a.W + cx;
        live[p] = conv_live_taps<TAPS>(cy, cx, a.H, a.W);
      }
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
  conv_mainloop<NPROD>(lds, a.wpack, nt, TAPS * KC, 0, fetch, acc);

  struct ScaleShift { float4 sc, sh; };
  conv_epilogue(acc, mt, nt, a.M, a.N,
      [&](int n) {                          // conv3x3.h's, expression for expression
        const float4 ga = *reinterpret_cast<const float4 *>(a.gamma + n);
        const float4 be = *reinterpret_cast<const float4 *>(a.beta + n);
        const float4 mu = *reinterpret_cast<const float4 *>(a.mean + n);
        const float4 va = *reinterpret_cast<const float4 *>(a.var + n);
        ScaleShift s;
        s.sc.x = ga.x / sqrtf(va.x + a.eps); s.sh.x = be.x - mu.x * s.sc.x;
        s.sc.y = ga.y / sqrtf(va.y + a.eps); s.sh.y = be.y - mu.y * s.sc.y;
        s.sc.z = ga.z / sqrtf(va.z + a.eps); s.sh.z = be.z - mu.z * s.sc.z;
        s.sc.w = ga.w / sqrtf(va.w + a.eps); s.sh.w = be.w - mu.w * s.sc.w;
        return s;
      },
      [&](const ScaleShift &s, int, long m, int n, float4 v) {
        v = make_float4(v.x * s.sc.x + s.sh.x, v.y * s.sc.y + s.sh.y, v.z * s.sc.z + s.sh.z, v.w * s.sc.w + s.sh.w);
        if (a.res) v = lin_add4(v, *reinterpret_cast<const float4 *>(a.res + m * a.ldres + n));
        if (a.relu) conv_relu4(v);
        *reinterpret_cast<float4 *>(a.y + m * a.ldy + n) = v;
      });
}

}  // namespace bevmsda
