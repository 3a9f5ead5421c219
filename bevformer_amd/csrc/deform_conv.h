// Modulated deformable 3 x 3 convolution (DCNv2) over channel-last rows on the CDNA4 matrix cores: conv2 of the stage-3 and
// stage-4 bottlenecks of the reference's ResNet-101 backbone (bevformer_base.py:43-53, dcn=dict(type='DCNv2', deform_groups=1)).
//
//   y[q, co] = act( ep( sum_{k = 3 i + j} sigmoid(logit_k(q)) sum_ci w[co, ci, i, j] *
//                       bilin(x[img, :, :, ci], S oy - 1 + i + dy_k(q), S ox - 1 + j + dx_k(q)) ) )
//
// q runs over the n_img * Ho * Wo OUTPUT pixels, (img, oy, ox) as in conv_rows.h, Ho = (H - 1) div S + 1; padding 1, dilation 1,
// groups 1, deform_groups 1.  bilin is bilinear interpolation in pixel coordinates whose corners outside [0, H) x [0, W)
// contribute zero (grid_sample(align_corners=True, padding_mode='zeros')).  A sample position that is not finite or lies
// outside (-1, H) x (-1, W) contributes exactly zero and addresses nothing.  The offsets are a row matrix: row q of offs holds
// the raw output of the pack's conv_offset at q — column 2 k is dy_k, 2 k + 1 is dx_k, 18 + k the mask logit (mmcv's chunk(3) +
// cat(o1, o2) with its interleaved offset layout, read in place); columns 27 .. 31 are padding.
//
// The GEMM is conv_mfma.h's, unchanged: the same main loop, weight image (k = tap * C_in + ci) and tile map as conv_rows_kernel.
// This header supplies the fetch — when a chunk is the first of its tap, the four corner rows and the four coefficients of
// the staged output row (sigmoid of the mask folded in) from its offs row; then 8 floats from each live corner, blended in
// fp32 — and the epilogue: + bias, or the inference BatchNorm of conv3x3.h, then an optional ReLU.
//
// Memory safety: the position is range-checked in floating point BEFORE any float -> int conversion (NaN, +-inf, 1e30 fail the
// compares and are dead taps), so the converted coordinates lie in [-1, H - 1] x [-1, W - 1]; a row of x is addressed only
// under m < M AND its corner inside the image; a row of offs and of y only under m < M.  Dead corners load nothing.
#pragma once
#include "conv_mfma.h"
#include "scalar_ops.h"

namespace bevmsda {

struct DeformConvArgs {
  const float *x;                       // (n_img * H * W, ldx) input rows
  long ldx;
  const float *offs;                    // (M, ldoffs >= 32) offset rows
  long ldoffs;
  const uint16_t *wpack;
  const float *bias;                    // (N) or nullptr
  const float *gamma, *beta, *mean, *var;       // all four (BatchNorm) or all nullptr
  float eps;
  float *y;
  long ldy;
  long M;                               // n_img * Ho * Wo
  int H, W, Ho, Wo;
  int C, N;                             // C_in, C_out: multiples of kConvGran
  int relu;
  int nblk_m, nblk_n;
};

// One tap of one output pixel, from its offs row (this kernel's fetch and the backward kernels of deform_conv_bwd.h): the row
// of corner (y0, x0) — the other three are + 1, + W, + W + 1 —, which corners lie inside the image (bits 0 .. 3 = (y0, x0),
// (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)), the bilinear fractions and the sigmoid of the mask logit.
struct DeformTap {
  int crow;
  unsigned live;                        // 0: a dead position — nothing else is set and nothing may be addressed
  float ly, lx, hy, hx, mask;
};

// orow: the pixel's offs row (addressed here: the caller holds m < M); (ty, tx) the window's top-left input pixel; img0 the
// first row of the image.  The range check is in floating point, before any conversion: NaN fails every compare.
__device__ __forceinline__ bool deform_tap(const float *orow, int tap, int ty, int tx, int img0, int H, int W, DeformTap &t) {
  const float2 d = *reinterpret_cast<const float2 *>(orow + 2 * tap);
  const float logit = orow[18 + tap];
  const float py = static_cast<float>(ty + tap / 3) + d.x;
  const float px = static_cast<float>(tx + tap % 3) + d.y;
  t.live = 0;
  if (!(py > -1.f && py < static_cast<float>(H) && px > -1.f && px < static_cast<float>(W))) return false;
  const float fy = floorf(py), fx = floorf(px);
  const int y0 = static_cast<int>(fy), x0 = static_cast<int>(fx);     // in [-1, H - 1] x [-1, W - 1]
  t.ly = py - fy;
  t.lx = px - fx;
  t.mask = 1.f / (1.f + expf(-logit));
  t.hy = 1.f - t.ly;
  t.hx = 1.f - t.lx;
  const bool tp = y0 >= 0, b = y0 + 1 < H, l = x0 >= 0, r = x0 + 1 < W;
  t.live = (tp && l ? 1u : 0u) | (tp && r ? 2u : 0u) | (b && l ? 4u : 0u) | (b && r ? 8u : 0u);
  t.crow = img0 + y0 * W + x0;
  return true;
}

// Register budget: the four corner loads of both staged rows raise the pressure over conv_rows_kernel; under
// amdgpu_waves_per_eu(3, 3) the compiler reports 154 (split) / 150 (bf16) VGPR, no AGPR, no scratch — inside the 168 of three
// waves per SIMD, which is also what the LDS allows (three workgroups per CU, conv_mfma.h).  Left at (2, 2) it takes 178 / 149.
template <int NPROD, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) deform_conv_rows_kernel(const DeformConvArgs a) {
  static_assert(STRIDE == 1 || STRIDE == 2, "stride 1 / 2");
  __shared__ __attribute__((aligned(16))) uint16_t lds[conv_lds_elems<NPROD>()];
  int mt, nt;
  if (!conv_tile(a.nblk_m, a.nblk_n, mt, nt)) return;

  const int tid = threadIdx.x;
  const int skq = (tid & 3) * 8;
  const int KC = a.C / kConvBK;             // channel chunks per tap

  // the staged output pixels of this thread: the offs row, the first row of the image, the window's top-left input pixel
  const float *orow[kConvNP];               // nullptr: m >= M
  int img0[kConvNP], ty[kConvNP], tx[kConvNP];
  const int HWo = a.Ho * a.Wo;
#pragma unroll
  for (int p = 0; p < kConvNP; ++p) {
    const long m = static_cast<long>(mt) * kConvBM + p * kConvRPP + (tid >> 2);
    orow[p] = nullptr;
    img0[p] = ty[p] = tx[p] = 0;
    if (m < a.M) {
      const int img = static_cast<int>(m / HWo);
      const int r = static_cast<int>(m - static_cast<long>(img) * HWo);
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      orow[p] = a.offs + m * a.ldoffs;
      img0[p] = img * a.H * a.W;            // < 2^24 (the entry point's bound)
      ty[p] = STRIDE * oy - 1;
      tx[p] = STRIDE * ox - 1;
    }
  }

  // per staged row, set by the fetch of a tap's first chunk: the row of corner (y0, x0) — the other three are + 1, + W,
  // + W + 1 —, which corners lie inside the image (bits 0 .. 3 = (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)) and
  // their coefficients
  int crow[kConvNP];
  unsigned live[kConvNP];
  float cf[kConvNP][4];
#pragma unroll
  for (int p = 0; p < kConvNP; ++p) {
    crow[p] = 0;
    live[p] = 0;
    cf[p][0] = cf[p][1] = cf[p][2] = cf[p][3] = 0.f;
  }

  auto fetch = [&](int c, int p, float4 &v0, float4 &v1) {
    const int tap = c / KC;
    const int kc = c - tap * KC;
    if (kc == 0) {                          // the chunk index crossed a multiple of C_in / 32: a new tap
      live[p] = 0;
      if (orow[p]) {
        DeformTap t;
        if (deform_tap(orow[p], tap, ty[p], tx[p], img0[p], a.H, a.W, t)) {
          cf[p][0] = mul_scalar(t.mask, mul_scalar(t.hy, t.hx));
          cf[p][1] = mul_scalar(t.mask, mul_scalar(t.hy, t.lx));
          cf[p][2] = mul_scalar(t.mask, mul_scalar(t.ly, t.hx));
          cf[p][3] = mul_scalar(t.mask, mul_scalar(t.ly, t.lx));
          live[p] = t.live;
          crow[p] = t.crow;
        }
      }
    }
    const float *base = a.x + kc * kConvBK + skq;
    float4 q[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q[k][0] = q[k][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((live[p] >> k) & 1u) {            // the only place a row of x is addressed
        const long row = crow[p] + (k >> 1) * a.W + (k & 1);
        const float4 *src = reinterpret_cast<const float4 *>(base + row * a.ldx);
        q[k][0] = src[0];
        q[k][1] = src[1];
      }
    }
    // the blend, in fp32, ((c0 q0 + c1 q1) + c2 q2) + c3 q3 with fused multiply-adds; scalar_ops.h: a coefficient broadcast from
    // the high half of a register pair is the packed form the library must not contain
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live[p]) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float4 &v = h ? v1 : v0;
        v.x = mul_scalar(cf[p][0], q[0][h].x); v.y = mul_scalar(cf[p][0], q[0][h].y);
        v.z = mul_scalar(cf[p][0], q[0][h].z); v.w = mul_scalar(cf[p][0], q[0][h].w);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
          v.x = fma_scalar(cf[p][k], q[k][h].x, v.x);
          v.y = fma_scalar(cf[p][k], q[k][h].y, v.y);
          v.z = fma_scalar(cf[p][k], q[k][h].z, v.z);
          v.w = fma_scalar(cf[p][k], q[k][h].w, v.w);
        }
      }
    }
  };

  lin_f32x16 acc[2][2];
  conv_mainloop<NPROD>(lds, a.wpack, nt, 9 * KC, 0, fetch, acc);

  struct ScaleShift { float4 sc, sh; };
  const bool bn = a.gamma != nullptr;
  conv_epilogue(acc, mt, nt, a.M, a.N,
      [&](int n) {
        ScaleShift s;
        s.sc = make_float4(1.f, 1.f, 1.f, 1.f);
        s.sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bn) {                           // conv3x3.h's: scale = gamma / sqrt(var + eps), shift = beta - mean * scale
          const float4 ga = *reinterpret_cast<const float4 *>(a.gamma + n);
          const float4 be = *reinterpret_cast<const float4 *>(a.beta + n);
          const float4 mu = *reinterpret_cast<const float4 *>(a.mean + n);
          const float4 va = *reinterpret_cast<const float4 *>(a.var + n);
          s.sc.x = ga.x / sqrtf(va.x + a.eps); s.sh.x = be.x - mu.x * s.sc.x;
          s.sc.y = ga.y / sqrtf(va.y + a.eps); s.sh.y = be.y - mu.y * s.sc.y;
          s.sc.z = ga.z / sqrtf(va.z + a.eps); s.sh.z = be.z - mu.z * s.sc.z;
          s.sc.w = ga.w / sqrtf(va.w + a.eps); s.sh.w = be.w - mu.w * s.sc.w;
        } else if (a.bias) {
          s.sh = *reinterpret_cast<const float4 *>(a.bias + n);
        }
        return s;
      },
      [&](const ScaleShift &s, int, long m, int n, float4 v) {
        if (bn) v = make_float4(v.x * s.sc.x + s.sh.x, v.y * s.sc.y + s.sh.y, v.z * s.sc.z + s.sh.z, v.w * s.sc.w + s.sh.w);
        else if (a.bias) v = lin_add4(v, s.sh);
        if (a.relu) conv_relu4(v);
        *reinterpret_cast<float4 *>(a.y + m * a.ldy + n) = v;
      });
}

}  // namespace bevmsda
