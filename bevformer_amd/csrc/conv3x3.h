// 3 x 3 convolution over channel-last BEV rows + inference BatchNorm (+ residual) (+ ReLU) on the CDNA4 matrix cores:
// the blocks of ResNetFusion (modules/transformer.py), BEVFormerV2's temporal fusion.
//
//   y[p, co] = act( bn_co( sum_{dy, dx in {-1, 0, 1}} sum_ci x[p + dy W + dx, ci] * w[co, ci, dy + 1, dx + 1] ) + res[p, co] )
//
// p runs over bs * H * W pixels, (y, x) = ((p mod H W) div W, p mod W); a tap contributes only where 0 <= y + dy < H and
// 0 <= x + dx < W (zero padding 1, stride 1, dilation 1, groups 1, no bias).  The BEV maps of this project ARE
// (bs, H W, C) rows, so the convolution is the NT GEMM of linear_mfma.h with K = 9 C_in whose A operand for K chunk
// (tap, ci) is the row matrix shifted by dy W + dx: no permute to NCHW, no im2col buffer.  C_in may be spread over up to
// kConvMaxSeg source tensors of equal width (the frames' BEV rows read in place instead of their concatenation); a
// segment may be listed more than once.
//
// This is the first form of the kernel: conv_mfma.h's main loop (128 x 128 block tile on four wavefronts, split-bf16 or bf16
// operands, fp32 accumulate, packed weight chunks by LDS-DMA) over K = 9 C_in chunks of 32, and its epilogue walk.  This
// header supplies what is this kernel's own: the fetch of a staged row — the segment of the chunk's channels, selected by
// compares, shifted by the chunk's tap, under that tap's predicate — and the epilogue on four columns.  A row of a tile is
// loaded nine times (once per tap); the form that stages the three halo runs once per channel chunk is not built.
//
// Memory safety: a row of x is addressed only under its tap's predicate (pixel inside the problem AND the tap inside the
// image), which keeps p + dy W + dx inside [0, bs H W); masked lanes load nothing and stage zeros.
//
// Epilogue: scale = gamma / sqrt(var + eps), shift = beta - mean * scale from the module's four vectors in the kernel
// (nothing derived from the running statistics lives on the host), y = acc * scale + shift, + res (16-byte reads), ReLU.
#pragma once
#include "conv_mfma.h"

namespace bevmsda {

constexpr int kConvMaxSeg = 8;

struct Conv3x3Args {
  const float *seg[kConvMaxSeg];        // A sources: segment s holds input channels [s cseg, (s + 1) cseg)
  long ldseg[kConvMaxSeg];              // row strides in floats
  int nseg, cseg;                       // cseg and N are multiples of kConvGran
  const uint16_t *wpack;                // conv3x3_pack_weight_kernel's image
  const float *gamma, *beta, *mean, *var;
  float eps;
  const float *res;                     // (M, ldres) or nullptr
  long ldres;
  float *y;
  long ldy;
  long M;                               // bs * H * W
  int H, W, N;                          // N = C_out
  int relu;
  int nblk_m, nblk_n;
};

template <int NPROD>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) conv3x3_bn_kernel(const Conv3x3Args a) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[conv_lds_elems<NPROD>()];
  int mt, nt;
  if (!conv_tile(a.nblk_m, a.nblk_n, mt, nt)) return;

  const int tid = threadIdx.x;
  const int skq = (tid & 3) * 8;
  const int KC = a.nseg * a.cseg / kConvBK;     // channel chunks per tap

  // the staged pixels of this thread and, per pixel, which of the nine taps lie inside its image
  long gm[kConvNP];
  unsigned live[kConvNP];
  const long HW = static_cast<long>(a.H) * a.W;
#pragma unroll
  for (int p = 0; p < kConvNP; ++p) {
    const long m = static_cast<long>(mt) * kConvBM + p * kConvRPP + (tid >> 2);
    gm[p] = m;
    live[p] = 0;
    if (m < a.M) {
      const int r = static_cast<int>(m % HW);
      const int py = r / a.W, px = r - py * a.W;
      live[p] = conv_live_taps<9>(py, px, a.H, a.W);
    }
  }

  // the chunk's segment (selected by compares), channel offset and tap shift: set by the fetch of the chunk's first row
  const float *base = nullptr;
  long ld = 0, shift = 0;
  int tap = 0;
  auto fetch = [&](int c, int p, float4 &v0, float4 &v1) {
    if (p == 0) {
      tap = c / KC;
      const int ch = (c - tap * KC) * kConvBK;  // first input channel of the chunk
      const int s = ch / a.cseg;
      const float *sp = a.seg[0];           // (selects, not a dynamic index into the kernel arguments: that goes through scratch)
      ld = a.ldseg[0];
#pragma unroll
      for (int i = 1; i < kConvMaxSeg; ++i)
        if (s == i) {
          sp = a.seg[i];
          ld = a.ldseg[i];
        }
      base = sp + (ch - s * a.cseg) + skq;
      shift = static_cast<long>(tap / 3 - 1) * a.W + (tap % 3 - 1);
    }
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((live[p] >> tap) & 1u) {            // the only place a row of x is addressed
      const float4 *src = reinterpret_cast<const float4 *>(base + (gm[p] + shift) * ld);
      v0 = src[0];
      v1 = src[1];
    }
  };

  lin_f32x16 acc[2][2];
  conv_mainloop<NPROD>(lds, a.wpack, nt, 9 * KC, 0, fetch, acc);

  struct ScaleShift { float4 sc, sh; };
  conv_epilogue(acc, mt, nt, a.M, a.N,
      [&](int n) {
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

// Weight image: the (C_out, C_in, 3, 3) weight as the (C_out, 9 C_in) matrix with k = tap * C_in + ci, in
// lin_pack_weight_kernel's format — for every (128-row tile, 32-deep chunk) a contiguous [plane hi | plane lo][128][32 + 8 pad]
// bf16 block, chunks in the order the main loop consumes them (tap-major).  One thread per 8 input channels of a (co, tap).
__global__ void __launch_bounds__(256) conv3x3_pack_weight_kernel(const float *__restrict__ w, int N, int C,
                                                                 uint16_t *__restrict__ blob) {
  constexpr int ROW = kConvRow, PLANE = kConvPlane;
  const int K = 9 * C;
  const int kch = K / 32;
  const long rows = static_cast<long>((N + 127) / 128) * 128;
  const long t = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= rows * (K / 8)) return;
  const int n = static_cast<int>(t / (K / 8));
  const int k = static_cast<int>(t % (K / 8)) * 8;
  uint4 hi = make_uint4(0, 0, 0, 0), lo = hi;
  if (n < N) {
    const int tap = k / C, ci = k - tap * C;        // C % 32 == 0: the 8 k share a tap
    const float *src = w + (static_cast<long>(n) * C + ci) * 9 + tap;
    lin_split8<true>(make_float4(src[0], src[9], src[18], src[27]), make_float4(src[36], src[45], src[54], src[63]), hi, lo);
  }
  uint16_t *chunk = blob + (static_cast<long>(n / 128) * kch + k / 32) * (2 * PLANE);
  const int off = (n % 128) * ROW + (k % 32);
  *reinterpret_cast<uint4 *>(chunk + off) = hi;
  *reinterpret_cast<uint4 *>(chunk + PLANE + off) = lo;
  if (k % 32 == 24) {       // the 16-byte row pad
    *reinterpret_cast<uint4 *>(chunk + off + 8) = make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4 *>(chunk + PLANE + off + 8) = make_uint4(0, 0, 0, 0);
  }
}

}  // namespace bevmsda
