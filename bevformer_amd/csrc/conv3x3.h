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
// This is the first form of the kernel: the body of linear_splitbf16_kernel<NPROD, false, 32, SWAP, 3> (128 x 128 block
// tile on four wavefronts, split-bf16 or bf16 operands, fp32 accumulate, packed weight chunks by LDS-DMA into a single
// W area) with a predicated, shifted A load.  A row of a tile is loaded nine times (once per tap); the form that stages
// the three halo runs once per channel chunk is not built.
//
// Memory safety: a row of x is addressed only under its tap's predicate (pixel inside the problem AND the tap inside the
// image), which keeps p + dy W + dx inside [0, bs H W); masked lanes load nothing and stage zeros.
//
// Epilogue: scale = gamma / sqrt(var + eps), shift = beta - mean * scale from the module's four vectors in the kernel
// (nothing derived from the running statistics lives on the host), y = acc * scale + shift, + res (16-byte reads), ReLU.
#pragma once
#include "linear_mfma.h"

namespace bevmsda {

constexpr int kConvMaxSeg = 8;
constexpr int kConvGran = 32;           // channels per segment and C_out are multiples of this

struct Conv3x3Args {
  const float *seg[kConvMaxSeg];        // A sources: segment s holds input channels [s cseg, (s + 1) cseg)
  long ldseg[kConvMaxSeg];              // row strides in floats
  int nseg, cseg;
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
  static_assert(NPROD == 1 || NPROD == 3, "NPROD: 1 = bf16 inputs, 3 = split-f32");
  constexpr bool LO = NPROD == 3;
  constexpr int BM = 128, BK = 32;
  constexpr int ROW = BK + 8;               // bf16 elements per LDS row (linear_mfma.h)
  constexpr int PLANE = 128 * ROW;
  constexpr int NPL = LO ? 2 : 1;
  constexpr int NP = 2, RPP = 64;           // staging: 4 threads per row, 64 rows per pass
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * NPL * PLANE];    // [A hi | A lo][W hi | W lo]
  uint16_t *const lds_a = lds;
  uint16_t *const lds_w = lds + NPL * PLANE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // XCD-aware tile map (linear_mfma.h)
  const int xcd = blockIdx.x & 7;
  const int seq = blockIdx.x >> 3;
  const int mt = (seq / a.nblk_n) * 8 + xcd;
  const int nt = seq % a.nblk_n;
  if (mt >= a.nblk_m) return;
  const long m0 = static_cast<long>(mt) * BM;
  const int n0 = nt * 128;

  const int srow = tid >> 2;
  const int skq = (tid & 3) * 8;
  const int KC = a.nseg * a.cseg / BK;      // channel chunks per tap
  const int nchunk = 9 * KC;

  // the staged pixels of this thread and, per pixel, which of the nine taps lie inside its image
  long gm[NP];
  unsigned live[NP];
  const long HW = static_cast<long>(a.H) * a.W;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const long m = m0 + p * RPP + srow;
    gm[p] = m;
    live[p] = 0;
    if (m < a.M) {
      const int r = static_cast<int>(m % HW);
      const int py = r / a.W, px = r - py * a.W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) live[p] |= 1u << t;
      }
    }
  }

  float4 xr[NP][2];
  auto load_chunk = [&](int c) {
    const int tap = c / KC;
    const int ch = (c - tap * KC) * BK;     // first input channel of the chunk
    const int s = ch / a.cseg;
    const float *sp = a.seg[0];             // (selects, not a dynamic index into the kernel arguments: that goes through scratch)
    long ld = a.ldseg[0];
#pragma unroll
    for (int i = 1; i < kConvMaxSeg; ++i)
      if (s == i) {
        sp = a.seg[i];
        ld = a.ldseg[i];
      }
    const float *base = sp + (ch - s * a.cseg) + skq;
    const long shift = static_cast<long>(tap / 3 - 1) * a.W + (tap % 3 - 1);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
      if ((live[p] >> tap) & 1u) {          // the only place a row of x is addressed
        const float4 *src = reinterpret_cast<const float4 *>(base + (gm[p] + shift) * ld);
        v0 = src[0];
        v1 = src[1];
      }
      xr[p][0] = v0;
      xr[p][1] = v1;
    }
  };
  // packed chunk (nt, c): NPL planes of 128 x 40 bf16, copied by LDS-DMA (destination = wave-uniform base + lane * 16)
  constexpr int WCH16 = NPL * PLANE / 8;
  constexpr int WPIECES = (WCH16 + 255) / 256;
  const uint4 *wchunk = reinterpret_cast<const uint4 *>(a.wpack) + static_cast<long>(nt) * nchunk * (2 * PLANE / 8);
  auto load_w = [&](int c) {
    const uint4 *src = wchunk + static_cast<long>(c) * (2 * PLANE / 8);
#pragma unroll
    for (int i = 0; i < WPIECES; ++i) {
      if (WCH16 % 256 == 0 || (i * 256 + (tid & ~63)) < WCH16) {     // wave-uniform tail guard
        uint16_t *dst = lds_w + (i * 256 + (tid & ~63)) * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i * 256 + tid),
                                         (__attribute__((address_space(3))) void *)(dst), 16, 0, 0);
      }
    }
  };

  lin_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31;
  const int fk = (lane >> 5) * 8;
  const int a_off = (wm * 64 + frow) * ROW + fk;
  const int b_off = (wn * 64 + frow) * ROW + fk;

  load_chunk(0);
  load_w(0);
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      uint4 hi, lo;
      const int off = (p * RPP + srow) * ROW + skq;
      lin_split8<LO>(xr[p][0], xr[p][1], hi, lo);
      *reinterpret_cast<uint4 *>(&lds_a[off]) = hi;
      if (LO) *reinterpret_cast<uint4 *>(&lds_a[PLANE + off]) = lo;
    }
    __syncthreads();          // staged chunk visible (the LDS-DMA in flight is drained here too)
    if (c + 1 < nchunk) load_chunk(c + 1);      // in flight under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      lin_bf16x8 ah[2], bh[2], al[2], bl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ao = a_off + t * 32 * ROW + ks * 16;
        const int bo = b_off + t * 32 * ROW + ks * 16;
        ah[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_a[ao]);
        bh[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_w[bo]);
        if (LO) {
          al[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_a[PLANE + ao]);
          bl[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_w[PLANE + bo]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {       // D[n][m]: the W fragment as the A operand (16-byte epilogue)
          if (LO) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], al[i], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl[j], ah[i], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], ah[i], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();          // every fragment of this chunk has been read
    if (c + 1 < nchunk) load_w(c + 1);
  }

  // Epilogue.  Registers 4g .. 4g + 3 of a lane are output columns nb + 8g .. + 3 of output row m = lane & 31.
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int nb = n0 + wn * 64 + j * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = nb + 8 * g;
      if (n >= a.N) continue;               // N % 4 == 0: n < N covers n .. n + 3
      const float4 ga = *reinterpret_cast<const float4 *>(a.gamma + n);
      const float4 be = *reinterpret_cast<const float4 *>(a.beta + n);
      const float4 mu = *reinterpret_cast<const float4 *>(a.mean + n);
      const float4 va = *reinterpret_cast<const float4 *>(a.var + n);
      float4 sc, sh;
      sc.x = ga.x / sqrtf(va.x + a.eps); sh.x = be.x - mu.x * sc.x;
      sc.y = ga.y / sqrtf(va.y + a.eps); sh.y = be.y - mu.y * sc.y;
      sc.z = ga.z / sqrtf(va.z + a.eps); sh.z = be.z - mu.z * sc.z;
      sc.w = ga.w / sqrtf(va.w + a.eps); sh.w = be.w - mu.w * sc.w;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long m = m0 + wm * 64 + i * 32 + (lane & 31);
        if (m >= a.M) continue;
        float4 v = make_float4(acc[i][j][4 * g] * sc.x + sh.x, acc[i][j][4 * g + 1] * sc.y + sh.y,
                               acc[i][j][4 * g + 2] * sc.z + sh.z, acc[i][j][4 * g + 3] * sc.w + sh.w);
        if (a.res) v = lin_add4(v, *reinterpret_cast<const float4 *>(a.res + m * a.ldres + n));
        if (a.relu) {                       // NaN stays NaN, as torch.relu
          v.x = v.x < 0.f ? 0.f : v.x;
          v.y = v.y < 0.f ? 0.f : v.y;
          v.z = v.z < 0.f ? 0.f : v.z;
          v.w = v.w < 0.f ? 0.f : v.w;
        }
        *reinterpret_cast<float4 *>(a.y + m * a.ldy + n) = v;
      }
    }
  }
}

// Weight image: the (C_out, C_in, 3, 3) weight as the (C_out, 9 C_in) matrix with k = tap * C_in + ci, in
// lin_pack_weight_kernel's format — for every (128-row tile, 32-deep chunk) a contiguous [plane hi | plane lo][128][32 + 8 pad]
// bf16 block, chunks in the order the main loop consumes them (tap-major).  One thread per 8 input channels of a (co, tap).
__global__ void __launch_bounds__(256) conv3x3_pack_weight_kernel(const float *__restrict__ w, int N, int C,
                                                                 uint16_t *__restrict__ blob) {
  constexpr int ROW = 40, PLANE = 128 * ROW;
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
