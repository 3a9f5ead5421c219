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
// The body is conv3x3_bn_kernel's (conv3x3.h; that kernel and its entry points are untouched): 128 x 128 block tile on
// four wavefronts, split-bf16 or bf16 operands with fp32 accumulate, packed weight chunks by LDS-DMA into a single W area,
// a predicated, shifted A load with the next chunk in flight under the MFMAs, the XCD-aware tile map, the transposed
// accumulator tile for 16-byte stores.  What differs: one source matrix instead of segments, the tap count and the stride
// as template parameters, the input row index through (img, oy, ox), an optional ReLU on the A operand before the split
// (relu_before_extra_convs; NaN stays NaN), and the epilogue: + bias, then + res, where res is a same-shape row matrix
// (mode 1) or the 2 x nearest upsampling of a coarser map (mode 2): rrow(q) = img Hc Wc + (oy >> 1) Wc + (ox >> 1) with
// Ho = 2 Hc, Wo = 2 Wc — F.interpolate(size=, mode='nearest') for an exact factor of 2.
//
// Memory safety: a row of x is addressed only under its tap's predicate (output pixel inside the problem AND the tap
// inside the input image), a row of res and of y only for an output pixel inside the problem; masked lanes load nothing
// and stage zeros.  The weight image is lin_pack_weight_kernel's over the (C_out, taps * C_in) matrix with
// k = tap * C_in + ci: conv3x3_pack_weight_kernel's for 9 taps, the linear pack of the (C_out, C_in) matrix for 1.
#pragma once
#include "linear_mfma.h"

namespace bevmsda {

constexpr int kConvRowsGran = 32;       // C_in and C_out are multiples of this

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
  int C, N;                             // C_in, C_out
  int relu_in;
  int nblk_m, nblk_n;
};

template <int NPROD, int TAPS, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) conv_rows_kernel(const ConvRowsArgs a) {
  static_assert(NPROD == 1 || NPROD == 3, "NPROD: 1 = bf16 inputs, 3 = split-f32");
  static_assert((TAPS == 9 && (STRIDE == 1 || STRIDE == 2)) || (TAPS == 1 && STRIDE == 1), "3 x 3 stride 1 / 2, or 1 x 1");
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
  const int KC = a.C / BK;                  // channel chunks per tap
  const int nchunk = TAPS * KC;

  // the staged output pixels of this thread: the input row under the centre tap and which taps lie inside the input image
  long gx[NP];
  unsigned live[NP];
  const int HWo = a.Ho * a.Wo;
  const long HW = static_cast<long>(a.H) * a.W;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const long m = m0 + p * RPP + srow;
    gx[p] = 0;
    live[p] = 0;
    if (m < a.M) {
      const long img = m / HWo;
      const int r = static_cast<int>(m - img * HWo);
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      const int cy = STRIDE * oy, cx = STRIDE * ox;       // inside the image: cy <= H - 1, cx <= W - 1
      gx[p] = img * HW + static_cast<long>(cy) * a.W + cx;
      if (TAPS == 1) {
        live[p] = 1u;
      } else {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int yy = cy + t / 3 - 1, xx = cx + t % 3 - 1;
          if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) live[p] |= 1u << t;
        }
      }
    }
  }

  float4 xr[NP][2];
  auto load_chunk = [&](int c) {
    const int tap = TAPS == 1 ? 0 : c / KC;
    const int ch = (c - tap * KC) * BK;     // first input channel of the chunk
    const float *base = a.x + ch + skq;
    const long shift = TAPS == 1 ? 0 : static_cast<long>(tap / 3 - 1) * a.W + (tap % 3 - 1);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
      if ((live[p] >> tap) & 1u) {          // the only place a row of x is addressed
        const float4 *src = reinterpret_cast<const float4 *>(base + (gx[p] + shift) * a.ldx);
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

  auto relu4 = [](float4 &v) {              // NaN stays NaN, as torch.relu
    v.x = v.x < 0.f ? 0.f : v.x;
    v.y = v.y < 0.f ? 0.f : v.y;
    v.z = v.z < 0.f ? 0.f : v.z;
    v.w = v.w < 0.f ? 0.f : v.w;
  };

  load_chunk(0);
  load_w(0);
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      uint4 hi, lo;
      const int off = (p * RPP + srow) * ROW + skq;
      if (a.relu_in) {                      // on the A operand, before the split
        relu4(xr[p][0]);
        relu4(xr[p][1]);
      }
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
  long rrow[2];               // the row of res an output row adds (addressed only where m < M)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = m0 + wm * 64 + i * 32 + (lane & 31);
    rrow[i] = m;
    if (a.res_mode == 2 && m < a.M) {
      const long img = m / HWo;
      const int r = static_cast<int>(m - img * HWo);
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      const int Wc = a.Wo >> 1;
      rrow[i] = img * (HWo >> 2) + static_cast<long>(oy >> 1) * Wc + (ox >> 1);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int nb = n0 + wn * 64 + j * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = nb + 8 * g;
      if (n >= a.N) continue;               // N % 4 == 0: n < N covers n .. n + 3
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.bias) b = *reinterpret_cast<const float4 *>(a.bias + n);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long m = m0 + wm * 64 + i * 32 + (lane & 31);
        if (m >= a.M) continue;
        float4 v = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        if (a.bias) v = lin_add4(v, b);
        if (a.res_mode) v = lin_add4(v, *reinterpret_cast<const float4 *>(a.res + rrow[i] * a.ldres + n));
        *reinterpret_cast<float4 *>(a.y + m * a.ldy + n) = v;
      }
    }
  }
}

}  // namespace bevmsda
