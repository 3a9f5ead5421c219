// Backward of the modulated deformable 3 x 3 convolution of deform_conv.h over channel-last rows on the CDNA4 matrix cores: the
// gradient with respect to the input rows, the offsets and mask logits, and the weight — conv2 of a stage-3 / stage-4 bottleneck
// trained with frozen norms (conv_bwd_rows.h).  In the forward's notation, stride S 1 or 2, taps k = 3 i + j:
//
//   col[q, k, ci] = m_k(q) * sum_{corner c} b_c(q, k) * x[row_c(q, k), ci]
//   z[q, co]      = sum_{k, ci} w[co, ci, i, j] * col[q, k, ci]
//
// m_k the sigmoid of the mask logit, b_c the four bilinear coefficients of ly, lx, hy = 1 - ly, hx = 1 - lx; a dead corner counts
// as zero, a dead position (not finite, or outside (-1, H) x (-1, W)) contributes nothing.  gz[q, co] is the gradient w.r.t. z,
// read through (g, y, gamma, var) as in conv_bwd_rows.h.  With dcol[q, k, ci] = sum_co gz[q, co] w[co, ci, i, j] and v_c =
// x[row_c, ci] (0 for a dead corner):
//
//   dW[co, ci, i, j]  = sum_q gz[q, co] * col[q, k, ci]
//   dx[row_c, ci]    += m_k * b_c * dcol[q, k, ci]                               (live corners only)
//   d logit_k(q)      = m_k (1 - m_k) * sum_ci dcol * sum_c b_c v_c
//   d dy_k(q)         = m_k * sum_ci dcol * ((v10 - v00) hx + (v11 - v01) lx)
//   d dx_k(q)         = m_k * sum_ci dcol * ((v01 - v00) hy + (v11 - v10) ly)
//
// floor has zero slope: at an integer position the slope is the one of the cell floor selects (lx = 0, x0 = px).  A dead position
// gives exactly zero for all three and addresses nothing.  m (1 - m) is formed from m: a logit of -inf gives 0, not NaN.
//
// Input and offset gradient (deform_conv_dgrad_rows_kernel): conv_mfma.h's main loop as the dcol GEMM — rows = output pixels,
// reduction = C_out (the fetch is conv_gz4 on the gz row), columns n = k C_in + ci (deform_dgrad_pack_weight_kernel's image).  dcol
// is never stored: in the epilogue a lane holds, for output row lane & 31 of two tiles, 16 columns of each 32-column group, and a
// group lies inside one tap (C_in % 32 == 0).  Per (row, tap) the lane rebuilds the position from the offs row (deform_tap), adds
// m_k b_c dcol to the live corners' dx rows with fp32 atomics, loads the corners' x values of its columns, forms its part of
// the three sums over ci, adds its partner's (lane ^ 32 holds the other 16 columns of the same row) and adds the result with
// atomics into doffs[q, 2 k], doffs[q, 2 k + 1], doffs[q, 18 + k] — an (M, >= 32) row matrix in offs's layout whose columns 27 ..
// 31 are never written.  The caller zero-fills dx and doffs; either may be left out (nullptr).  Run-to-run bit equality is not a
// goal.  Atomics per launch: 4 * 9 * C_in * M for dx (fewer at dead corners), 27 * C_in / 32 * M for doffs.
//
// Weight gradient (deform_conv_wgrad_rows_kernel): conv_wgrad_rows_kernel with a deformable x operand — the same tile (128 co x
// 128 ci of one tap over a slice of output pixels), LDS ring, XCD map and atomics into w's own layout; a staged x row is
// col[q, tap, ci .. ci + 3]: the coefficients from the offs row, four predicated corner loads and the forward's fp32 blend.
//
// Memory safety: the position is range-checked in floating point BEFORE any float -> int conversion (NaN, +-inf, 1e30 fail the
// compares and are dead taps), so the converted coordinates lie in [-1, H - 1] x [-1, W - 1]; a row of x or dx is addressed only
// under m < M AND its corner inside the image; a row of offs, doffs, g or y only under m < M.  Dead corners and dead positions
// load nothing, add nothing and stage zeros.  Every row index is below 2^24 (the C ABI's bound) and is multiplied by a row stride
// in 64 bits.
#pragma once
#include "conv_bwd_rows.h"
#include "deform_conv.h"

namespace bevmsda {

// ---- the input gradient and the offset / mask gradient
struct DeformDgradArgs {
  ConvGzSrc s;                          // over the M output pixels, N columns
  const uint16_t *wpack;                // deform_dgrad_pack_weight_kernel's image
  const float *x;                       // (n_img * H * W, ldx) input rows (read for doffs only)
  long ldx;
  const float *offs;                    // (M, ldoffs >= 32) offset rows
  long ldoffs;
  float *dx;                            // (n_img * H * W, lddx), accumulated into, or nullptr
  long lddx;
  float *doffs;                         // (M, lddoffs >= 32), accumulated into, or nullptr
  long lddoffs;
  long M;                               // n_img * Ho * Wo
  int H, W, Ho, Wo;
  int C, N;                             // C_in, C_out (the reduction): multiples of kConvGran
  int nblk_m, nblk_n;                   // row tiles, column tiles of the (M, 9 C_in) dcol matrix
};

template <int NPROD, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) deform_conv_dgrad_rows_kernel(const DeformDgradArgs a) {
  static_assert(STRIDE == 1 || STRIDE == 2, "stride 1 / 2");
  __shared__ __attribute__((aligned(16))) uint16_t lds[conv_lds_elems<NPROD>()];
  int mt, nt;
  if (!conv_tile(a.nblk_m, a.nblk_n, mt, nt)) return;

  const int tid = threadIdx.x;
  const int skq = (tid & 3) * 8;

  long mrow[kConvNP];                       // the staged output pixels of this thread; -1: m >= M
#pragma unroll
  for (int p = 0; p < kConvNP; ++p) {
    const long m = static_cast<long>(mt) * kConvBM + p * kConvRPP + (tid >> 2);
    mrow[p] = m < a.M ? m : -1;
  }

  const bool scaled = a.s.gamma != nullptr;
  float4 sc0 = make_float4(1.f, 1.f, 1.f, 1.f), sc1 = sc0;     // the scale of the chunk's 8 channels: set by the chunk's first fetch
  auto fetch = [&](int c, int p, float4 &v0, float4 &v1) {
    const int ch = c * kConvBK + skq;       // first of this thread's 8 output channels: ch + 7 < C_out
    if (p == 0 && scaled) {
      sc0 = conv_scale4(a.s.gamma, a.s.var, a.s.eps, ch);
      sc1 = conv_scale4(a.s.gamma, a.s.var, a.s.eps, ch + 4);
    }
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mrow[p] >= 0) {                     // the only place a row of g or y is addressed
      v0 = conv_gz4(a.s, mrow[p], ch, scaled, sc0);
      v1 = conv_gz4(a.s, mrow[p], ch + 4, scaled, sc1);
    }
  };

  lin_f32x16 acc[2][2];
  conv_mainloop<NPROD>(lds, a.wpack, nt, a.N / kConvBK, 0, fetch, acc);

  // epilogue: registers 4 g .. 4 g + 3 of tile (i, j) are columns n32 + 4 (lane >> 5) + 8 g .. + 3 of output row conv_out_row(mt, i)
  const int lane = tid & 63;
  const int wn = (tid >> 6) & 1;
  const int HWo = a.Ho * a.Wo;
  const int NT = 9 * a.C;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = conv_out_row(mt, i);
    const bool row_ok = m < a.M;
    const float *orow = nullptr;
    int img0 = 0, ty = 0, tx = 0;
    if (row_ok) {
      const int img = static_cast<int>(m / HWo);
      const int r = static_cast<int>(m - static_cast<long>(img) * HWo);
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      orow = a.offs + m * a.ldoffs;
      img0 = img * a.H * a.W;               // < 2^24 (the entry point's bound)
      ty = STRIDE * oy - 1;
      tx = STRIDE * ox - 1;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n32 = nt * 128 + wn * 64 + j * 32;      // wave-uniform
      if (n32 >= NT) continue;
      const int tap = n32 / a.C;
      const int ci = n32 - tap * a.C + 4 * (lane >> 5);
      float s_y = 0.f, s_x = 0.f, s_l = 0.f;
      bool ok = false;
      DeformTap t;
      if (row_ok) ok = deform_tap(orow, tap, ty, tx, img0, a.H, a.W, t);
      if (ok) {
        const float b[4] = {mul_scalar(t.hy, t.hx), mul_scalar(t.hy, t.lx), mul_scalar(t.ly, t.hx), mul_scalar(t.ly, t.lx)};
        float sv[4] = {0.f, 0.f, 0.f, 0.f};         // sum over this lane's columns of dcol * v_c
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((t.live >> k) & 1u)) continue;      // the only place a row of x or dx is addressed
          const long row = t.crow + (k >> 1) * a.W + (k & 1);
          if (a.doffs) {
            const float *xs = a.x + row * a.ldx + ci;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const float4 v = *reinterpret_cast<const float4 *>(xs + 8 * g);
              sv[k] = fma_scalar(acc[i][j][4 * g], v.x, sv[k]);
              sv[k] = fma_scalar(acc[i][j][4 * g + 1], v.y, sv[k]);
              sv[k] = fma_scalar(acc[i][j][4 * g + 2], v.z, sv[k]);
              sv[k] = fma_scalar(acc[i][j][4 * g + 3], v.w, sv[k]);
            }
          }
          if (a.dx) {
            const float cm = mul_scalar(t.mask, b[k]);
            float *ds = a.dx + row * a.lddx + ci;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int e = 0; e < 4; ++e) unsafeAtomicAdd(ds + 8 * g + e, mul_scalar(cm, acc[i][j][4 * g + e]));
          }
        }
        if (a.doffs) {
          const float dm = mul_scalar(t.mask, sub_scalar(1.f, t.mask));
          float bl = mul_scalar(b[0], sv[0]);
          bl = fma_scalar(b[1], sv[1], bl);
          bl = fma_scalar(b[2], sv[2], bl);
          bl = fma_scalar(b[3], sv[3], bl);
          s_l = mul_scalar(dm, bl);
          s_y = mul_scalar(t.mask, fma_scalar(sub_scalar(sv[3], sv[1]), t.lx, mul_scalar(sub_scalar(sv[2], sv[0]), t.hx)));
          s_x = mul_scalar(t.mask, fma_scalar(sub_scalar(sv[3], sv[2]), t.ly, mul_scalar(sub_scalar(sv[1], sv[0]), t.hy)));
        }
      }
      if (a.doffs) {                        // wave-uniform: partners (lane ^ 32) share row, tap and position
        s_y += __shfl_xor(s_y, 32);
        s_x += __shfl_xor(s_x, 32);
        s_l += __shfl_xor(s_l, 32);
        if (ok && lane < 32) {              // the only place a row of doffs is addressed
          float *dr = a.doffs + m * a.lddoffs;
          unsafeAtomicAdd(dr + 2 * tap, s_y);
          unsafeAtomicAdd(dr + 2 * tap + 1, s_x);
          unsafeAtomicAdd(dr + 18 + tap, s_l);
        }
      }
    }
  }
}

// Weight image of the kernel above: the (C_out, C_in, 3, 3) weight as the (9 C_in, C_out) matrix whose row n = k C_in + ci holds
// w[:, ci, k], read in place, in lin_pack_weight_kernel's format (conv_dgrad_pack_weight_kernel's layout, rows padded to 128 with
// zeros).  One thread per 8 output channels of a row.
__global__ void __launch_bounds__(256) deform_dgrad_pack_weight_kernel(const float *__restrict__ w, int N, int C,
                                                                      uint16_t *__restrict__ blob) {
  constexpr int ROW = kConvRow, PLANE = kConvPlane;
  const int kch = N / 32;
  const long R = 9L * C;
  const long rows = ((R + 127) / 128) * 128;
  const long t = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= rows * (N / 8)) return;
  const long n = t / (N / 8);
  const int k = static_cast<int>(t % (N / 8)) * 8;        // first of 8 output channels
  uint4 hi = make_uint4(0, 0, 0, 0), lo = hi;
  if (n < R) {
    const int tap = static_cast<int>(n / C), ci = static_cast<int>(n - static_cast<long>(tap) * C);
    const long s = 9L * C;                  // from one output channel to the next
    const float *src = w + (static_cast<long>(k) * C + ci) * 9 + tap;
    lin_split8<true>(make_float4(src[0], src[s], src[2 * s], src[3 * s]), make_float4(src[4 * s], src[5 * s], src[6 * s], src[7 * s]),
                     hi, lo);
  }
  uint16_t *chunk = blob + ((n / 128) * kch + k / 32) * (2 * PLANE);
  const int off = static_cast<int>(n % 128) * ROW + (k % 32);
  *reinterpret_cast<uint4 *>(chunk + off) = hi;
  *reinterpret_cast<uint4 *>(chunk + PLANE + off) = lo;
  if (k % 32 == 24) {       // the 16-byte row pad
    *reinterpret_cast<uint4 *>(chunk + off + 8) = make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4 *>(chunk + PLANE + off + 8) = make_uint4(0, 0, 0, 0);
  }
}

// ---- the weight gradient
struct DeformWgradArgs {
  ConvGzSrc s;                          // over the M output pixels, N columns
  const float *x;                       // (n_img * H * W, ldx) input rows, C columns
  long ldx;
  const float *offs;                    // (M, ldoffs >= 32) offset rows
  long ldoffs;
  float *dw;                            // (N, C, 3, 3) contiguous, accumulated into
  long M;                               // n_img * Ho * Wo
  int H, W, Ho, Wo;
  int C, N;                             // C_in, C_out
  int rows_per_block;                   // multiple of 32
  int tiles_n, tiles_k;
};

template <int NPROD, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) deform_conv_wgrad_rows_kernel(const DeformWgradArgs a) {
  static_assert(STRIDE == 1 || STRIDE == 2, "stride 1 / 2");
  constexpr bool LO = NPROD == 3;
  constexpr int TAPS = 9;
  __shared__ __attribute__((aligned(16))) float lds[4 * kConvWgStage];       // [stage][gz | col]
  // conv_wgrad_rows_kernel's map: all tiles of one row slice run on one XCD, back to back
  const int ntile = a.tiles_n * a.tiles_k * TAPS;
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int tile = seq % ntile, slice = (seq / ntile) * 8 + xcd;
  const int tn = tile / (a.tiles_k * TAPS), rem = tile - tn * (a.tiles_k * TAPS);
  const int tk = rem / TAPS, tap = rem - tk * TAPS;
  const int n0 = tn * 128, k0 = tk * 128;
  const long m_begin = static_cast<long>(slice) * a.rows_per_block;
  if (m_begin >= a.M) return;
  const long m_end = m_begin + a.rows_per_block < a.M ? m_begin + a.rows_per_block : a.M;
  const int nchunks = static_cast<int>((m_end - m_begin + 31) / 32);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  // staging: a chunk tile = 32 rows x 32 pieces of 4 floats; piece i of this thread is row 8 i + (tid >> 5), columns c4 .. + 3
  const int srow = tid >> 5, c4 = (tid & 31) * 4;
  const bool g_col = n0 + c4 < a.N, x_col = k0 + c4 < a.C;        // (N, C % 4 == 0: the four columns share it)
  const bool scaled = a.s.gamma != nullptr;
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
  if (scaled && g_col) sc = conv_scale4(a.s.gamma, a.s.var, a.s.eps, n0 + c4);
  const long HWo = static_cast<long>(a.Ho) * a.Wo;

  float4 gr[4], xr[4];
  auto load = [&](int c) {
    const long mb = m_begin + static_cast<long>(c) * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long m = mb + i * 8 + srow;
      gr[i] = xr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m >= m_end) continue;
      if (g_col) gr[i] = conv_gz4(a.s, m, n0 + c4, scaled, sc);       // the only place a row of g or y is addressed
      if (x_col) {
        const int img = static_cast<int>(m / HWo);
        const int r = static_cast<int>(m - img * HWo);
        const int oy = r / a.Wo, ox = r - oy * a.Wo;
        DeformTap t;                        // the only place a row of offs is addressed: m < M
        if (deform_tap(a.offs + m * a.ldoffs, tap, STRIDE * oy - 1, STRIDE * ox - 1, img * a.H * a.W, a.H, a.W, t)) {
          const float cf[4] = {mul_scalar(t.mask, mul_scalar(t.hy, t.hx)), mul_scalar(t.mask, mul_scalar(t.hy, t.lx)),
                               mul_scalar(t.mask, mul_scalar(t.ly, t.hx)), mul_scalar(t.mask, mul_scalar(t.ly, t.lx))};
          float4 q[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((t.live >> k) & 1u) {       // the only place a row of x is addressed
              const long row = t.crow + (k >> 1) * a.W + (k & 1);
              q[k] = *reinterpret_cast<const float4 *>(a.x + row * a.ldx + k0 + c4);
            }
          }
          // the forward's blend: ((c0 q0 + c1 q1) + c2 q2) + c3 q3 with fused multiply-adds (scalar_ops.h)
          float4 v;
          v.x = mul_scalar(cf[0], q[0].x); v.y = mul_scalar(cf[0], q[0].y);
          v.z = mul_scalar(cf[0], q[0].z); v.w = mul_scalar(cf[0], q[0].w);
#pragma unroll
          for (int k = 1; k < 4; ++k) {
            v.x = fma_scalar(cf[k], q[k].x, v.x);
            v.y = fma_scalar(cf[k], q[k].y, v.y);
            v.z = fma_scalar(cf[k], q[k].z, v.z);
            v.w = fma_scalar(cf[k], q[k].w, v.w);
          }
          xr[i] = v;
        }
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

  const int fcol = lane & 31, fm8 = (lane >> 5) * 8;
  load(0);
  for (int c = 0; c < nchunks; ++c) {
    float *gs = lds + ((c & 1) * 2) * kConvWgStage;
    float *xs = lds + ((c & 1) * 2 + 1) * kConvWgStage;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<float4 *>(gs + (i * 8 + srow) * 128 + c4) = gr[i];
      *reinterpret_cast<float4 *>(xs + (i * 8 + srow) * 128 + c4) = xr[i];
    }
    __syncthreads();            // chunk c is staged; everyone has left chunk c - 1, whose stage the next iteration overwrites
    if (c + 1 < nchunks) load(c + 1);           // in flight under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      lin_bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float ga[8], xa[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {           // rows past the slice and dead positions were staged as zeros
          const int m = ks * 16 + fm8 + e;
          ga[e] = gs[m * 128 + wn * 64 + t * 32 + fcol];
          xa[e] = xs[m * 128 + wk * 64 + t * 32 + fcol];
        }
        uint4 hi, lo;
        lin_split8<LO>(make_float4(ga[0], ga[1], ga[2], ga[3]), make_float4(ga[4], ga[5], ga[6], ga[7]), hi, lo);
        ah[t] = __builtin_bit_cast(lin_bf16x8, hi);
        if (LO) al[t] = __builtin_bit_cast(lin_bf16x8, lo);
        lin_split8<LO>(make_float4(xa[0], xa[1], xa[2], xa[3]), make_float4(xa[4], xa[5], xa[6], xa[7]), hi, lo);
        bh[t] = __builtin_bit_cast(lin_bf16x8, hi);
        if (LO) bl[t] = __builtin_bit_cast(lin_bf16x8, lo);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {       // D[n][k]: gz fragment as the A operand, col fragment as B
          if (LO) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
  }

  // epilogue: D tile lane layout (wgrad_mfma.h): column (ci) = lane & 31, row (co) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wk * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (n < a.N && k < a.C) unsafeAtomicAdd(a.dw + (static_cast<long>(n) * a.C + k) * TAPS + tap, acc[i][j][r]);
      }
    }
}

}  // namespace bevmsda
