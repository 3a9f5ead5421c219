// Backward of convolution + frozen (inference) BatchNorm (+ residual) (+ ReLU) over channel-last rows on the CDNA4 matrix cores:
// the input gradient and the weight gradient of conv_bn_rows.h's operator, for a backbone trained with norm_eval=True and
// requires_grad=False norms (bevformer_base.py:43-53, bevformer_small.py, bevformer_tiny.py), where every BatchNorm is a constant
// scale and shift.  In the forward's notation
//
//   y[q, co]  = act( scale[co] * conv(x, w)[q, co] + shift[co] + res[q, co] ),    scale = gamma / sqrt(var + eps)
//   gz[q, co] = g[q, co] * (y[q, co] > 0 if relu else 1) * scale[co]
//
// with q over the n_img * Ho * Wo OUTPUT pixels and row(q, dy, dx) = img H W + (S oy + dy) W + (S ox + dx) as in conv_bn_rows.h.
// The mask comes from the saved forward output: y > 0 gives 0 at exactly 0, as torch.relu's backward; it is a PRODUCT with 0 or
// 1, so a NaN in g stays NaN.  The residual's gradient is g * mask: the caller's (conv_gz_rows_kernel without a scale).
//
// Both kernels read gz through registers and so can form it on the way from (g, y, gamma, var): y == nullptr leaves the mask
// out, gamma == nullptr the scale — a materialised gz is the case with both left out (which one a block uses where).
//
// Input gradient (conv_dgrad_rows_kernel): a gather over the INPUT pixels p = (img, iy, ix),
//
//   dx[p, ci] = sum_{taps (dy, dx)} sum_co gz[q(p, dy, dx), co] * w[co, ci, dy + 1, dx + 1]  (+ add[p, ci])
//
// where q(p, dy, dx) is the output pixel whose tap (dy, dx) reads p: oy = (iy - dy) / S, ox = (ix - dx) / S.  A tap is live where
// iy - dy and ix - dx are >= 0 and multiples of S and (oy, ox) lies inside the Ho x Wo output map; at stride 2 q is computed
// per tap (it is no constant row shift).  The GEMM is conv_mfma.h's main loop with this fetch: rows = input pixels, columns =
// C_in, reduction = taps x C_out.  Its weight image is the in/out-swapped weight, tap-mirrored (conv_dgrad_pack_weight_kernel:
// the (C_in, taps C_out) matrix with k = t C_out + co holding w[co, ci, taps - 1 - t], so that chunk tap t = (ey + 1) 3 + (ex + 1)
// reads output pixel ((iy + ey) / S, (ix + ex) / S)).  This is the plain gather form: at stride 2 a pixel has 1, 2, 2 or 4 live
// taps of 9 and the others stage zeros (a 1 x 1 at stride 2: odd pixels receive exactly add, or 0); the form that tiles one
// parity class is not built.  Epilogue, each optional: + add rows (the other branch's gradient; may BE dx: every element is read
// and then written by the one thread that owns it), then * (next_mask > 0) * next_scale — the result is then the gz of the
// convolution that produced x, at no extra launch.  Two options for a neck without norms (the FPN's backward): add_pool2 — add is
// the rows of the (2H, 2W) map and a pixel adds ((a[2y, 2x] + a[2y, 2x + 1]) + (a[2y + 1, 2x] + a[2y + 1, 2x + 1])), the transpose of
// conv_rows.h's 2 x nearest upsampled residual; the four rows are other pixels' rows of a dx that aliased it, so add is never dx
// here — and add_after_mask — the mask and scale apply to the convolution path only and add joins afterwards (an extra level's
// gradient is its own output gradient plus the masked input gradient of the next extra convolution).
//
// Weight gradient (conv_wgrad_rows_kernel): wgrad_mfma.h's tile and accumulation,
//
//   dW[co, ci, tap] += sum_q gz[q, co] * x[row(q, tap), ci]
//
// a 128 (co) x 128 (ci) tile of ONE tap over a slice of the output pixels per workgroup, 32-row chunks through a 2-stage fp32
// LDS ring with one barrier per chunk, the transposing ds_read_b32 gather, split-bf16 or bf16 operands, fp32 accumulate,
// fp32 atomics into the parameter's own (C_out, C_in, k, k) layout (the caller zero-fills; run-to-run bit equality is not a
// goal).  The operand rows travel through registers, not LDS-DMA: x's row is addressed per tap under its predicate and a dead
// tap stages zeros, and gz can be formed from g and y on the way.  relu_x stages max(x, 0) (the forward's relu_in).  dbias: the
// workgroups of the centre tap and the first C_in tile stage every gz row of their slice exactly once; their wk == 0 waves sum the
// gz fragments they read for the MFMAs per column (wgrad_mfma.h's colsum), the two half-waves are combined with one shuffle and
// one fp32 atomicAdd per column per workgroup goes into dbias (the caller zero-fills it with dw).  The sum is a wave-uniform branch
// and two registers: every instance stays within amdgpu_waves_per_eu(2, 2) without scratch, with the sum and without.
//
// Memory safety: a row of g, y, x, add, next_mask or dx is addressed only under its predicate (pixel inside the problem, tap
// live, column inside the matrix); masked lanes load nothing and stage zeros.  Every row index is below 2^24 (the C ABI's bound)
// and is multiplied by a row stride in 64 bits.
#pragma once
#include "conv_mfma.h"

namespace bevmsda {

// where gz comes from: g rows, optionally masked by the saved output y and scaled by gamma / sqrt(var + eps)
struct ConvGzSrc {
  const float *g;                       // (M, ldg)
  long ldg;
  const float *y;                       // (M, ldy) or nullptr: no mask
  long ldy;
  const float *gamma, *var;             // (C_out) each or both nullptr: scale 1
  float eps;
};

__device__ __forceinline__ float4 conv_scale4(const float *gamma, const float *var, float eps, int n) {
  const float4 ga = *reinterpret_cast<const float4 *>(gamma + n);
  const float4 va = *reinterpret_cast<const float4 *>(var + n);
  // conv_bn_rows.h's expression
  return make_float4(ga.x / sqrtf(va.x + eps), ga.y / sqrtf(va.y + eps), ga.z / sqrtf(va.z + eps), ga.w / sqrtf(va.w + eps));
}

__device__ __forceinline__ float4 conv_mask4(const float4 &v, const float4 &y) {      // v * (y > 0): NaN in v stays NaN
  return make_float4(v.x * (y.x > 0.f ? 1.f : 0.f), v.y * (y.y > 0.f ? 1.f : 0.f), v.z * (y.z > 0.f ? 1.f : 0.f),
                     v.w * (y.w > 0.f ? 1.f : 0.f));
}

__device__ __forceinline__ float4 conv_mul4(const float4 &a, const float4 &b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// gz[q, n .. n + 3]; the caller holds the predicate (q inside the problem, n inside the matrix) and the scale of these columns
__device__ __forceinline__ float4 conv_gz4(const ConvGzSrc &s, long q, int n, bool scaled, const float4 &sc) {
  float4 v = *reinterpret_cast<const float4 *>(s.g + q * s.ldg + n);
  if (s.y) v = conv_mask4(v, *reinterpret_cast<const float4 *>(s.y + q * s.ldy + n));
  if (scaled) v = conv_mul4(v, sc);
  return v;
}

// ---- gz as rows of its own: the one mask launch of a block (its last convolution's gradient and the identity's)
struct ConvGzArgs {
  ConvGzSrc s;
  float *gz;
  long ldgz;
  long M;
  int N;                                // columns: a multiple of 4
};

__global__ void __launch_bounds__(256) conv_gz_rows_kernel(const ConvGzArgs a) {
  const int n4 = a.N / 4;
  const long t = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= a.M * n4) return;
  const long q = t / n4;
  const int n = static_cast<int>(t - q * n4) * 4;
  const bool scaled = a.s.gamma != nullptr;
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
  if (scaled) sc = conv_scale4(a.s.gamma, a.s.var, a.s.eps, n);
  *reinterpret_cast<float4 *>(a.gz + q * a.ldgz + n) = conv_gz4(a.s, q, n, scaled, sc);
}

// ---- the input gradient
struct ConvDgradArgs {
  ConvGzSrc s;                          // over the n_img * Ho * Wo output pixels, C columns
  const uint16_t *wpack;                // conv_dgrad_pack_weight_kernel's image
  const float *add;                     // (M, ldadd) or nullptr; may be dx.  add_pool2: the rows of the (2H, 2W) map, never dx
  long ldadd;
  int add_pool2;                        // add[p] = the sum of the 2 x 2 fine pixels under p: the transpose of CONV_RES_UP2
  int add_after_mask;                   // the add joins after the mask and scale (which then belong to the convolution path only)
  const float *nmask;                   // (M, ldnmask) or nullptr: the saved output of the convolution that produced x
  long ldnmask;
  const float *ngamma, *nvar;           // (N) each or both nullptr (with nmask only)
  float neps;
  float *dx;
  long lddx;
  long M;                               // n_img * H * W input pixels
  int H, W, Ho, Wo;
  int C, N;                             // C_out (the reduction), C_in (the columns): multiples of kConvGran
  int nblk_m, nblk_n;
};

template <int NPROD, int TAPS, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) conv_dgrad_rows_kernel(const ConvDgradArgs a) {
  static_assert((TAPS == 9 || TAPS == 1) && (STRIDE == 1 || STRIDE == 2), "3 x 3 or 1 x 1, stride 1 / 2");
  __shared__ __attribute__((aligned(16))) uint16_t lds[conv_lds_elems<NPROD>()];
  int mt, nt;
  if (!conv_tile(a.nblk_m, a.nblk_n, mt, nt)) return;

  const int tid = threadIdx.x;
  const int skq = (tid & 3) * 8;
  const int KC = a.C / kConvBK;             // output-channel chunks per tap

  // the staged input pixels of this thread: the first output row of their image and their position in it
  // (a pixel outside the problem sits at row kConvFar: none of its taps is live)
  constexpr int kConvFar = -(1 << 28);
  long qimg[kConvNP];
  int iy[kConvNP], ix[kConvNP];
  const long HW = static_cast<long>(a.H) * a.W;
  const long HWo = static_cast<long>(a.Ho) * a.Wo;
#pragma unroll
  for (int p = 0; p < kConvNP; ++p) {
    const long m = static_cast<long>(mt) * kConvBM + p * kConvRPP + (tid >> 2);
    qimg[p] = 0;
    iy[p] = kConvFar;
    ix[p] = 0;
    if (m < a.M) {
      if (TAPS == 1 && STRIDE == 1) {       // input pixel p is output pixel p
        qimg[p] = m;
        iy[p] = 0;
      } else {
        const long img = m / HW;
        const int r = static_cast<int>(m - img * HW);
        iy[p] = r / a.W;
        ix[p] = r - iy[p] * a.W;
        qimg[p] = img * HWo;
      }
    }
  }

  const bool scaled = a.s.gamma != nullptr;
  float4 sc0 = make_float4(1.f, 1.f, 1.f, 1.f), sc1 = sc0;     // the scale of the chunk's 8 channels: set by the chunk's first fetch
  auto fetch = [&](int c, int p, float4 &v0, float4 &v1) {
    const int tap = TAPS == 1 ? 0 : c / KC;
    const int ch = (c - tap * KC) * kConvBK + skq;      // first of this thread's 8 output channels: ch + 7 < C
    if (p == 0 && scaled) {
      sc0 = conv_scale4(a.s.gamma, a.s.var, a.s.eps, ch);
      sc1 = conv_scale4(a.s.gamma, a.s.var, a.s.eps, ch + 4);
    }
    bool live = iy[p] >= 0;
    long q = qimg[p];
    if (!(TAPS == 1 && STRIDE == 1)) {
      const int yy = iy[p] + (TAPS == 1 ? 0 : tap / 3 - 1), xx = ix[p] + (TAPS == 1 ? 0 : tap % 3 - 1);
      live = yy >= 0 && xx >= 0 && (STRIDE == 1 || ((yy | xx) & 1) == 0);
      const int oy = STRIDE == 1 ? yy : yy >> 1, ox = STRIDE == 1 ? xx : xx >> 1;     // used under `live` only
      live = live && oy < a.Ho && ox < a.Wo;
      q += static_cast<long>(oy) * a.Wo + ox;
    }
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {                             // the only place a row of g or y is addressed
      v0 = conv_gz4(a.s, q, ch, scaled, sc0);
      v1 = conv_gz4(a.s, q, ch + 4, scaled, sc1);
    }
  };

  lin_f32x16 acc[2][2];
  conv_mainloop<NPROD>(lds, a.wpack, nt, TAPS * KC, 0, fetch, acc);

  long arow[2];               // the row of add an input pixel reads; add_pool2: its top-left fine pixel (addressed only where m < M)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = conv_out_row(mt, i);
    arow[i] = m;
    if (a.add_pool2 && m < a.M) {
      const long img = m / HW;
      const int r = static_cast<int>(m - img * HW);
      const int py = r / a.W, px = r - py * a.W;
      arow[i] = img * (4 * HW) + static_cast<long>(2 * py) * (2 * a.W) + 2 * px;        // below 4 M <= 2^24 (the C ABI's bound)
    }
  }
  conv_epilogue(acc, mt, nt, a.M, a.N,
      [&](int n) {
        return a.nmask && a.ngamma ? conv_scale4(a.ngamma, a.nvar, a.neps, n) : make_float4(1.f, 1.f, 1.f, 1.f);
      },
      [&](const float4 &nsc, int i, long m, int n, float4 v) {
        float4 ad = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.add) {                            // the only place a row of add is addressed: m < M, n < N
          const float *p = a.add + arow[i] * a.ldadd + n;
          ad = *reinterpret_cast<const float4 *>(p);
          if (a.add_pool2) {                    // ((a[2y, 2x] + a[2y, 2x + 1]) + (a[2y + 1, 2x] + a[2y + 1, 2x + 1])), in this order
            const float *p1 = p + static_cast<long>(2 * a.W) * a.ldadd;
            ad = lin_add4(lin_add4(ad, *reinterpret_cast<const float4 *>(p + a.ldadd)),
                          lin_add4(*reinterpret_cast<const float4 *>(p1), *reinterpret_cast<const float4 *>(p1 + a.ldadd)));
          }
          if (!a.add_after_mask) v = lin_add4(v, ad);
        }
        if (a.nmask) v = conv_mul4(conv_mask4(v, *reinterpret_cast<const float4 *>(a.nmask + m * a.ldnmask + n)), nsc);
        if (a.add && a.add_after_mask) v = lin_add4(v, ad);
        *reinterpret_cast<float4 *>(a.dx + m * a.lddx + n) = v;
      });
}

// Weight image of the input gradient: the (C_out, C_in, k, k) weight as the (C_in, taps C_out) matrix with k = t C_out + co
// holding w[co, ci, taps - 1 - t], in lin_pack_weight_kernel's format (conv3x3_pack_weight_kernel's layout: [plane hi | plane lo]
// [128][32 + 8 pad] bf16 per (128-row tile, 32-deep chunk), chunks tap-major).  One thread per 8 output channels of a (ci, t).
__global__ void __launch_bounds__(256) conv_dgrad_pack_weight_kernel(const float *__restrict__ w, int N, int C, int taps,
                                                                    uint16_t *__restrict__ blob) {
  constexpr int ROW = kConvRow, PLANE = kConvPlane;
  const int K = taps * N;
  const int kch = K / 32;
  const long rows = static_cast<long>((C + 127) / 128) * 128;
  const long t = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= rows * (K / 8)) return;
  const int ci = static_cast<int>(t / (K / 8));
  const int k = static_cast<int>(t % (K / 8)) * 8;
  uint4 hi = make_uint4(0, 0, 0, 0), lo = hi;
  if (ci < C) {
    const int tap = k / N, co = k - tap * N;        // N % 32 == 0: the 8 k share a tap
    const long s = static_cast<long>(C) * taps;     // from one output channel to the next
    const float *src = w + (static_cast<long>(co) * C + ci) * taps + (taps - 1 - tap);
    lin_split8<true>(make_float4(src[0], src[s], src[2 * s], src[3 * s]), make_float4(src[4 * s], src[5 * s], src[6 * s], src[7 * s]),
                     hi, lo);
  }
  uint16_t *chunk = blob + (static_cast<long>(ci / 128) * kch + k / 32) * (2 * PLANE);
  const int off = (ci % 128) * ROW + (k % 32);
  *reinterpret_cast<uint4 *>(chunk + off) = hi;
  *reinterpret_cast<uint4 *>(chunk + PLANE + off) = lo;
  if (k % 32 == 24) {       // the 16-byte row pad
    *reinterpret_cast<uint4 *>(chunk + off + 8) = make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4 *>(chunk + PLANE + off + 8) = make_uint4(0, 0, 0, 0);
  }
}

// ---- the weight gradient
struct ConvWgradArgs {
  ConvGzSrc s;                          // over the M output pixels, N columns
  const float *x;                       // (n_img * H * W, ldx) input rows, C columns
  long ldx;
  float *dw;                            // (N, C, k, k) contiguous, accumulated into
  float *dbias;                         // (N) accumulated into, or nullptr: dbias[co] += sum_q gz[q, co]
  int relu_x;                           // stage max(x, 0) in place of x (the forward's relu_in)
  long M;                               // n_img * Ho * Wo
  int H, W, Ho, Wo;
  int C, N;                             // C_in, C_out
  int rows_per_block;                   // multiple of 32
  int tiles_n, tiles_k;
};

constexpr int kConvWgStage = 32 * 128;      // floats of one operand tile of a chunk

template <int NPROD, int TAPS, int STRIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) conv_wgrad_rows_kernel(const ConvWgradArgs a) {
  static_assert((TAPS == 9 || TAPS == 1) && (STRIDE == 1 || STRIDE == 2), "3 x 3 or 1 x 1, stride 1 / 2");
  constexpr bool LO = NPROD == 3;
  __shared__ __attribute__((aligned(16))) float lds[4 * kConvWgStage];       // [stage][gz | x]
  // wgrad_mfma.h's XCD-aware map: all tiles of one row slice run on one XCD, back to back
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
  const int dy = TAPS == 1 ? 0 : tap / 3 - 1, dx = TAPS == 1 ? 0 : tap % 3 - 1;
  const long HW = static_cast<long>(a.H) * a.W;
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
        long row = m;
        bool live = true;
        if (!(TAPS == 1 && STRIDE == 1)) {
          const long img = m / HWo;
          const int r = static_cast<int>(m - img * HWo);
          const int oy = r / a.Wo, ox = r - oy * a.Wo;
          const int yy = STRIDE * oy + dy, xx = STRIDE * ox + dx;
          live = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
          row = img * HW + static_cast<long>(yy) * a.W + xx;
        }
        if (live) xr[i] = *reinterpret_cast<const float4 *>(a.x + row * a.ldx + k0 + c4);     // the only place a row of x is addressed
        if (a.relu_x) conv_relu4(xr[i]);
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

  // The bias gradient (wgrad_mfma.h's colsum): the workgroups of the centre tap and the first c_in tile stage every gz row of
  // their slice exactly once, and their wk == 0 waves read each of the tile's 128 columns as MFMA fragments
  const bool bias_wave = a.dbias != nullptr && tap == TAPS / 2 && tk == 0 && wk == 0;
  float colsum[2] = {0.f, 0.f};             // my column of each of my two n tiles

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
        for (int e = 0; e < 8; ++e) {           // rows past the slice and dead taps were staged as zeros
          const int m = ks * 16 + fm8 + e;
          ga[e] = gs[m * 128 + wn * 64 + t * 32 + fcol];
          xa[e] = xs[m * 128 + wk * 64 + t * 32 + fcol];
        }
        if (bias_wave) colsum[t] += ((ga[0] + ga[1]) + (ga[2] + ga[3])) + ((ga[4] + ga[5]) + (ga[6] + ga[7]));
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
        for (int j = 0; j < 2; ++j) {       // D[n][k]: gz fragment as the A operand, x fragment as B
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
  if (bias_wave) {            // lanes l and l + 32 hold the same column over different rows: one atomic per column per workgroup
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float s = colsum[t] + __shfl_xor(colsum[t], 32, 64);
      const int n = n0 + wn * 64 + t * 32 + fcol;
      if (lane < 32 && n < a.N) atomicAdd(a.dbias + n, s);
    }
  }
}

}  // namespace bevmsda
