// BatchNorm with BATCH statistics over channel-last rows: what a ResNet bottleneck whose norms are in train() mode needs
// around its raw convolutions (conv_bn_rows.h with an identity norm) — the per-channel mean and biased variance over the M rows
// of z, the normalisation with the affine, the residual sum and the ReLU, and the backward that carries the gradient through
// the statistics.  All arithmetic is fp32, whatever the GEMM mode: statistics are not GEMM operands.
//
//   mean[c] = sum_m z[m, c] / M            var[c] = sum_m (z[m, c] - mean[c])^2 / M            (biased)
//   xhat    = (z - mean) * invstd          invstd = 1 / sqrtf(var + eps)
//   y       = act(xhat * gamma + beta + res)
//   gy      = g * (y > 0 ? 1 : 0)          S1[c] = sum_m gy            S2[c] = sum_m gy * xhat
//   dz      = gamma * invstd * (gy - S1 / M - xhat * S2 / M)
//
// These are bandwidth kernels and share one geometry: a workgroup of 256 threads owns a tile of LX * 4 channels (LX lanes of
// 16 bytes along the channels: 32, 64 or 128 channels, the widest that divides C) and a chunk of `chunk` consecutive rows; its
// 256 / LX row lanes walk the chunk's rows.  A lane keeps its four channels for the whole chunk, so the per-channel vectors
// (and the sqrt and the division behind invstd) are formed once per thread, not once per element.
//
// The two reductions never subtract large sums.  A thread sums (z - K) and (z - K)^2 with K the first value it meets — a constant
// column gives exact zeros —, turns them into (count, mean, M2) and the workgroup merges its row lanes pairwise in LDS with
// Chan's formula; the chunk's (mean, M2) goes to a slab the caller owns.  A second small kernel of the same C call merges the
// chunks of a channel in a fixed order (8 strided runs, then a tree).  M2 is a sum of squares and of non-negative terms only:
// never negative, exactly 0 for a constant column.  No floating-point atomics and no in-launch hand-off between workgroups:
// two calls on the same input give the same bits.  S1 and S2 take the same route with plain sums.
//
// Memory safety: a row is addressed only for m < M, a column tile only inside C (C is a multiple of 32 and the tile width
// divides it); the slab is written at [chunk][2][C] for chunk < nchunks and read the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bevmsda {

constexpr int kBnThreads = 256;
constexpr int kBnMinChunk = 1024;           // rows per workgroup: at least this many ...
constexpr int kBnMaxChunks = 2048;          // ... and at most this many chunks (M <= 2^24: a chunk is at most 8192 rows)

// rows per workgroup for M rows: a multiple of 32 (every row-lane count divides it)
inline long bn_chunk_rows(long M) {
  long rows = (M + kBnMaxChunks - 1) / kBnMaxChunks;
  rows = ((rows + 31) / 32) * 32;
  return rows < kBnMinChunk ? kBnMinChunk : rows;
}
inline long bn_num_chunks(long M) { return (M + bn_chunk_rows(M) - 1) / bn_chunk_rows(M); }
// lanes along the channels: the widest tile of 128, 64 or 32 channels that divides C
inline int bn_lanes_x(int C) { return C % 128 == 0 ? 32 : C % 64 == 0 ? 16 : 8; }

struct BnRowsArgs {
  const float *z;                       // (M, ldz) the raw convolution's rows
  long ldz;
  const float *mean, *var;              // (C) batch statistics
  const float *gamma, *beta;            // (C)
  float eps;
  const float *res;                     // apply: (M, ldres) or nullptr
  long ldres;
  float *y;                             // apply: (M, ldy)
  long ldy;
  int relu;
  const float *g;                       // backward: (M, ldg) the gradient w.r.t. the output
  long ldg;
  const float *mask;                    // backward: (M, ldmask) the saved output whose sign is the ReLU's mask, or nullptr
  long ldmask;
  const float *sums;                    // backward apply: (2, C) S1 then S2
  float *dz;                            // backward apply: (M, lddz)
  long lddz;
  float *gy;                            // backward apply: (M, ldgy) or nullptr
  long ldgy;
  float *slab;                          // reductions: (nchunks, 2, C) partials
  long M, chunk;
  int C;
};

struct BnFinalArgs {
  const float *slab;                    // (nchunks, 2, C)
  long M, chunk;
  int nchunks, C;
  int welford;                          // 1: (mean, M2) partials merged with Chan's formula; 0: plain sums
  const float *shift;                   // welford: (C) row 0 of z, which the partial means are measured from
  float *out0, *out1;                   // (C) each: mean and biased var, or S1 and S2
  float *running_mean, *running_var;    // (C) or nullptr: updated in place
  long long *num_batches_tracked;       // or nullptr: += 1
  float momentum;
};

__device__ __forceinline__ float4 bn_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void bn_st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float4 bn_invstd4(const float4 &var, float eps) {
  return make_float4(1.f / sqrtf(var.x + eps), 1.f / sqrtf(var.y + eps), 1.f / sqrtf(var.z + eps), 1.f / sqrtf(var.w + eps));
}
__device__ __forceinline__ float4 bn_xhat4(const float4 &z, const float4 &mu, const float4 &is) {
  return make_float4((z.x - mu.x) * is.x, (z.y - mu.y) * is.y, (z.z - mu.z) * is.z, (z.w - mu.w) * is.w);
}
// g * (y > 0 ? 1 : 0): a product, so that a NaN in g stays NaN
__device__ __forceinline__ float4 bn_mask4(const float4 &g, const float4 &y) {
  return make_float4(g.x * (y.x > 0.f ? 1.f : 0.f), g.y * (y.y > 0.f ? 1.f : 0.f), g.z * (y.z > 0.f ? 1.f : 0.f),
                     g.w * (y.w > 0.f ? 1.f : 0.f));
}

// Chan's merge of (na, ma, qa) with (nb, mb, qb) into a; counts are exact in fp32 (<= 2^24)
__device__ __forceinline__ void bn_chan(float &na, float &ma, float &qa, float nb, float mb, float qb) {
  if (nb == 0.f) return;
  if (na == 0.f) {
    na = nb; ma = mb; qa = qb;
    return;
  }
  const float n = na + nb, d = mb - ma;
  ma = ma + d * (nb / n);
  qa = qa + qb + d * d * (na * (nb / n));
  na = n;
}

// ---- statistics, pass 1: one (mean, M2) pair per chunk and channel
template <int LX>
__global__ void __launch_bounds__(kBnThreads) bn_stats_partial_kernel(const BnRowsArgs a) {
  constexpr int RL = kBnThreads / LX;                   // row lanes
  __shared__ float s_n[RL], s_m[RL][LX * 4], s_q[RL][LX * 4];
  const int cx = threadIdx.x % LX, r = threadIdx.x / LX;
  const int col = (blockIdx.x * LX + cx) * 4;           // < C: the grid has C / (4 LX) column tiles
  const long row0 = static_cast<long>(blockIdx.y) * a.chunk;
  const long row1 = row0 + a.chunk < a.M ? row0 + a.chunk : a.M;
  float4 k = make_float4(0.f, 0.f, 0.f, 0.f), s1 = k, s2 = k;
  float n = 0.f;
  long m = row0 + r;
  if (m < row1) k = bn_ld4(a.z + m * a.ldz + col);
  for (; m < row1; m += RL) {
    const float4 v = bn_ld4(a.z + m * a.ldz + col);
    const float dx = v.x - k.x, dy = v.y - k.y, dz = v.z - k.z, dw = v.w - k.w;
    s1.x += dx; s1.y += dy; s1.z += dz; s1.w += dw;
    s2.x += dx * dx; s2.y += dy * dy; s2.z += dz * dz; s2.w += dw * dw;
    n += 1.f;
  }
  // (count, mean, M2) of this thread: M2 = s2 - s1^2 / n is 0 for equal values and clamped at 0 against rounding.  The mean is
  // kept as its distance from row 0 of z (k - z0 is small and all but exact; z0 comes back in pass 2): a column far from zero
  // (mean 4096, spread 1) would otherwise round every partial mean to an ulp of 4096 and the merges' (mean_b - mean_a)^2 with it
  const float4 z0 = bn_ld4(a.z + col);
  float mu[4] = {k.x - z0.x, k.y - z0.y, k.z - z0.z, k.w - z0.w}, q[4] = {0.f, 0.f, 0.f, 0.f};
  if (n > 0.f) {
    const float sa[4] = {s1.x, s1.y, s1.z, s1.w}, sb[4] = {s2.x, s2.y, s2.z, s2.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = sa[j] / n;
      mu[j] += d;
      q[j] = fmaxf(sb[j] - sa[j] * d, 0.f);
    }
  }
  if (cx == 0) s_n[r] = n;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s_m[r][cx * 4 + j] = mu[j];
    s_q[r][cx * 4 + j] = q[j];
  }
  __syncthreads();
  // pairwise tree over the row lanes, in a fixed order
  for (int half = RL / 2; half >= 1; half >>= 1) {
    if (r < half) {
      const float nb = s_n[r + half];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float na = n;
        bn_chan(na, mu[j], q[j], nb, s_m[r + half][cx * 4 + j], s_q[r + half][cx * 4 + j]);
        if (j == 3) n = na;
      }
    }
    __syncthreads();
    if (r < half) {
      if (cx == 0) s_n[r] = n;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s_m[r][cx * 4 + j] = mu[j];
        s_q[r][cx * 4 + j] = q[j];
      }
    }
    __syncthreads();
  }
  if (r == 0) {
    float *p = a.slab + static_cast<long>(blockIdx.y) * 2 * a.C + col;
    bn_st4(p, make_float4(mu[0], mu[1], mu[2], mu[3]));
    bn_st4(p + a.C, make_float4(q[0], q[1], q[2], q[3]));
  }
}

// ---- backward, pass 1: one (S1, S2) pair per chunk and channel
template <int LX>
__global__ void __launch_bounds__(kBnThreads) bn_bwd_partial_kernel(const BnRowsArgs a) {
  constexpr int RL = kBnThreads / LX;
  __shared__ __attribute__((aligned(16))) float s_a[RL][LX * 4], s_b[RL][LX * 4];       // (16-byte rows: float4 accesses)
  const int cx = threadIdx.x % LX, r = threadIdx.x / LX;
  const int col = (blockIdx.x * LX + cx) * 4;
  const long row0 = static_cast<long>(blockIdx.y) * a.chunk;
  const long row1 = row0 + a.chunk < a.M ? row0 + a.chunk : a.M;
  const float4 mu = bn_ld4(a.mean + col), is = bn_invstd4(bn_ld4(a.var + col), a.eps);
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  for (long m = row0 + r; m < row1; m += RL) {
    float4 gy = bn_ld4(a.g + m * a.ldg + col);
    if (a.mask) gy = bn_mask4(gy, bn_ld4(a.mask + m * a.ldmask + col));
    const float4 xh = bn_xhat4(bn_ld4(a.z + m * a.ldz + col), mu, is);
    s1.x += gy.x; s1.y += gy.y; s1.z += gy.z; s1.w += gy.w;
    s2.x += gy.x * xh.x; s2.y += gy.y * xh.y; s2.z += gy.z * xh.z; s2.w += gy.w * xh.w;
  }
  bn_st4(&s_a[r][cx * 4], s1);
  bn_st4(&s_b[r][cx * 4], s2);
  __syncthreads();
  for (int half = RL / 2; half >= 1; half >>= 1) {
    if (r < half) {
      const float4 b1 = bn_ld4(&s_a[r + half][cx * 4]), b2 = bn_ld4(&s_b[r + half][cx * 4]);
      s1.x += b1.x; s1.y += b1.y; s1.z += b1.z; s1.w += b1.w;
      s2.x += b2.x; s2.y += b2.y; s2.z += b2.z; s2.w += b2.w;
      bn_st4(&s_a[r][cx * 4], s1);          // (this round reads rows >= half only: row r < half is nobody's operand)
      bn_st4(&s_b[r][cx * 4], s2);
    }
    __syncthreads();
  }
  if (r == 0) {
    float *p = a.slab + static_cast<long>(blockIdx.y) * 2 * a.C + col;
    bn_st4(p, s1);
    bn_st4(p + a.C, s2);
  }
}

// ---- pass 2 of both reductions: the chunks of a channel merged in a fixed order.  A workgroup of 256 threads owns 32 channels:
// thread (run, c) merges chunks run, run + 8, ... in ascending order, then the 8 runs are merged as a tree.
constexpr int kBnRuns = 8;

__global__ void __launch_bounds__(kBnThreads) bn_final_kernel(const BnFinalArgs a) {
  __shared__ float s_n[kBnRuns][32], s_a[kBnRuns][32], s_b[kBnRuns][32];
  const int c = threadIdx.x % 32, run = threadIdx.x / 32;
  const int col = blockIdx.x * 32 + c;                  // < C: the grid has C / 32 workgroups
  float n = 0.f, va = 0.f, vb = 0.f;
  for (int i = run; i < a.nchunks; i += kBnRuns) {
    const float *p = a.slab + static_cast<long>(i) * 2 * a.C + col;
    if (a.welford) {
      const long row0 = static_cast<long>(i) * a.chunk;
      const long cnt = row0 + a.chunk < a.M ? a.chunk : a.M - row0;
      bn_chan(n, va, vb, static_cast<float>(cnt), p[0], p[a.C]);
    } else {
      va += p[0];
      vb += p[a.C];
    }
  }
  s_n[run][c] = n; s_a[run][c] = va; s_b[run][c] = vb;
  __syncthreads();
  for (int half = kBnRuns / 2; half >= 1; half >>= 1) {
    if (run < half) {
      if (a.welford) bn_chan(n, va, vb, s_n[run + half][c], s_a[run + half][c], s_b[run + half][c]);
      else {
        va += s_a[run + half][c];
        vb += s_b[run + half][c];
      }
    }
    __syncthreads();
    if (run < half) {
      s_n[run][c] = n; s_a[run][c] = va; s_b[run][c] = vb;
    }
    __syncthreads();
  }
  if (run != 0) return;
  if (!a.welford) {
    a.out0[col] = va;
    a.out1[col] = vb;
    return;
  }
  const float M = static_cast<float>(a.M);
  va += a.shift[col];                                   // the partial means are distances from row 0 of z
  a.out0[col] = va;
  a.out1[col] = vb / M;                                 // biased; M2 >= 0, so never negative
  if (a.running_mean) {
    a.running_mean[col] = (1.f - a.momentum) * a.running_mean[col] + a.momentum * va;
    a.running_var[col] = (1.f - a.momentum) * a.running_var[col] + a.momentum * (vb / (M - 1.f));    // unbiased: M2 / (M - 1)
  }
  if (a.num_batches_tracked && blockIdx.x == 0 && c == 0) *a.num_batches_tracked += 1;
}

// ---- y = act(xhat * gamma + beta + res)
template <int LX>
__global__ void __launch_bounds__(kBnThreads) bn_apply_kernel(const BnRowsArgs a) {
  constexpr int RL = kBnThreads / LX;
  const int cx = threadIdx.x % LX, r = threadIdx.x / LX;
  const int col = (blockIdx.x * LX + cx) * 4;
  const long row0 = static_cast<long>(blockIdx.y) * a.chunk;
  const long row1 = row0 + a.chunk < a.M ? row0 + a.chunk : a.M;
  const float4 mu = bn_ld4(a.mean + col), is = bn_invstd4(bn_ld4(a.var + col), a.eps);
  const float4 ga = bn_ld4(a.gamma + col), be = bn_ld4(a.beta + col);
  for (long m = row0 + r; m < row1; m += RL) {
    const float4 xh = bn_xhat4(bn_ld4(a.z + m * a.ldz + col), mu, is);
    float4 v = make_float4(xh.x * ga.x + be.x, xh.y * ga.y + be.y, xh.z * ga.z + be.z, xh.w * ga.w + be.w);
    if (a.res) {
      const float4 rr = bn_ld4(a.res + m * a.ldres + col);
      v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
    }
    if (a.relu) {                                       // NaN stays NaN, as torch.relu
      v.x = v.x < 0.f ? 0.f : v.x;
      v.y = v.y < 0.f ? 0.f : v.y;
      v.z = v.z < 0.f ? 0.f : v.z;
      v.w = v.w < 0.f ? 0.f : v.w;
    }
    bn_st4(a.y + m * a.ldy + col, v);
  }
}

// ---- dz = gamma * invstd * (gy - S1 / M - xhat * S2 / M), and gy itself when a destination is given
template <int LX>
__global__ void __launch_bounds__(kBnThreads) bn_bwd_apply_kernel(const BnRowsArgs a) {
  constexpr int RL = kBnThreads / LX;
  const int cx = threadIdx.x % LX, r = threadIdx.x / LX;
  const int col = (blockIdx.x * LX + cx) * 4;
  const long row0 = static_cast<long>(blockIdx.y) * a.chunk;
  const long row1 = row0 + a.chunk < a.M ? row0 + a.chunk : a.M;
  const float M = static_cast<float>(a.M);
  const float4 mu = bn_ld4(a.mean + col), is = bn_invstd4(bn_ld4(a.var + col), a.eps);
  const float4 ga = bn_ld4(a.gamma + col), s1 = bn_ld4(a.sums + col), s2 = bn_ld4(a.sums + a.C + col);
  const float4 sc = make_float4(ga.x * is.x, ga.y * is.y, ga.z * is.z, ga.w * is.w);
  const float4 m1 = make_float4(s1.x / M, s1.y / M, s1.z / M, s1.w / M), m2 = make_float4(s2.x / M, s2.y / M, s2.z / M, s2.w / M);
  for (long m = row0 + r; m < row1; m += RL) {
    float4 gy = bn_ld4(a.g + m * a.ldg + col);
    if (a.mask) gy = bn_mask4(gy, bn_ld4(a.mask + m * a.ldmask + col));
    const float4 xh = bn_xhat4(bn_ld4(a.z + m * a.ldz + col), mu, is);
    const float4 d = make_float4(sc.x * (gy.x - m1.x - xh.x * m2.x), sc.y * (gy.y - m1.y - xh.y * m2.y),
                                 sc.z * (gy.z - m1.z - xh.z * m2.z), sc.w * (gy.w - m1.w - xh.w * m2.w));
    bn_st4(a.dz + m * a.lddz + col, d);
    if (a.gy) bn_st4(a.gy + m * a.ldgy + col, gy);
  }
}

}  // namespace bevmsda
