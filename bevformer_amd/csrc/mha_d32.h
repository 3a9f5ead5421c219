// Self-attention core of the detection decoder: out = softmax(Q K^T * scale) V per (batch, head), head width D = 32, no
// masks.  Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) for both products in every GEMM mode: the two products
// are 0.83 GFLOP per layer at 900 queries, the kernel is bound by its dependent chain, not by the matrix rate.
//
// One workgroup per (32-query block, head, batch), kMhaWaves wavefronts.  The keys are walked in blocks of 32; wavefront w
// takes blocks w, w + kMhaWaves, ... with an online softmax of its own (running max m, running sum l, unnormalised O) and the
// wavefronts' partial results are merged through LDS at the end — the split-key form: at 900 keys every wavefront has a
// chain of 3 or 4 blocks instead of 29.  Nothing is staged in LDS on the way in: a head's K and V (115 KB each at 900
// keys) are read by the 29 workgroups of that head from L2, each operand fragment straight into the registers the MFMA
// wants, the next block's loads issued before the current block's arithmetic.
//
// Register layouts (v_mfma_f32_32x32x2_f32: lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], the 32 x 32
// result has its column j on the lane and row (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r):
//   S^T = K Q^T   A = K block (row = key), B = Q^T (column = query); MFMA step i sums d = 16 (l >> 5) + i, so that a lane
//                 reads 16 consecutive floats of its row (the order of the sum over d is free)
//   -> a lane holds, for ITS query, the scores of 16 keys: the softmax is a reduction over registers + one exchange between
//      the two lane halves, and m / l / the rescale factor are per-lane scalars
//   O^T = V^T P^T the probabilities stay where they are: register r is the B operand of step r (k = lane half <-> keys
//                 row(r), row(r) + 4), A = V[key][d = l & 31] — coalesced 128-byte rows.  O^T has the query on the lane again.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "scalar_ops.h"

namespace bevmsda {

constexpr int kMhaD = 32;          // head width
constexpr int kMhaBQ = 32;         // queries per workgroup
constexpr int kMhaBK = 32;         // keys per block
constexpr int kMhaWaves = 8;       // wavefronts per workgroup (key blocks are dealt round-robin)
static_assert(kMhaWaves * 64 == kMhaBQ * kMhaD / 2, "the merge step gives every thread two outputs");

struct MhaArgs {
  const float *q, *k, *v;          // row (t * bs + b) of a matrix with row stride ld*, head h in columns [32 h, 32 h + 32)
  float *o;
  long ldq, ldk, ldv, ldo;
  int nq, nk, bs;
  float scale;
};

typedef float mha_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int mha_tile_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ void mha_load_row16(const float *p, float (&f)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = reinterpret_cast<const float4 *>(p)[i];
    f[4 * i + 0] = t.x; f[4 * i + 1] = t.y; f[4 * i + 2] = t.z; f[4 * i + 3] = t.w;
  }
}

// K and V fragments of key block `blk` (rows beyond nk - 1 read row nk - 1: their scores are masked)
__device__ __forceinline__ void mha_load_kv(const MhaArgs &a, int blk, int b, int hcol, int col, int half, float (&kf)[16],
                                            float (&vf)[16]) {
  const int kr = min(blk * kMhaBK + col, a.nk - 1);
  mha_load_row16(a.k + (static_cast<long>(kr) * a.bs + b) * a.ldk + hcol + 16 * half, kf);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int vr = min(blk * kMhaBK + mha_tile_row(r, half), a.nk - 1);
    vf[r] = a.v[(static_cast<long>(vr) * a.bs + b) * a.ldv + hcol + col];
  }
}

__global__ __launch_bounds__(kMhaWaves * 64) void mha_d32_kernel(MhaArgs a) {
  __shared__ float s_m[kMhaWaves][kMhaBQ];
  __shared__ float s_l[kMhaWaves][kMhaBQ];
  __shared__ float s_o[kMhaWaves][kMhaBQ][kMhaD + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int q0 = blockIdx.x * kMhaBQ, hcol = blockIdx.y * kMhaD, b = blockIdx.z;
  const int nblk = (a.nk + kMhaBK - 1) / kMhaBK;
  const float ninf = -INFINITY;

  float qf[16];
  {
    const int qr = min(q0 + col, a.nq - 1);       // tail queries compute row nq - 1 again and store nothing
    mha_load_row16(a.q + (static_cast<long>(qr) * a.bs + b) * a.ldq + hcol + 16 * half, qf);
  }

  float m = ninf, l = 0.f;                         // (l: this lane half's keys only, the halves are summed at the end)
  mha_f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;

  float kf[16], vf[16];
  if (wave < nblk) mha_load_kv(a, wave, b, hcol, col, half, kf, vf);
  for (int blk = wave; blk < nblk; blk += kMhaWaves) {
    float kn[16], vn[16];
    mha_load_kv(a, min(blk + kMhaWaves, nblk - 1), b, hcol, col, half, kn, vn);     // next block in flight

    mha_f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[i], qf[i], s, 0, 0, 0);

    float mx = ninf;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float x = mul_scalar(s[r], a.scale);
      s[r] = blk * kMhaBK + mha_tile_row(r, half) < a.nk ? x : ninf;
      mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);              // finite: key blk * 32 of a block that is walked exists
    const float alpha = expf(sub_scalar(m, m_new));    // (first block: exp(-inf) = 0)
    float lsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(sub_scalar(s[r], m_new));
      lsum = add_scalar(lsum, s[r]);
    }
    l = fma_scalar(l, alpha, lsum);
    m = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = mul_scalar(o[r], alpha);
#pragma unroll
    for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[r], s[r], o, 0, 0, 0);

#pragma unroll
    for (int i = 0; i < 16; ++i) { kf[i] = kn[i]; vf[i] = vn[i]; }
  }

  // merge the wavefronts' (m, l, O): a wavefront without a block has m = -inf, l = 0, O = 0 and weighs exp(-inf) = 0
  l = add_scalar(l, __shfl_xor(l, 32));
  if (half == 0) { s_m[wave][col] = m; s_l[wave][col] = l; }
#pragma unroll
  for (int r = 0; r < 16; ++r) s_o[wave][col][mha_tile_row(r, half)] = o[r];
  __syncthreads();

  const int qi = threadIdx.x >> 4, d0 = (threadIdx.x & 15) * 2;      // 512 threads x 2 outputs = 32 queries x 32 channels
  float mall = ninf;
#pragma unroll
  for (int w = 0; w < kMhaWaves; ++w) mall = fmaxf(mall, s_m[w][qi]);
  float lall = 0.f, y0 = 0.f, y1 = 0.f;
#pragma unroll
  for (int w = 0; w < kMhaWaves; ++w) {
    const float f = expf(sub_scalar(s_m[w][qi], mall));
    lall = fma_scalar(s_l[w][qi], f, lall);
    y0 = fma_scalar(s_o[w][qi][d0], f, y0);
    y1 = fma_scalar(s_o[w][qi][d0 + 1], f, y1);
  }
  if (q0 + qi < a.nq) {
    float2 y;
    y.x = y0 / lall;
    y.y = y1 / lall;
    *reinterpret_cast<float2 *>(a.o + (static_cast<long>(q0 + qi) * a.bs + b) * a.ldo + hcol + d0) = y;
  }
}

}  // namespace bevmsda
