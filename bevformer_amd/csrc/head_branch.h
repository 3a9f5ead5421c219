// The branches of the detection head as ONE launch (bevformer_head.py:118-213 of the reference; decoder.py:68-74):
//
//   reg   t = W3 relu(W2 relu(W1 x + b1) + b2) + b3                      256 -> 256 -> 256 -> code_size (8 | 10)
//   cls   s = V3 relu(LN(V2 relu(LN(V1 x + c1)) + c2)) + c3              256 -> 256 -> 256 -> cls_out (<= 32)
//
// followed, for the reg branch, by the reference-point arithmetic of the head (sigmoid(t + inverse_sigmoid(ref)) on columns
// 0, 1, 4, scaled to pc_range) or of the decoder's refinement (the same three columns as the layer's new reference point).
// Every step is local to a row of 256 floats, so one workgroup owns a panel of 32 rows and runs the whole branch on the
// machinery of the seam kernels (linear_chain.h, workgroup shape <1, 2, 4>): the panel is fetched whole by LDS-DMA and split
// once into [hi | lo] bf16 planes, weight fragments come from L2 in MFMA operand order, 4 wavefronts x 2 column tiles own the
// 256 columns of a stage, and the accumulators of a stage are written as the next stage's planes with the slot map of
// linear_panel.h (tests/test_linear_layout_model.py replays it).  The last projection has at most 32 output columns: its
// weight image is zero-padded to one 32-column tile, its K axis is split over the 4 wavefronts (4 k16 steps each) and the
// partial tiles are summed through LDS in wavefront order 0, 1, 2, 3 — a fixed order: results are run-to-run bit-equal.
//
// Grid: x = row panel, y = decoder layer (its own weights: a table indexed layer * layer_stride, stride 0 = one shared
// module), z = branch (0 reg, 1 cls).  Input rows arrive in the decoder's order (layer, query, batch), outputs are written
// as (layer, batch, query, .).  Rows past the end of a tail panel are computed from a clamped row and never stored.
//
// LDS: 2 x 32 KiB plane buffers + 0.5 KiB row statistics + 6.1 KiB per-column constants = 70.6 KiB: two workgroups per CU.
#pragma once
#include "linear_panel.h"
#include "scalar_ops.h"

namespace bevmsda {

constexpr int kHeadMaxLayers = 8;
constexpr int kHeadC = 256;

struct HeadBranchW {
  const uint16_t *w1, *w2, *w3;     // fragment-order images: (256, 256), (256, 256), (n_out <= 32 padded, 256)
  const float *b1, *b2, *b3;
  const float *g1, *be1, *g2, *be2; // cls: LayerNorm affine parameters; reg: unused
  float eps1, eps2;
};

struct HeadArgs {
  const float *x;                   // rows (layer, query, batch): x + layer * ld_layer + (q * bs + b) * ld_x
  long ld_x, ld_layer;
  const float *ref;                 // (L, bs, nq, 3): the reference point each layer consumed
  float *out_box;                   // head mode: (L, bs, nq, code_size); refine mode: (bs, nq, 3)
  float *out_cls;                   // (L, bs, nq, cls_out)
  int nq, bs, code_size, cls_out;
  int mode;                         // 0 head, 1 refine
  int layer_stride;                 // 1: entry `layer` of the tables, 0: entry 0 for every layer
  float pc[6];                      // pc_range: [0..2] the low ends, [3..5] the spans (high - low)
  HeadBranchW reg[kHeadMaxLayers], cls[kHeadMaxLayers];
};

// decoder.py:34-50 with eps = 1e-5 (plain fp32 scalar code)
__device__ __forceinline__ float head_inverse_sigmoid(float x) {
  x = fminf(fmaxf(x, 0.f), 1.f);
  const float x1 = fmaxf(x, 1e-5f);
  const float x2 = fmaxf(sub_scalar(1.f, x), 1e-5f);
  return logf(x1 / x2);
}
__device__ __forceinline__ float head_sigmoid(float x) { return 1.f / add_scalar(1.f, expf(-x)); }

template <int NPROD>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
head_branch_kernel(const HeadArgs a) {
  static_assert(NPROD == 1 || NPROD == 3, "NPROD");
  constexpr bool LO = NPROD == 3;
  constexpr int NPL = LO ? 2 : 1;
  constexpr int NT = 2, NW = 4, BM = 32;
  constexpr int BUF = (BM / 8) * 4 * 2048;     // one plane buffer: 32 KiB
  constexpr int NCST = 6 * kHeadC + 32;        // b1, b2, g1, be1, g2, be2 | b3
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF + NW * BM * 4 + NCST * 4];
  unsigned char *const buf0 = lds, *const buf1 = lds + BUF;
  float *const stat = reinterpret_cast<float *>(lds + 2 * BUF);       // [wave][row]
  float *const cst = stat + NW * BM;
  float *const c_b1 = cst, *const c_b2 = cst + 256, *const c_g1 = cst + 512, *const c_be1 = cst + 768;
  float *const c_g2 = cst + 1024, *const c_be2 = cst + 1280, *const c_b3 = cst + 1536;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int layer = blockIdx.y;
  const bool is_cls = blockIdx.z != 0;
  const long M = static_cast<long>(a.nq) * a.bs;
  const long m0 = static_cast<long>(blockIdx.x) * BM;
  const HeadBranchW &wt = is_cls ? a.cls[layer * a.layer_stride] : a.reg[layer * a.layer_stride];
  const int n_out = is_cls ? a.cls_out : a.code_size;

  {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t4 = tid * 4; t4 < 6 * kHeadC; t4 += 256 * 4) {
      const float *src;
      if (t4 < 256) src = wt.b1 + t4;
      else if (t4 < 512) src = wt.b2 + (t4 - 256);
      else if (t4 < 768) src = is_cls ? wt.g1 + (t4 - 512) : nullptr;
      else if (t4 < 1024) src = is_cls ? wt.be1 + (t4 - 768) : nullptr;
      else if (t4 < 1280) src = is_cls ? wt.g2 + (t4 - 1024) : nullptr;
      else src = is_cls ? wt.be2 + (t4 - 1280) : nullptr;
      *reinterpret_cast<float4 *>(cst + t4) = src ? *reinterpret_cast<const float4 *>(src) : z4;
    }
    if (tid < 32) c_b3[tid] = tid < n_out ? wt.b3[tid] : 0.f;
  }                                            // (visible after the barrier that closes the panel fetch)

  // fragment read addresses and accumulator -> plane write addresses (linear_panel.h / linear_chain.h)
  const int f_r = lane & 31, f_h = lane >> 5;
  const int f_q0 = ((f_r >> 2) & 1) | ((f_r >> 4) << 1);
  const int f_rl = ((f_r & 3) << 1) | ((f_r >> 3) & 1);
  const int f_x = f_r & 7;
  unsigned f_addr[4];
#pragma unroll
  for (int sc = 0; sc < 4; ++sc)
    f_addr[sc] = static_cast<unsigned>(f_q0 * 4 * 2048 + (f_rl * 8 + (((2 * sc + f_h) ^ f_x))) * 16);
  unsigned p_addr[NT][4];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int line = NT * wave + j;
      p_addr[j][g] = static_cast<unsigned>((f_q0 * 4 + (line >> 1)) * 2048 + (f_rl * 8 + ((f_h + 2 * g) ^ f_x)) * 16 + (line & 1) * 8);
    }

  const int wlane = lane * 16;
  lin_f32x16 acc[NT];
  constexpr int WD = 2;                        // weight fragments in flight (k16 steps ahead)
  lin_bf16x8 wf[WD + 1][NT][NPL];
  auto wload = [&](__amdgpu_buffer_rsrc_t wrsrc, int st, int sg) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
        wf[st][j][pl] = __builtin_bit_cast(lin_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                                         wrsrc, wlane, (((wave * NT + j) * 16 + sg) * 2 + pl) * 1024, 0));
  };
  auto wprefetch = [&](__amdgpu_buffer_rsrc_t wrsrc) {
#pragma unroll
    for (int k = 0; k < WD; ++k) wload(wrsrc, k, k);
  };
  // acc += planes(buf) x W[this wavefront's two column tiles]^T over K = 256; ring stages 0 .. WD - 1 hold steps 0 .. WD - 1
  auto gemm16 = [&](const unsigned char *buf, __amdgpu_buffer_rsrc_t wrsrc) {
    lin_bf16x8 af[2][NPL];
    auto aload = [&](int set, int s) {
      const unsigned base = f_addr[s & 3] + (s >> 2) * 2048;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) af[set][pl] = *reinterpret_cast<const lin_bf16x8 *>(buf + base + pl * 1024);
    };
    aload(0, 0);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s + WD < 16) wload(wrsrc, (s + WD) % (WD + 1), s + WD);
      if (s + 1 < 16) aload((s + 1) & 1, s + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if constexpr (LO) {
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s % (WD + 1)][j][0], af[s & 1][1], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s % (WD + 1)][j][1], af[s & 1][0], acc[j], 0, 0, 0);
        }
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s % (WD + 1)][j][0], af[s & 1][0], acc[j], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto zero = [&]() {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  };
  auto to_planes = [&](unsigned char *buf) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float v0 = acc[j][4 * g], v1 = acc[j][4 * g + 1], v2 = acc[j][4 * g + 2], v3 = acc[j][4 * g + 3];
        uint2 hi, lo;
        hi.x = lin_pack2(v0, v1);
        hi.y = lin_pack2(v2, v3);
        unsigned char *dst = buf + p_addr[j][g];
        *reinterpret_cast<uint2 *>(dst) = hi;
        if (LO) {
          lo.x = lin_pack2(v0 - __uint_as_float(hi.x << 16), v1 - __uint_as_float(hi.x & 0xffff0000u));
          lo.y = lin_pack2(v2 - __uint_as_float(hi.y << 16), v3 - __uint_as_float(hi.y & 0xffff0000u));
          *reinterpret_cast<uint2 *>(dst + 1024) = lo;
        }
      }
  };
  auto ncol = [&](int j) { return (NT * wave + j) * 32 + 4 * (lane >> 5); };
  // + bias [-> LayerNorm over the row's 256 columns, statistics exchanged through LDS as linear_chain.h does] -> relu
  auto epilogue = [&](const float *bias, const float *gamma, const float *beta, float eps) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = *reinterpret_cast<const float4 *>(bias + ncol(j) + 8 * g);
        acc[j][4 * g] += v.x; acc[j][4 * g + 1] += v.y; acc[j][4 * g + 2] += v.z; acc[j][4 * g + 3] += v.w;
      }
    if (is_cls) {                              // (uniform over the workgroup: every wavefront reaches the barriers)
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += acc[j][r];
      sum += __shfl_xor(sum, 32, 64);
      if (lane < 32) stat[wave * BM + lane] = sum;
      __syncthreads();
      float mean = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) mean += stat[w * BM + (lane & 31)];
      mean *= (1.0f / kHeadC);
      __syncthreads();
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = acc[j][r] - mean;
          ss = fmaf(d, d, ss);
        }
      ss += __shfl_xor(ss, 32, 64);
      if (lane < 32) stat[wave * BM + lane] = ss;
      __syncthreads();
      float var = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) var += stat[w * BM + (lane & 31)];
      const float rstd = rsqrtf(fma_scalar(var, 1.0f / kHeadC, eps));
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = ncol(j) + 8 * g;
          const float4 ga = *reinterpret_cast<const float4 *>(gamma + n);
          const float4 be = *reinterpret_cast<const float4 *>(beta + n);
          acc[j][4 * g] = (acc[j][4 * g] - mean) * rstd * ga.x + be.x;
          acc[j][4 * g + 1] = (acc[j][4 * g + 1] - mean) * rstd * ga.y + be.y;
          acc[j][4 * g + 2] = (acc[j][4 * g + 2] - mean) * rstd * ga.z + be.z;
          acc[j][4 * g + 3] = (acc[j][4 * g + 3] - mean) * rstd * ga.w + be.w;
        }
      __syncthreads();                         // `stat` may be written again
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = acc[j][r] < 0.f ? 0.f : acc[j][r];     // NaN stays NaN, as torch.relu
  };

  const unsigned wfull = 8u * 16 * 2 * 1024, wlast = 2u * 16 * 2 * 1024;      // image bytes: 256 rows; 32 rows padded to 64
  __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(wt.w1), 0, static_cast<int>(wfull), 0x00020000);
  __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(wt.w2), 0, static_cast<int>(wfull), 0x00020000);
  __amdgpu_buffer_rsrc_t r3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(wt.w3), 0, static_cast<int>(wlast), 0x00020000);
  wprefetch(r1);

  // ------------------------------------------------------------------ fetch + split the panel of x (buffer 0)
  {
    const int d_rl = lane >> 3, d_cc = lane & 7;
    const int row = panel_row_of(wave, d_rl);  // one row block (4 line pairs) per wavefront
    const int cx = d_cc ^ (row & 7);
    long gm = m0 + row;
    if (gm >= M) gm = M - 1;                   // clamped rows are computed and never stored
    const float *xrow = a.x + layer * a.ld_layer + gm * a.ld_x;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float *src = xrow + (2 * p) * 32 + cx * 4;
      unsigned char *dst = buf0 + (wave * 4 + p) * 2048;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src),
                                       (__attribute__((address_space(3))) void *)(dst), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + 32),
                                       (__attribute__((address_space(3))) void *)(dst + 1024), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my own DMA slots have landed
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      unsigned char *slot = buf0 + (wave * 4 + p) * 2048 + lane * 16;
      const float4 va = *reinterpret_cast<const float4 *>(slot);
      const float4 vb = *reinterpret_cast<const float4 *>(slot + 1024);
      uint4 hi, lo;
      lin_split8<LO>(va, vb, hi, lo);
      *reinterpret_cast<uint4 *>(slot) = hi;
      if (LO) *reinterpret_cast<uint4 *>(slot + 1024) = lo;
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ stage 1 and stage 2
  zero();
  gemm16(buf0, r1);
  wprefetch(r2);
  epilogue(c_b1, c_g1, c_be1, wt.eps1);
  to_planes(buf1);
  __syncthreads();                             // stage 1's planes complete, every wavefront is done with buffer 0
  zero();
  gemm16(buf1, r2);
  epilogue(c_b2, c_g2, c_be2, wt.eps2);
  to_planes(buf0);
  __syncthreads();                             // stage 2's planes complete, every wavefront is done with buffer 1

  // ------------------------------------------------------------------ last projection: one 32-column tile, K split 4 ways
  float *const part = reinterpret_cast<float *>(buf1);                // [wave][row][32] partial tiles
  float *const fin = part + NW * BM * 32;                             // [row][32] the branch's output rows
  {
    lin_f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    lin_bf16x8 w3f[4][NPL], a3f[4][NPL];
#pragma unroll
    for (int ss = 0; ss < 4; ++ss)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        w3f[ss][pl] = __builtin_bit_cast(lin_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                                       r3, wlane, ((wave * 4 + ss) * 2 + pl) * 1024, 0));
        a3f[ss][pl] = *reinterpret_cast<const lin_bf16x8 *>(buf0 + f_addr[ss] + wave * 2048 + pl * 1024);
      }
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {
      if constexpr (LO) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3f[ss][0], a3f[ss][1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3f[ss][1], a3f[ss][0], c, 0, 0, 0);
      }
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3f[ss][0], a3f[ss][0], c, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4 *>(part + (wave * BM + (lane & 31)) * 32 + 4 * (lane >> 5) + 8 * g) =
          make_float4(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
  }
  __syncthreads();
  {
    const int row = tid >> 3, c0 = (tid & 7) * 4;                     // 256 threads x 4 columns = 32 x 32
    const float4 p0 = *reinterpret_cast<const float4 *>(part + (0 * BM + row) * 32 + c0);
    const float4 p1 = *reinterpret_cast<const float4 *>(part + (1 * BM + row) * 32 + c0);
    const float4 p2 = *reinterpret_cast<const float4 *>(part + (2 * BM + row) * 32 + c0);
    const float4 p3 = *reinterpret_cast<const float4 *>(part + (3 * BM + row) * 32 + c0);
    float *f = fin + row * 32 + c0;
    f[0] = add_scalar(add_scalar(add_scalar(add_scalar(p0.x, p1.x), p2.x), p3.x), c_b3[c0]);
    f[1] = add_scalar(add_scalar(add_scalar(add_scalar(p0.y, p1.y), p2.y), p3.y), c_b3[c0 + 1]);
    f[2] = add_scalar(add_scalar(add_scalar(add_scalar(p0.z, p1.z), p2.z), p3.z), c_b3[c0 + 2]);
    f[3] = add_scalar(add_scalar(add_scalar(add_scalar(p0.w, p1.w), p2.w), p3.w), c_b3[c0 + 3]);
  }
  __syncthreads();

  // ------------------------------------------------------------------ stores: row m = q * bs + b -> (layer, b, q, .)
  if (is_cls) {
    const int total = BM * n_out;
    for (int idx = tid; idx < total; idx += 256) {
      const int row = idx / n_out, c = idx - row * n_out;
      const long m = m0 + row;
      if (m >= M) continue;
      const long q = m / a.bs, b = m - q * a.bs;
      a.out_cls[((static_cast<long>(layer) * a.bs + b) * a.nq + q) * n_out + c] = fin[row * 32 + c];
    }
    return;
  }
  if (tid < BM) {
    const long m = m0 + tid;
    if (m >= M) return;
    const long q = m / a.bs, b = m - q * a.bs;
    const long orow = (static_cast<long>(layer) * a.bs + b) * a.nq + q;
    const float *t = fin + tid * 32;
    const float *rf = a.ref + orow * 3;
    const float s0 = head_sigmoid(add_scalar(t[0], head_inverse_sigmoid(rf[0])));
    const float s1 = head_sigmoid(add_scalar(t[1], head_inverse_sigmoid(rf[1])));
    const float s4 = head_sigmoid(add_scalar(t[4], head_inverse_sigmoid(rf[2])));
    if (a.mode == 1) {
      float *o = a.out_box + orow * 3;
      o[0] = s0; o[1] = s1; o[2] = s4;
      return;
    }
    float *o = a.out_box + orow * a.code_size;
    // bevformer_head.py:187-192: x * (hi - lo) + lo, as two rounded steps
    o[0] = add_scalar(mul_scalar(s0, a.pc[3]), a.pc[0]);
    o[1] = add_scalar(mul_scalar(s1, a.pc[4]), a.pc[1]);
    o[2] = t[2];
    o[3] = t[3];
    o[4] = add_scalar(mul_scalar(s4, a.pc[5]), a.pc[2]);
    for (int c = 5; c < a.code_size; ++c) o[c] = t[c];
  }
}

}  // namespace bevmsda
