// The optimizer step on the device: clip_grad_norm_(norm_type = 2) + torch's single-tensor AdamW in TWO launches over a
// device-resident job table (one job per parameter tensor that has a gradient this step; the idea of
// lin_pack_weights_multi_kernel's PackJob table in linear_pack_multi.h).  Every scalar of the step — the norm, the clip
// coefficient, the skip flag, each parameter's step count, the groups' hyperparameters — lives in device memory, so the two
// launches can be captured in a HIP graph together with the forward, the loss and the backward.
//
//   optim_grad_norm_kernel   block b sums the squares of its <= 4096 gradient elements: <= 16 per thread in fp32 (the issue's
//                            bound is 128), then double over the wave and the block -> partials[b].  The block whose ticket
//                            is the last sums the partials in a FIXED order (each thread a contiguous run in index order,
//                            thread 0 the 256 run sums in index order): no float atomics, bit-reproducible.  It writes
//                            total_norm, clip_coef = min(1, max_norm / (total_norm + 1e-6)) (torch's statement; 1 with
//                            clipping off; a NaN norm stays NaN as torch.clamp keeps it), the skip flag, and either bumps
//                            `skipped` or adds 1 to every job's step scalar.  The ticket goes back to 0 for the next launch.
//   optim_adamw_kernel       4096 elements per block; 16-byte lanes when p, g, exp_avg, exp_avg_sq of the job are all 16-byte
//                            aligned, else element by element (flatten_linear_params hands out bias views at 4-byte
//                            offsets); g is scaled by clip_coef in registers and never written.  Algorithmic bytes per
//                            element: 16 read + 12 written (the norm kernel: 4 read).
//
// Hand-off of the partials (per-XCD L2s are not coherent, a CU's L1 is never refreshed by another CU's stores): lane 0 of every block stores its partial with an
// agent-scope 8-byte store, waits for it, fences and takes a ticket with an agent-scope atomic add whose value it uses; the
// last block acquires at agent scope behind a workgroup barrier and reads the partials with agent-scope loads.
// The arithmetic is written with scalar_ops.h: one opaque VALU instruction per operation, in the order of torch's
// statements, the same on the 16-byte and the element path — and nothing for the vectoriser to pair (tests/test_build_flags.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "scalar_ops.h"

namespace bevmsda {

constexpr int kOptimThreads = 256;
constexpr int kOptimBlockElems = 4096;      // elements of one job per block, both kernels
constexpr int kOptimScalarWords = 8;        // the scalars block, 4-byte words (include/bevmsda.h)

struct OptimJob {                           // = bevmsda_optim_job
  float *p;
  const float *g;
  float *exp_avg;
  float *exp_avg_sq;
  float *step;                              // the parameter's step count, a float32 scalar as in torch's state
  long long numel;
  int group;
  int first_block;
};

struct OptimGroup {                         // = bevmsda_optim_group
  double lr, beta1, beta2, eps, weight_decay;
};

struct OptimScalars {                       // = the `scalars` argument, 8 words
  float total_norm;
  float clip_coef;
  int skip;                                 // 1: this step is skipped (non-finite norm with skip_nonfinite)
  int skipped;                              // steps skipped so far
  unsigned ticket;                          // 0 between launches
  int reserved[3];
};

// the job whose block range holds block b (uniform: scalar loads); jobs without a block are never found
__device__ __forceinline__ int optim_find_job(const OptimJob *__restrict__ jobs, int njobs, int b) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ double optim_wave_sum(double x) {      // lanes 0 .. 63 in a fixed tree
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

__global__ void __launch_bounds__(kOptimThreads) optim_grad_norm_kernel(const OptimJob *__restrict__ jobs, int njobs,
                                                                         int blocks, double max_norm, int flags,
                                                                         double *partials, OptimScalars *scalars) {
  __shared__ double s_part[kOptimThreads];
  __shared__ int s_last, s_skip;
  const int tid = static_cast<int>(threadIdx.x);
  const int b = static_cast<int>(blockIdx.x);
  float acc = 0.f;
  if (b < blocks) {                                              // (blocks = 0: one block with nothing to sum)
    const OptimJob &j = jobs[optim_find_job(jobs, njobs, b)];
    const long long base = static_cast<long long>(b - j.first_block) * kOptimBlockElems;
    const long long n = j.numel;
    const float *__restrict__ g = j.g;
    if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long i = base + k * (kOptimThreads * 4) + tid * 4;
        if (i + 4 <= n) {
          const float4 x = *reinterpret_cast<const float4 *>(g + i);
          acc = fma_scalar(x.x, x.x, acc); acc = fma_scalar(x.y, x.y, acc);
          acc = fma_scalar(x.z, x.z, acc); acc = fma_scalar(x.w, x.w, acc);
        } else {
          for (int e = 0; e < 4; ++e)
            if (i + e < n) { const float x = g[i + e]; acc = fma_scalar(x, x, acc); }
        }
      }
    } else {
#pragma unroll 4
      for (int k = 0; k < kOptimBlockElems / kOptimThreads; ++k) {
        const long long i = base + k * kOptimThreads + tid;
        if (i < n) { const float x = g[i]; acc = fma_scalar(x, x, acc); }
      }
    }
  }
  const double w = optim_wave_sum(static_cast<double>(acc));
  if ((tid & 63) == 0) s_part[tid >> 6] = w;
  __syncthreads();
  if (tid == 0) {
    const double sum = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
    __hip_atomic_store(partials + b, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(&scalars->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;

  // ---- the last block: every partial has been stored and released
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int nb = static_cast<int>(gridDim.x);
  const int run = (nb + kOptimThreads - 1) / kOptimThreads;
  double s = 0.0;
  for (int i = tid * run, e = min(nb, (tid + 1) * run); i < e; ++i)
    s += __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s_part[tid] = s;                                               // (thread 0 read s_part before the barrier above)
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int i = 0; i < kOptimThreads; ++i) total += s_part[i];
    const float norm = static_cast<float>(sqrt(total));
    float coef = 1.f;
    if (flags & 1) {                                             // clip_coef_clamped of torch.nn.utils.clip_grad_norm_
      const float c = static_cast<float>(max_norm) / (norm + 1e-6f);
      coef = c > 1.f ? 1.f : c;                                  // (a NaN stays a NaN, as in torch.clamp)
    }
    const int skip = ((flags & 2) && !isfinite(norm)) ? 1 : 0;
    scalars->total_norm = norm;
    scalars->clip_coef = coef;
    scalars->skip = skip;
    if (skip) scalars->skipped = scalars->skipped + 1;
    __hip_atomic_store(&scalars->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_skip = skip;
  }
  __syncthreads();
  if (!s_skip)
    for (int i = tid; i < njobs; i += kOptimThreads) {
      float *st = jobs[i].step;
      *st = *st + 1.f;
    }
}

struct OptimConsts {          // per block, rounded once from the double statements
  float clip, decay, w1, beta2, w2, bc2_sqrt, eps, neg_step;
};

// torch/optim/adamw.py, _single_tensor_adamw: param.mul_(1 - lr * wd); exp_avg.lerp_(grad, 1 - beta1);
// exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2); denom = exp_avg_sq.sqrt() / sqrt(bias2) + eps;
// param.addcdiv_(exp_avg, denom, value = -lr / bias1)
__device__ __forceinline__ void optim_adamw_element(float &p, float g, float &m, float &v, const OptimConsts &c) {
  g = mul_scalar(g, c.clip);
  const float pd = mul_scalar(p, c.decay);
  m = fma_scalar(sub_scalar(g, m), c.w1, m);
  v = fma_scalar(mul_scalar(g, g), c.w2, mul_scalar(v, c.beta2));
  const float denom = add_scalar(sqrtf(v) / c.bc2_sqrt, c.eps);      // (correctly rounded: hipcc's default for fp32 / and sqrt)
  p = fma_scalar(c.neg_step, m / denom, pd);
}

__global__ void __launch_bounds__(kOptimThreads) optim_adamw_kernel(const OptimJob *__restrict__ jobs, int njobs,
                                                                     const OptimGroup *__restrict__ groups,
                                                                     const OptimScalars *__restrict__ scalars) {
  if (scalars->skip) return;
  const int tid = static_cast<int>(threadIdx.x);
  const int b = static_cast<int>(blockIdx.x);
  const OptimJob &j = jobs[optim_find_job(jobs, njobs, b)];
  const OptimGroup &gr = groups[j.group];
  const double t = static_cast<double>(*j.step);                 // already advanced by the norm kernel
  const double bias1 = 1.0 - pow(gr.beta1, t), bias2 = 1.0 - pow(gr.beta2, t);
  OptimConsts c;
  c.clip = scalars->clip_coef;
  c.decay = static_cast<float>(1.0 - gr.lr * gr.weight_decay);
  c.w1 = static_cast<float>(1.0 - gr.beta1);
  c.beta2 = static_cast<float>(gr.beta2);
  c.w2 = static_cast<float>(1.0 - gr.beta2);
  c.bc2_sqrt = static_cast<float>(sqrt(bias2));
  c.eps = static_cast<float>(gr.eps);
  c.neg_step = static_cast<float>(-(gr.lr / bias1));
  const long long base = static_cast<long long>(b - j.first_block) * kOptimBlockElems;
  const long long n = j.numel;
  float *__restrict__ p = j.p;
  const float *__restrict__ g = j.g;
  float *__restrict__ m = j.exp_avg;
  float *__restrict__ v = j.exp_avg_sq;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                         reinterpret_cast<uintptr_t>(v);
  if ((bits & 15u) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = base + k * (kOptimThreads * 4) + tid * 4;
      if (i + 4 <= n) {
        const float4 pp = *reinterpret_cast<const float4 *>(p + i), gg = *reinterpret_cast<const float4 *>(g + i);
        const float4 mm = *reinterpret_cast<const float4 *>(m + i), vv = *reinterpret_cast<const float4 *>(v + i);
        float pa[4] = {pp.x, pp.y, pp.z, pp.w}, ma[4] = {mm.x, mm.y, mm.z, mm.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
        const float ga[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) optim_adamw_element(pa[e], ga[e], ma[e], va[e], c);
        *reinterpret_cast<float4 *>(p + i) = make_float4(pa[0], pa[1], pa[2], pa[3]);
        *reinterpret_cast<float4 *>(m + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
        *reinterpret_cast<float4 *>(v + i) = make_float4(va[0], va[1], va[2], va[3]);
      } else {
        for (int e = 0; e < 4; ++e)
          if (i + e < n) {
            float pe = p[i + e], me = m[i + e], ve = v[i + e];
            optim_adamw_element(pe, g[i + e], me, ve, c);
            p[i + e] = pe; m[i + e] = me; v[i + e] = ve;
          }
      }
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < kOptimBlockElems / kOptimThreads; ++k) {
      const long long i = base + k * kOptimThreads + tid;
      if (i < n) {
        float pe = p[i], me = m[i], ve = v[i];
        optim_adamw_element(pe, g[i], me, ve, c);
        p[i] = pe; m[i] = me; v[i] = ve;
      }
    }
  }
}

}  // namespace bevmsda
