// BEVFormerHead.loss_single (dense_heads/bevformer_head.py:325-393 of the reference) for every decoder layer in one launch,
// given the assignment: sigmoid focal loss (mmdet's FocalLoss) against the one-hot of the matched gt's label — background:
// all zeros — and L1 (mmdet's L1Loss) over the code_size columns against normalize_bbox of the matched gt, times
// code_weights; each summed over the layer's bs * nq rows, divided by its averaging factor and multiplied by its weight:
//
//   losses[l] = (cls_weight * sum_focal / factors[0], box_weight * sum_l1 / factors[1])            nan_to_num applied
//   grad_cls[l, b, q, c] = d losses[l, 0] / d cls[l, b, q, c]        grad_box[l, b, q, c] = d losses[l, 1] / d box[l, b, q, c]
//
// factors: two fp32 in DEVICE memory (the caller's max(num_pos, 1), after its all-reduce under DDP): nothing is read by the
// host.  A row whose normalised target has a non-finite entry (a gt of zero width: log 0) has box weight 0, as the
// reference drops it; an `assigned` entry outside [0, count[b]) is background.
//
// Values: everything is evaluated in fp64 and rounded to fp32 once.  One workgroup per layer: each lane adds its elements
// in index order, the wavefront adds by a fixed butterfly and lane 0 adds the wavefronts in order — no floating-point
// atomics, so the loss is bit-reproducible from run to run.  The sigmoid is det_cost.h's (1 - p follows p's rounding, as in
// torch's autograd formulas).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_cost.h"

namespace bevmsda {

constexpr int kDetLossThreads = 512;

struct DetLossArgs {
  const float *cls;           // (L, bs, nq, cls_out)
  const float *box;           // (L, bs, nq, code_size)
  const float *gt;            // (bs, gmax, code_size - 1)
  const int *label;           // (bs, gmax)
  const int *count;           // (bs)
  const int *assigned;        // (L, bs, nq): 0-based gt of each query, -1 background
  const float *code_weights;  // (code_size)
  const float *factors;       // (2): cls_avg_factor, num_total_pos
  float *losses;              // (L, 2)
  float *grad_cls;            // (L, bs, nq, cls_out)
  float *grad_box;            // (L, bs, nq, code_size)
  int bs, nq, cls_out, code_size, gmax;
  double alpha, gamma, cls_weight, box_weight;
};

__device__ __forceinline__ float det_nan_to_num(float x) {
  if (x != x) return 0.f;
  if (x > 3.402823466e+38f) return 3.402823466e+38f;
  if (x < -3.402823466e+38f) return -3.402823466e+38f;
  return x;
}

__device__ __forceinline__ double det_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

__global__ void __launch_bounds__(kDetLossThreads) det_loss_kernel(const DetLossArgs a) {
  __shared__ double part[2][kDetLossThreads / 64];
  const int tid = threadIdx.x;
  const int l = blockIdx.x;
  const long rows = static_cast<long>(a.bs) * a.nq;
  const double k_cls = a.cls_weight / static_cast<double>(a.factors[0]);
  const double k_box = a.box_weight / static_cast<double>(a.factors[1]);
  const int *assigned = a.assigned + l * rows;

  // ---- focal loss: one (row, class) element at a time
  double acc_cls = 0.0;
  const float *cls = a.cls + l * rows * a.cls_out;
  float *gcls = a.grad_cls + l * rows * a.cls_out;
  for (long e = tid; e < rows * a.cls_out; e += kDetLossThreads) {
    const long row = e / a.cls_out;
    const int c = static_cast<int>(e - row * a.cls_out);
    const int b = static_cast<int>(row / a.nq);
    int n = a.count[b];
    n = n < 0 ? 0 : (n > a.gmax ? a.gmax : n);
    const int ai = assigned[row];
    const bool hit = ai >= 0 && ai < n && a.label[static_cast<long>(b) * a.gmax + ai] == c;
    const double x = static_cast<double>(cls[e]);
    const double p = det_sigmoid(x);
    const double t = hit ? 1.0 : 0.0;
    const double pt = hit ? 1.0 - p : p;
    const double at = hit ? a.alpha : 1.0 - a.alpha;
    const double fw = at * pow(pt, a.gamma);
    const double bce = fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));
    const double dpt = (hit ? -1.0 : 1.0) * p * (1.0 - p);
    const double dfw = at * a.gamma * pow(pt, a.gamma - 1.0) * dpt;
    acc_cls += bce * fw;
    gcls[e] = static_cast<float>(k_cls * ((p - t) * fw + bce * dfw));
  }

  // ---- L1 loss: one row at a time (the positives are few)
  double acc_box = 0.0;
  const float *box = a.box + l * rows * a.code_size;
  float *gbox = a.grad_box + l * rows * a.code_size;
  for (long row = tid; row < rows; row += kDetLossThreads) {
    const int b = static_cast<int>(row / a.nq);
    int n = a.count[b];
    n = n < 0 ? 0 : (n > a.gmax ? a.gmax : n);
    const int ai = assigned[row];
    float *go = gbox + row * a.code_size;
    bool pos = ai >= 0 && ai < n;
    double tgt[10];
    if (pos) {
      const float *gt = a.gt + (static_cast<long>(b) * a.gmax + ai) * (a.code_size - 1);
      for (int c = 0; c < a.code_size; ++c) {
        tgt[c] = det_normalized_entry(gt, c);
        const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(tgt[c]));
        if ((bits & 0x7ff0000000000000ULL) == 0x7ff0000000000000ULL) pos = false;       // inf or NaN: the row is dropped
      }
    }
    if (!pos) {
      for (int c = 0; c < a.code_size; ++c) go[c] = 0.f;
      continue;
    }
    const float *bx = box + row * a.code_size;
    for (int c = 0; c < a.code_size; ++c) {
      const double w = static_cast<double>(a.code_weights[c]);
      const double d = static_cast<double>(bx[c]) - tgt[c];
      acc_box += fabs(d) * w;
      go[c] = static_cast<float>(d > 0.0 ? k_box * w : (d < 0.0 ? -(k_box * w) : 0.0));
    }
  }

  acc_cls = det_wave_sum(acc_cls);
  acc_box = det_wave_sum(acc_box);
  if ((tid & 63) == 0) {
    part[0][tid >> 6] = acc_cls;
    part[1][tid >> 6] = acc_box;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int w = 0; w < kDetLossThreads / 64; ++w) {
      s0 += part[0][w];
      s1 += part[1][w];
    }
    a.losses[2 * l] = det_nan_to_num(static_cast<float>(s0 * k_cls));
    a.losses[2 * l + 1] = det_nan_to_num(static_cast<float>(s1 * k_box));
  }
}

}  // namespace bevmsda
