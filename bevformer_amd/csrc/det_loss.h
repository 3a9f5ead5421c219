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
// Values: everything is evaluated in fp64 and rounded to fp32 once.  One workgroup per layer (per layer and group in the
// Group-DETR form below): each lane adds its elements in index order, the wavefront adds by a fixed butterfly and lane 0
// adds the wavefronts in order — no floating-point atomics, so the loss is bit-reproducible from run to run.  The sigmoid
// is det_cost.h's (1 - p follows p's rounding, as in torch's autograd formulas).
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

// The sums of one workgroup over the bs * nq rows of layer `l`, group `g` of `G` (query g * nq + q of a sample is query q
// of the group; G = 1, g = 0: the layer's rows as they lie), and the gradients of those rows with the factors `kg_cls` /
// `kg_box` in place of the loss's.  The sums are thread 0's when the call returns.
__device__ __forceinline__ void det_loss_sums(const DetLossArgs &a, const int l, const int G, const int g, const double kg_cls,
                                              const double kg_box, double (*part)[kDetLossThreads / 64], double *sum_cls,
                                              double *sum_box) {
  const int tid = threadIdx.x;
  const long rows = static_cast<long>(a.bs) * a.nq;

  // ---- focal loss: one (row, class) element at a time
  double acc_cls = 0.0;
  for (long e = tid; e < rows * a.cls_out; e += kDetLossThreads) {
    const long row = e / a.cls_out;
    const int c = static_cast<int>(e - row * a.cls_out);
    const int b = static_cast<int>(row / a.nq);
    const long at_row = ((static_cast<long>(l) * a.bs + b) * G + g) * a.nq + (row - static_cast<long>(b) * a.nq);
    int n = a.count[b];
    n = n < 0 ? 0 : (n > a.gmax ? a.gmax : n);
    const int ai = a.assigned[at_row];
    const bool hit = ai >= 0 && ai < n && a.label[static_cast<long>(b) * a.gmax + ai] == c;
    const double x = static_cast<double>(a.cls[at_row * a.cls_out + c]);
    const double p = det_sigmoid(x);
    const double t = hit ? 1.0 : 0.0;
    const double pt = hit ? 1.0 - p : p;
    const double at = hit ? a.alpha : 1.0 - a.alpha;
    const double fw = at * pow(pt, a.gamma);
    const double bce = fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));
    const double dpt = (hit ? -1.0 : 1.0) * p * (1.0 - p);
    const double dfw = at * a.gamma * pow(pt, a.gamma - 1.0) * dpt;
    acc_cls += bce * fw;
    a.grad_cls[at_row * a.cls_out + c] = static_cast<float>(kg_cls * ((p - t) * fw + bce * dfw));
  }

  // ---- L1 loss: one row at a time (the positives are few)
  double acc_box = 0.0;
  for (long row = tid; row < rows; row += kDetLossThreads) {
    const int b = static_cast<int>(row / a.nq);
    const long at_row = ((static_cast<long>(l) * a.bs + b) * G + g) * a.nq + (row - static_cast<long>(b) * a.nq);
    int n = a.count[b];
    n = n < 0 ? 0 : (n > a.gmax ? a.gmax : n);
    const int ai = a.assigned[at_row];
    float *go = a.grad_box + at_row * a.code_size;
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
    const float *bx = a.box + at_row * a.code_size;
    for (int c = 0; c < a.code_size; ++c) {
      const double w = static_cast<double>(a.code_weights[c]);
      const double d = static_cast<double>(bx[c]) - tgt[c];
      acc_box += fabs(d) * w;
      go[c] = static_cast<float>(d > 0.0 ? kg_box * w : (d < 0.0 ? -(kg_box * w) : 0.0));
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
    *sum_cls = s0;
    *sum_box = s1;
  }
}

// grid (L), kDetLossThreads threads
__global__ void __launch_bounds__(kDetLossThreads) det_loss_kernel(const DetLossArgs a) {
  __shared__ double part[2][kDetLossThreads / 64];
  const int l = blockIdx.x;
  const double k_cls = a.cls_weight / static_cast<double>(a.factors[0]);
  const double k_box = a.box_weight / static_cast<double>(a.factors[1]);
  double s0 = 0.0, s1 = 0.0;
  det_loss_sums(a, l, 1, 0, k_cls, k_box, part, &s0, &s1);
  if (threadIdx.x == 0) {
    a.losses[2 * l] = det_nan_to_num(static_cast<float>(s0 * k_cls));
    a.losses[2 * l + 1] = det_nan_to_num(static_cast<float>(s1 * k_box));
  }
}

// Group-DETR (BEVFormerHead_GroupDETR.loss, dense_heads/bevformer_head.py:665-682): predictions and `assigned` are
// (L, bs, G * nq, .), every group of nq queries has the loss above against the same gt and factors, and the layer's loss is
// the mean over the groups.  One workgroup per (layer, group) writes the group's two fp32 losses — det_loss_kernel's values
// on the group's rows — to group_losses (L, G, 2) and the rows' gradients with 1 / G in the fp64 factor (one rounding);
// det_loss_group_mean_kernel then adds a layer's G values in fp64 in group order, divides by G and rounds once.  A second
// launch instead of an arrival count: nothing to reset between replays of a graph, and no atomics.
// grid (G, L), kDetLossThreads threads
__global__ void __launch_bounds__(kDetLossThreads) det_loss_grouped_kernel(const DetLossArgs a, float *group_losses) {
  __shared__ double part[2][kDetLossThreads / 64];
  const int G = gridDim.x, g = blockIdx.x, l = blockIdx.y;
  const double k_cls = a.cls_weight / static_cast<double>(a.factors[0]);
  const double k_box = a.box_weight / static_cast<double>(a.factors[1]);
  double s0 = 0.0, s1 = 0.0;
  det_loss_sums(a, l, G, g, k_cls / static_cast<double>(G), k_box / static_cast<double>(G), part, &s0, &s1);
  if (threadIdx.x == 0) {
    float *out = group_losses + (static_cast<long>(l) * G + g) * 2;
    out[0] = det_nan_to_num(static_cast<float>(s0 * k_cls));
    out[1] = det_nan_to_num(static_cast<float>(s1 * k_box));
  }
}

// losses[l, j] = mean over g of group_losses[l, g, j]; one thread per (l, j), grid (ceil(2 L / 64)), 64 threads
__global__ void __launch_bounds__(64) det_loss_group_mean_kernel(const float *group_losses, float *losses, const int L,
                                                                 const int G) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= 2 * L) return;
  const float *in = group_losses + static_cast<long>(i >> 1) * G * 2 + (i & 1);
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += static_cast<double>(in[2 * g]);
  losses[i] = static_cast<float>(s / static_cast<double>(G));
}

}  // namespace bevmsda
