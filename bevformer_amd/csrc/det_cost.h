// The match costs of HungarianAssigner3D (core/bbox/assigners/hungarian_assigner_3d.py:106-115 of the reference) for every
// decoder layer and sample in one launch:
//
//   cost[l, b, g, q] = cls_weight * (pos - neg)(sigmoid(cls[l, b, q, label[b, g]]))           mmdet's FocalLossCost
//                    + reg_weight * sum_{c < 8} |box[l, b, q, c] - normalize_bbox(gt[b, g])[c]|   BBox3DL1Cost over cdist(p=1)
//
// gt-major: a gt's row of nq query costs is contiguous, which is how the assignment solver (match_lsap.h) scans it.  Rows
// g >= count[b] (padding) are NOT written.
//
// Values: sigmoid, log, pow, sin and cos are evaluated in fp64 and the ten terms (pos, neg, eight differences) are summed in
// fp64; the stored fp32 is one rounding of that.  The sigmoid is 1 / (1 + exp(-x)) with an IEEE division, the form torch's
// CPU kernel has: `1 - p` cancels for large logits, and the cost of a saturated logit (|x| ~ 30) follows the ROUNDING of p,
// so a second formula for the same function would move such costs in the fifth digit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bevmsda {

constexpr int kLossMaxQueries = 2048;
constexpr int kLossMaxGt = 512;
constexpr int kLossMaxCls = 32;

struct DetCostArgs {
  const float *cls;        // (L, bs, nq, cls_out) logits
  const float *box;        // (L, bs, nq, code_size)
  const float *gt;         // (bs, gmax, code_size - 1): cx, cy, cz, w, l, h, rot[, vx, vy]
  const int *label;        // (bs, gmax)
  const int *count;        // (bs)
  float *cost;             // (L, bs, gmax, nq)
  int bs, nq, cls_out, code_size, gmax;
  double cls_weight, reg_weight, alpha, gamma, eps;
};

__device__ __forceinline__ double det_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// normalize_bbox (core/bbox/util.py:4-24), the first `n` (<= 10) entries of the normalised row of a (code_size - 1)-wide gt
__device__ __forceinline__ double det_normalized_entry(const float *g, int c) {
  switch (c) {
    case 0: return static_cast<double>(g[0]);
    case 1: return static_cast<double>(g[1]);
    case 2: return log(static_cast<double>(g[3]));
    case 3: return log(static_cast<double>(g[4]));
    case 4: return static_cast<double>(g[2]);
    case 5: return log(static_cast<double>(g[5]));
    case 6: return sin(static_cast<double>(g[6]));
    case 7: return cos(static_cast<double>(g[6]));
    default: return static_cast<double>(g[c - 1]);       // 8, 9: vx, vy (9-wide gt only)
  }
}

// one (gt, query) pair per thread: gt blockIdx.y of sample `b` against query blockIdx.x * 256 + threadIdx.x of problem `p`,
// whose a.nq prediction rows start at row p * nq; `ngt`: eight doubles of LDS
__device__ __forceinline__ void det_cost_problem(const DetCostArgs &a, const int p, const int b, double *ngt) {
  const int g = blockIdx.y;
  int n = a.count[b];
  n = n < 0 ? 0 : (n > a.gmax ? a.gmax : n);
  if (g >= n) return;                       // (uniform over the workgroup)
  const float *gt = a.gt + (static_cast<long>(b) * a.gmax + g) * (a.code_size - 1);
  if (threadIdx.x < 8) ngt[threadIdx.x] = det_normalized_entry(gt, threadIdx.x);
  __syncthreads();
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.nq) return;
  const int lab = a.label[static_cast<long>(b) * a.gmax + g];
  const long row = static_cast<long>(p) * a.nq + q;
  double acc = 0.0;
  if (lab >= 0 && lab < a.cls_out) {
    const double pr = det_sigmoid(static_cast<double>(a.cls[row * a.cls_out + lab]));
    const double neg = -log(1.0 - pr + a.eps) * (1.0 - a.alpha) * pow(pr, a.gamma);
    const double pos = -log(pr + a.eps) * a.alpha * pow(1.0 - pr, a.gamma);
    acc = (pos - neg) * a.cls_weight;
  }
  const float *bx = a.box + row * a.code_size;
  double l1 = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) l1 += fabs(static_cast<double>(bx[c]) - ngt[c]);
  acc += l1 * a.reg_weight;
  a.cost[(static_cast<long>(p) * a.gmax + g) * a.nq + q] = static_cast<float>(acc);
}

// grid (ceil(nq / 256), gmax, L * bs), 256 threads
__global__ void __launch_bounds__(256) det_cost_kernel(const DetCostArgs a) {
  __shared__ double ngt[8];
  const int p = blockIdx.z;                 // l * bs + b
  det_cost_problem(a, p, p % a.bs, ngt);
}

// Group-DETR (BEVFormerHead_GroupDETR.loss, dense_heads/bevformer_head.py:665-674): the predictions (L, bs, groups * nq, .)
// hold `groups` blocks of a.nq queries, query g * nq + q of a sample is query q of group g, and every (layer, sample, group)
// is a matching problem of its own against the sample's gt.  Problem p = (l * bs + b) * groups + g: its rows start at row
// p * nq of the predictions as they lie, and cost is (L, bs, groups, gmax, nq).  The values are det_cost_kernel's.
// grid (ceil(nq / 256), gmax, L * bs * groups), 256 threads
__global__ void __launch_bounds__(256) det_cost_grouped_kernel(const DetCostArgs a, const int groups) {
  __shared__ double ngt[8];
  const int p = blockIdx.z;
  det_cost_problem(a, p, (p / groups) % a.bs, ngt);
}

}  // namespace bevmsda
