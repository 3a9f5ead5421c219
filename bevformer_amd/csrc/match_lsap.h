// Batched rectangular linear sum assignment: P problems of n_p <= nq rows (ground-truth boxes) by nq columns (queries), one
// workgroup per problem, by shortest augmenting paths (Jonker-Volgenant as restated by Crouse, "On implementing 2D
// rectangular assignment algorithms", 2016 — the method scipy.optimize.linear_sum_assignment uses).  It replaces the host
// round trip of HungarianAssigner3D (core/bbox/assigners/hungarian_assigner_3d.py:117-127 of the reference).
//
// cost: fp32, problem p's row i at cost + p * gmax * nq + i * nq (the layout det_cost.h writes); n_p = count[p], read on the
// device and clamped to [0, min(gmax, nq)].  Outputs: match (P, gmax) the column of each row, -1 on padding; assigned
// (P, nq) the row of each column, -1 for none (background); status (P): 0 solved, 1 a non-finite cost in the problem's n_p
// rows (nothing is assigned; the module path's equivalent is scipy's ValueError), 2 the step bound ran out (cannot happen on
// finite costs; nothing is assigned).
//
// One augmentation per row.  Its scan keeps, per column, the shortest path cost `spc`, the predecessor row `path` and the
// visited flag in LDS, each column owned by one lane (column j by lane j mod 256); a step relaxes the unvisited columns
// from the current row, finds the minimum by a wavefront shuffle + four-entry LDS reduction, and either ends at an
// unassigned column or moves on to the row that owns the column.  Dual variables and spc are fp64; costs are widened.
// Ties: the smaller spc, then an unassigned column before an assigned one (as scipy), then the lower column: the result
// does not depend on the schedule.
//
// Every loop has a fixed trip bound: n_p augmentations, at most (assigned rows + 1) <= n_p steps each — a step visits one
// more column, and only the columns of assigned rows lead on — so G (G + 1) / 2 steps per problem at worst; the trace-back
// is bounded the same way.  Nothing waits on floating-point progress.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_cost.h"

namespace bevmsda {

constexpr int kLsapThreads = 256;

struct LsapArgs {
  const float *cost;
  const int *count;
  int *match;
  int *assigned;
  int *status;
  int gmax, nq;
};

__device__ __forceinline__ bool lsap_better(double av, int ak, double bv, int bk) { return av < bv || (av == bv && ak < bk); }

__global__ void __launch_bounds__(kLsapThreads) lsap_kernel(const LsapArgs a) {
  __shared__ double spc[kLossMaxQueries];
  __shared__ double v[kLossMaxQueries];
  __shared__ double u[kLossMaxGt];
  __shared__ int path[kLossMaxQueries];
  __shared__ int row4col[kLossMaxQueries];
  __shared__ int col4row[kLossMaxGt];
  __shared__ unsigned char visited[kLossMaxQueries];
  __shared__ double red_val[2][kLsapThreads / 64];
  __shared__ int red_key[2][kLsapThreads / 64];
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  const int nq = a.nq;
  int n = a.count[p];
  const int cap = a.gmax < nq ? a.gmax : nq;
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const float *cost = a.cost + static_cast<long>(p) * a.gmax * nq;
  int *match = a.match + static_cast<long>(p) * a.gmax;
  int *assigned = a.assigned + static_cast<long>(p) * nq;
  const double kInf = __longlong_as_double(0x7ff0000000000000LL);

  int bad = 0;
  for (int e = tid; e < n * nq; e += kLsapThreads) {
    const unsigned bits = __float_as_uint(cost[e]);
    bad |= (bits & 0x7f800000u) == 0x7f800000u;            // inf or NaN
  }
  bad = __syncthreads_or(bad);
  for (int j = tid; j < nq; j += kLsapThreads) {
    v[j] = 0.0;
    row4col[j] = -1;
  }
  for (int i = tid; i < n; i += kLsapThreads) {
    u[i] = 0.0;
    col4row[i] = -1;
  }
  __syncthreads();
  int status = bad ? 1 : 0;

  for (int cur = 0; cur < n && status == 0; ++cur) {
    for (int j = tid; j < nq; j += kLsapThreads) {
      spc[j] = kInf;
      visited[j] = 0;
    }
    int i = cur, sink = -1;
    double min_val = 0.0;
    for (int step = 0; step <= cur && sink < 0; ++step) {
      const float *row = cost + static_cast<long>(i) * nq;
      const double ui = u[i];
      double best = kInf;
      int key = 0x7fffffff;
      for (int j = tid; j < nq; j += kLsapThreads) {
        if (visited[j]) continue;
        const double r = min_val + static_cast<double>(row[j]) - ui - v[j];
        double s = spc[j];
        if (r < s) {
          s = r;
          spc[j] = r;
          path[j] = i;
        }
        const int k = (row4col[j] >= 0 ? 4096 : 0) | j;
        if (lsap_better(s, k, best, key)) {
          best = s;
          key = k;
        }
      }
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        const double ov = __shfl_xor(best, m);
        const int ok = __shfl_xor(key, m);
        if (lsap_better(ov, ok, best, key)) {
          best = ov;
          key = ok;
        }
      }
      const int buf = step & 1;
      if ((tid & 63) == 0) {
        red_val[buf][tid >> 6] = best;
        red_key[buf][tid >> 6] = key;
      }
      __syncthreads();
      best = red_val[buf][0];
      key = red_key[buf][0];
#pragma unroll
      for (int w = 1; w < kLsapThreads / 64; ++w)
        if (lsap_better(red_val[buf][w], red_key[buf][w], best, key)) {
          best = red_val[buf][w];
          key = red_key[buf][w];
        }
      if (key == 0x7fffffff) break;                        // no column left: cannot happen with n <= nq (status 2 below)
      const int j = key & 4095;
      min_val = best;
      if ((j & (kLsapThreads - 1)) == tid) visited[j] = 1;
      if (key & 4096) i = row4col[j];
      else sink = j;
    }
    if (sink < 0) {                                        // (uniform: every lane read the same reduction)
      status = 2;
      break;
    }
    // dual update: the rows visited besides `cur` are the owners of the visited columns
    for (int j = tid; j < nq; j += kLsapThreads)
      if (visited[j]) {
        const double d = min_val - spc[j];
        v[j] -= d;
        const int r = row4col[j];
        if (r >= 0) u[r] += d;
      }
    if (tid == 0) u[cur] += min_val;
    __syncthreads();
    if (tid == 0) {                                        // augment along the predecessor rows, at most cur + 1 links
      int j = sink;
      for (int t = 0; t <= cur; ++t) {
        const int r = path[j];
        row4col[j] = r;
        const int prev = col4row[r];
        col4row[r] = j;
        j = prev;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }

  const bool solved = status == 0;
  for (int i = tid; i < a.gmax; i += kLsapThreads) match[i] = (solved && i < n) ? col4row[i] : -1;
  for (int j = tid; j < nq; j += kLsapThreads) assigned[j] = solved ? row4col[j] : -1;
  if (tid == 0) a.status[p] = status;
}

}  // namespace bevmsda
