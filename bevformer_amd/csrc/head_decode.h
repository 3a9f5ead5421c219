// NMSFreeCoder.decode_single (core/bbox/coders/nms_free_coder.py:40-100 of the reference) with denormalize_bbox
// (core/bbox/util.py:26-53) as one kernel, one workgroup per batch entry, fixed-shape outputs:
//
//   the max_num largest of the nq * C class logits (ranked on the LOGIT: sigmoid is monotone, so the selection does not
//   depend on expf rounding), ordered by logit descending, ties by the lower flat index q * C + c;
//   for rank r: scores[r] = sigmoid(logit), labels[r] = idx % C, boxes[r] = (cx, cy, cz, exp(w), exp(l), exp(h),
//   atan2(sin, cos)[, vx, vy]) of box row idx / C, keep[r] = centre inside post_center_range (both ends inclusive) and the
//   score test; count = number of kept ranks.
//
// Score test: the reference lowers its threshold by 0.9 until a score passes (:65-73).  The host passes that ladder
// (thr, 0.9 thr, ... while >= 0.01); scores are sorted, so "anything passes rung i" is a test of rank 0 alone: the first
// rung that rank 0 passes ('>' for rung 0, '>=' after it) is the threshold, and when no rung passes every score does.
// No ladder: no score test.
//
// Values: the sigmoid, the three exponentials and the angle are evaluated in fp64 and rounded to fp32: each stored value is
// within half an fp32 ulp of the exact one, up to the fp64 library's own error (and the rare double rounding).  An fp32
// evaluation of the same formula, the reference's included, is typically one or two ulp off, so a score that sits within an
// ulp of a threshold rung can pass here and fail there, or the reverse: keep[] follows THIS kernel's stored score.
// At most max_num <= 1,024 ranks per entry: the cost does not show beside the sort.
//
// Selection: a bitonic sort in LDS of 64-bit keys (order-preserving image of the logit << 32 | ~index): keys are unique,
// so the order is total and the result does not depend on the schedule.  N2 = the padded problem size (a power of two).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bevmsda {

constexpr int kDecodeMaxScores = 16384;
constexpr int kDecodeMaxNum = 1024;
constexpr int kDecodeMaxLadder = 64;

struct DecodeArgs {
  const float *cls;                 // (bs, nq, C) logits
  const float *box;                 // (bs, nq, code_size) box codes
  float ladder[kDecodeMaxLadder];   // thresholds, by value: no device table, nothing to keep alive for a captured graph
  int n_ladder;                     // 0: no score test
  int nq, C, code_size, max_num;
  float range[6];                   // post_center_range
  float *scores;                    // (bs, max_num)
  long long *labels;                // (bs, max_num)
  float *boxes;                     // (bs, max_num, code_size - 1)
  unsigned char *keep;              // (bs, max_num)
  int *count;                       // (bs)
};

__device__ __forceinline__ float decode_sigmoid(float logit) {
  return static_cast<float>(1.0 / (1.0 + exp(-static_cast<double>(logit))));
}

__device__ __forceinline__ float decode_exp(float x) { return static_cast<float>(exp(static_cast<double>(x))); }

template <int N2, int NTH>
__global__ void __launch_bounds__(NTH) nms_free_decode_kernel(const DecodeArgs a) {
  __shared__ unsigned long long key[N2];
  __shared__ int kept;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int n = a.nq * a.C;
  const float *cls = a.cls + static_cast<long>(b) * n;
  for (int i = tid; i < N2; i += NTH) {
    unsigned long long k = 0ull;                           // padding: below every real key
    if (i < n) {
      unsigned u = __float_as_uint(cls[i] + 0.0f);         // (-0 -> +0: equal logits, tie by index)
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // unsigned order = float order
      k = (static_cast<unsigned long long>(u) << 32) | static_cast<unsigned>(~static_cast<unsigned>(i));
    }
    key[i] = k;
  }
  if (tid == 0) kept = 0;
  __syncthreads();
  for (int k = 2; k <= N2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N2 / 2; t += NTH) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const unsigned long long x = key[i], y = key[l];
        const bool desc = (i & k) == 0;
        if ((x < y) == desc) {
          key[i] = y;
          key[l] = x;
        }
      }
      __syncthreads();
    }
  // rank 0's score picks the rung of the ladder
  float thr = 0.f;
  int mode = 0;                                            // 0 no test, 1 '>', 2 '>='
  if (a.n_ladder > 0) {
    const unsigned u0 = static_cast<unsigned>(key[0] >> 32);
    const float l0 = __uint_as_float((u0 & 0x80000000u) ? (u0 & 0x7fffffffu) : ~u0);
    const float s0 = decode_sigmoid(l0);
    for (int i = 0; i < a.n_ladder; ++i) {
      const float t = a.ladder[i];
      if (i == 0 ? s0 > t : s0 >= t) {
        thr = t;
        mode = i == 0 ? 1 : 2;
        break;
      }
    }
  }
  const int W = a.code_size - 1;
  for (int r = tid; r < a.max_num; r += NTH) {
    const unsigned long long kk = key[r];
    const unsigned u = static_cast<unsigned>(kk >> 32);
    const int idx = static_cast<int>(~static_cast<unsigned>(kk & 0xffffffffull));
    const float logit = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
    const float s = decode_sigmoid(logit);
    const int q = idx / a.C, c = idx - q * a.C;
    const float *br = a.box + (static_cast<long>(b) * a.nq + q) * a.code_size;
    const long o = static_cast<long>(b) * a.max_num + r;
    float *ob = a.boxes + o * W;
    const float cx = br[0], cy = br[1], cz = br[4];
    ob[0] = cx;
    ob[1] = cy;
    ob[2] = cz;
    ob[3] = decode_exp(br[2]);
    ob[4] = decode_exp(br[3]);
    ob[5] = decode_exp(br[5]);
    ob[6] = static_cast<float>(atan2(static_cast<double>(br[6]), static_cast<double>(br[7])));
    if (a.code_size > 8) {
      ob[7] = br[8];
      ob[8] = br[9];
    }
    bool ok = cx >= a.range[0] && cy >= a.range[1] && cz >= a.range[2] && cx <= a.range[3] && cy <= a.range[4] && cz <= a.range[5];
    if (mode == 1) ok = ok && s > thr;
    else if (mode == 2) ok = ok && s >= thr;
    a.scores[o] = s;
    a.labels[o] = c;
    a.keep[o] = ok ? 1 : 0;
    if (ok) atomicAdd(&kept, 1);
  }
  __syncthreads();
  if (tid == 0) a.count[b] = kept;
}

}  // namespace bevmsda
