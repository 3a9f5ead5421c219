// Many weight images in one launch: lin_pack_weights_multi_kernel over the per-thread packers of linear_mfma.h and
// linear_panel.h.  The kernel is no template, so this header belongs to the one unit that launches it (bevmsda_linear.hip):
// a second including unit would define its host stub a second time.
#pragma once
#include "linear_panel.h"

namespace bevmsda {

// Many weight images in ONE launch (round 6): the training step re-packs the images of every trainable weight from the
// weights' current values — 52 launches of ~5 us each at base, now one.  `jobs` lives in DEVICE memory (a captured graph
// replays the launch with the table it was captured with); job j owns the blocks [first_block[j], first_block[j + 1]).
struct PackJob {
  const float *w;         // the weight matrix, or (kind & 1) the memory its transpose lies in
  long long ldw;
  unsigned short *blob;
  int N, K;
  int kind;               // bit 0: transposed source; bit 1: row-panel image (fragment order), else the first kernel's
  int first_block;
};

__global__ void __launch_bounds__(256) lin_pack_weights_multi_kernel(const PackJob *__restrict__ jobs, int njobs) {
  int lo = 0, hi = njobs - 1;                   // the job whose block range holds blockIdx.x (uniform: scalar loads)
  const int b = static_cast<int>(blockIdx.x);
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  const PackJob j = jobs[lo];
  const long t = static_cast<long>(b - j.first_block) * 256 + threadIdx.x;
  uint16_t *blob = reinterpret_cast<uint16_t *>(j.blob);
  switch (j.kind) {
    case 0: lin_pack_weight_thread<false>(t, j.w, j.ldw, j.N, j.K, blob); break;
    case 1: lin_pack_weight_thread<true>(t, j.w, j.ldw, j.N, j.K, blob); break;
    case 2: lin_panel_pack_weight_thread<false>(t, j.w, j.ldw, j.N, j.K, ((j.N + 63) / 64) * 2, blob); break;
    default: lin_panel_pack_weight_thread<true>(t, j.w, j.ldw, j.N, j.K, ((j.N + 63) / 64) * 2, blob); break;
  }
}

}  // namespace bevmsda
