// Host-side helpers the C ABI units (bevmsda_*.hip) share for their argument checks and launch epilogues: pointer
// alignment, the status of the last launch, the XCD-rounded grid of the 2-D tiled kernels.  No kernels, no state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/bevmsda.h"

template <unsigned N>
inline bool aligned_to(const void *p) {
  static_assert(N != 0 && (N & (N - 1)) == 0, "a power of two");
  return (reinterpret_cast<uintptr_t>(p) & (N - 1)) == 0;
}
// (a null pointer is aligned: optional arguments are checked without a guard)
inline bool misaligned(const void *p) { return !aligned_to<16>(p); }   // float4 / LDS-DMA rows
inline bool off8(const void *p) { return !aligned_to<8>(p); }
inline bool off4(const void *p) { return !aligned_to<4>(p); }

// what an entry point returns behind its launches
inline int launch_status() { return hipGetLastError() == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH; }

// 1-D grid over nbm x nbn tiles with the row tiles rounded up to the 8 XCDs (the kernels deal row tile 8 i + xcd to XCD
// `xcd` and drop the padding): BEVMSDA_ERR_TOO_LARGE when the grid or the kernels' 32-bit tile arithmetic would overflow
inline int xcd_grid(long long nbm, long long nbn, unsigned *grid) {
  const long long g = ((nbm + 7) / 8) * 8 * nbn;
  if (g >= (1LL << 31) || nbm >= (1LL << 28)) return BEVMSDA_ERR_TOO_LARGE;
  *grid = static_cast<unsigned>(g);
  return BEVMSDA_OK;
}
