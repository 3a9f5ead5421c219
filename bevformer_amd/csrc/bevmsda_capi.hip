// C ABI of libbevmsda.so (declared in include/bevmsda.h): argument checks,
// kernel selection and launches.  No torch, no allocation, no global state.
#include <stdlib.h>

// This file is compiled TWICE (bevformer_amd/build.py): as itself — every entry point except the sampling backward — and through
// bevmsda_capi_backward.hip with BEVMSDA_PART_BACKWARD — the bevmsda_backward_* entry points only, without the SLP vectorizer
// (the reason is written there).
#ifdef BEVMSDA_PART_BACKWARD
#define BEVMSDA_FWD_PART 0
#else
#define BEVMSDA_FWD_PART 1
#endif

#include "capi_checks.h"
#include "msda_kernels.h"
#include "msda_d32.h"
#include "msda_bwd_lds.h"
#include "msda_bwd_gather.h"
#if BEVMSDA_FWD_PART
#include "rowops.h"
#include "prologue.h"
#endif

namespace {

using bevmsda::KArgs;
using bevmsda::bf16_t;

// library defaults (chosen from the sweeps recorded in DESIGN.md)
#ifndef BEVMSDA_QTILE_FWD
#define BEVMSDA_QTILE_FWD 8          // A/B builds: rows of one head in adjacent lane groups (a power of two; 8 = one wavefront)
#endif
constexpr int kDefaultQtileFwd = BEVMSDA_QTILE_FWD;
constexpr int kDefaultQtileBwd = 8;
constexpr long kDynGridBlocks = 2048;        // grid of the device-row-count sampling launches (multiple of 8)
                                             // (128 rows with 320 + 128 pixels, two workgroups per CU: 320 us vs 270 us)

int check_common(const void *value, const int64_t *shapes, const int64_t *lstart, const float *loc,
                 const float *attn, int N, int S, int M, int D, int L, int Q, int P) {
  if (N < 0 || S < 0 || M < 0 || D < 0 || L < 0 || Q < 0 || P < 0) return BEVMSDA_ERR_BAD_SHAPE;
  const long long rows = 1LL * N * Q * M;
  if (rows == 0 || D == 0) return 1;  // nothing to compute
  if (L > 0 && P > 0) {
    if (!shapes || !lstart || !loc || !attn) return BEVMSDA_ERR_NULL_POINTER;
    if (S > 0 && !value) return BEVMSDA_ERR_NULL_POINTER;
    if (misaligned(value) || misaligned(loc) || misaligned(attn)) return BEVMSDA_ERR_MISALIGNED;
  }
  if (1LL * S * M * D >= (1LL << 31) || 1LL * L * P * 2 >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  return BEVMSDA_OK;
}

int ilog2_exact(long v) {
  if (v <= 0 || (v & (v - 1)) != 0) return -1;
  int s = 0;
  while ((1L << s) < v) ++s;
  return s;
}

// D = 32 forward through the buffer-descriptor kernel (msda_d32.h): needs P in {4, 8}
// and the whole value tensor addressable with a 31-bit byte offset.
template <typename T>
bool d32_fwd_eligible(const KArgs &a) {
  const unsigned long long bytes = 1ULL * a.N * a.S * a.M * a.D * sizeof(T);
  return a.D == 32 && a.L >= 1 && (a.P == 4 || a.P == 8) && bytes < (1ULL << 31);
}

int resolve_qtile(const bevmsda_tuning *t, int dflt, long NQ) {
  int q = (t && t->qtile > 0) ? t->qtile : dflt;
  if (q < 1 || q > 1024) return -1;
  (void)NQ;
  return q;
}

template <typename T, int CPL, int LPG, bool BWD>
int launch_grouped(const KArgs &base, hipStream_t stream) {
  KArgs a = base;
  constexpr int GPB = 256 / LPG;
  const long tiles = (a.NQ + a.qtile - 1) / a.qtile;
  const long groups = tiles * a.qtile * a.M;
  const long nb = (groups + GPB - 1) / GPB;
  if (nb >= (1LL << 31) - 8) return BEVMSDA_ERR_TOO_LARGE;
  a.nblocks = static_cast<int>(nb);
  const unsigned grid = a.xcd_remap ? static_cast<unsigned>(((nb + 7) / 8) * 8) : static_cast<unsigned>(nb);
  if constexpr (BWD) {            // (if constexpr: each of the two translation units instantiates only its own kernels)
  if (a.D == 32 && a.variant != 1) {
    KArgs b = a;
    const long g8 = tiles * a.qtile * a.M;
    const long nb8 = (g8 + 31) / 32;
    b.nblocks = static_cast<int>(nb8);
    const unsigned grid8 = b.xcd_remap ? static_cast<unsigned>(((nb8 + 7) / 8) * 8) : static_cast<unsigned>(nb8);
    // grad_value through LDS tiles (msda_bwd_lds.h) unless variant 3 asks for the first-generation kernel
    // (one memory-side atomic per tap) or the shape does not fit the tiled kernel
    // point groups of the sort key (points p with equal p % G get their own bucket range): SpatialCrossAttention's points
    // cycle through 4 pillar anchors at different heights — disjoint footprints per anchor, G = 4; a single-level call
    // (TemporalSelfAttention: all points around ONE reference point, offsets of a few pixels) has overlapping footprints,
    // and keying them apart flushes every shared pixel once per point: G = 1 there (round 4: 1,166 -> ~680 flushes per
    // (tile, head, queue entry) by tools/flush_sim.py's count; measured below)
#ifndef BEVMSDA_GV_GROUPS_MULTI
#define BEVMSDA_GV_GROUPS_MULTI 4
#endif
#ifndef BEVMSDA_GV_GROUPS_SINGLE
#define BEVMSDA_GV_GROUPS_SINGLE 1
#endif
    int G = a.P % 4 == 0 ? 4 : (a.P % 2 == 0 ? 2 : 1);
    const int gcap = a.L == 1 ? BEVMSDA_GV_GROUPS_SINGLE : BEVMSDA_GV_GROUPS_MULTI;
    if (G > gcap) G = gcap;
    // (entries carry the pixel index of a level in 23 bits and the row of the block in 8)
    // 128 rows / 512 threads per workgroup (two per CU: one sorts while the other's flushes drain) — measured on the padded base
    // SCA call, image-ordered rows, against 256 rows / 1,024 threads (one per CU): 1.13 vs 1.27 ms in round 2, 0.97 vs 1.01 ms
    // on round 6's walk (64 rows: 1.15).  Dense single-level calls (TemporalSelfAttention) take grid tiles of that many rows
    // instead of consecutive rows (until round 6 only the 256-row shape had tiles: 0.42 ms against 0.90 ms for 128 CONSECUTIVE
    // rows; with 16 x 8 tiles the two-per-CU shape is ahead there too).  tuning->reserved[0] = 64 / 128 / 256 forces one.
    const int gv_forced = a.gv_rows;           // bevmsda_tuning.reserved[0]
#ifndef BEVMSDA_GV_ROWS_MULTI
#define BEVMSDA_GV_ROWS_MULTI 128
#endif
    // (single-level dense calls — TemporalSelfAttention's grid in 16 x (rows / 16) tiles: 16 x 8 tiles on two workgroups per CU
    // measured 267 vs 273-278 us for sort + gather at base, profiles/r6/r6q_gv_rows_tsa_tiles_ab.txt)
#ifndef BEVMSDA_GV_ROWS_SINGLE
#define BEVMSDA_GV_ROWS_SINGLE 128
#endif
    const int gv_rows = gv_forced == 64 || gv_forced == 128 || gv_forced == 256 ? gv_forced : (a.L > 1 ? BEVMSDA_GV_ROWS_MULTI : BEVMSDA_GV_ROWS_SINGLE);
    const int gv_threads = gv_rows == 64 ? 256 : (gv_rows == 128 ? 512 : bevmsda::kGvThreads);
    const int rpt = (gv_rows * a.P + gv_threads - 1) / gv_threads;
    bool tiled = a.variant != 3 && a.L >= 1 && a.L <= bevmsda::kGvMaxLevels && a.P >= 1 && (rpt == 1 || rpt == 2);   // P <= 8: 112 KB of LDS
    tiled = tiled && 1LL * a.S < (1LL << 23) && a.NQ < (1LL << 30) && 1LL * a.N * (1LL * a.Q * 3 / 512 + 4) * 256 < (1LL << 30);
    if ((a.nrows_dev || a.gout_rows > 0 || a.gv_stride > 0) && !(tiled && d32_fwd_eligible<T>(a))) return BEVMSDA_ERR_UNSUPPORTED;   // (no first-generation kernel reads the device count / shares grad_out rows)
    if (tiled) {
      bevmsda::GradValueArgs s{};
      s.k = a;
      s.rows_per_block = gv_rows;
      s.gbits = G == 4 ? 2 : (G == 2 ? 1 : 0);
      long chunks = (a.NQ + s.rows_per_block - 1) / s.rows_per_block;
      if (!a.row_batch && a.L == 1 && a.Q >= 1024) {
        // dense single-level call: room for the 16 x (rows / 16) tiles of a roughly square grid (msda_bwd_lds.h)
        s.dense_tiles = static_cast<int>(1LL * a.Q * 3 / (s.rows_per_block * 2) + 4 * (256 / s.rows_per_block));
        chunks = 1L * a.N * s.dense_tiles;
      }
      if (chunks * a.M >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
      const size_t lds_bytes = bevmsda::gv_lds_bytes(gv_threads, s.rows_per_block, a.P);
      const dim3 ggrid(static_cast<unsigned>(chunks * a.M)), gblock(gv_threads);
      // tuning->reserved[1..2] = device address of 8 uint64 (low, high word): phase clocks of the sort kernel (tools/gvprof.py)
      unsigned long long *const pe = a.gv_prof;
      if (pe) s.prof = pe;
#define BEVMSDA_GV(RPT_)                                                                                                \
  do {                                                                                                                  \
    if (pe) {                                                                                                           \
      auto kern = bevmsda::msda_gradvalue_sort_kernel<T, RPT_, true>;                                                   \
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,         \
                              static_cast<int>(lds_bytes)) != hipSuccess) return BEVMSDA_ERR_LAUNCH;                    \
      hipLaunchKernelGGL(kern, ggrid, gblock, lds_bytes, stream, s);                                                    \
    } else {                                                                                                            \
      auto kern = bevmsda::msda_gradvalue_sort_kernel<T, RPT_, false>;                                                  \
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,         \
                              static_cast<int>(lds_bytes)) != hipSuccess) return BEVMSDA_ERR_LAUNCH;                    \
      hipLaunchKernelGGL(kern, ggrid, gblock, lds_bytes, stream, s);                                                    \
    }                                                                                                                   \
  } while (0)
      if (gv_threads == 256) {
        auto k1 = bevmsda::msda_gradvalue_sort_kernel<T, 1, false, 256>;
        auto k2 = bevmsda::msda_gradvalue_sort_kernel<T, 2, false, 256>;
        auto kern = rpt == 1 ? k1 : k2;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds_bytes)) != hipSuccess) return BEVMSDA_ERR_LAUNCH;
        hipLaunchKernelGGL(kern, ggrid, gblock, lds_bytes, stream, s);
      } else if (gv_threads == 512) {
        auto k1 = bevmsda::msda_gradvalue_sort_kernel<T, 1, false, 512>;
        auto k2 = bevmsda::msda_gradvalue_sort_kernel<T, 2, false, 512>;
        auto k2p = bevmsda::msda_gradvalue_sort_kernel<T, 2, true, 512>;       // phase clocks (tools/gvprof.py)
        auto kern = rpt == 1 ? k1 : (pe ? k2p : k2);
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds_bytes)) != hipSuccess) return BEVMSDA_ERR_LAUNCH;
        hipLaunchKernelGGL(kern, ggrid, gblock, lds_bytes, stream, s);
      } else if (rpt == 1) BEVMSDA_GV(1);
      else BEVMSDA_GV(2);
#undef BEVMSDA_GV
      // grad_loc / grad_attn: the forward-style gather kernel (buffer loads: value < 2 GiB, P in {4, 8}),
      // else the first-generation kernel without its scatter
      if (d32_fwd_eligible<T>(a)) {
        // (P = 8 in fp32 needs 140 VGPRs for two batches of 16 taps in flight: 3 waves / SIMD)
        // bf16 storage: the 16-byte-lane form (2 requests per point); tuning->reserved[3] = 1 keeps the 8-byte-lane one
        const bool lanes8 = a.bf16_lanes8 != 0;
        if (sizeof(T) == 2 && !lanes8 && !misaligned(a.grad_out)) {
          if (a.P == 8) hipLaunchKernelGGL((bevmsda::msda_gradloc_d32_bf16x8_kernel<8, 4>), dim3(grid8), dim3(256), 0, stream, b);
          else hipLaunchKernelGGL((bevmsda::msda_gradloc_d32_bf16x8_kernel<4, 4>), dim3(grid8), dim3(256), 0, stream, b);
        } else if (a.P == 8) hipLaunchKernelGGL((bevmsda::msda_gradloc_d32_kernel<T, 8, sizeof(T) == 4 ? 3 : 4>), dim3(grid8), dim3(256), 0, stream, b);
        else hipLaunchKernelGGL((bevmsda::msda_gradloc_d32_kernel<T, 4, 4>), dim3(grid8), dim3(256), 0, stream, b);
      } else {
        switch (a.P) {
          case 4: hipLaunchKernelGGL((bevmsda::msda_bwd_d32_kernel<T, 4, false>), dim3(grid8), dim3(256), 0, stream, b); break;
          case 8: hipLaunchKernelGGL((bevmsda::msda_bwd_d32_kernel<T, 8, false>), dim3(grid8), dim3(256), 0, stream, b); break;
          default: hipLaunchKernelGGL((bevmsda::msda_bwd_d32_kernel<T, 0, false>), dim3(grid8), dim3(256), 0, stream, b); break;
        }
      }
    } else {
      // D = 32, first generation: line-shaped atomics (8 rows per wave in float4 lane groups)
      switch (a.P) {
        case 4: hipLaunchKernelGGL((bevmsda::msda_bwd_d32_kernel<T, 4>), dim3(grid8), dim3(256), 0, stream, b); break;
        case 8: hipLaunchKernelGGL((bevmsda::msda_bwd_d32_kernel<T, 8>), dim3(grid8), dim3(256), 0, stream, b); break;
        default: hipLaunchKernelGGL((bevmsda::msda_bwd_d32_kernel<T, 0>), dim3(grid8), dim3(256), 0, stream, b); break;
      }
    }
  } else {
    switch (a.P) {
      case 4: hipLaunchKernelGGL((bevmsda::msda_bwd_kernel<T, CPL, LPG, 4>), dim3(grid), dim3(256), 0, stream, a); break;
      case 8: hipLaunchKernelGGL((bevmsda::msda_bwd_kernel<T, CPL, LPG, 8>), dim3(grid), dim3(256), 0, stream, a); break;
      default: hipLaunchKernelGGL((bevmsda::msda_bwd_kernel<T, CPL, LPG, 0>), dim3(grid), dim3(256), 0, stream, a); break;
    }
  }
  } else {
  if (a.variant != 1 && d32_fwd_eligible<T>(a)) {
    // variant 0 / 3: registers for 4 waves per SIMD; 4: 8 waves; 5: 2 waves (msda_d32.h)
    const int wpe = a.variant == 4 ? 8 : (a.variant == 5 ? 2 : 4);
    KArgs b = a;
    const long nb8 = (tiles * a.qtile * a.M + 31) / 32;
    b.nblocks = static_cast<int>(nb8);
    const dim3 g8(b.xcd_remap ? static_cast<unsigned>(((nb8 + 7) / 8) * 8) : static_cast<unsigned>(nb8));
#define BEVMSDA_D32(PT_, W_) \
  hipLaunchKernelGGL((bevmsda::msda_fwd_d32_kernel<T, PT_, W_>), g8, dim3(256), 0, stream, b)
    if (a.P == 8) {
      if (wpe == 8) BEVMSDA_D32(8, 8);
      else if (wpe == 2) BEVMSDA_D32(8, 2);
      else BEVMSDA_D32(8, 4);
    } else {
      if (wpe == 8) BEVMSDA_D32(4, 8);
      else if (wpe == 2) BEVMSDA_D32(4, 2);
      else BEVMSDA_D32(4, 4);
    }
#undef BEVMSDA_D32
  } else {
    switch (a.P) {
      case 4: hipLaunchKernelGGL((bevmsda::msda_fwd_kernel<T, CPL, LPG, 4>), dim3(grid), dim3(256), 0, stream, a); break;
      case 8: hipLaunchKernelGGL((bevmsda::msda_fwd_kernel<T, CPL, LPG, 8>), dim3(grid), dim3(256), 0, stream, a); break;
      default: hipLaunchKernelGGL((bevmsda::msda_fwd_kernel<T, CPL, LPG, 0>), dim3(grid), dim3(256), 0, stream, a); break;
    }
  }
  }
  return launch_status();
}

template <typename T, bool BWD>
int launch_scalar(const KArgs &a, hipStream_t stream) {
  const long long total = 1LL * a.NQ * a.M * a.D;
  const long long nb = (total + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  if constexpr (BWD) {
    const size_t npts = static_cast<size_t>(a.NQ) * a.M * a.L * a.P;
    if (hipMemsetAsync(a.grad_attn, 0, npts * sizeof(float), stream) != hipSuccess) return BEVMSDA_ERR_LAUNCH;
    if (hipMemsetAsync(a.grad_loc, 0, npts * 2 * sizeof(float), stream) != hipSuccess) return BEVMSDA_ERR_LAUNCH;
    hipLaunchKernelGGL((bevmsda::msda_bwd_scalar_kernel<T>), dim3(static_cast<unsigned>(nb)), dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL((bevmsda::msda_fwd_scalar_kernel<T>), dim3(static_cast<unsigned>(nb)), dim3(256), 0, stream, a);
  }
  return launch_status();
}

// CPL = channels per lane for the 16-byte path of element type T
template <typename T> struct Wide;
template <> struct Wide<float> { static constexpr int cpl = 4; };
template <> struct Wide<bf16_t> { static constexpr int cpl = 8; };

template <typename T, bool BWD>
int dispatch(const KArgs &a, int variant, hipStream_t stream) {
  constexpr int CPL = Wide<T>::cpl;
  const int D = a.D;
  if (variant == 2 || D % CPL != 0) return launch_scalar<T, BWD>(a, stream);
  switch (D / CPL) {
    case 1: return launch_grouped<T, CPL, 1, BWD>(a, stream);
    case 2: return launch_grouped<T, CPL, 2, BWD>(a, stream);
    case 4: return launch_grouped<T, CPL, 4, BWD>(a, stream);
    case 8: return launch_grouped<T, CPL, 8, BWD>(a, stream);
    case 16: return launch_grouped<T, CPL, 16, BWD>(a, stream);
    case 32: return launch_grouped<T, CPL, 32, BWD>(a, stream);
    case 64: return launch_grouped<T, CPL, 64, BWD>(a, stream);
    default: return launch_scalar<T, BWD>(a, stream);
  }
}

template <typename T>
int forward_impl(const T *value, const int64_t *shapes, const int64_t *lstart, const float *loc,
                 const float *attn, int N, int S, int M, int D, int L, int Q, int P, T *out,
                 void *stream, const bevmsda_tuning *tuning, const int32_t *row_batch = nullptr,
                 int R = -1) {
  // ragged mode: R rows in total, row r samples value[row_batch[r]]; expressed
  // to the kernels as one batch of Q = R queries plus the row->batch table
  const int Nv = N;
  if (R >= 0) {
    if (R > 0 && !row_batch) return BEVMSDA_ERR_NULL_POINTER;
    N = 1;
    Q = R;
  }
  const int rc = check_common(value, shapes, lstart, loc, attn, N, S, M, D, L, Q, P);
  if (rc < 0) return rc;
  if (rc == 1) return BEVMSDA_OK;
  if (!out) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(out)) return BEVMSDA_ERR_MISALIGNED;
  KArgs a{};
  a.value = value; a.shapes = shapes; a.lstart = lstart; a.loc = loc; a.attn = attn; a.out = out;
  a.row_batch = (R >= 0) ? row_batch : nullptr;
  a.NQ = 1L * N * Q; a.N = Nv; a.S = S; a.M = M; a.D = D; a.L = L; a.Q = Q; a.P = P;
  a.qtile = resolve_qtile(tuning, kDefaultQtileFwd, a.NQ);
  if (a.qtile < 0) return BEVMSDA_ERR_BAD_OPTION;
  const int xr = tuning ? tuning->xcd_remap : 0;
  if (xr < 0 || xr > 2) return BEVMSDA_ERR_BAD_OPTION;
  a.xcd_remap = (xr == 1) ? 0 : 1;
  const int variant = tuning ? tuning->variant : 0;
  if (variant < 0 || variant > 5) return BEVMSDA_ERR_BAD_OPTION;
  a.variant = variant;
  a.mshift = ilog2_exact(M);
  a.qshift = ilog2_exact(a.qtile);
  return dispatch<T, false>(a, variant, static_cast<hipStream_t>(stream));
}

template <typename T>
int backward_impl(const T *value, const int64_t *shapes, const int64_t *lstart, const float *loc,
                  const float *attn, const T *grad_out, int N, int S, int M, int D, int L, int Q,
                  int P, float *grad_value, float *grad_loc, float *grad_attn, void *stream,
                  const bevmsda_tuning *tuning, const int32_t *row_batch = nullptr, int R = -1,
                  const int32_t *nrows_dev = nullptr, long gout_rows = 0, float gout_scale = 1.f, long gv_stride = 0,
                  const bevmsda_loc_source *ls = nullptr) {
  const int Nv = N;
  if (ls) {          // locations recomputed from the fused forward's operands: the rows form of the second-generation kernels only
    if (!ls->offs || !ls->ref) return BEVMSDA_ERR_NULL_POINTER;
    if (loc || !nrows_dev || R < 0) return BEVMSDA_ERR_UNSUPPORTED;
    if (ls->A < 1 || ls->proj_row < 0 || ls->off_head < 0 || ls->proj_row % 2 != 0 || ls->off_head % 2 != 0) return BEVMSDA_ERR_BAD_SHAPE;
    if (off8(ls->offs) || off8(ls->ref)) return BEVMSDA_ERR_MISALIGNED;
    loc = ls->offs;   // (for the operand checks below; the kernels get KArgs::loc = nullptr)
  }
  if (R >= 0) {
    if (R > 0 && !row_batch) return BEVMSDA_ERR_NULL_POINTER;
    N = 1;
    Q = R;
  }
  const int rc = check_common(value, shapes, lstart, loc, attn, N, S, M, D, L, Q, P);
  if (rc < 0) return rc;
  if (rc == 1 || L == 0 || P == 0) return BEVMSDA_OK;
  if (!grad_out || !grad_loc || !grad_attn || (S > 0 && !grad_value)) return BEVMSDA_ERR_NULL_POINTER;
  // device-side row count: only the second-generation D = 32 kernels read it
  if (nrows_dev && (R < 0 || D != 32 || !(P == 4 || P == 8) || L > bevmsda::kGvMaxLevels || tuning)) return BEVMSDA_ERR_UNSUPPORTED;
  if (misaligned(grad_out) || misaligned(grad_value) || misaligned(grad_loc) || misaligned(grad_attn))
    return BEVMSDA_ERR_MISALIGNED;
  KArgs a{};
  a.value = value; a.shapes = shapes; a.lstart = lstart; a.loc = loc; a.attn = attn;
  if (ls) {
    a.loc = nullptr;
    a.loc_offs = ls->offs; a.loc_ref = ls->ref; a.loc_row_src = ls->row_src;
    a.loc_proj_row = static_cast<long>(ls->proj_row); a.loc_off_head = ls->off_head; a.loc_A = ls->A;
  }
  a.grad_out = grad_out; a.grad_value = grad_value; a.grad_loc = grad_loc; a.grad_attn = grad_attn;
  a.row_batch = (R >= 0) ? row_batch : nullptr;
  a.NQ = 1L * N * Q; a.N = Nv; a.S = S; a.M = M; a.D = D; a.L = L; a.Q = Q; a.P = P;
  a.qtile = resolve_qtile(tuning, kDefaultQtileBwd, a.NQ);
  if (a.qtile < 0) return BEVMSDA_ERR_BAD_OPTION;
  const int xr = tuning ? tuning->xcd_remap : 0;
  if (xr < 0 || xr > 2) return BEVMSDA_ERR_BAD_OPTION;
  a.xcd_remap = (xr == 1) ? 0 : 1;
  int variant = tuning ? tuning->variant : 0;
  if (variant < 0 || variant > 5) return BEVMSDA_ERR_BAD_OPTION;
  if (variant > 3) variant = 0;  // 4, 5 select forward kernels only; 3 = first-generation D = 32 backward
  a.variant = variant;
  a.gv_rows = tuning ? tuning->reserved[0] : 0;
  a.gv_prof = tuning ? reinterpret_cast<unsigned long long *>((static_cast<unsigned long long>(static_cast<uint32_t>(tuning->reserved[2])) << 32) |
                                                              static_cast<uint32_t>(tuning->reserved[1]))
                     : nullptr;
  a.bf16_lanes8 = tuning ? tuning->reserved[3] : 0;
  a.nrows_dev = nrows_dev;
  // shared grad_out rows (second-generation D = 32 kernels only)
  if (gout_rows < 0 || (gout_rows > 0 && (D != 32 || !(P == 4 || P == 8) || L > bevmsda::kGvMaxLevels || tuning))) return BEVMSDA_ERR_UNSUPPORTED;
  a.gout_rows = gout_rows; a.gout_scale = gout_scale;
  // grad_value rows of a wider array: the sort kernel of the second generation only
  if (gv_stride < 0 || (gv_stride > 0 && (gv_stride < 1L * M * D || gv_stride % 4 != 0 || D != 32 || !(P == 4 || P == 8) || L > bevmsda::kGvMaxLevels || tuning)))
    return gv_stride < 0 ? BEVMSDA_ERR_BAD_SHAPE : BEVMSDA_ERR_UNSUPPORTED;
  a.gv_stride = gv_stride;
  a.mshift = ilog2_exact(M);
  a.qshift = ilog2_exact(a.qtile);
  return dispatch<T, true>(a, variant, static_cast<hipStream_t>(stream));
}

template <typename T>
int fused_impl(const T *value, const int64_t *shapes, const int64_t *lstart, const float *offs,
               const float *logits, const float *ref, const int32_t *row_batch, const int32_t *row_src,
               const bevmsda_fused_desc *d, T *out, void *stream, const int32_t *nrows = nullptr,
               float *save_loc = nullptr, float *save_attn = nullptr, const int32_t *need = nullptr, int need_shift = 0,
               int64_t need_len = 0, int32_t *halo_flag = nullptr) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->R < 0 || d->N < 0 || d->S < 0 || d->M <= 0 || d->L < 0 || d->P < 0 || d->Q < 0 || d->K < 0 ||
      d->A <= 0)
    return BEVMSDA_ERR_BAD_SHAPE;
  const unsigned long long bytes = 1ULL * d->N * d->S * d->M * d->D * sizeof(T);
  if (d->D != 32 || !(d->P == 4 || d->P == 8) || d->L < 1 || d->L > 4 || d->P * d->K > 8 || !(d->K == 1 || d->K == 2) ||
      bytes >= (1ULL << 31) || (d->proj_row & 1) || (d->off_head & 1) || (d->off_k & 1) ||
      (d->ref_mode != 0 && d->ref_mode != 1) || (d->ref_mode == 1 && d->A != d->L))
    return BEVMSDA_ERR_UNSUPPORTED;
  if (d->R == 0) return BEVMSDA_OK;
  if (!value || !shapes || !lstart || !offs || !logits || !ref || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (!row_batch && d->Q <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(value) || misaligned(out) || off8(offs) || off8(ref) || off4(logits))
    return BEVMSDA_ERR_MISALIGNED;
  if (d->R * static_cast<long long>(d->M) >= (1LL << 36)) return BEVMSDA_ERR_TOO_LARGE;
  // desc->reserved is validated HERE, for every entry point and before anything is launched: a retired value (include/bevmsda.h)
  // must not be accepted and silently ignored — an A/B run would then report the knob as set and measure the default.
  // [5]: 0 = the default bodies (TemporalSelfAttention's fp32 shape on the one with compile-time head / level counts, msda_d32.h
  // LC / MC: 70 vs 72.4 us), 1 = the generic bodies only (tools/fwd_knob_ab.sh); [3]: the row-count hint of the device-side row count
  if (d->reserved[5] != 0 && d->reserved[5] != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->reserved[0] != 0 || d->reserved[4] != 0) return BEVMSDA_ERR_BAD_OPTION;
  if (!nrows && d->reserved[3] != 0) return BEVMSDA_ERR_BAD_OPTION;
  bevmsda::FusedArgs f{};
  KArgs &a = f.k;
  a.value = value; a.shapes = shapes; a.lstart = lstart; a.out = out; a.row_batch = row_batch;
  a.NQ = d->R; a.N = d->N; a.S = d->S; a.M = d->M; a.D = d->D; a.L = d->L; a.Q = d->Q > 0 ? d->Q : 1; a.P = d->P;
  a.qtile = kDefaultQtileFwd; a.xcd_remap = 1;
  a.mshift = ilog2_exact(a.M); a.qshift = ilog2_exact(a.qtile);
  // SAVE kernels (training forward): SCA's shape only — device-side row count, one queue entry, 8 points, several levels
  const bool save = save_loc != nullptr || save_attn != nullptr;
  if (save && !save_attn) return BEVMSDA_ERR_NULL_POINTER;      // (save_loc may be null: the backward recomputes the locations)
  if (save && (!nrows || d->K != 1 || d->P != 8 || d->L < 2)) return BEVMSDA_ERR_UNSUPPORTED;
  if (save && ((save_loc && misaligned(save_loc)) || misaligned(save_attn))) return BEVMSDA_ERR_MISALIGNED;
  f.save_loc = save_loc; f.save_attn = save_attn;
  f.offs = offs; f.logits = logits; f.ref = ref; f.row_src = row_src; f.proj_row = d->proj_row;
  f.off_head = d->off_head; f.off_k = d->off_k; f.lg_head = d->lg_head; f.lg_k = d->lg_k;
  f.K = d->K; f.A = d->A; f.ref_mode = d->ref_mode; f.vmul = d->vmul; f.vadd = d->vadd;
  f.out_scale = 1.0f / static_cast<float>(d->K);
  f.out_f32 = 0;
  if constexpr (sizeof(T) == 2) {
    // desc->reserved[2] = 1: `out` is an fp32 (R, M*D) matrix (16-byte-lane bf16 kernel only)
    if (d->reserved[2] != 0 && d->reserved[1] != 0) return BEVMSDA_ERR_BAD_OPTION;
    f.out_f32 = d->reserved[2] ? 1 : 0;
  }
  const long tiles = (a.NQ + a.qtile - 1) / a.qtile;
  const long nb = (tiles * a.qtile * a.M + 31) / 32;
  if (nb >= (1LL << 31) - 8) return BEVMSDA_ERR_TOO_LARGE;
  a.nblocks = static_cast<int>(nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nrows) {
    // device-side row count (frame_plan.h): d->R is the capacity of the row arrays, desc->reserved[3] the
    // caller's hint of the count (0: none).  Head launch: one workgroup per logical block of the hint;
    // tail launch: a small grid striding over rows beyond the hint (msda_d32.h, DynRows).
    if (d->R >= (1LL << 27)) return BEVMSDA_ERR_TOO_LARGE;
    f.nrows = nrows;
    long long hint = d->reserved[3];
    if (hint < 0) return BEVMSDA_ERR_BAD_OPTION;
    if (hint > d->R) hint = d->R;
    f.launch_rows = static_cast<int>(hint);
    const long htiles = (hint + a.qtile - 1) / a.qtile;
    const long hnb = (htiles * a.qtile * a.M + 31) / 32;
    const dim3 hgrid(static_cast<unsigned>(((hnb + 7) / 8) * 8));
    const long rest = ((nb - hnb + 7) / 8) * 8;
    const dim3 tgrid(static_cast<unsigned>(rest < 8 ? 8 : (rest < kDynGridBlocks ? rest : kDynGridBlocks)));
#define BEVMSDA_DYN(HEAD_, TAIL_)                                                                          \
  do {                                                                                                     \
    if (hint > 0) hipLaunchKernelGGL(HEAD_, hgrid, dim3(256), 0, st, f);                                   \
    if (hint < d->R) hipLaunchKernelGGL(TAIL_, tgrid, dim3(256), 0, st, f);                                \
  } while (0)
    if constexpr (sizeof(T) == 2) {
      if (d->reserved[1] != 0) return BEVMSDA_ERR_BAD_OPTION;
      if (d->P == 8 && save) BEVMSDA_DYN((bevmsda::msda_fused_d32_bf16x8_head_kernel<8, 1, 4, true>), (bevmsda::msda_fused_d32_bf16x8_dyn_kernel<8, 1, 4, true>));
      else if (d->P == 8) BEVMSDA_DYN((bevmsda::msda_fused_d32_bf16x8_head_kernel<8, 1, 4>), (bevmsda::msda_fused_d32_bf16x8_dyn_kernel<8, 1, 4>));
      else if (d->K == 2) BEVMSDA_DYN((bevmsda::msda_fused_d32_bf16x8_head_kernel<4, 2, 4>), (bevmsda::msda_fused_d32_bf16x8_dyn_kernel<4, 2, 4>));
      else BEVMSDA_DYN((bevmsda::msda_fused_d32_bf16x8_head_kernel<4, 1, 4>), (bevmsda::msda_fused_d32_bf16x8_dyn_kernel<4, 1, 4>));
    } else {
      // (the generic bodies for either value of desc->reserved[5]: SpatialCrossAttention's shape with compile-time head / level
      // counts ran at the generic body's speed, 239-241 us — the kernel is bound by the L1 / TA path, not by instruction issue)
      if (d->P == 8) {
        if (d->L > 1 && save) BEVMSDA_DYN((bevmsda::msda_fused_d32_head_kernel<T, 8, 1, 4, true>), (bevmsda::msda_fused_d32_dyn_kernel<T, 8, 1, 4, true>));
        else if (d->L > 1) BEVMSDA_DYN((bevmsda::msda_fused_d32_head_kernel<T, 8, 1, 4>), (bevmsda::msda_fused_d32_dyn_kernel<T, 8, 1, 4>));
        else BEVMSDA_DYN((bevmsda::msda_fused_d32_head_kernel<T, 8, 1, 8>), (bevmsda::msda_fused_d32_dyn_kernel<T, 8, 1, 8>));
      } else if (d->K == 2) {
        BEVMSDA_DYN((bevmsda::msda_fused_d32_head_kernel<T, 4, 2, 8>), (bevmsda::msda_fused_d32_dyn_kernel<T, 4, 2, 8>));
      } else {
        BEVMSDA_DYN((bevmsda::msda_fused_d32_head_kernel<T, 4, 1, 8>), (bevmsda::msda_fused_d32_dyn_kernel<T, 4, 1, 8>));
      }
    }
#undef BEVMSDA_DYN
    return launch_status();
  }
  const dim3 grid(static_cast<unsigned>(((nb + 7) / 8) * 8));
  if (need) {
    // out-of-band check (bevmsda_fused_forward_halo_f32; msda_d32.h HALO): the two-entry fp32 shape on the body with
    // compile-time counts (8 heads, one level) or on the generic one (also desc->reserved[5] = 1)
    if constexpr (sizeof(T) == 4) {
      if (d->K != 2 || d->P != 4) return BEVMSDA_ERR_UNSUPPORTED;
      if (need_shift < 0 || need_shift > 30 || need_len <= 0 || ((static_cast<int64_t>(d->S) - 1) >> need_shift) >= need_len)
        return BEVMSDA_ERR_BAD_SHAPE;                       // (the table covers every cell of a value batch entry)
      bevmsda::HaloArgs h;
      h.need = need; h.need_shift = need_shift; h.flag = halo_flag;
      if (d->M == 8 && a.qtile == 8 && d->reserved[5] != 1 && d->L == 1)
        hipLaunchKernelGGL((bevmsda::msda_fused_d32_halo_kernel<T, 4, 2, 4, 1, 8>), grid, dim3(256), 0, st, f, h);
      else if (d->L > 1) hipLaunchKernelGGL((bevmsda::msda_fused_d32_halo_kernel<T, 4, 2, 4>), grid, dim3(256), 0, st, f, h);
      else hipLaunchKernelGGL((bevmsda::msda_fused_d32_halo_kernel<T, 4, 2, 8>), grid, dim3(256), 0, st, f, h);
      return launch_status();
    } else {
      return BEVMSDA_ERR_UNSUPPORTED;
    }
  }
  if constexpr (sizeof(T) == 2) {
    // bf16 storage: the 16-byte-lane kernels at 4 waves / SIMD (8 accumulators: the 64-VGPR form spills); desc->reserved[1] = 1
    // selects the 8-byte-lane form of the fp32 kernels below instead
    if (d->reserved[1] == 0) {
      if (d->P == 8) hipLaunchKernelGGL((bevmsda::msda_fused_d32_bf16x8_kernel<8, 1, 4>), grid, dim3(256), 0, st, f);
      else if (d->K == 2) hipLaunchKernelGGL((bevmsda::msda_fused_d32_bf16x8_kernel<4, 2, 4>), grid, dim3(256), 0, st, f);
      else hipLaunchKernelGGL((bevmsda::msda_fused_d32_bf16x8_kernel<4, 1, 4>), grid, dim3(256), 0, st, f);
      return launch_status();
    }
  }
  // register budget: 4 waves / SIMD (more taps in flight) for multi-level calls (SCA), 8 for the 1-level call (TSA)
  // (tools/kbench.py sweep, profiles/r1) — except TemporalSelfAttention's own fp32 shape (8 heads, query tiles of 8 rows, one
  // level, two queue entries x 4 points), which takes the body with compile-time head / level counts at 128 registers (70 vs
  // 72.4 us; at 64 registers it spills: 131 us) unless desc->reserved[5] = 1
  const bool wide = d->L > 1;
  if (sizeof(T) == 4 && d->M == 8 && a.qtile == 8 && d->P == 4 && d->K == 2 && d->L == 1 && d->reserved[5] == 0) {
    hipLaunchKernelGGL((bevmsda::msda_fused_d32_kernel<T, 4, 2, 4, 1, 8>), grid, dim3(256), 0, st, f);
  } else if (d->P == 8) {
    if (wide) hipLaunchKernelGGL((bevmsda::msda_fused_d32_kernel<T, 8, 1, 4>), grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL((bevmsda::msda_fused_d32_kernel<T, 8, 1, 8>), grid, dim3(256), 0, st, f);
  } else if (d->K == 2) {
    if (wide) hipLaunchKernelGGL((bevmsda::msda_fused_d32_kernel<T, 4, 2, 4>), grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL((bevmsda::msda_fused_d32_kernel<T, 4, 2, 8>), grid, dim3(256), 0, st, f);
  } else {
    if (wide) hipLaunchKernelGGL((bevmsda::msda_fused_d32_kernel<T, 4, 1, 4>), grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL((bevmsda::msda_fused_d32_kernel<T, 4, 1, 8>), grid, dim3(256), 0, st, f);
  }
  return launch_status();
}

}  // namespace

extern "C" {

#if BEVMSDA_FWD_PART
int bevmsda_abi_version(void) { return BEVMSDA_ABI_VERSION; }

const char *bevmsda_error_string(int code) {
  switch (code) {
    case BEVMSDA_OK: return "ok";
    case BEVMSDA_ERR_NULL_POINTER: return "null pointer";
    case BEVMSDA_ERR_BAD_SHAPE: return "bad shape";
    case BEVMSDA_ERR_TOO_LARGE: return "problem too large for 32-bit indexing";
    case BEVMSDA_ERR_MISALIGNED: return "pointer not 16-byte aligned";
    case BEVMSDA_ERR_LAUNCH: return "kernel launch failed";
    case BEVMSDA_ERR_BAD_OPTION: return "bad tuning option";
    case BEVMSDA_ERR_UNSUPPORTED: return "shape not supported by the fused entry point";
    default: return "unknown error";
  }
}

int bevmsda_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                        const float *loc, const float *attn, int N, int S, int M, int D, int L, int Q,
                        int P, float *out, void *stream) {
  return forward_impl<float>(value, spatial_shapes, level_start, loc, attn, N, S, M, D, L, Q, P, out, stream, nullptr);
}

int bevmsda_forward_f32_ex(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                           const float *loc, const float *attn, int N, int S, int M, int D, int L, int Q,
                           int P, float *out, void *stream, const bevmsda_tuning *tuning) {
  return forward_impl<float>(value, spatial_shapes, level_start, loc, attn, N, S, M, D, L, Q, P, out, stream, tuning);
}

#endif
#if !BEVMSDA_FWD_PART
int bevmsda_backward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                         const float *loc, const float *attn, const float *grad_out, int N, int S, int M,
                         int D, int L, int Q, int P, float *grad_value, float *grad_loc, float *grad_attn,
                         void *stream) {
  return backward_impl<float>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Q, P,
                              grad_value, grad_loc, grad_attn, stream, nullptr);
}

int bevmsda_backward_f32_ex(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                            const float *loc, const float *attn, const float *grad_out, int N, int S, int M,
                            int D, int L, int Q, int P, float *grad_value, float *grad_loc, float *grad_attn,
                            void *stream, const bevmsda_tuning *tuning) {
  return backward_impl<float>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Q, P,
                              grad_value, grad_loc, grad_attn, stream, tuning);
}

#endif
#if BEVMSDA_FWD_PART
int bevmsda_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                         const float *loc, const float *attn, int N, int S, int M, int D, int L, int Q,
                         int P, uint16_t *out, void *stream) {
  return forward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, N, S, M, D, L, Q, P, out, stream, nullptr);
}

#endif
#if !BEVMSDA_FWD_PART
int bevmsda_backward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                          const float *loc, const float *attn, const uint16_t *grad_out, int N, int S, int M,
                          int D, int L, int Q, int P, float *grad_value, float *grad_loc, float *grad_attn,
                          void *stream) {
  return backward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Q, P,
                               grad_value, grad_loc, grad_attn, stream, nullptr);
}

#endif
#if BEVMSDA_FWD_PART
int bevmsda_forward_bf16_ex(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                            const float *loc, const float *attn, int N, int S, int M, int D, int L, int Q,
                            int P, uint16_t *out, void *stream, const bevmsda_tuning *tuning) {
  return forward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, N, S, M, D, L, Q, P, out, stream, tuning);
}

#endif
#if !BEVMSDA_FWD_PART
int bevmsda_backward_bf16_ex(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                             const float *loc, const float *attn, const uint16_t *grad_out, int N, int S, int M,
                             int D, int L, int Q, int P, float *grad_value, float *grad_loc, float *grad_attn,
                             void *stream, const bevmsda_tuning *tuning) {
  return backward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Q, P,
                               grad_value, grad_loc, grad_attn, stream, tuning);
}

#endif
#if BEVMSDA_FWD_PART
int bevmsda_forward_ragged_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                               const float *loc, const float *attn, const int32_t *row_batch, int N, int S,
                               int M, int D, int L, int R, int P, float *out, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  return forward_impl<float>(value, spatial_shapes, level_start, loc, attn, N, S, M, D, L, 0, P, out, stream,
                             nullptr, row_batch, R);
}

#endif
#if !BEVMSDA_FWD_PART
int bevmsda_backward_ragged_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                const float *loc, const float *attn, const int32_t *row_batch,
                                const float *grad_out, int N, int S, int M, int D, int L, int R, int P,
                                float *grad_value, float *grad_loc, float *grad_attn, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  return backward_impl<float>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, 0, P,
                              grad_value, grad_loc, grad_attn, stream, nullptr, row_batch, R);
}

#endif
#if BEVMSDA_FWD_PART
int bevmsda_forward_ragged_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                const float *loc, const float *attn, const int32_t *row_batch, int N, int S,
                                int M, int D, int L, int R, int P, uint16_t *out, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  return forward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, N, S, M, D, L, 0, P, out, stream,
                              nullptr, row_batch, R);
}

#endif
#if !BEVMSDA_FWD_PART
int bevmsda_backward_ragged_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                 const float *loc, const float *attn, const int32_t *row_batch,
                                 const uint16_t *grad_out, int N, int S, int M, int D, int L, int R, int P,
                                 float *grad_value, float *grad_loc, float *grad_attn, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  return backward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, 0, P,
                               grad_value, grad_loc, grad_attn, stream, nullptr, row_batch, R);
}

int bevmsda_backward_rows_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                              const float *loc, const float *attn, const int32_t *row_batch, const float *grad_out,
                              const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                              float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (!nrows) return BEVMSDA_ERR_NULL_POINTER;
  return backward_impl<float>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, 0, P,
                              grad_value, grad_loc, grad_attn, stream, nullptr, row_batch, R, nrows, 0, 1.f, static_cast<long>(grad_value_stride));
}

int bevmsda_backward_rows_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                               const float *loc, const float *attn, const int32_t *row_batch, const uint16_t *grad_out,
                               const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                               float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (!nrows) return BEVMSDA_ERR_NULL_POINTER;
  return backward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, 0, P,
                               grad_value, grad_loc, grad_attn, stream, nullptr, row_batch, R, nrows, 0, 1.f, static_cast<long>(grad_value_stride));
}

int bevmsda_backward_rows_offs_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const bevmsda_loc_source *loc_source, const float *attn, const int32_t *row_batch,
                                   const float *grad_out, const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                                   float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (!nrows || !loc_source) return BEVMSDA_ERR_NULL_POINTER;
  return backward_impl<float>(value, spatial_shapes, level_start, nullptr, attn, grad_out, N, S, M, D, L, 0, P, grad_value, grad_loc,
                              grad_attn, stream, nullptr, row_batch, R, nrows, 0, 1.f, static_cast<long>(grad_value_stride), loc_source);
}

int bevmsda_backward_rows_offs_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                    const bevmsda_loc_source *loc_source, const float *attn, const int32_t *row_batch,
                                    const uint16_t *grad_out, const int32_t *nrows, int N, int S, int M, int D, int L, int R, int P,
                                    float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn, void *stream) {
  if (R < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (!nrows || !loc_source) return BEVMSDA_ERR_NULL_POINTER;
  return backward_impl<bf16_t>(value, spatial_shapes, level_start, nullptr, attn, grad_out, N, S, M, D, L, 0, P, grad_value, grad_loc,
                               grad_attn, stream, nullptr, row_batch, R, nrows, 0, 1.f, static_cast<long>(grad_value_stride), loc_source);
}

int bevmsda_backward_shared_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *loc,
                                const float *attn, const float *grad_out, int64_t grad_rows, float grad_scale, int N, int S, int M,
                                int D, int L, int Q, int P, float *grad_value, int64_t grad_value_stride, float *grad_loc, float *grad_attn,
                                void *stream) {
  if (grad_rows <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  return backward_impl<float>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Q, P, grad_value, grad_loc,
                              grad_attn, stream, nullptr, nullptr, -1, nullptr, static_cast<long>(grad_rows), grad_scale,
                              static_cast<long>(grad_value_stride));
}

int bevmsda_backward_shared_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *loc,
                                 const float *attn, const uint16_t *grad_out, int64_t grad_rows, float grad_scale, int N, int S,
                                 int M, int D, int L, int Q, int P, float *grad_value, int64_t grad_value_stride, float *grad_loc,
                                 float *grad_attn, void *stream) {
  if (grad_rows <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  return backward_impl<bf16_t>(value, spatial_shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Q, P, grad_value, grad_loc,
                               grad_attn, stream, nullptr, nullptr, -1, nullptr, static_cast<long>(grad_rows), grad_scale,
                              static_cast<long>(grad_value_stride));
}

#endif
#if BEVMSDA_FWD_PART
int bevmsda_rows_from_slots_f32(const float *slots, int64_t ld_slots, const float *scale, const int32_t *row_slot,
                                const int32_t *nrows, int64_t R, int C, float *rows, void *stream) {
  if (R < 0 || C <= 0 || ld_slots < C) return BEVMSDA_ERR_BAD_SHAPE;
  if (C % 4 != 0 || ld_slots % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (R == 0) return BEVMSDA_OK;
  if (!slots || !scale || !row_slot || !rows) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(slots) || misaligned(rows)) return BEVMSDA_ERR_MISALIGNED;
  const long long total = R * static_cast<long long>(C / 4);
  const long long nb = (total + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::rows_from_slots_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), slots, static_cast<long>(ld_slots), scale, row_slot, nrows,
                     static_cast<long>(R), C, rows);
  return launch_status();
}

int bevmsda_cast_rows_bf16(const float *in, const int32_t *nrows, int64_t R, int C, float scale, uint16_t *out, void *stream) {
  if (R < 0 || C <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (C % 8 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (R == 0) return BEVMSDA_OK;
  if (!in || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(in) || misaligned(out)) return BEVMSDA_ERR_MISALIGNED;
  const long long nb = (R * static_cast<long long>(C / 8) + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::cast_rows_bf16_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, nrows, static_cast<long>(R), C, scale, out);
  return launch_status();
}

int bevmsda_fused_forward_halo_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                   const int32_t *row_src, const bevmsda_fused_desc *desc, const int32_t *need, int need_shift,
                                   int64_t need_len, int32_t *halo_flag, float *out, void *stream) {
  if (!need || !halo_flag) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(need) || off4(halo_flag)) return BEVMSDA_ERR_MISALIGNED;
  return fused_impl<float>(value, spatial_shapes, level_start, offs, logits, ref, row_batch, row_src, desc, out, stream, nullptr,
                           nullptr, nullptr, need, need_shift, need_len, halo_flag);
}

int bevmsda_fused_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                              const float *offs, const float *logits, const float *ref,
                              const int32_t *row_batch, const int32_t *row_src,
                              const bevmsda_fused_desc *desc, float *out, void *stream) {
  return fused_impl<float>(value, spatial_shapes, level_start, offs, logits, ref, row_batch, row_src, desc, out,
                           stream);
}

int bevmsda_fused_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                               const float *offs, const float *logits, const float *ref,
                               const int32_t *row_batch, const int32_t *row_src,
                               const bevmsda_fused_desc *desc, uint16_t *out, void *stream) {
  return fused_impl<bf16_t>(value, spatial_shapes, level_start, offs, logits, ref, row_batch, row_src, desc, out,
                            stream);
}

int bevmsda_fused_forward_rows_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const float *offs, const float *logits, const float *ref,
                                   const int32_t *row_batch, const int32_t *row_src, const int32_t *nrows,
                                   const bevmsda_fused_desc *desc, float *out, void *stream) {
  if (!nrows) return BEVMSDA_ERR_NULL_POINTER;
  return fused_impl<float>(value, spatial_shapes, level_start, offs, logits, ref, row_batch, row_src, desc, out,
                           stream, nrows);
}

int bevmsda_fused_forward_rows_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                    const float *offs, const float *logits, const float *ref,
                                    const int32_t *row_batch, const int32_t *row_src, const int32_t *nrows,
                                    const bevmsda_fused_desc *desc, uint16_t *out, void *stream) {
  if (!nrows) return BEVMSDA_ERR_NULL_POINTER;
  return fused_impl<bf16_t>(value, spatial_shapes, level_start, offs, logits, ref, row_batch, row_src, desc, out,
                            stream, nrows);
}

int bevmsda_fused_forward_rows_save_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                        const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                        const int32_t *row_src, const int32_t *nrows, const bevmsda_fused_desc *desc, float *out,
                                        float *save_loc, float *save_attn, void *stream) {
  if (!nrows || !save_attn) return BEVMSDA_ERR_NULL_POINTER;
  return fused_impl<float>(value, spatial_shapes, level_start, offs, logits, ref, row_batch, row_src, desc, out, stream, nrows,
                           save_loc, save_attn);
}

int bevmsda_fused_forward_rows_save_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                         const float *offs, const float *logits, const float *ref, const int32_t *row_batch,
                                         const int32_t *row_src, const int32_t *nrows, const bevmsda_fused_desc *desc,
                                         uint16_t *out, float *save_loc, float *save_attn, void *stream) {
  if (!nrows || !save_attn) return BEVMSDA_ERR_NULL_POINTER;
  return fused_impl<bf16_t>(value, spatial_shapes, level_start, offs, logits, ref, row_batch, row_src, desc, out, stream, nrows,
                            save_loc, save_attn);
}

int bevmsda_add_layernorm_f32(const float *x, const float *res, const float *gamma, const float *beta,
                              float eps, int64_t rows, int C, float *out, void *stream) {
  if (rows < 0 || C <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (C != 256 && C != 512 && C != 1024) return BEVMSDA_ERR_UNSUPPORTED;
  if (rows == 0) return BEVMSDA_OK;
  if (!x || !gamma || !beta || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(x) || misaligned(out) || misaligned(gamma) || misaligned(beta) || (res && misaligned(res)))
    return BEVMSDA_ERR_MISALIGNED;
  const long long nb = (rows + 3) / 4;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  const dim3 grid(static_cast<unsigned>(nb));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (C == 256) hipLaunchKernelGGL((bevmsda::add_layernorm_kernel<1>), grid, dim3(256), 0, st, x, res, gamma, beta, eps, static_cast<long>(rows), out);
  else if (C == 512) hipLaunchKernelGGL((bevmsda::add_layernorm_kernel<2>), grid, dim3(256), 0, st, x, res, gamma, beta, eps, static_cast<long>(rows), out);
  else hipLaunchKernelGGL((bevmsda::add_layernorm_kernel<4>), grid, dim3(256), 0, st, x, res, gamma, beta, eps, static_cast<long>(rows), out);
  return launch_status();
}

int64_t bevmsda_add_layernorm_backward_partials(int64_t rows) {
  if (rows <= 0) return 0;
  const int64_t nb = (rows + 3) / 4;
  return nb > 2048 ? 2048 : nb;           // 8 workgroups per CU; every wavefront walks rows / 8192 rows
}

static int ln_backward_launch(const float *x, const float *res, const float *gamma, const float *grad_out,
                              const float *grad_out2, float eps, int64_t rows, int C, float *grad_x, float *scratch,
                              float *grad_gamma_beta, void *stream);

int bevmsda_add_layernorm_backward_f32(const float *x, const float *res, const float *gamma, const float *grad_out,
                                       float eps, int64_t rows, int C, float *grad_x, float *scratch,
                                       float *grad_gamma_beta, void *stream) {
  return ln_backward_launch(x, res, gamma, grad_out, nullptr, eps, rows, C, grad_x, scratch, grad_gamma_beta, stream);
}

int bevmsda_add_layernorm_backward2_f32(const float *x, const float *res, const float *gamma, const float *grad_out,
                                        const float *grad_out2, float eps, int64_t rows, int C, float *grad_x,
                                        float *scratch, float *grad_gamma_beta, void *stream) {
  if (grad_out2 && misaligned(grad_out2)) return BEVMSDA_ERR_MISALIGNED;
  return ln_backward_launch(x, res, gamma, grad_out, grad_out2, eps, rows, C, grad_x, scratch, grad_gamma_beta, stream);
}

static int ln_backward_launch(const float *x, const float *res, const float *gamma, const float *grad_out,
                              const float *grad_out2, float eps, int64_t rows, int C, float *grad_x, float *scratch,
                              float *grad_gamma_beta, void *stream) {
  if (rows < 0 || C <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (C != 256 && C != 512) return BEVMSDA_ERR_UNSUPPORTED;
  if (!grad_gamma_beta) return BEVMSDA_ERR_NULL_POINTER;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (rows == 0) return hipMemsetAsync(grad_gamma_beta, 0, 2 * static_cast<size_t>(C) * sizeof(float), st) == hipSuccess ? BEVMSDA_OK : BEVMSDA_ERR_LAUNCH;
  if (!x || !gamma || !grad_out || !grad_x || !scratch) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(x) || misaligned(grad_out) || misaligned(grad_x) || misaligned(gamma) || (res && misaligned(res)) ||
      off4(scratch) || off4(grad_gamma_beta))
    return BEVMSDA_ERR_MISALIGNED;
  const long long nb = bevmsda_add_layernorm_backward_partials(rows);
  const dim3 grid(static_cast<unsigned>(nb));
  if (C == 256) hipLaunchKernelGGL((bevmsda::add_layernorm_bwd_kernel<1>), grid, dim3(256), 0, st, x, res, gamma, grad_out, eps, static_cast<long>(rows), grad_x, scratch, static_cast<float *>(nullptr), grad_out2);
  else hipLaunchKernelGGL((bevmsda::add_layernorm_bwd_kernel<2>), grid, dim3(256), 0, st, x, res, gamma, grad_out, eps, static_cast<long>(rows), grad_x, scratch, static_cast<float *>(nullptr), grad_out2);
  if (hipMemsetAsync(grad_gamma_beta, 0, 2 * static_cast<size_t>(C) * sizeof(float), st) != hipSuccess) return BEVMSDA_ERR_LAUNCH;
  hipLaunchKernelGGL(bevmsda::colsum_partials_kernel, dim3(static_cast<unsigned>((2 * C + 63) / 64), 16), dim3(256), 0, st,
                     scratch, static_cast<long>(nb), 2 * C, grad_gamma_beta);
  return launch_status();
}

int bevmsda_gather_mean_f32(const float *rows, const int32_t *idx, const float *scale, int64_t Q, int J, int C,
                            float *out, void *stream) {
  if (Q < 0 || J < 0 || C <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (C % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (Q == 0) return BEVMSDA_OK;
  if (!scale || !out || (J > 0 && (!rows || !idx))) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(out) || (rows && misaligned(rows))) return BEVMSDA_ERR_MISALIGNED;
  const long long total = Q * static_cast<long long>(C / 4);
  const long long nb = (total + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipLaunchKernelGGL(bevmsda::gather_mean_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), rows, idx, scale, static_cast<long>(Q), J, C, out);
  return launch_status();
}

static int rotate_launch(const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int H, int W, int C,
                         const float *theta, const float *theta_dev, void *stream);

int bevmsda_rotate_bev_f32(const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int H, int W, int C,
                           const float *theta, void *stream) {
  if (!theta) return BEVMSDA_ERR_NULL_POINTER;
  return rotate_launch(src, ld_src, dst, ld_dst, H, W, C, theta, nullptr, stream);
}

int bevmsda_rotate_bev_dev_f32(const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int H, int W, int C,
                               const float *theta_dev, void *stream) {
  if (!theta_dev) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(theta_dev)) return BEVMSDA_ERR_MISALIGNED;
  return rotate_launch(src, ld_src, dst, ld_dst, H, W, C, nullptr, theta_dev, stream);
}

static int rotate_launch(const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int H, int W, int C,
                         const float *theta, const float *theta_dev, void *stream) {
  if (H < 0 || W < 0 || C <= 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (C != 256 && C != 512) return BEVMSDA_ERR_UNSUPPORTED;
  if (H == 0 || W == 0) return BEVMSDA_OK;
  if (!src || !dst) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_src < C || ld_dst < C) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_src % 4 != 0 || ld_dst % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (misaligned(src) || misaligned(dst)) return BEVMSDA_ERR_MISALIGNED;
  if (src == dst) return BEVMSDA_ERR_BAD_OPTION;          // a gather cannot run in place
  bevmsda::RotateArgs a;
  a.src = src; a.dst = dst; a.ld_src = ld_src; a.ld_dst = ld_dst; a.H = H; a.W = W; a.C = C;
  a.theta_dev = theta_dev;
  if (theta) { a.t00 = theta[0]; a.t01 = theta[1]; a.t02 = theta[2]; a.t10 = theta[3]; a.t11 = theta[4]; a.t12 = theta[5]; }
  else a.t00 = a.t01 = a.t02 = a.t10 = a.t11 = a.t12 = 0.f;
  const long long nb = (static_cast<long long>(H) * W + 3) / 4;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (C == 256) hipLaunchKernelGGL((bevmsda::rotate_bev_kernel<1>), dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::rotate_bev_kernel<2>), dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, a);
  return launch_status();
}

int bevmsda_flatten_feats_f32(const float *feat, const float *cams_embeds, const float *level_embed, float *out,
                              int bs, int Nc, int C, int hw, int S, int s0, void *stream) {
  if (bs < 0 || Nc < 0 || C <= 0 || hw < 0 || S < 0 || s0 < 0 || s0 + hw > S) return BEVMSDA_ERR_BAD_SHAPE;
  if (C % 64 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (bs == 0 || Nc == 0 || hw == 0) return BEVMSDA_OK;
  if (!feat || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (misaligned(out) || (cams_embeds && misaligned(cams_embeds)) || (level_embed && misaligned(level_embed)) ||
      off4(feat))
    return BEVMSDA_ERR_MISALIGNED;
  const long long bz = static_cast<long long>(bs) * Nc;
  if (bz > 65535 || C / 64 > 65535) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::FlattenArgs a;
  a.feat = feat; a.cams_embeds = cams_embeds; a.level_embed = level_embed; a.out = out;
  a.bs = bs; a.Nc = Nc; a.C = C; a.hw = hw; a.S = S; a.s0 = s0;
  const dim3 grid(static_cast<unsigned>((hw + 63) / 64), static_cast<unsigned>(C / 64), static_cast<unsigned>(bz));
  const bool vec = hw % 4 == 0 && !misaligned(feat);
  if (vec) hipLaunchKernelGGL(bevmsda::flatten_feats_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(bevmsda::flatten_feats_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

int bevmsda_flatten_rows_f32(const float *rows, int64_t ld_rows, const float *cams_embeds, const float *level_embed, float *out,
                             int bs, int Nc, int C, int hw, int S, int s0, void *stream) {
  if (bs < 0 || Nc < 0 || C <= 0 || hw < 0 || S < 0 || s0 < 0 || s0 + hw > S) return BEVMSDA_ERR_BAD_SHAPE;
  if (C % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (bs == 0 || Nc == 0 || hw == 0) return BEVMSDA_OK;
  if (!rows || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_rows < C) return BEVMSDA_ERR_BAD_SHAPE;
  if (ld_rows % 4 != 0 || misaligned(rows) || misaligned(out) || (cams_embeds && misaligned(cams_embeds)) ||
      (level_embed && misaligned(level_embed)))
    return BEVMSDA_ERR_MISALIGNED;
  const long long threads = static_cast<long long>(bs) * Nc * hw * (C / 4);
  const long long nb = (threads + 255) / 256;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::FlattenRowsArgs a;
  a.rows = rows; a.ld = ld_rows; a.cams_embeds = cams_embeds; a.level_embed = level_embed; a.out = out;
  a.bs = bs; a.Nc = Nc; a.C = C; a.hw = hw; a.S = S; a.s0 = s0;
  hipLaunchKernelGGL(bevmsda::flatten_rows_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

#endif
}  // extern "C"
