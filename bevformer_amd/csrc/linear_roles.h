// Dense projections, role-split row-panel form: y = [x | xb rows] W^T + b for the hoisted value projections (K = 256).
//
// Same arithmetic and data layout as linear_panel.h, so the output is bit-identical to its kernel: the same weight image
// (lin_panel_pack_weight_kernel), the same LDS-DMA panel fetch and in-place [hi | lo] split with the same slot map, the
// same k16 order and product order (NPROD = 3 or 1), the same bias add / ReLU and fp32 or bf16 rounding on the way out.
// What differs is who stores.  In linear_panel_kernel every wavefront both issues MFMAs and stores its finished tiles, and
// the two phases add up instead of overlapping: a store blocks at issue once the write path is full, and
// the vector-memory counter retires in order, so a wavefront's next weight fragments queue behind its own epilogue stores.
// Here a workgroup of 768 threads has two wavefront roles:
//
//   * 8 MFMA wavefronts (two per SIMD) fetch and split the 64-row panel as the 8-wavefront panel kernel does, then each
//     walks its column tiles (64 rows x 32 columns: MT = 2, NT = 1, column tile ct = wave, wave + 8, ...) with its weight
//     fragments streamed from L2 into registers.  A finished tile (bias added) goes to the wavefront's own C slot in LDS
//     and is published by a FULL word; the wavefront then computes its next tile in its accumulators while the slot
//     drains, and waits on its FREE word before writing the slot again.  It never issues a global store: its vmcnt
//     carries weight loads only;
//   * 4 store wavefronts (one per SIMD: wavefront 8 + s shares SIMD s's two MFMA wavefronts s and s + 4, by the cyclic
//     placement of a workgroup's wavefronts) poll the FULL words of those two, read a slot with ds_read_b128 and write it
//     as whole row segments (8 lanes x 16 bytes = one 128-byte fp32 row segment, 8 x 8 bytes in bf16) with buffer
//     stores, then advance the FREE word.
//
// LDS: A planes 32 pairs x 2 KiB = 64 KiB (linear_panel.h map, BM = 64) + 8 C slots of 64 x 32 fp32 = 8 KiB each = 64 KiB
// + 16 flag words = 128 KiB + 64 B: one 768-thread workgroup per CU.
// C slot: row r (0 .. 63) at r * 128 bytes, 16-byte column chunk c (columns 4c .. 4c + 3) at ((c ^ (r & 7)) * 16).  The
// MFMA wavefront writes lane (r & 31, c & 1) of tile i = r >> 5 with ds_write_b128 (groups of 8 consecutive lanes: 8 rows,
// one chunk, 8 distinct 16-byte positions of a 128-byte bank row); the store wavefront reads row 8p + (lane >> 3), chunk
// lane & 7 (each 16-lane service group of ds_read_b128 covers 4 rows whose chunks land on 16 distinct positions of the
// 256-byte bank row: tests/test_linear_roles_model.py replays both maps).
// Handshake: FULL[w] = tiles wavefront w has published, FREE[w] = tiles its store wavefront has read out; one writer per
// word, monotonic counts.  Writer: slot stores -> s_waitcnt lgkmcnt(0) -> FULL store.  Reader: FULL poll -> slot reads ->
// s_waitcnt lgkmcnt(0) -> FREE store -> global stores from registers.  Every poll is an atomic LDS load (never cached in a
// register) and every failed poll sleeps.
#pragma once
#include "linear_panel.h"

namespace bevmsda {

constexpr int kRolesMfmaWaves = 8;
constexpr int kRolesStoreWaves = 4;
constexpr int kRolesThreads = (kRolesMfmaWaves + kRolesStoreWaves) * 64;

__device__ __forceinline__ int roles_flag_load(int *p) {
  return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
__device__ __forceinline__ void roles_flag_set(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// STAUX: cache policy bits of the global stores (0 default, 2 nt); PRIO: the MFMA wavefronts run at s_setprio 1.
// Plain projections only (PRE = 0: one source, or two row blocks; optional row segments), K = 256, N % 32 == 0: the
// launcher checks.
template <int NPROD, int STAUX, bool PRIO, bool MASKED = false>
__global__ void __launch_bounds__(kRolesThreads) linear_roles_kernel(const PanelArgs a) {
  static_assert(NPROD == 1 || NPROD == 3, "NPROD");
  constexpr bool LO = NPROD == 3;
  constexpr int NPL = LO ? 2 : 1;
  constexpr int MT = 2;
  constexpr int NW = kRolesMfmaWaves;
  constexpr int BM = MT * 32;
  constexpr int NPAIR = (BM / 8) * 4;
  constexpr int QPW = NPAIR / NW / 4;          // row blocks per MFMA wavefront (1)
  constexpr int PANEL_BYTES = NPAIR * 2048;
  constexpr int SLOT_BYTES = BM * 32 * 4;
  constexpr int WD = 2, RS = WD + 1;
  static_assert(QPW == 1, "one row block per MFMA wavefront");
  __shared__ __attribute__((aligned(16))) unsigned char lds[PANEL_BYTES + NW * SLOT_BYTES];
  __shared__ int flags[2 * NW];                // [w]: FULL (tiles published), [NW + w]: FREE (tiles read out)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long m0 = static_cast<long>(blockIdx.x) * BM;
  if (a.seg_start != nullptr) {                // unused row segments: as linear_panel_kernel (uniform over the workgroup)
    long halo = 0;
    for (int l = 0; l < a.num_levels; ++l) halo = a.level_shapes[2 * l + 1] > halo ? a.level_shapes[2 * l + 1] : halo;
    halo += a.num_levels > 0 ? 1 : 0;
    const long first = m0 - halo > 0 ? m0 - halo : 0;
    const long last = (m0 + BM + halo < a.M ? m0 + BM + halo : a.M) - 1;
    const int s_lo = static_cast<int>(first / a.seg_len), s_hi = static_cast<int>(last / a.seg_len);
    int used = 0;
    for (int sg = s_lo; sg <= s_hi; ++sg) used |= a.seg_start[sg + 1] - a.seg_start[sg];
    if (used == 0) return;
  }
  if constexpr (MASKED) {                      // needed-panel table (linear_panel.h)
    if (!panel_rows_needed(a, m0, BM)) return;
  }
  const int nct = a.N / 32;                    // column tiles of 32
  const int nstep = kPanelK / 16;
  unsigned char *slots = lds + PANEL_BYTES;
  const long rows_here = a.M - m0 < BM ? a.M - m0 : BM;

  // ================================================================ MFMA wavefronts: panel fetch and split (linear_panel.h)
  const int d_rl = lane >> 3, d_cc = lane & 7;
  __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(a.wp), 0,
                                                                   static_cast<int>(a.wp_bytes), 0x00020000);
  const int wlane = lane * 16;
  lin_f32x16 acc[MT];
  lin_bf16x8 wf[RS][NPL];
  auto wload = [&](int st, int ct, int sg) {
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
      const int so = ((ct * nstep + sg) * 2 + pl) * 1024;
      wf[st][pl] = __builtin_bit_cast(lin_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, so, 0));
    }
  };
  if (wave < NW) {
    const float *xs = a.x0;
    const long ldx = a.ldx0;
    __builtin_amdgcn_sched_barrier(0);
    {
      const int row = panel_row_of(wave, d_rl);
      long gm = m0 + row;
      if (gm >= a.M) gm = a.M - 1;             // clamped rows are computed and never stored
      const bool second_block = a.xb != nullptr && gm >= a.m_split;
      const float *src = (second_block ? a.xb + (gm - a.m_split) * ldx : xs + gm * ldx) + (d_cc ^ (row & 7)) * 4;
      unsigned char *dst = lds + (wave * 4) * 2048;
      panel_dma_pair<0, 0>(src, dst);
      panel_dma_pair<1, 0>(src, dst + 2048);
      panel_dma_pair<2, 0>(src, dst + 2 * 2048);
      panel_dma_pair<3, 0>(src, dst + 3 * 2048);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    if (wave < nct) {
#pragma unroll
      for (int k = 0; k < WD; ++k) wload(k, wave, k);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my own DMA slots have landed
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      unsigned char *slot = lds + (wave * 4 + p) * 2048 + lane * 16;
      const float4 va = *reinterpret_cast<const float4 *>(slot);
      const float4 vb = *reinterpret_cast<const float4 *>(slot + 1024);
      uint4 hi, lo;
      lin_split8<LO>(va, vb, hi, lo);
      *reinterpret_cast<uint4 *>(slot) = hi;
      if (LO) *reinterpret_cast<uint4 *>(slot + 1024) = lo;
    }
  } else if (wave == NW && lane < 2 * NW) {
    flags[lane] = 0;
  }
  __syncthreads();                             // planes complete, flags zeroed: the only barrier of the kernel
  if (wave >= NW) {
    // ================================================================ store wavefronts: drain the C slots
    const int w0 = wave - NW, w1 = w0 + 4;
    const int n0 = w0 < nct ? (nct - w0 + NW - 1) / NW : 0;
    const int n1 = w1 < nct ? (nct - w1 + NW - 1) / NW : 0;
    const int rr = lane >> 3, c = lane & 7;
    const int es = a.out_bf16 ? 2 : 4;
    const unsigned ldy_b = static_cast<unsigned>(a.ldy) * es;
    auto drain = [&](int w, int t) {
      const unsigned char *sl = slots + w * SLOT_BYTES + rr * 128 + ((c ^ rr) << 4);
      float4 v[8];
#pragma unroll
      for (int p = 0; p < 8; ++p) v[p] = *reinterpret_cast<const float4 *>(sl + p * 1024);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      roles_flag_set(&flags[NW + w], t + 1);   // the slot is in registers: the MFMA wavefront may write it again
      const int ct = w + t * NW;
      const int n0c = ct * 32;
      const int grp = a.group_cols > 0 ? n0c / a.group_cols : 0;
      const int soff_e = n0c - grp * a.group_cols;
      const long firstel = (static_cast<long>(grp) * a.M + m0) * a.ldy;
      unsigned char *base = reinterpret_cast<unsigned char *>(a.y) + firstel * es;
      // (records end with the panel's last row: rows >= M are dropped by the bounds check)
      const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(base, 0, static_cast<int>(rows_here * ldy_b), 0x00020000);
      if (a.out_bf16) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          const panel_u32x2 d = {lin_pack2(v[p].x, v[p].y), lin_pack2(v[p].z, v[p].w)};
          __builtin_amdgcn_raw_buffer_store_b64(d, yr, static_cast<int>((p * 8 + rr) * ldy_b) + c * 8, soff_e * 2, STAUX);
        }
      } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          const panel_u32x4 d = {__float_as_uint(v[p].x), __float_as_uint(v[p].y), __float_as_uint(v[p].z), __float_as_uint(v[p].w)};
          __builtin_amdgcn_raw_buffer_store_b128(d, yr, static_cast<int>((p * 8 + rr) * ldy_b) + c * 16, soff_e * 4, STAUX);
        }
      }
    };
    int d0 = 0, d1 = 0;
    while (d0 < n0 || d1 < n1) {
      bool did = false;
      if (d0 < n0 && roles_flag_load(&flags[w0]) > d0) { drain(w0, d0); ++d0; did = true; }
      if (d1 < n1 && roles_flag_load(&flags[w1]) > d1) { drain(w1, d1); ++d1; did = true; }
      if (!did) __builtin_amdgcn_s_sleep(1);
    }
    return;
  }

  // ================================================================ MFMA wavefronts: column tiles into the C slots
  if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);

  unsigned f_addr[4];
  unsigned c_off[MT][4];                       // this lane's 16-byte C-slot positions: (tile i, register group g)
  {
    int ll = lane;
    asm volatile("" : "+v"(ll));
    const int r_ = ll & 31, h_ = ll >> 5;
    const int q0_ = ((r_ >> 2) & 1) | ((r_ >> 4) << 1);
    const int rl_ = ((r_ & 3) << 1) | ((r_ >> 3) & 1);
#pragma unroll
    for (int sc = 0; sc < 4; ++sc) f_addr[sc] = static_cast<unsigned>(q0_ * 4 * 2048 + (rl_ * 8 + (((2 * sc + h_) ^ (r_ & 7)))) * 16);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = i * 32 + r_, cc = 2 * g + h_;
        c_off[i][g] = static_cast<unsigned>(wave * SLOT_BYTES + r * 128 + ((cc ^ (r & 7)) << 4));
      }
  }
  float4 bfr[4];
  int t = 0;
  for (int ct = wave; ct < nct; ct += NW, ++t) {
    const int ct_next = ct + NW;
    lin_bf16x8 af[2][MT][NPL];
    auto aload = [&](int set, int s) {
      const unsigned base = f_addr[s & 3] + (s >> 2) * 2048;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
          af[set][i][pl] = *reinterpret_cast<const lin_bf16x8 *>(lds + base + i * (4 * 4 * 2048) + pl * 1024);
    };
    aload(0, 0);
    if (a.bias != nullptr) {
#pragma unroll
      for (int g = 0; g < 4; ++g) bfr[g] = *reinterpret_cast<const float4 *>(a.bias + ct * 32 + 4 * (lane >> 5) + 8 * g);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s + WD < 16) {
        wload((s + WD) % RS, ct, s + WD);
      } else if (ct_next < nct) {
        wload((s + WD) % RS, ct_next, s + WD - 16);
      }
      if (s + 1 < 16) aload((s + 1) & 1, s + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (LO) {
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s % RS][0], af[s & 1][i][1], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s % RS][1], af[s & 1][i][0], acc[i], 0, 0, 0);
        }
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s % RS][0], af[s & 1][i][0], acc[i], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ct_next < nct && (16 % RS) != 0) {     // the next tile's steps 0 .. WD - 1 sit in stages (16 + k) % RS
      lin_bf16x8 tmp[WD][NPL];
#pragma unroll
      for (int k = 0; k < WD; ++k)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) tmp[k][pl] = wf[(16 + k) % RS][pl];
#pragma unroll
      for (int k = 0; k < WD; ++k)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) wf[k][pl] = tmp[k][pl];
    }
    // epilogue: bias, ReLU (as linear_panel_kernel's store_tile), then into the C slot
    if (a.bias != nullptr) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          acc[i][4 * g] += bfr[g].x; acc[i][4 * g + 1] += bfr[g].y;
          acc[i][4 * g + 2] += bfr[g].z; acc[i][4 * g + 3] += bfr[g].w;
        }
    }
    if (a.relu) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = acc[i][r] < 0.f ? 0.f : acc[i][r];
    }
    while (roles_flag_load(&flags[NW + wave]) < t) __builtin_amdgcn_s_sleep(1);     // FREE: my slot has been read out
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4 *>(slots + c_off[i][g]) =
            make_float4(acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    roles_flag_set(&flags[wave], t + 1);       // FULL
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  }
}

}  // namespace bevmsda
