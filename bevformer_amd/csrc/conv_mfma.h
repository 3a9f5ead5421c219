// The GEMM under the channel-last convolutions (conv3x3.h, conv_rows.h) on the CDNA4 matrix cores, once: the body of
// linear_splitbf16_kernel<NPROD, false, 32, SWAP, 3> (linear_mfma.h) with the A load left to the caller.
//
//   acc[m, n] = sum_c sum_{k < 32} relu?(row_c(m)[k]) * w[n, 32 c + k]
//
// over a 128 x 128 block tile on four wavefronts (2 x 2, 64 x 64 each as 2 x 2 MFMA 32 x 32 x 16 tiles), split-bf16
// (NPROD 3: hi * hi + hi * lo + lo * hi) or bf16 (NPROD 1) operands, fp32 accumulate.  A chunk c is 32 input channels of
// one tap; what row of which matrix that is for output row m is the kernel's fetch functor, and nothing here addresses x.
// The weight chunks are lin_pack_weight_kernel's image — [plane hi | plane lo][128][32 + 8 pad] bf16 per (128-column
// tile, chunk), chunks in the order the loop consumes them — copied by LDS-DMA into a single W area.
//
// LDS: [A hi | A lo][W hi | W lo], 4 planes of 128 x 40 bf16 = 40,960 bytes (split) or 2 planes = 20,480 bytes (bf16);
// three workgroups per CU under amdgpu_waves_per_eu(3, 3).
#pragma once
#include "linear_mfma.h"

namespace bevmsda {

constexpr int kConvGran = 32;                   // channel counts (per segment, C_in, C_out) are multiples of this
constexpr int kConvBM = 128, kConvBK = 32;      // block tile: 128 output rows x 128 output columns; K chunk
constexpr int kConvRow = kConvBK + 8, kConvPlane = 128 * kConvRow;      // bf16 elements per LDS row (linear_mfma.h), per plane
constexpr int kConvNP = 2, kConvRPP = 64;       // staging: 4 threads per row, 64 rows per pass, 2 passes

template <int NPROD>
constexpr int conv_lds_elems() { return 2 * (NPROD == 3 ? 2 : 1) * kConvPlane; }

// XCD-aware tile map (linear_mfma.h): blockIdx -> (mt, nt); false: this block has no tile
__device__ __forceinline__ bool conv_tile(int nblk_m, int nblk_n, int &mt, int &nt) {
  const int xcd = blockIdx.x & 7;
  const int seq = blockIdx.x >> 3;
  mt = (seq / nblk_n) * 8 + xcd;
  nt = seq % nblk_n;
  return mt < nblk_m;
}

// bit t = (dy + 1) * 3 + (dx + 1) set where tap (dy, dx) of the pixel (cy, cx) lies inside the H x W image; 1 tap: the pixel
template <int TAPS>
__device__ __forceinline__ unsigned conv_live_taps(int cy, int cx, int H, int W) {
  static_assert(TAPS == 1 || TAPS == 9, "1 x 1 or 3 x 3");
  if (TAPS == 1) return 1u;
  unsigned live = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = cy + t / 3 - 1, xx = cx + t % 3 - 1;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) live |= 1u << t;
  }
  return live;
}

__device__ __forceinline__ void conv_relu4(float4 &v) {    // NaN stays NaN, as torch.relu
  v.x = v.x < 0.f ? 0.f : v.x;
  v.y = v.y < 0.f ? 0.f : v.y;
  v.z = v.z < 0.f ? 0.f : v.z;
  v.w = v.w < 0.f ? 0.f : v.w;
}

// The main loop.  fetch(c, p, v0, v1): floats 8 (tid & 3) .. + 7 of chunk c of the row staged for tile row
// p * 64 + (tid >> 2), zeros under a dead predicate; within a chunk it is called for p = 0 first, then p = 1.
// lds: conv_lds_elems<NPROD>() bf16, 16-byte aligned.  wpack: the weight image, nchunk chunks per column tile.  Leaves the
// transposed tile in acc: D[n][m], the W fragment as the A operand, so that a lane holds 4 consecutive output columns.
template <int NPROD, class Fetch>
__device__ __forceinline__ void conv_mainloop(uint16_t *lds, const uint16_t *wpack, int nt, int nchunk, int relu_in,
                                              Fetch fetch, lin_f32x16 (&acc)[2][2]) {
  static_assert(NPROD == 1 || NPROD == 3, "NPROD: 1 = bf16 inputs, 3 = split-f32");
  constexpr bool LO = NPROD == 3;
  constexpr int ROW = kConvRow, PLANE = kConvPlane, NP = kConvNP, RPP = kConvRPP;
  constexpr int NPL = LO ? 2 : 1;
  uint16_t *const lds_a = lds;
  uint16_t *const lds_w = lds + NPL * PLANE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int srow = tid >> 2, skq = (tid & 3) * 8;

  float4 xr[NP][2];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int p = 0; p < NP; ++p) fetch(c, p, xr[p][0], xr[p][1]);
  };
  // packed chunk (nt, c): NPL planes of 128 x 40 bf16, copied by LDS-DMA (destination = wave-uniform base + lane * 16)
  constexpr int WCH16 = NPL * PLANE / 8;
  constexpr int WPIECES = (WCH16 + 255) / 256;
  const uint4 *wchunk = reinterpret_cast<const uint4 *>(wpack) + static_cast<long>(nt) * nchunk * (2 * PLANE / 8);
  auto load_w = [&](int c) {
    const uint4 *src = wchunk + static_cast<long>(c) * (2 * PLANE / 8);
#pragma unroll
    for (int i = 0; i < WPIECES; ++i) {
      if (WCH16 % 256 == 0 || (i * 256 + (tid & ~63)) < WCH16) {     // wave-uniform tail guard
        uint16_t *dst = lds_w + (i * 256 + (tid & ~63)) * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i * 256 + tid),
                                         (__attribute__((address_space(3))) void *)(dst), 16, 0, 0);
      }
    }
  };

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, fk = (lane >> 5) * 8;
  const int a_off = (wm * 64 + frow) * ROW + fk;
  const int b_off = (wn * 64 + frow) * ROW + fk;

  load_chunk(0);
  load_w(0);
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      uint4 hi, lo;
      const int off = (p * RPP + srow) * ROW + skq;
      if (relu_in) {                        // on the A operand, before the split
        conv_relu4(xr[p][0]);
        conv_relu4(xr[p][1]);
      }
      lin_split8<LO>(xr[p][0], xr[p][1], hi, lo);
      *reinterpret_cast<uint4 *>(&lds_a[off]) = hi;
      if (LO) *reinterpret_cast<uint4 *>(&lds_a[PLANE + off]) = lo;
    }
    __syncthreads();          // staged chunk visible (the LDS-DMA in flight is drained here too)
    if (c + 1 < nchunk) load_chunk(c + 1);      // in flight under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      lin_bf16x8 ah[2], bh[2], al[2], bl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ao = a_off + t * 32 * ROW + ks * 16;
        const int bo = b_off + t * 32 * ROW + ks * 16;
        ah[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_a[ao]);
        bh[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_w[bo]);
        if (LO) {
          al[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_a[PLANE + ao]);
          bl[t] = *reinterpret_cast<const lin_bf16x8 *>(&lds_w[PLANE + bo]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {       // D[n][m]: the W fragment as the A operand (16-byte epilogue)
          if (LO) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], al[i], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl[j], ah[i], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], ah[i], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();          // every fragment of this chunk has been read
    if (c + 1 < nchunk) load_w(c + 1);
  }
}

// The output row of accumulator tile i (0 / 1) of this lane in tile row mt; it may lie past M.
__device__ __forceinline__ long conv_out_row(int mt, int i) {
  const int tid = threadIdx.x;
  return static_cast<long>(mt) * kConvBM + (tid >> 7) * 64 + i * 32 + (tid & 31);
}

// The epilogue walk.  Registers 4g .. 4g + 3 of a lane are output columns nb + 8g .. + 3 of output row m = lane & 31.
// column(n) -> the state of columns n .. n + 3 (n < N, N % 4 == 0); store(state, i, m, n, v): v = acc[m, n .. n + 3] of
// tile i, m < M.
template <class Column, class Store>
__device__ __forceinline__ void conv_epilogue(const lin_f32x16 (&acc)[2][2], int mt, int nt, long M, int N, Column column,
                                              Store store) {
  const int lane = threadIdx.x & 63;
  const int wn = (threadIdx.x >> 6) & 1;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int nb = nt * 128 + wn * 64 + j * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = nb + 8 * g;
      if (n >= N) continue;                 // N % 4 == 0: n < N covers n .. n + 3
      const auto state = column(n);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long m = conv_out_row(mt, i);
        if (m >= M) continue;
        store(state, i, m, n, make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]));
      }
    }
  }
}

}  // namespace bevmsda
