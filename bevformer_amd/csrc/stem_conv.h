// The backbone's stem in one launch on the CDNA4 matrix cores: 7 x 7 stride-2 convolution (padding 3, no bias) of an NCHW
// fp32 image batch, inference BatchNorm, ReLU and the 3 x 3 stride-2 max pooling (padding 1), written as the channel-last
// rows the first bottleneck reads (mmdet's ResNet stem as the reference configs build it, bevformer_base.py:43-53).
//
//   c[img, oy, ox, co] = relu( bn_co( sum_{ci < 3} sum_{i < 7} sum_{j < 7} x[img, ci, 2 oy - 3 + i, 2 ox - 3 + j] w[co, ci, i, j] ) )
//   y[img, py, px, co] = max over the 3 x 3 window { c[img, 2 py - 1 + a, 2 px - 1 + b, co] }, taps outside the conv map left out
//
// Hc = (H - 1) div 2 + 1, Wc likewise; Hp = (Hc - 1) div 2 + 1, Wp likewise.  An input tap outside the image counts zero and
// addresses nothing.  bn_co(v) = v * scale + shift, scale = gamma / sqrt(var + eps), shift = beta - mean * scale: conv_bn_rows.h's
// epilogue, expression for expression.  The norm and the ReLU (NaN stays NaN) come BEFORE the maximum — gamma may be negative —,
// and the maximum is torch.max_pool2d's: a NaN in the window wins.  pool = 0 writes the rows of c instead of y.
//
// Tile: a workgroup of four wavefronts owns kStemPH x kStemPW = 7 x 8 pooled pixels of one image and computes the 15 x 17 = 255
// conv pixels under them (a one-pixel halo, recomputed by the neighbours: 255 / 224 = 1.14 x the arithmetic).  255 conv pixels
// are the 256 rows of a GEMM tile but one: wavefront w owns rows 64 w .. 64 w + 63 (2 MFMA tiles) x all 64 columns (2 tiles),
// conv_mfma.h's wavefront tile and accumulator layout (D[n][m]: the weight fragment is the A operand, a lane holds four
// consecutive output channels of one conv pixel).
//
// Input fetch: the 35 x 39 x 3 input patch under the conv patch is staged ONCE into LDS as fp32 (pitch 40) with coalesced
// 4-byte loads — NCHW rows are only 4-byte aligned —, out-of-image pixels as exact zeros under a predicate that addresses
// nothing.  The B operand of an MFMA is built from there: the K axis is laid out (ci, i) x j with j padded from 7 to 8, so that
// the eight k of a lane are eight CONSECUTIVE floats of the patch (row 2 cy + i of channel ci from column 2 cx on), split to
// bf16 hi / lo in registers.  Lane j = 7 is set to an exact zero in the register; the 22nd (ci, i) group — K = 21 x 8 = 168
// padded to 11 k-steps of 16 = 176 — likewise.  The padding weights are exact zeros in the image.
//
// Weight image (stem_pack_weight_kernel): [plane hi | plane lo][k-step 11][column tile 2][lane 64][8 bf16] = 45,056 bytes, a
// lane's fragment of a (k-step, column tile) at lane * 16 bytes: copied once per workgroup into LDS, read back with
// conflict-free 16-byte reads.  The bf16 kernel reads the hi plane only.
//
// LDS: [input patch 16,800 B][weights 45,056 B (split) / 22,528 B (bf16)] while the GEMM runs; after a barrier the same bytes
// hold the normed, rectified conv patch, 256 rows x (64 + 4 pad) fp32 = 69,632 bytes, which is pooled there and leaves as whole
// 256-byte rows.  69,632 bytes: two workgroups per CU.  The conv map never reaches memory.
//
// Memory safety: a pixel of x is addressed only under (0 <= iy < H and 0 <= ix < W) of its own image, a row of y only for an
// output pixel inside the problem, and only its 64 columns.
#pragma once
#include "conv_mfma.h"

namespace bevmsda {

constexpr int kStemCin = 3, kStemCout = 64, kStemK = 7;
constexpr int kStemPH = 7, kStemPW = 8;                                 // pooled pixels per workgroup
constexpr int kStemCH = 2 * kStemPH + 1, kStemCW = 2 * kStemPW + 1;     // 15 x 17 conv pixels under them
constexpr int kStemIH = 4 * kStemPH + 7, kStemIW = 4 * kStemPW + 7;     // 35 x 39 input pixels under those
constexpr int kStemPitch = kStemIW + 1;                                 // 40: the j = 7 lane of the last conv column stays inside
constexpr int kStemPatch = kStemCin * kStemIH * kStemPitch;             // 4,200 floats
constexpr int kStemGroups = kStemCin * kStemK;                          // 21 (ci, i) groups of 8 k
constexpr int kStemKSteps = (kStemGroups + 1) / 2;                      // 11 MFMA k-steps of 16
constexpr int kStemPlane16 = kStemKSteps * 2 * 64;                      // 1,408 16-byte fragments per plane
constexpr int kStemCPitch = kStemCout + 4;                              // fp32 per conv-patch row in LDS
constexpr int kStemLdsBytes = 256 * kStemCPitch * 4;                    // 69,632
static_assert(kStemCH * kStemCW <= 256, "the conv patch is one 256-row GEMM tile");
static_assert(kStemPatch * 4 + 2 * kStemPlane16 * 16 <= kStemLdsBytes, "patch + weights fit under the conv patch");

struct StemArgs {
  const float *x;                       // (n_img, 3, H, W), unit column stride
  long ld_img, ld_ch, ld_row;
  const uint16_t *wpack;
  const float *gamma, *beta, *mean, *var;       // (64) each
  float eps;
  float *y;                             // pool: (n_img Hp Wp, ldy) rows; else (n_img Hc Wc, ldy)
  long ldy;
  int H, W, Hc, Wc, Hp, Wp;
  int tiles_y, tiles_x;                 // tiles of kStemPH x kStemPW pooled pixels per image
  int pool;
};

// One thread per (k-step, column tile, lane): the fragment w[32 jt + (lane & 31)][group 2 s + (lane >> 5)][0 .. 7] as bf16 hi and
// lo; the eighth element and the 22nd group are exact zeros.  w: (64, 3, 7, 7) contiguous.
__global__ void stem_pack_weight_kernel(const float *__restrict__ w, uint16_t *__restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= kStemPlane16) return;
  const int lane = t & 63, jt = (t >> 6) & 1, s = t >> 7;
  const int n = 32 * jt + (lane & 31), grp = 2 * s + (lane >> 5);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (grp < kStemGroups && e < kStemK) ? w[(n * kStemGroups + grp) * kStemK + e] : 0.f;
  uint4 hi, lo;
  lin_split8<true>(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), hi, lo);
  reinterpret_cast<uint4 *>(out)[t] = hi;
  reinterpret_cast<uint4 *>(out)[kStemPlane16 + t] = lo;
}

// torch.max_pool2d's update: a larger value or a NaN replaces the maximum
__device__ __forceinline__ float stem_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <int NPROD>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) stem_kernel(const StemArgs a) {
  static_assert(NPROD == 1 || NPROD == 3, "NPROD: 1 = bf16 inputs, 3 = split-f32");
  constexpr bool LO = NPROD == 3;
  constexpr int NPL = LO ? 2 : 1;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kStemLdsBytes];
  float *const patch = reinterpret_cast<float *>(lds_raw);
  uint4 *const wl = reinterpret_cast<uint4 *>(lds_raw + kStemPatch * 4);
  float *const cpatch = reinterpret_cast<float *>(lds_raw);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int t = blockIdx.x;
  const int tx = t % a.tiles_x;
  t /= a.tiles_x;
  const int ty = t % a.tiles_y;
  const long img = t / a.tiles_y;
  const int py0 = ty * kStemPH, px0 = tx * kStemPW;
  const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;       // conv pixel of patch position (0, 0)
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;       // input pixel of patch position (0, 0)

  // ---- the input patch -> LDS (the only place x is addressed), the weight image -> LDS
  // (every load is issued before the first LDS write: 17 pixels and up to 11 weight fragments in flight per thread)
  const float *ximg = a.x + img * a.ld_img;
  constexpr int PIT = (kStemPatch + 255) / 256, WIT = (NPL * kStemPlane16 + 255) / 256;
  float pv[PIT];
  uint4 wv[WIT];
#pragma unroll
  for (int it = 0; it < PIT; ++it) {
    const int e = it * 256 + tid;
    const int col = e % kStemPitch, rr = e / kStemPitch;
    const int r = rr % kStemIH, ci = rr / kStemIH;      // (e >= kStemPatch: ci = 3, never loaded and never stored)
    const int iy = iy0 + r, ix = ix0 + col;
    pv[it] = 0.f;
    if (e < kStemPatch && col < kStemIW && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
      pv[it] = ximg[ci * a.ld_ch + static_cast<long>(iy) * a.ld_row + ix];
  }
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.wpack);
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int e = it * 256 + tid;
      wv[it] = make_uint4(0u, 0u, 0u, 0u);
      if (e < NPL * kStemPlane16) wv[it] = src[e];
    }
  }
#pragma unroll
  for (int it = 0; it < PIT; ++it) {
    const int e = it * 256 + tid;
    if (e < kStemPatch) patch[e] = pv[it];
  }
#pragma unroll
  for (int it = 0; it < WIT; ++it) {
    const int e = it * 256 + tid;
    if (e < NPL * kStemPlane16) wl[e] = wv[it];
  }
  __syncthreads();

  // ---- the GEMM: rows = conv pixels of the patch (cy * 17 + cx), K = 11 k-steps, 64 columns
  int aoff[2];                          // patch offset of this lane's conv pixel (row 2 cy, column 2 cx of channel 0), per tile
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int m = wave * 64 + i * 32 + (lane & 31);
    m = m < kStemCH * kStemCW ? m : kStemCH * kStemCW - 1;       // the 256th row repeats the 255th: never stored
    const int cy = m / kStemCW, cx = m - cy * kStemCW;
    aoff[i] = 2 * cy * kStemPitch + 2 * cx;
  }
  const int khalf = lane >> 5;
  lin_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
  for (int s = 0; s < kStemKSteps; ++s) {
    const int grp = 2 * s + khalf;                      // (ci, i) = (grp / 7, grp % 7): patch row ci * 35 + 2 cy + i
    const bool live = grp < kStemGroups;
    const int goff = (grp / kStemK) * (kStemIH * kStemPitch) + (grp % kStemK) * kStemPitch;
    lin_bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f), q = p;
      if (live) {
        const float2 *src = reinterpret_cast<const float2 *>(patch + goff + aoff[i]);    // 2 cx: 8-byte aligned
        const float2 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
        p = make_float4(v0.x, v0.y, v1.x, v1.y);
        q = make_float4(v2.x, v2.y, v3.x, 0.f);         // j = 7: an exact zero, whatever the patch holds there
      }
      uint4 hi, lo;
      lin_split8<LO>(p, q, hi, lo);
      ah[i] = __builtin_bit_cast(lin_bf16x8, hi);
      if (LO) al[i] = __builtin_bit_cast(lin_bf16x8, lo);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bh[j] = __builtin_bit_cast(lin_bf16x8, wl[(s * 2 + j) * 64 + lane]);
      if (LO) bl[j] = __builtin_bit_cast(lin_bf16x8, wl[kStemPlane16 + (s * 2 + j) * 64 + lane]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {         // D[n][m], conv_mfma.h's order of products
        if (LO) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], al[i], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl[j], ah[i], acc[i][j], 0, 0, 0);
        }
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[j], ah[i], acc[i][j], 0, 0, 0);
      }
  }
  __syncthreads();              // every fragment has been read: the patch and the weights may be overwritten

  // ---- BatchNorm + ReLU -> the conv patch in LDS.  Registers 4 g .. 4 g + 3 of a lane: columns nb + 8 g .. + 3 of row lane & 31
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = j * 32 + 4 * (lane >> 5) + 8 * g;
      const float4 ga = *reinterpret_cast<const float4 *>(a.gamma + n);       // conv_bn_rows.h's, expression for expression
      const float4 be = *reinterpret_cast<const float4 *>(a.beta + n);
      const float4 mu = *reinterpret_cast<const float4 *>(a.mean + n);
      const float4 va = *reinterpret_cast<const float4 *>(a.var + n);
      float4 sc, sh;
      sc.x = ga.x / sqrtf(va.x + a.eps); sh.x = be.x - mu.x * sc.x;
      sc.y = ga.y / sqrtf(va.y + a.eps); sh.y = be.y - mu.y * sc.y;
      sc.z = ga.z / sqrtf(va.z + a.eps); sh.z = be.z - mu.z * sc.z;
      sc.w = ga.w / sqrtf(va.w + a.eps); sh.w = be.w - mu.w * sc.w;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = wave * 64 + i * 32 + (lane & 31);
        float4 v = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        v = make_float4(v.x * sc.x + sh.x, v.y * sc.y + sh.y, v.z * sc.z + sh.z, v.w * sc.w + sh.w);
        conv_relu4(v);
        *reinterpret_cast<float4 *>(cpatch + m * kStemCPitch + n) = v;
      }
    }
  }
  __syncthreads();

  const int n4 = (tid & 15) * 4;        // 16 threads write one 256-byte row
  if (a.pool) {
    // ---- 3 x 3 stride-2 maximum over the conv patch: pooled pixel (py, px) of the tile reads patch rows 2 py .. 2 py + 2
    for (int e = tid >> 4; e < kStemPH * kStemPW; e += 16) {
      const int ly = e / kStemPW, lx = e - ly * kStemPW;
      const int py = py0 + ly, px = px0 + lx;
      if (py >= a.Hp || px >= a.Wp) continue;
      const float ninf = -__builtin_inff();
      float4 mx = make_float4(ninf, ninf, ninf, ninf);
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int gy = cy0 + 2 * ly + dy;
        if (gy < 0 || gy >= a.Hc) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int gx = cx0 + 2 * lx + dx;
          if (gx < 0 || gx >= a.Wc) continue;           // a tap outside the conv map is left out
          const float4 v = *reinterpret_cast<const float4 *>(cpatch + ((2 * ly + dy) * kStemCW + 2 * lx + dx) * kStemCPitch + n4);
          mx.x = stem_max(mx.x, v.x); mx.y = stem_max(mx.y, v.y); mx.z = stem_max(mx.z, v.z); mx.w = stem_max(mx.w, v.w);
        }
      }
      const long q = (img * a.Hp + py) * a.Wp + px;
      *reinterpret_cast<float4 *>(a.y + q * a.ldy + n4) = mx;
    }
  } else {
    // ---- the conv rows this tile owns: patch rows 1 .. 14, columns 1 .. 16 (conv pixels 2 py0 .. + 13, 2 px0 .. + 15)
    for (int e = tid >> 4; e < (kStemCH - 1) * (kStemCW - 1); e += 16) {
      const int ly = e / (kStemCW - 1) + 1, lx = e % (kStemCW - 1) + 1;
      const int gy = cy0 + ly, gx = cx0 + lx;
      if (gy >= a.Hc || gx >= a.Wc) continue;
      const float4 v = *reinterpret_cast<const float4 *>(cpatch + (ly * kStemCW + lx) * kStemCPitch + n4);
      const long q = (img * a.Hc + gy) * a.Wc + gx;
      *reinterpret_cast<float4 *>(a.y + q * a.ldy + n4) = v;
    }
  }
}

}  // namespace bevmsda
