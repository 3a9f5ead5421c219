// RETIRED (round 6; not compiled, not exported): the LDS-tile TemporalSelfAttention sampling kernel (msda_tsa_lds.inc here,
// msda_fused_d32_tsa_lds_kernel; in csrc/msda_d32.h until round 11) as a resident, software-pipelined grid.  It was bit-equal
// to the default kernel on every case of the LDS-tile kernel's bit-equality test (grids, ego shifts and offset scales) and
// SLOWER than both: 67.8-72 us against 55-57 (one workgroup per tile and head) and 52-54 us (default) at the base grid,
// 79-83 us inside the frame (profiles/r6/r6z_tsa_lds_ab2.txt, r6z_tsa_lds_ab3.txt).  Ablations (r6z_tsa_lds_variants2.txt):
// skeleton 17.5 us, + staging 27 us, + taps 31 us, all three 68 us — the stage of unit u + 1 does run under the taps of unit
// u, but with one workgroup of 8 wavefronts per CU a unit's 72 KiB of LDS-DMA takes longer to land (2.5 us: the 72 KiB are all
// the bytes the CU has in flight) than the unit's taps take (1.5 us), and LDS has no room for a third buffer.  The register
// file of a CU holds 512 KiB, its LDS 160: a design that lands tap lines in registers keeps 3-5 x the bytes in flight
// (16 wavefronts x 24 KiB in the default kernel).  To revive: paste into csrc/msda_d32.h behind msda_tsa_lds.inc's kernel
// and add the launch (dim3(256) workgroups of 512 threads) to fused_impl in csrc/bevmsda_capi.hip.
// The LDS-tile kernel as a RESIDENT, software-pipelined grid (round 6): the ablations of msda_fused_d32_tsa_lds_kernel say its
// staging (19 us), its taps (22 us) and its skeleton (17 us) ADD — two co-resident workgroups run their phases in step.  Here one
// workgroup per CU (512 threads, two region buffers of 72 KiB) walks its XCD's range of (tile, head) blocks and stages unit
// u + 1 = the next (tile, head, queue entry) while the lane groups take unit u's taps out of the other buffer; the front-end
// operands of the next block are requested a unit ahead too.  The LDS-DMA is issued through inline assembly: the compiler's own
// wait-count pass knows nothing of it (it would drain the memory counter in front of every LDS read that might alias a pending
// DMA), the kernel waits `vmcnt(0)` once per unit, in front of the unit's barrier — by then the unit's lines have had a whole tap
// phase to land.  One barrier per unit: it publishes the unit's lines and retires the previous unit's readers.
// Same parameters, coefficients and order of sums: bit-equal to msda_fused_d32_kernel<float, 4, 2, 4, 1, 8>.
constexpr int kTsaLdsPipeLines = ((kTsaLdsRW * kTsaLdsRH + 63) / 64) * 64;      // whole rounds of 8 wavefronts x 8 lines

__device__ __forceinline__ void tsa_lds_dma16(const void *src, uint32_t lds_byte) {
  const unsigned d = __builtin_amdgcn_readfirstlane(lds_byte);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(src), "s"(d) : "memory", "m0");
}

template <int WPE>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
msda_fused_d32_tsa_lds_pipe_kernel(const FusedArgs f) {
  using T = float;
  constexpr int D = 32, PT = 4, Mh = 8, TX = kTsaLdsTX, TY = kTsaLdsTY, RW = kTsaLdsRW, RH = kTsaLdsRH, HALO = kTsaLdsHalo;
  constexpr int NL = kTsaLdsPipeLines;                         // 576 lines = 72 KiB per buffer (560 used)
  constexpr int NR = TX * TY / 64;
  static_assert(NR == 2, "two rows per lane group");
  __shared__ __attribute__((aligned(16))) unsigned char region[2][NL * 128];
  const KArgs &a = f.k;
  const int tid = threadIdx.x, lig = tid & 7, grp = tid >> 3, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = static_cast<int>(a.shapes[0]), W = static_cast<int>(a.shapes[1]);
  const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
  const int nb = tiles_x * tiles_y * Mh;
  const int per = (nb + 7) >> 3;
  const int wpx = static_cast<int>(gridDim.x >> 3);            // workgroups per XCD
  const int xcd = blockIdx.x & 7;
  const int hi = (xcd + 1) * per < nb ? (xcd + 1) * per : nb;
  int lb = xcd * per + static_cast<int>(blockIdx.x >> 3);
  if (lb >= hi) return;
  const uint32_t pix_bytes = static_cast<uint32_t>(Mh) * D * sizeof(T);
  const uint32_t lane_term = lig * 4 * static_cast<uint32_t>(sizeof(T));
  const uint32_t lbytes = static_cast<uint32_t>(a.lstart[0]) * pix_bytes;
  const uint32_t total_bytes = static_cast<uint32_t>(static_cast<unsigned long long>(a.N) * a.S * pix_bytes);
  __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.value), 0,
                                                                  static_cast<int>(total_bytes), 0x00020000);
  const float sc = f.out_scale;
  const uint32_t q = lig / PT, pj = lig % PT;
  const uint32_t nq = q * static_cast<uint32_t>(f.vadd);
  const float2 *__restrict__ rf2 = reinterpret_cast<const float2 *>(f.ref);
  const char *vbase = static_cast<const char *>(a.value);
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char *)&region[0][0]));
  const int gx = grp & 15, gy = grp >> 4;

  // region origin of (block, entry): HALO pixels up and left of the tile's first query as the entry sees it.  The entry's view
  // of the grid is the grid shifted by a whole number of pixels (the ego-motion shift of the history entry), read ONCE from
  // cell 0's reference points — no load in front of a unit's DMA.  (Reference points that are not such a grid stay exact: a
  // footprint outside the staged region takes the global-memory taps.)
  int dx[2], dy[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float2 c = rf2[e * f.A];
    dx[e] = static_cast<int>(floorf(c.x * static_cast<float>(W) - 0.5f)) - HALO;
    dy[e] = static_cast<int>(floorf(c.y * static_cast<float>(H) - 0.5f)) - HALO;
  }
  // the lines of (block, entry) into buffer `bi`: NL / 64 DMA instructions per wavefront (lines past the region: never read)
  auto stage = [&](int b, int e, int bi) {
    const int tile = b >> 3, m = b & 7;
    const int ox = (tile % tiles_x) * TX + dx[e], oy = (tile / tiles_x) * TY + dy[e];
    const unsigned long long ebase = (static_cast<unsigned long long>(e) * f.vadd * a.S + static_cast<unsigned long long>(a.lstart[0])) * pix_bytes
                                     + static_cast<unsigned long long>(m) * D * sizeof(T) + lane_term;
#pragma unroll
    for (int k = 0; k < ((BEVMSDA_TSA_LDS_DIAG & 1) ? 0 : NL / 64); ++k) {
      const int l0 = wave * 8 + k * 64;
      const int li = l0 + (lane >> 3);
      const int ry = li / RW, rx = li - ry * RW;
      int sx = ox + rx, sy = oy + ry;
      sx = sx < 0 ? 0 : (sx >= W ? W - 1 : sx);
      sy = sy < 0 ? 0 : (sy >= H ? H - 1 : sy);
      tsa_lds_dma16(vbase + ebase + static_cast<unsigned long long>(sy * W + sx) * pix_bytes, lds0 + static_cast<uint32_t>(bi * NL + l0) * 128u);
    }
  };
  // front-end operands of a block's two rows (my point's logit, offset pair, reference point)
  struct Front { float lg[NR]; float2 of[NR], rf[NR]; };
  auto front_load = [&](int b, Front &F) {
    const int m = b & 7, tile = b >> 3;
    const int x = (tile % tiles_x) * TX + gx, ybase = (tile / tiles_x) * TY + gy;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int y = ybase + 4 * i;
      const long r = (x < W && y < H) ? static_cast<long>(y) * W + x : a.NQ - 1;
      F.lg[i] = f.logits[r * f.proj_row + m * f.lg_head + q * f.lg_k + pj];
      F.of[i] = reinterpret_cast<const float2 *>(f.offs + r * f.proj_row + m * f.off_head + q * f.off_k)[pj];
      F.rf[i] = rf2[(r * f.K + q) * f.A];
    }
  };
  const int mdx = q ? dx[1] : dx[0], mdy = q ? dy[1] : dy[0];   // my entry's

  // Schedule of block t (every wait for the memory counter comes a whole tap phase after the last request):
  //   parameters(t) | wait, barrier 1 | stores(t - 1), DMA (t, entry 1), front-end loads (t + 1) | taps (t, entry 0)
  //                 | wait, barrier 2 | DMA (t + 1, entry 0)                                      | taps (t, entry 1)
  Front F;
  front_load(lb, F);
  stage(lb, 0, 0);
  f32x4 pacc[NR];                                              // the previous block's rows, stored under this block's taps
  uint32_t prow[NR];
  bool pact[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) { pacc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; prow[i] = 0; pact[i] = false; }
#pragma nounroll
  for (;;) {
    const int m = lb & 7, tile = lb >> 3;
    const int x0 = (tile % tiles_x) * TX, y0 = (tile / tiles_x) * TY;
    const int next = lb + wpx;
    const bool more = next < hi;                               // (uniform)
    const uint32_t level_base = static_cast<uint32_t>((static_cast<unsigned long long>(nq) * a.S * Mh + m) * D * sizeof(T)) + lbytes;
    const int ox = x0 + mdx, oy = y0 + mdy;
    PointParams pp[NR];
    uint32_t line[NR], orow[NR];
    bool act[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int x = x0 + gx, y = y0 + gy + 4 * i;
      act[i] = x < W && y < H;
      const long r = act[i] ? static_cast<long>(y) * W + x : a.NQ - 1;
      orow[i] = static_cast<uint32_t>((r * Mh + m) * D + lig * 4);
      const float mx = lanes_max<PT>(F.lg[i]);
      const float e = expf(F.lg[i] - mx);
      const float sum = lanes_sum<PT>(e);
      const float lx = F.rf[i].x + F.of[i].x / static_cast<float>(W);
      const float ly = F.rf[i].y + F.of[i].y / static_cast<float>(H);
      const float aw = act[i] ? e / sum : 0.f;
      int fx0, fy0;
      pp[i] = point_params_xy(lx, ly, aw, H, W, level_base, pix_bytes, fx0, fy0);
      const int px = fx0 - ox, py = fy0 - oy;
      const bool in = pp[i].off != kOobOffset && px >= 0 && px + 1 < RW && py >= 0 && py + 1 < RH;
      line[i] = in ? static_cast<uint32_t>(py * RW + px) * 128u : kTsaLdsNoLine;
    }
    f32x4 acc[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ---- entry 0 (buffer 0): its lines were requested a tap phase ago
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NR; ++i)
      if (pact[i]) *reinterpret_cast<float4 *>(static_cast<T *>(a.out) + prow[i]) = make_float4(pacc[i][0], pacc[i][1], pacc[i][2], pacc[i][3]);
    stage(lb, 1, 1);
    if (more) front_load(next, F);
#pragma unroll
    for (int i = 0; i < ((BEVMSDA_TSA_LDS_DIAG & 2) ? 0 : NR); ++i) {
      const bool slow = __builtin_amdgcn_ballot_w64((lig >> 2) == 0 && line[i] == kTsaLdsNoLine) != 0;
      if (slow) sample_points<0, PT, T>(pp[i], rsrc, lane_term, pix_bytes, static_cast<uint32_t>(W) * pix_bytes, acc[i]);
      else sample_points_lds<0, PT>(pp[i], line[i], region[0], lane_term, acc[i]);
    }
    // ---- entry 1 (buffer 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (more) stage(next, 0, 0);
#pragma unroll
    for (int i = 0; i < ((BEVMSDA_TSA_LDS_DIAG & 2) ? 0 : NR); ++i) {
      const bool slow = __builtin_amdgcn_ballot_w64((lig >> 2) == 1 && line[i] == kTsaLdsNoLine) != 0;
      if (slow) sample_points<PT, PT, T>(pp[i], rsrc, lane_term, pix_bytes, static_cast<uint32_t>(W) * pix_bytes, acc[i]);
      else sample_points_lds<PT, PT>(pp[i], line[i], region[1], lane_term, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      pacc[i] = f32x4{acc[i][0] * sc, acc[i][1] * sc, acc[i][2] * sc, acc[i][3] * sc};
      prow[i] = orow[i];
      pact[i] = act[i];
    }
    if (!more) break;
    lb = next;
  }
#pragma unroll
  for (int i = 0; i < NR; ++i)
    if (pact[i]) *reinterpret_cast<float4 *>(static_cast<T *>(a.out) + prow[i]) = make_float4(pacc[i][0], pacc[i][1], pacc[i][2], pacc[i][3]);
}

