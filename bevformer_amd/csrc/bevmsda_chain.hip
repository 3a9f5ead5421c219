// C ABI of libbevmsda.so, row-local chains of an encoder layer in one kernel (linear_chain.h):
// bevmsda_proj_ffn_chain_*_f32 and bevmsda_proj_ln_proj_chain_*_f32, forward and backward.
#include "capi_checks.h"
#include "linear_chain.h"

namespace {
// linear_chain.h workgroup shape by measurement (tools/chain_small_m.py, profiles/r3): 32-row panels up to this many
// rows (a rank's tile of a BEV-tiled frame: 5,000 rows 20 vs 28 us), 64-row panels above (40,000 rows: 103 vs 103-110 us,
// half the weight traffic from L2)
constexpr long long kChainSmallRows = 8192;

// The mixed workgroup shape (desc->reserved[1] = 3; round 4): whole rounds of the 64-row shape (one workgroup
// per CU: 256 x 64 rows per round) and the remainder — a partial round that would leave most CUs idle behind a few 64-row
// workgroups — on the 32-row shape at two workgroups per CU, as a second launch over the tail rows.  Without whole rounds, without
// a remainder or with one of more than a round of 32-row panels it is one launch of one shape.
// `launch(o, desc)` launches the rows [o, o + desc.M) of the call with desc.reserved[1] as the shape.
template <class Launch>
int chain_mixed(const bevmsda_chain_desc &d, Launch launch) {
  const long long round64 = 256LL * 64;
  const long long head = (d.M / round64) * round64;
  const long long tail = d.M - head;
  bevmsda_chain_desc dh = d, dt = d;
  if (head == 0 || tail == 0 || tail > 256LL * 2 * 32) {
    dh.reserved[1] = (head == 0) ? 2 : 1;
    return launch(0LL, dh);
  }
  dh.M = head; dh.reserved[1] = 1;
  dt.M = tail; dt.reserved[1] = 2;
  const int rc = launch(0LL, dh);
  return rc != BEVMSDA_OK ? rc : launch(head, dt);
}
// p + o * stride for the optional pointers of a chain call
template <class T>
T *rows_at(T *p, long long o, long long stride) { return p ? p + o * stride : nullptr; }
}  // namespace

extern "C" {

// ---- row-local tail of an encoder layer in one kernel (linear_chain.h)
// the next layer's [first | y + pos] projection behind y (linear_chain.h TP; bevmsda_proj_ffn_chain_tail_f32)
struct ChainTail {
  const float *first; long long ld_first;
  const float *pos; long long ld_pos;
  const uint16_t *w3p; const float *b3;
  float *proj; long long ld_proj;
  int n3;
};

static int ffn_chain_launch(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                            const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                            const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                            const bevmsda_chain_desc *d, float *y, void *stream, bool save, float *sv_z0, float *sv_x,
                            float *sv_h, float *sv_z1, const float *dk0 = nullptr, const float *dkh = nullptr,
                            const float *dk1 = nullptr, const ChainTail *tp = nullptr) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  const bool drop = dk0 || dkh || dk1;
  if (tp) {
    if (save || drop) return BEVMSDA_ERR_BAD_OPTION;
    if (tp->n3 <= 0 || tp->n3 > 256 || tp->n3 % 64 != 0) return BEVMSDA_ERR_UNSUPPORTED;      // (whole tiles of both workgroup shapes)
    if (d->M > 0 && (!tp->first || !tp->w3p || !tp->proj)) return BEVMSDA_ERR_NULL_POINTER;
    if (tp->ld_first % 4 != 0 || tp->ld_proj % 4 != 0 || (tp->pos && tp->ld_pos % 4 != 0)) return BEVMSDA_ERR_UNSUPPORTED;
    if (tp->ld_first < 256 || tp->ld_proj < tp->n3 || (tp->pos && tp->ld_pos < 256)) return BEVMSDA_ERR_BAD_SHAPE;
    if (misaligned(tp->first) || misaligned(tp->w3p) || misaligned(tp->proj) || (tp->pos && misaligned(tp->pos)) ||
        (tp->b3 && misaligned(tp->b3)))
      return BEVMSDA_ERR_MISALIGNED;
  }
  if (drop && !save) return BEVMSDA_ERR_BAD_OPTION;
  if ((dk0 && misaligned(dk0)) || (dkh && misaligned(dkh)) || (dk1 && misaligned(dk1))) return BEVMSDA_ERR_MISALIGNED;
  if (save && d->M > 0 && (!sv_z0 || !sv_x || !sv_h || !sv_z1)) return BEVMSDA_ERR_NULL_POINTER;
  if (save && (misaligned(sv_z0) || misaligned(sv_x) || misaligned(sv_h) || misaligned(sv_z1))) return BEVMSDA_ERR_MISALIGNED;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->C != bevmsda::kChainC || d->F != bevmsda::kChainF) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!rows || !w0p || !w1p || !w2p || !gamma0 || !beta0 || !gamma1 || !beta1 || !y) return BEVMSDA_ERR_NULL_POINTER;
  if ((idx == nullptr) != (scale == nullptr)) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_rows % 4 != 0 || d->ld_y % 4 != 0 || (res && d->ld_res % 4 != 0)) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->ld_rows < d->C || d->ld_y < d->C || (res && d->ld_res < d->C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(rows) || misaligned(w0p) || misaligned(w1p) || misaligned(w2p) || misaligned(y) || (res && misaligned(res)) ||
      (b0 && misaligned(b0)) || (b1 && misaligned(b1)) || (b2 && misaligned(b2)) || misaligned(gamma0) || misaligned(beta0) ||
      misaligned(gamma1) || misaligned(beta1))
    return BEVMSDA_ERR_MISALIGNED;
  // workgroup shape (desc->reserved[1]): 1 = 64-row panels (8 wavefronts, one workgroup per CU), 2 = 32-row panels
  // (4 wavefronts, two workgroups per CU); 0 = default
  int shape = d->reserved[1];
  if (shape < 0 || shape > 3) return BEVMSDA_ERR_BAD_OPTION;
  // desc->reserved[2]: columns of idx (0 = 2; J > 2: rows idx[m, 2..] >= 0 are added to the first row's — inference launches only)
  const int gst = d->reserved[2] == 0 ? 2 : d->reserved[2];
  if (gst < 2 || gst > 64 || (gst > 2 && (!idx || save))) return BEVMSDA_ERR_BAD_OPTION;
  // default: 32-row panels up to kChainSmallRows rows, mixed from one whole round of 64-row panels on (measured at 40,000
  // rows, interleaved runs on one box: 103.2-103.6 vs 106.6-107.2 us; profiles/r4/r4f_chain_mixed_shape_ab.txt)
  // (with the next layer's projection behind it the 32-row shape wins at every row count: two workgroups per CU cover each
  // other's fetch / split / barrier phases of the extra stage — 127 vs 140 us at 40,000 rows, base frame 4.09 vs 4.20 ms;
  // profiles/r6/r6u_seam_ab.txt)
  // (round 6, last day — at FRAME level, in a replayed graph, the inference launches are fastest as ONE launch of 32-row panels at
  // every row count: the mixed shape's isolated 3 us per launch do not pay for its second launch and the round of one workgroup
  // per CU — base frame 4.00 against 4.03 ms, bf16 2.78 against 2.81, first frame 3.94 against 4.03, small4 1.29 against 1.32,
  // queue 17.02 against 17.27; the training step too, by less: small4 bf16 4.96-4.97 against 4.98-5.00 ms, base 18.65-18.73 against
  // 18.70-18.76; profiles/r6z/r6zz_chain_shape_frame_ab.txt)
  // (between 8,192 and 16,384 rows — a tile of four ranks — one partial round of 64-row panels stays ahead: rank 1 of 4 1.61
  // against 1.66 ms)
  if (shape == 0) shape = (tp || d->M <= kChainSmallRows) ? 2 : (d->M >= 256LL * 64 ? 2 : 1);
  if (shape == 3)                              // mixed: chain_mixed above (gathered rows are addressed through idx, not by row)
    return chain_mixed(*d, [&](long long o, const bevmsda_chain_desc &part) {
      ChainTail tt{};
      if (tp) {
        tt = *tp;
        tt.first += o * tp->ld_first;
        tt.pos = rows_at(tt.pos, o, tp->ld_pos);
        tt.proj += o * tp->ld_proj;
      }
      return ffn_chain_launch(idx ? rows : rows + o * d->ld_rows, rows_at(idx, o, gst), rows_at(scale, o, 1), w0p, b0,
                              rows_at(res, o, d->ld_res), gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, &part, y + o * d->ld_y,
                              stream, save, rows_at(sv_z0, o, 256), rows_at(sv_x, o, 256), rows_at(sv_h, o, 512),
                              rows_at(sv_z1, o, 256), rows_at(dk0, o, 256), rows_at(dkh, o, 512), rows_at(dk1, o, 256),
                              tp ? &tt : nullptr);
    });
  const int bm = shape == 1 ? 64 : 32;
  const long long nb = (d->M + bm - 1) / bm;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  a.rows = rows; a.ld_rows = d->ld_rows; a.gidx = idx; a.gscale = scale; a.gstride = gst;
  a.w0 = w0p; a.w1 = w1p; a.w2 = w2p; a.b0 = b0; a.b1 = b1; a.b2 = b2;
  a.res = res; a.ld_res = d->ld_res; a.gamma0 = gamma0; a.beta0 = beta0; a.gamma1 = gamma1; a.beta1 = beta1;
  a.eps0 = d->eps0; a.eps1 = d->eps1; a.y = y; a.ld_y = d->ld_y; a.M = d->M;
  a.sv_z0 = sv_z0; a.sv_x = sv_x; a.sv_h = sv_h; a.sv_z1 = sv_z1;
  a.dk0 = dk0; a.dkh = dkh; a.dk1 = dk1;
  if (tp) {
    a.tp_first = tp->first; a.ld_tp_first = tp->ld_first; a.tp_pos = tp->pos; a.ld_tp_pos = tp->ld_pos;
    a.w3 = tp->w3p; a.b3 = tp->b3; a.y3 = tp->proj; a.ld_y3 = tp->ld_proj; a.N3 = tp->n3;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
#define BEVMSDA_CHAIN_TP(NP_, PRE_)                                                                                               \
  do {                                                                                                                            \
    if (shape == 1) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 2, 1, 8, false, false, true>), grid, dim3(512), 0, st, a); \
    else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 1, 2, 4, false, false, true>), grid, dim3(256), 0, st, a);            \
  } while (0)
  if (tp) {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN_TP(3, 2); else BEVMSDA_CHAIN_TP(3, 0); }
    else { if (idx) BEVMSDA_CHAIN_TP(1, 2); else BEVMSDA_CHAIN_TP(1, 0); }
    return launch_status();
  }
#undef BEVMSDA_CHAIN_TP
#define BEVMSDA_CHAIN(NP_, PRE_, SV_, DR_)                                                                                        \
  do {                                                                                                                            \
    if (shape == 1) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 2, 1, 8, SV_, DR_>), grid, dim3(512), 0, st, a); \
    else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 0, 1, 2, 4, SV_, DR_>), grid, dim3(256), 0, st, a);            \
  } while (0)
  if (drop) {                                  // (train() mode with active dropout: the gather form only)
    if (!idx) return BEVMSDA_ERR_UNSUPPORTED;
    if (d->precision == 0) BEVMSDA_CHAIN(3, 2, true, true); else BEVMSDA_CHAIN(1, 2, true, true);
  } else if (save) {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN(3, 2, true, false); else BEVMSDA_CHAIN(3, 0, true, false); }
    else { if (idx) BEVMSDA_CHAIN(1, 2, true, false); else BEVMSDA_CHAIN(1, 0, true, false); }
  } else {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN(3, 2, false, false); else BEVMSDA_CHAIN(3, 0, false, false); }
    else { if (idx) BEVMSDA_CHAIN(1, 2, false, false); else BEVMSDA_CHAIN(1, 0, false, false); }
  }
#undef BEVMSDA_CHAIN
  return launch_status();
}

int bevmsda_proj_ffn_chain_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                               const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                               const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                               const bevmsda_chain_desc *d, float *y, void *stream) {
  return ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, d, y, stream, false,
                          nullptr, nullptr, nullptr, nullptr);
}

int bevmsda_proj_ffn_chain_tail_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                    const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                    const uint16_t *w2p, const float *b2, const float *gamma1, const float *beta1,
                                    const bevmsda_chain_desc *d, float *y, const float *first, int64_t ld_first,
                                    const float *pos, int64_t ld_pos, const uint16_t *w3p, const float *b3, int n3,
                                    float *proj_out, int64_t ld_proj, void *stream) {
  const ChainTail tp{first, ld_first, pos, ld_pos, w3p, b3, proj_out, ld_proj, n3};
  return ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, d, y, stream, false,
                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &tp);
}

int bevmsda_proj_ffn_chain_train_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                     const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p,
                                     const float *b1, const uint16_t *w2p, const float *b2, const float *gamma1,
                                     const float *beta1, const bevmsda_chain_desc *d, float *y, float *save_z0, float *save_x,
                                     float *save_h, float *save_z1, const float *drop0, const float *droph,
                                     const float *drop1, void *stream) {
  return ffn_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, w2p, b2, gamma1, beta1, d, y, stream, true,
                          save_z0, save_x, save_h, save_z1, drop0, droph, drop1);
}

// ---- backward of the projection + FFN chain (linear_chain.h, MODE 2)
int bevmsda_proj_ffn_chain_backward_f32(const float *grad_y, int64_t ld_grad_y, const float *save_z0, const float *save_h,
                                        const float *save_z1, const float *gamma0, const float *gamma1, const uint16_t *w0t_p,
                                        const uint16_t *w1t_p, const uint16_t *w2t_p, const bevmsda_chain_desc *d, float *grad_z1,
                                        float *grad_h, float *grad_z0, float *grad_in, float *grad_gamma_beta1,
                                        float *grad_gamma_beta0, const float *drop0, const float *drop1, float hidden_scale,
                                        float *grad_zp, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->C != bevmsda::kChainC || d->F != bevmsda::kChainF) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!grad_y || !save_z0 || !save_h || !save_z1 || !gamma0 || !gamma1 || !w0t_p || !w1t_p || !w2t_p || !grad_z1 || !grad_h ||
      !grad_z0 || !grad_in || !grad_gamma_beta1 || !grad_gamma_beta0)
    return BEVMSDA_ERR_NULL_POINTER;
  if (ld_grad_y % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ld_grad_y < d->C) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(grad_y) || misaligned(save_z0) || misaligned(save_h) || misaligned(save_z1) || misaligned(gamma0) ||
      misaligned(gamma1) || misaligned(w0t_p) || misaligned(w1t_p) || misaligned(w2t_p) || misaligned(grad_z1) ||
      misaligned(grad_h) || misaligned(grad_z0) || misaligned(grad_in) || off4(grad_gamma_beta1) ||
      off4(grad_gamma_beta0))
    return BEVMSDA_ERR_MISALIGNED;
  const long long nb = (d->M + 31) / 32;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  // the three GEMMs of the backward read the images of the TRANSPOSED weights in the slots of the forward's: stage "0" =
  // gz0 W0 (256 x 256), stage "1" = gz1 W2 (512 columns, K = 256), stage "2" = gh W1 (256 columns, K = 512)
  a.w0 = w0t_p; a.w1 = w2t_p; a.w2 = w1t_p;
  a.gamma0 = gamma0; a.gamma1 = gamma1; a.eps0 = d->eps0; a.eps1 = d->eps1; a.M = d->M;
  a.bw_gy = grad_y; a.bw_ld_gy = ld_grad_y; a.bw_z1 = save_z1; a.bw_h = save_h; a.bw_z0 = save_z0;
  a.bw_gz1 = grad_z1; a.bw_gh = grad_h; a.bw_gz0 = grad_z0; a.bw_din = grad_in;
  a.bw_dgb1 = grad_gamma_beta1; a.bw_dgb0 = grad_gamma_beta0;
  if (drop0 && !grad_zp) return BEVMSDA_ERR_NULL_POINTER;
  if ((drop0 && misaligned(drop0)) || (drop1 && misaligned(drop1)) || (grad_zp && misaligned(grad_zp))) return BEVMSDA_ERR_MISALIGNED;
  a.dk0 = drop0; a.dk1 = drop1; a.bw_hscale = hidden_scale; a.bw_gzp = grad_zp;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
  if (d->precision == 0) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<3, 0, 2, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<1, 0, 2, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  return launch_status();
}

// ---- backward of the projection + LayerNorm + projection chain (linear_chain.h, MODE 3)
int bevmsda_proj_ln_proj_chain_backward_f32(const float *grad_proj, int64_t ld_grad_proj, const float *grad_x, const float *save_z0,
                                            const float *gamma0, const uint16_t *w0t_p, const uint16_t *w1t_p,
                                            const bevmsda_chain_desc *d, float *grad_z0, float *grad_in, float *grad_gamma_beta0,
                                            const float *drop0, float *grad_zp, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  const int N2 = d->reserved[0];
  if (d->C != bevmsda::kChainC || N2 <= 0 || N2 % 256 != 0 || N2 > bevmsda::kChainMaxN2) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!grad_proj || !save_z0 || !gamma0 || !w0t_p || !w1t_p || !grad_z0 || !grad_in || !grad_gamma_beta0) return BEVMSDA_ERR_NULL_POINTER;
  if (ld_grad_proj % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  if (ld_grad_proj < N2) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(grad_proj) || (grad_x && misaligned(grad_x)) || misaligned(save_z0) || misaligned(gamma0) || misaligned(w0t_p) ||
      misaligned(w1t_p) || misaligned(grad_z0) || misaligned(grad_in) || off4(grad_gamma_beta0))
    return BEVMSDA_ERR_MISALIGNED;
  const long long nb = (d->M + 31) / 32;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  a.w0 = w0t_p; a.w1 = w1t_p; a.N2 = N2;
  a.gamma0 = gamma0; a.eps0 = d->eps0; a.M = d->M;
  a.bw_gy = grad_proj; a.bw_ld_gy = ld_grad_proj; a.bw_z1 = grad_x; a.bw_z0 = save_z0;
  a.bw_gz0 = grad_z0; a.bw_din = grad_in; a.bw_dgb0 = grad_gamma_beta0;
  if (drop0 && !grad_zp) return BEVMSDA_ERR_NULL_POINTER;
  if ((drop0 && misaligned(drop0)) || (grad_zp && misaligned(grad_zp))) return BEVMSDA_ERR_MISALIGNED;
  a.dk0 = drop0; a.bw_gzp = grad_zp; a.bw_hscale = 1.f;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
  if (d->precision == 0) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<3, 0, 3, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<1, 0, 3, 1, 2, 4, false, false>), grid, dim3(256), 0, st, a);
  return launch_status();
}

static int ln_proj_chain_launch(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                const bevmsda_chain_desc *d, float *x_out, float *proj_out, void *stream, bool save,
                                float *sv_z0, const float *dk0 = nullptr) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (dk0 && (!save || misaligned(dk0))) return BEVMSDA_ERR_BAD_OPTION;
  if (save && d->M > 0 && !sv_z0) return BEVMSDA_ERR_NULL_POINTER;
  if (save && misaligned(sv_z0)) return BEVMSDA_ERR_MISALIGNED;
  if (d->M < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  const long ld_y2 = d->reserved[0];
  if (d->C != bevmsda::kChainC || d->F <= 0 || d->F % 32 != 0 || d->F > bevmsda::kChainMaxN2) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->M == 0) return BEVMSDA_OK;
  if (!rows || !w0p || !w1p || !gamma0 || !beta0 || !x_out || !proj_out) return BEVMSDA_ERR_NULL_POINTER;
  if ((idx == nullptr) != (scale == nullptr)) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_rows % 4 != 0 || d->ld_y % 4 != 0 || ld_y2 % 4 != 0 || (res && d->ld_res % 4 != 0)) return BEVMSDA_ERR_UNSUPPORTED;
  if (d->ld_rows < d->C || d->ld_y < d->C || ld_y2 < d->F || (res && d->ld_res < d->C)) return BEVMSDA_ERR_BAD_SHAPE;
  if (misaligned(rows) || misaligned(w0p) || misaligned(w1p) || misaligned(x_out) || misaligned(proj_out) || (res && misaligned(res)) ||
      (b0 && misaligned(b0)) || (b1 && misaligned(b1)) || misaligned(gamma0) || misaligned(beta0))
    return BEVMSDA_ERR_MISALIGNED;
  int shape = d->reserved[1];
  if (shape < 0 || shape > 3) return BEVMSDA_ERR_BAD_OPTION;
  // (isolated: mixed 100.4-101.5 vs 103.8-105.7 us at 40,000 rows; in the frame one launch of 32-row panels wins — see ffn_chain_launch)
  if (shape == 0) shape = d->M <= kChainSmallRows ? 2 : (d->M >= 256LL * 64 ? 2 : 1);
  if (d->F % 64 != 0) shape = 1;               // the 32-row shape walks 64-column tiles
  if (shape == 3)                              // mixed: whole rounds on the 64-row shape, the tail on the 32-row shape
    return chain_mixed(*d, [&](long long o, const bevmsda_chain_desc &part) {
      return ln_proj_chain_launch(idx ? rows : rows + o * d->ld_rows, rows_at(idx, o, 2), rows_at(scale, o, 1), w0p, b0,
                                  rows_at(res, o, d->ld_res), gamma0, beta0, w1p, b1, &part, x_out + o * d->ld_y,
                                  proj_out + o * ld_y2, stream, save, rows_at(sv_z0, o, 256), rows_at(dk0, o, 256));
    });
  const int bm = shape == 1 ? 64 : 32;
  const long long nb = (d->M + bm - 1) / bm;
  if (nb >= (1LL << 31)) return BEVMSDA_ERR_TOO_LARGE;
  bevmsda::ChainArgs a{};
  a.rows = rows; a.ld_rows = d->ld_rows; a.gidx = idx; a.gscale = scale;
  a.w0 = w0p; a.w1 = w1p; a.w2 = nullptr; a.b0 = b0; a.b1 = b1; a.b2 = nullptr;
  a.res = res; a.ld_res = d->ld_res; a.gamma0 = gamma0; a.beta0 = beta0; a.gamma1 = a.beta1 = nullptr;
  a.eps0 = d->eps0; a.eps1 = 0.f; a.y = x_out; a.ld_y = d->ld_y; a.M = d->M; a.y2 = proj_out; a.ld_y2 = ld_y2; a.N2 = d->F;
  a.sv_z0 = sv_z0;
  a.dk0 = dk0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nb));
#define BEVMSDA_CHAIN(NP_, PRE_, SV_, DR_)                                                                                        \
  do {                                                                                                                            \
    if (shape == 1) hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 1, 2, 1, 8, SV_, DR_>), grid, dim3(512), 0, st, a); \
    else hipLaunchKernelGGL((bevmsda::linear_chain_kernel<NP_, PRE_, 1, 1, 2, 4, SV_, DR_>), grid, dim3(256), 0, st, a);            \
  } while (0)
  if (save) {                                  // (the autograd path's forward has no gather prepass: plain rows only)
    if (idx) return BEVMSDA_ERR_UNSUPPORTED;
    if (dk0) { if (d->precision == 0) BEVMSDA_CHAIN(3, 0, true, true); else BEVMSDA_CHAIN(1, 0, true, true); }
    else { if (d->precision == 0) BEVMSDA_CHAIN(3, 0, true, false); else BEVMSDA_CHAIN(1, 0, true, false); }
  } else {
    if (d->precision == 0) { if (idx) BEVMSDA_CHAIN(3, 2, false, false); else BEVMSDA_CHAIN(3, 0, false, false); }
    else { if (idx) BEVMSDA_CHAIN(1, 2, false, false); else BEVMSDA_CHAIN(1, 0, false, false); }
  }
#undef BEVMSDA_CHAIN
  return launch_status();
}

int bevmsda_proj_ln_proj_chain_f32(const float *rows, const int32_t *idx, const float *scale, const uint16_t *w0p, const float *b0,
                                   const float *res, const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                   const bevmsda_chain_desc *d, float *x_out, float *proj_out, void *stream) {
  return ln_proj_chain_launch(rows, idx, scale, w0p, b0, res, gamma0, beta0, w1p, b1, d, x_out, proj_out, stream, false, nullptr);
}

int bevmsda_proj_ln_proj_chain_train_f32(const float *rows, const uint16_t *w0p, const float *b0, const float *res,
                                         const float *gamma0, const float *beta0, const uint16_t *w1p, const float *b1,
                                         const bevmsda_chain_desc *d, float *x_out, float *proj_out, float *save_z0,
                                         const float *drop0, void *stream) {
  return ln_proj_chain_launch(rows, nullptr, nullptr, w0p, b0, res, gamma0, beta0, w1p, b1, d, x_out, proj_out, stream, true,
                              save_z0, drop0);
}

}  // extern "C"
