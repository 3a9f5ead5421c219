// C ABI of libbevmsda.so, decoder self-attention core and detection head (mha_d32.h, head_branch.h, head_decode.h):
// bevmsda_mha_d32_f32, bevmsda_head_branches_f32, bevmsda_nms_free_decode_f32.
#include "capi_checks.h"
#include "mha_d32.h"
#include "head_branch.h"
#include "head_decode.h"

extern "C" {

int bevmsda_mha_d32_f32(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, int nq, int nk,
                        int bs, int heads, int D, float scale, float *out, int64_t ldo, void *stream) {
  if (nq < 0 || nk < 0 || bs < 0 || heads < 0 || D < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (D != bevmsda::kMhaD) return BEVMSDA_ERR_UNSUPPORTED;
  if (nq == 0 || bs == 0 || heads == 0) return BEVMSDA_OK;
  if (nk == 0) return BEVMSDA_ERR_BAD_SHAPE;                     // a softmax over no keys
  if (!q || !k || !v || !out) return BEVMSDA_ERR_NULL_POINTER;
  if (ldq % 4 != 0 || ldk % 4 != 0 || ldv % 4 != 0 || ldo % 4 != 0) return BEVMSDA_ERR_UNSUPPORTED;
  const int64_t width = static_cast<int64_t>(heads) * bevmsda::kMhaD;
  if (ldq < width || ldk < width || ldv < width || ldo < width) return BEVMSDA_ERR_BAD_SHAPE;
  if (heads > 65535 || bs > 65535) return BEVMSDA_ERR_TOO_LARGE;  // grid y / z
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(out)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::MhaArgs a;
  a.q = q; a.k = k; a.v = v; a.o = out;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.nq = nq; a.nk = nk; a.bs = bs; a.scale = scale;
  const dim3 grid((nq + bevmsda::kMhaBQ - 1) / bevmsda::kMhaBQ, heads, bs), block(bevmsda::kMhaWaves * 64);
  hipLaunchKernelGGL(bevmsda::mha_d32_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

// ---- detection head (head_branch.h, head_decode.h): argument checks and launches

static int head_branch_table(const bevmsda_head_branch *src, int n, bool norms, bevmsda::HeadBranchW *dst) {
  for (int l = 0; l < n; ++l) {
    const bevmsda_head_branch &s = src[l];
    if (!s.w1 || !s.w2 || !s.w3 || !s.b1 || !s.b2 || !s.b3) return BEVMSDA_ERR_NULL_POINTER;
    if (norms && (!s.gamma1 || !s.beta1 || !s.gamma2 || !s.beta2)) return BEVMSDA_ERR_NULL_POINTER;
    if (misaligned(s.w1) || misaligned(s.w2) || misaligned(s.w3) || misaligned(s.b1) || misaligned(s.b2) ||
        off4(s.b3))
      return BEVMSDA_ERR_MISALIGNED;
    if (norms && (misaligned(s.gamma1) || misaligned(s.beta1) || misaligned(s.gamma2) || misaligned(s.beta2)))
      return BEVMSDA_ERR_MISALIGNED;
    bevmsda::HeadBranchW &d = dst[l];
    d.w1 = s.w1; d.w2 = s.w2; d.w3 = s.w3;
    d.b1 = s.b1; d.b2 = s.b2; d.b3 = s.b3;
    d.g1 = s.gamma1; d.be1 = s.beta1; d.g2 = s.gamma2; d.be2 = s.beta2;
    d.eps1 = s.eps1; d.eps2 = s.eps2;
  }
  return BEVMSDA_OK;
}

int bevmsda_head_branches_f32(const float *x, const float *ref, const bevmsda_head_branch *reg, const bevmsda_head_branch *cls,
                              const bevmsda_head_desc *d, float *out_box, float *out_cls, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->mode != BEVMSDA_HEAD_MODE_HEAD && d->mode != BEVMSDA_HEAD_MODE_REFINE) return BEVMSDA_ERR_BAD_OPTION;
  if (d->precision != 0 && d->precision != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->layer_stride != 0 && d->layer_stride != 1) return BEVMSDA_ERR_BAD_OPTION;
  if (d->L < 0 || d->nq < 0 || d->bs < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->L > BEVMSDA_HEAD_MAX_LAYERS || (d->mode == BEVMSDA_HEAD_MODE_REFINE && d->L > 1)) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  const bool with_cls = d->mode == BEVMSDA_HEAD_MODE_HEAD;
  if (with_cls && (d->cls_out < 1 || d->cls_out > 32)) return BEVMSDA_ERR_BAD_SHAPE;
  const long long M = 1LL * d->nq * d->bs;
  if (M > (1LL << 24)) return BEVMSDA_ERR_TOO_LARGE;
  if (d->L == 0 || M == 0) return BEVMSDA_OK;
  if (!x || !ref || !reg || !out_box || (with_cls && (!cls || !out_cls))) return BEVMSDA_ERR_NULL_POINTER;
  if (d->ld_x < 256 || (d->L > 1 && d->ld_layer < M * d->ld_x)) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->ld_x % 4 != 0 || d->ld_layer % 4 != 0) return BEVMSDA_ERR_MISALIGNED;       // rows must start on 16 bytes (LDS-DMA)
  if (misaligned(x) || off4(ref) || off4(out_box) ||
      (with_cls && off4(out_cls)))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::HeadArgs a = {};
  const int ntab = d->layer_stride == 0 ? 1 : d->L;
  int rc = head_branch_table(reg, ntab, false, a.reg);
  if (rc != BEVMSDA_OK) return rc;
  if (with_cls) {
    rc = head_branch_table(cls, ntab, true, a.cls);
    if (rc != BEVMSDA_OK) return rc;
  }
  a.x = x; a.ld_x = d->ld_x; a.ld_layer = d->ld_layer;
  a.ref = ref; a.out_box = out_box; a.out_cls = out_cls;
  a.nq = d->nq; a.bs = d->bs; a.code_size = d->code_size; a.cls_out = with_cls ? d->cls_out : 0;
  a.mode = d->mode; a.layer_stride = d->layer_stride;
  for (int i = 0; i < 3; ++i) {
    // the reference scales by the Python (double) difference pc_range[3 + i] - pc_range[i], rounded to fp32 by the multiply
    a.pc[i] = static_cast<float>(d->pc_range[i]);
    a.pc[3 + i] = static_cast<float>(d->pc_range[3 + i] - d->pc_range[i]);
  }
  const dim3 grid(static_cast<unsigned>((M + 31) / 32), d->L, with_cls ? 2 : 1), block(256);
  if (d->precision == 0) hipLaunchKernelGGL(bevmsda::head_branch_kernel<3>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(bevmsda::head_branch_kernel<1>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

int bevmsda_nms_free_decode_f32(const float *cls, const float *box, const bevmsda_decode_desc *d,
                                float *scores, int64_t *labels, float *boxes, uint8_t *keep, int32_t *count, void *stream) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->bs < 0 || d->nq < 0 || d->num_classes < 0 || d->max_num < 0 || d->n_ladder < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->bs > 65535) return BEVMSDA_ERR_TOO_LARGE;
  const long long n = 1LL * d->nq * d->num_classes;
  if (n > bevmsda::kDecodeMaxScores || d->max_num > bevmsda::kDecodeMaxNum || d->n_ladder > bevmsda::kDecodeMaxLadder)
    return BEVMSDA_ERR_TOO_LARGE;
  if (d->max_num > n) return BEVMSDA_ERR_BAD_SHAPE;               // as torch.topk: k out of range
  if (d->bs == 0) return BEVMSDA_OK;
  if (!count) return BEVMSDA_ERR_NULL_POINTER;
  if (d->max_num > 0 && (!cls || !box || !scores || !labels || !boxes || !keep)) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(scores) ||
      off8(labels) || off4(boxes) ||
      off4(count))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DecodeArgs a = {};
  a.cls = cls; a.box = box; a.n_ladder = d->n_ladder;
  for (int i = 0; i < d->n_ladder; ++i) a.ladder[i] = d->ladder[i];
  a.nq = d->nq; a.C = d->num_classes; a.code_size = d->code_size; a.max_num = d->max_num;
  for (int i = 0; i < 6; ++i) a.range[i] = d->post_center_range[i];
  a.scores = scores; a.labels = reinterpret_cast<long long *>(labels); a.boxes = boxes; a.keep = keep; a.count = count;
  const dim3 grid(d->bs);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n <= 2048) hipLaunchKernelGGL((bevmsda::nms_free_decode_kernel<2048, 256>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((bevmsda::nms_free_decode_kernel<16384, 1024>), grid, dim3(1024), 0, st, a);
  return launch_status();
}

}  // extern "C"
