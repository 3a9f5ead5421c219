// C ABI of libbevmsda.so, detection loss (det_cost.h, match_lsap.h, det_loss.h):
// bevmsda_match_cost*_f32, bevmsda_lsap_f32, bevmsda_det_loss*_f32.
#include "capi_checks.h"
#include "det_cost.h"
#include "match_lsap.h"
#include "det_loss.h"

extern "C" {

static int loss_desc_check(const bevmsda_loss_desc *d) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->L < 0 || d->bs < 0 || d->nq < 0 || d->gmax < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->cls_out < 1 || d->cls_out > bevmsda::kLossMaxCls) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->nq > bevmsda::kLossMaxQueries || d->gmax > bevmsda::kLossMaxGt) return BEVMSDA_ERR_TOO_LARGE;
  if (1LL * d->L * d->bs > 65535) return BEVMSDA_ERR_TOO_LARGE;
  return BEVMSDA_OK;
}

int bevmsda_match_cost_f32(const float *cls, const float *box, const float *gt, const int32_t *label, const int32_t *count,
                           const bevmsda_loss_desc *d, float *cost, void *stream) {
  const int rc = loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0 || d->gmax == 0) return BEVMSDA_OK;
  if (!cls || !box || !gt || !label || !count || !cost) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(cost)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetCostArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.cost = cost;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.cls_weight = d->cost_cls_weight; a.reg_weight = d->cost_reg_weight;
  a.alpha = d->cost_alpha; a.gamma = d->cost_gamma; a.eps = d->cost_eps;
  const dim3 grid((d->nq + 255) / 256, d->gmax, d->L * d->bs);
  hipLaunchKernelGGL(bevmsda::det_cost_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

int bevmsda_lsap_f32(const float *cost, const int32_t *count, int P, int gmax, int nq, int32_t *match, int32_t *assigned,
                     int32_t *status, void *stream) {
  if (P < 0 || gmax < 0 || nq < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (nq > bevmsda::kLossMaxQueries || gmax > bevmsda::kLossMaxGt) return BEVMSDA_ERR_TOO_LARGE;
  if (P == 0) return BEVMSDA_OK;
  if (!count || !status || (gmax > 0 && !match) || (nq > 0 && !assigned) || (gmax > 0 && nq > 0 && !cost))
    return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cost) || off4(count) || off4(match) || off4(assigned) || off4(status)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::LsapArgs a = {};
  a.cost = cost; a.count = count; a.match = match; a.assigned = assigned; a.status = status;
  a.gmax = gmax; a.nq = nq;
  hipLaunchKernelGGL(bevmsda::lsap_kernel, dim3(P), dim3(bevmsda::kLsapThreads), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

int bevmsda_det_loss_f32(const float *cls, const float *box, const float *gt, const int32_t *label, const int32_t *count,
                         const int32_t *assigned, const float *code_weights, const float *factors,
                         const bevmsda_loss_desc *d, float *losses, float *grad_cls, float *grad_box, void *stream) {
  const int rc = loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0) return BEVMSDA_OK;
  if (!cls || !box || !count || !assigned || !code_weights || !factors || !losses || !grad_cls || !grad_box)
    return BEVMSDA_ERR_NULL_POINTER;
  if (d->gmax > 0 && (!gt || !label)) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(assigned) || off4(code_weights) ||
      off4(factors) || off4(losses) || off4(grad_cls) || off4(grad_box))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetLossArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.assigned = assigned;
  a.code_weights = code_weights; a.factors = factors; a.losses = losses; a.grad_cls = grad_cls; a.grad_box = grad_box;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.alpha = d->loss_alpha; a.gamma = d->loss_gamma; a.cls_weight = d->loss_cls_weight; a.box_weight = d->loss_box_weight;
  hipLaunchKernelGGL(bevmsda::det_loss_kernel, dim3(d->L), dim3(bevmsda::kDetLossThreads), 0, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

// ---- Group-DETR form of the detection loss: `groups` blocks of nq queries per sample, problem (l * bs + b) * groups + g

static int group_loss_desc_check(const bevmsda_group_loss_desc *d) {
  if (!d) return BEVMSDA_ERR_NULL_POINTER;
  if (d->L < 0 || d->bs < 0 || d->nq < 0 || d->gmax < 0 || d->groups < 1) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->code_size != 8 && d->code_size != 10) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->cls_out < 1 || d->cls_out > bevmsda::kLossMaxCls) return BEVMSDA_ERR_BAD_SHAPE;
  if (d->nq > bevmsda::kLossMaxQueries || d->gmax > bevmsda::kLossMaxGt) return BEVMSDA_ERR_TOO_LARGE;
  if (1LL * d->L * d->bs * d->groups > 65535) return BEVMSDA_ERR_TOO_LARGE;     // (the problems ride on gridDim.z)
  return BEVMSDA_OK;
}

int bevmsda_match_cost_grouped_f32(const float *cls, const float *box, const float *gt, const int32_t *label,
                                   const int32_t *count, const bevmsda_group_loss_desc *d, float *cost, void *stream) {
  const int rc = group_loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0 || d->gmax == 0) return BEVMSDA_OK;
  if (!cls || !box || !gt || !label || !count || !cost) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(cost)) return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetCostArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.cost = cost;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.cls_weight = d->cost_cls_weight; a.reg_weight = d->cost_reg_weight;
  a.alpha = d->cost_alpha; a.gamma = d->cost_gamma; a.eps = d->cost_eps;
  const dim3 grid((d->nq + 255) / 256, d->gmax, d->L * d->bs * d->groups);
  hipLaunchKernelGGL(bevmsda::det_cost_grouped_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a, d->groups);
  return launch_status();
}

int bevmsda_det_loss_grouped_f32(const float *cls, const float *box, const float *gt, const int32_t *label,
                                 const int32_t *count, const int32_t *assigned, const float *code_weights,
                                 const float *factors, const bevmsda_group_loss_desc *d, float *group_losses, float *losses,
                                 float *grad_cls, float *grad_box, void *stream) {
  const int rc = group_loss_desc_check(d);
  if (rc != BEVMSDA_OK) return rc;
  if (d->L == 0 || d->bs == 0 || d->nq == 0) return BEVMSDA_OK;
  if (!cls || !box || !count || !assigned || !code_weights || !factors || !group_losses || !losses || !grad_cls || !grad_box)
    return BEVMSDA_ERR_NULL_POINTER;
  if (d->gmax > 0 && (!gt || !label)) return BEVMSDA_ERR_NULL_POINTER;
  if (off4(cls) || off4(box) || off4(gt) || off4(label) || off4(count) || off4(assigned) || off4(code_weights) ||
      off4(factors) || off4(group_losses) || off4(losses) || off4(grad_cls) || off4(grad_box))
    return BEVMSDA_ERR_MISALIGNED;
  bevmsda::DetLossArgs a = {};
  a.cls = cls; a.box = box; a.gt = gt; a.label = label; a.count = count; a.assigned = assigned;
  a.code_weights = code_weights; a.factors = factors; a.losses = losses; a.grad_cls = grad_cls; a.grad_box = grad_box;
  a.bs = d->bs; a.nq = d->nq; a.cls_out = d->cls_out; a.code_size = d->code_size; a.gmax = d->gmax;
  a.alpha = d->loss_alpha; a.gamma = d->loss_gamma; a.cls_weight = d->loss_cls_weight; a.box_weight = d->loss_box_weight;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bevmsda::det_loss_grouped_kernel, dim3(d->groups, d->L), dim3(bevmsda::kDetLossThreads), 0, st, a,
                     group_losses);
  if (hipGetLastError() != hipSuccess) return BEVMSDA_ERR_LAUNCH;
  hipLaunchKernelGGL(bevmsda::det_loss_group_mean_kernel, dim3((2 * d->L + 63) / 64), dim3(64), 0, st, group_losses, losses,
                     d->L, d->groups);
  return launch_status();
}

}  // extern "C"
