// C ABI of libbevmsda.so, optimizer step (optim.h):
// bevmsda_optim_job_blocks, bevmsda_optim_workspace_bytes, bevmsda_optim_grad_norm_f32, bevmsda_optim_adamw_f32.
#include "capi_checks.h"
#include "optim.h"

extern "C" {

int64_t bevmsda_optim_job_blocks(int64_t numel) {
  if (numel < 0) return -1;
  return (numel + bevmsda::kOptimBlockElems - 1) / bevmsda::kOptimBlockElems;
}

// one double per block of the norm kernel (which runs one block when there is none)
int64_t bevmsda_optim_workspace_bytes(int64_t blocks) {
  if (blocks < 0) return -1;
  return (blocks > 0 ? blocks : 1) * static_cast<int64_t>(sizeof(double));
}

int bevmsda_optim_grad_norm_f32(const bevmsda_optim_job *jobs, int njobs, int64_t blocks, double max_norm, int flags,
                                void *workspace, void *scalars, void *stream) {
  static_assert(sizeof(bevmsda_optim_job) == sizeof(bevmsda::OptimJob) && sizeof(bevmsda_optim_job) == 56, "bevmsda_optim_job layout");
  static_assert(sizeof(bevmsda::OptimScalars) == 4 * BEVMSDA_OPTIM_SCALAR_WORDS, "scalars layout");
  if (njobs < 0 || blocks < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (blocks >= (1LL << 30)) return BEVMSDA_ERR_TOO_LARGE;
  if (flags & ~(BEVMSDA_OPTIM_CLIP | BEVMSDA_OPTIM_SKIP_NONFINITE)) return BEVMSDA_ERR_BAD_OPTION;
  if ((flags & BEVMSDA_OPTIM_CLIP) && !(max_norm >= 0.0)) return BEVMSDA_ERR_BAD_OPTION;
  if (njobs == 0) return BEVMSDA_OK;
  if (!jobs || !workspace || !scalars) return BEVMSDA_ERR_NULL_POINTER;
  if (off8(jobs) || off8(workspace) || off4(scalars)) return BEVMSDA_ERR_MISALIGNED;
  hipLaunchKernelGGL(bevmsda::optim_grad_norm_kernel, dim3(static_cast<unsigned>(blocks > 0 ? blocks : 1)),
                     dim3(bevmsda::kOptimThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const bevmsda::OptimJob *>(jobs), njobs, static_cast<int>(blocks), max_norm, flags,
                     static_cast<double *>(workspace), static_cast<bevmsda::OptimScalars *>(scalars));
  return launch_status();
}

int bevmsda_optim_adamw_f32(const bevmsda_optim_job *jobs, int njobs, int64_t blocks, const bevmsda_optim_group *groups,
                            int ngroups, const void *scalars, void *stream) {
  static_assert(sizeof(bevmsda_optim_group) == sizeof(bevmsda::OptimGroup) && sizeof(bevmsda_optim_group) == 40, "bevmsda_optim_group layout");
  if (njobs < 0 || blocks < 0 || ngroups < 0) return BEVMSDA_ERR_BAD_SHAPE;
  if (blocks >= (1LL << 30)) return BEVMSDA_ERR_TOO_LARGE;
  if (njobs == 0) return BEVMSDA_OK;
  if (!jobs || !groups || ngroups == 0 || !scalars) return BEVMSDA_ERR_NULL_POINTER;
  if (off8(jobs) || off8(groups) || off4(scalars)) return BEVMSDA_ERR_MISALIGNED;
  if (blocks == 0) return BEVMSDA_OK;             // (every job is empty: the steps were counted by the norm launch)
  hipLaunchKernelGGL(bevmsda::optim_adamw_kernel, dim3(static_cast<unsigned>(blocks)), dim3(bevmsda::kOptimThreads), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const bevmsda::OptimJob *>(jobs), njobs,
                     reinterpret_cast<const bevmsda::OptimGroup *>(groups), static_cast<const bevmsda::OptimScalars *>(scalars));
  return launch_status();
}

}  // extern "C"
