"""The optimizer step on the device (csrc/optim.h): ``optim_grad_norm`` (the 2-norm of all gradients, the clip coefficient, the
skip flag and the step counts, one launch) and ``optim_adamw`` (torch's single-tensor AdamW over a job table, one launch), the
planner of the job table and ``fused_reject``, which says why an optimizer configuration is not what the two kernels compute.
GPU only: there is no CPU implementation and no fallback — ``bevformer_amd.optim.AdamW2`` raises with the reason."""
import ctypes

import torch

from .. import _lib
from ._base import _launch

OPTIM_BLOCK_ELEMS = 4096          # elements of one job per block (csrc/optim.h: kOptimBlockElems)
OPTIM_JOB_WORDS = 7               # struct bevmsda_optim_job as 8-byte words
OPTIM_GROUP_WORDS = 5             # struct bevmsda_optim_group: five doubles


def optim_job_blocks(numel):
    """Blocks of a job of ``numel`` elements: ``bevmsda_optim_job_blocks`` restated (tests pin the two together)."""
    if numel < 0:
        raise ValueError("numel must not be negative")
    return (numel + OPTIM_BLOCK_ELEMS - 1) // OPTIM_BLOCK_ELEMS


def optim_plan(numels):
    """``(first_block of every job, total blocks)`` for jobs of ``numels`` elements in table order.  A job without elements
    has no block (it shares its ``first_block`` with the next job and is never found by a block) and still counts its step."""
    first, total = [], 0
    for n in numels:
        first.append(total)
        total += optim_job_blocks(int(n))
    if total >= 1 << 30:
        raise ValueError(f"optimizer step: {total} blocks of {OPTIM_BLOCK_ELEMS} elements exceed the kernels' 2^30")
    return first, total


def optim_job_rows(entries):
    """``entries``: ``(p_ptr, g_ptr, exp_avg_ptr, exp_avg_sq_ptr, step_ptr, numel, group)`` per job -> the table as rows of
    seven 8-byte words (``group | first_block << 32`` in the last) and the total block count."""
    first, total = optim_plan([e[5] for e in entries])
    rows = [[e[0], e[1], e[2], e[3], e[4], e[5], e[6] | (fb << 32)] for e, fb in zip(entries, first)]
    return rows, total


def fused_reject(params, amsgrad=False, grad_clip=None, maximize=False, check_grads=False):
    """Why the device path does not cover an optimizer over ``params`` (a short reason), or ``None`` when it does: dense fp32
    parameters on ONE GPU, contiguous; no amsgrad, no maximize; ``grad_clip`` ``None`` or a dict with ``max_norm`` >= 0 and
    ``norm_type`` 2.  ``check_grads``: also the gradients that are present (dense fp32, contiguous, on the parameter's
    device).  Parameters are looked at through their attributes only (``dtype``, ``is_sparse``, ``is_cuda``, ``device``,
    ``is_contiguous()``, ``grad``)."""
    if amsgrad:
        return "amsgrad is not implemented by the device kernels"
    if maximize:
        return "maximize is not implemented by the device kernels"
    if grad_clip is not None:
        if not isinstance(grad_clip, dict) or "max_norm" not in grad_clip:
            return "grad_clip must be None or a dict with max_norm"
        if set(grad_clip) - {"max_norm", "norm_type"}:
            return f"grad_clip has keys the device path does not know: {sorted(set(grad_clip) - {'max_norm', 'norm_type'})}"
        if float(grad_clip.get("norm_type", 2)) != 2.0:
            return f"norm_type {grad_clip.get('norm_type')} is not 2"
        if not float(grad_clip["max_norm"]) >= 0.0:
            return f"max_norm {grad_clip['max_norm']} is negative or NaN"
    device = None
    for i, p in enumerate(params):
        if p.is_sparse:
            return f"parameter {i} is sparse"
        if p.dtype != torch.float32:
            return f"parameter {i} is {p.dtype}, not float32"
        if not p.is_cuda:
            return f"parameter {i} is on {p.device}, not on a GPU (there is no CPU path)"
        if not p.is_contiguous():
            return f"parameter {i} is not contiguous"
        if device is None:
            device = p.device
        elif p.device != device:
            return f"parameters on more than one device ({device} and {p.device})"
        g = p.grad if check_grads else None
        if g is not None:
            if g.is_sparse:
                return f"the gradient of parameter {i} is sparse"
            if g.dtype != torch.float32 or g.device != p.device:
                return f"the gradient of parameter {i} is {g.dtype} on {g.device}, not float32 on {p.device}"
            if not g.is_contiguous():
                return f"the gradient of parameter {i} is not contiguous"
    return None


def optim_workspace_elems(blocks):
    """Doubles of the norm kernel's workspace for ``blocks`` blocks."""
    return _lib.load().bevmsda_optim_workspace_bytes(int(blocks)) // 8


def optim_grad_norm(table, njobs, blocks, workspace, scalars, max_norm=None, skip_nonfinite=False):
    """``bevmsda_optim_grad_norm_f32``: ``table`` (njobs, 7) int64 on the device, ``workspace`` float64
    (``optim_workspace_elems``), ``scalars`` the 8-word block (fp32 view).  ``max_norm`` ``None``: no clipping."""
    flags = (_lib.OPTIM_CLIP if max_norm is not None else 0) | (_lib.OPTIM_SKIP_NONFINITE if skip_nonfinite else 0)
    _launch(scalars.device, "optim_grad_norm", lambda lib, stream: lib.bevmsda_optim_grad_norm_f32(
        table.data_ptr() if njobs else None, njobs, blocks, float(max_norm) if max_norm is not None else 0.0, flags,
        workspace.data_ptr(), scalars.data_ptr(), stream), required=True)


def optim_adamw(table, njobs, blocks, groups, ngroups, scalars):
    """``bevmsda_optim_adamw_f32``: the update of every job of ``table`` with the hyperparameters of ``groups`` (ngroups, 5)
    float64 on the device and the scalars ``optim_grad_norm`` wrote on the same stream."""
    _launch(scalars.device, "optim_adamw", lambda lib, stream: lib.bevmsda_optim_adamw_f32(
        table.data_ptr() if njobs else None, njobs, blocks, groups.data_ptr(), ngroups, scalars.data_ptr(), stream), required=True)


assert ctypes.sizeof(_lib.OptimJob) == 8 * OPTIM_JOB_WORDS and ctypes.sizeof(_lib.OptimGroup) == 8 * OPTIM_GROUP_WORDS
