"""The detection loss on the device (csrc/det_cost.h, match_lsap.h, det_loss.h): the match costs of every decoder layer and
sample (``match_cost``), the batched assignment solver (``lsap``) and the focal + L1 loss with its unit gradients
(``det_loss``) — three launches, no host read — and ``detection_loss``, the autograd Function over them.  GPU only: CPU
tensors raise; ``BEVFormerHead.loss`` decides with ``detection_loss_reject`` whether a call is covered and runs its modules
otherwise.

``groups`` (default 1) is Group-DETR's: the query axis holds ``groups`` blocks of ``nq // groups`` queries, query
``g * n + q`` is query ``q`` of group ``g``, every (layer, sample, group) is matched on its own and a layer's loss is the mean
over its groups (``BEVFormerHead_GroupDETR.loss``).  ``groups=1`` calls the entry points above; ``groups > 1`` the grouped
ones (``bevmsda_match_cost_grouped_f32``, ``bevmsda_det_loss_grouped_f32``: four launches, the last the means)."""
import collections
import ctypes

import torch
from torch.autograd.function import Function, once_differentiable

from .. import _lib
from ..ext import _ptr
from ._base import _launch

LOSS_MAX_NQ = 2048
LOSS_MAX_GT = 512
LOSS_MAX_PROBLEMS = 65535       # L * bs * groups of the grouped entry points (the grid limit)
LOSS_MAX_CLS_OUT = 32
LOSS_CODE_SIZES = (8, 10)

# FocalLossCost(weight, alpha, gamma, eps), BBox3DL1Cost(weight); FocalLoss(alpha, gamma, loss_weight), L1Loss(loss_weight);
# the defaults are the reference configs' (bevformer_base.py:139-160)
LossParams = collections.namedtuple(
    "LossParams", ["cost_cls_weight", "cost_reg_weight", "cost_alpha", "cost_gamma", "cost_eps", "loss_alpha", "loss_gamma",
                   "loss_cls_weight", "loss_box_weight"], defaults=[2.0, 0.25, 0.25, 2.0, 1e-12, 0.25, 2.0, 2.0, 0.25])


def _need(t, dtype, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype:
        raise RuntimeError(f"{what} must be a CUDA {dtype} tensor (this path has no CPU implementation)")
    return t.contiguous()


def _desc(L, bs, nq, cls_out, code_size, gmax, params):
    return _lib.LossDesc(L=L, bs=bs, nq=nq, cls_out=cls_out, code_size=code_size, gmax=gmax,
                         **{k: float(v) for k, v in params._asdict().items()})


def _group_desc(L, bs, groups, n, cls_out, code_size, gmax, params):
    return _lib.GroupLossDesc(L=L, bs=bs, groups=groups, nq=n, cls_out=cls_out, code_size=code_size, gmax=gmax,
                              **{k: float(v) for k, v in params._asdict().items()})


def _per_group(nq, groups):
    groups = int(groups)
    if groups < 1 or nq % groups:
        raise ValueError(f"detection loss: {nq} queries do not split into {groups} groups")
    return groups, nq // groups


def pack_gt(gt_bboxes_list, gt_labels_list, device, gmax=None):
    """The gt lists of ``BEVFormerHead.loss`` (plain (G, code_size - 1) tensors, (G,) labels) as the kernels' buffers:
    ``(gt (bs, Gmax, code_size - 1) fp32, label (bs, Gmax) int32, count (bs,) int32)`` on ``device``, ``Gmax`` the largest
    count rounded up to a multiple of 8 (at least 8; ``gmax`` asks for more room, e.g. for a captured graph whose gt
    changes).  The counts come from the list lengths: no device value is read."""
    counts = [int(g.shape[0]) for g in gt_bboxes_list]
    width = gt_bboxes_list[0].shape[-1]
    G = max(8, (max(counts + [0]) + 7) // 8 * 8, int(gmax or 0))
    gt = torch.zeros((len(counts), G, width), dtype=torch.float32, device=device)
    label = torch.zeros((len(counts), G), dtype=torch.int32, device=device)
    for i, (g, lab) in enumerate(zip(gt_bboxes_list, gt_labels_list)):
        if counts[i]:
            gt[i, :counts[i]] = g.to(device=device, dtype=torch.float32)
            label[i, :counts[i]] = lab.to(device=device, dtype=torch.int32)
    return gt, label, torch.tensor(counts, dtype=torch.int32, device=device)


def _shapes(cls, box, gt, label, count):
    L, bs, nq, cls_out = cls.shape
    code = box.shape[-1]
    gmax = gt.shape[1]
    if tuple(box.shape[:3]) != (L, bs, nq) or tuple(gt.shape) != (bs, gmax, code - 1) or tuple(label.shape) != (bs, gmax) \
            or tuple(count.shape) != (bs,):
        raise ValueError(f"detection loss: shapes cls {tuple(cls.shape)}, box {tuple(box.shape)}, gt {tuple(gt.shape)}, label "
                         f"{tuple(label.shape)}, count {tuple(count.shape)} do not belong together")
    return L, bs, nq, cls_out, code, gmax


def match_cost(cls, box, gt, label, count, params=LossParams(), out=None, groups=1, grouped_entry=False):
    """``bevmsda_match_cost_f32``: ``cls`` (L, bs, nq, cls_out) logits, ``box`` (L, bs, nq, code_size), packed gt ->
    ``cost`` (L, bs, Gmax, nq) fp32, gt-major; rows at and beyond ``count[b]`` are not written (``out``: the buffer to
    write into).  ``groups > 1`` (``bevmsda_match_cost_grouped_f32``; ``grouped_entry``: that entry point for one group
    too): ``cost`` is (L, bs, groups, Gmax, nq // groups)."""
    cls, box = _need(cls, torch.float32, "cls"), _need(box, torch.float32, "box")
    gt, label, count = _need(gt, torch.float32, "gt"), _need(label, torch.int32, "label"), _need(count, torch.int32, "count")
    L, bs, nq, cls_out, code, gmax = _shapes(cls, box, gt, label, count)
    groups, n = _per_group(nq, groups)
    if groups > 1 or grouped_entry:
        cost = out if out is not None else torch.empty((L, bs, groups, gmax, n), dtype=torch.float32, device=cls.device)
        assert tuple(cost.shape) == (L, bs, groups, gmax, n) and cost.is_contiguous() and cost.dtype == torch.float32
        desc = _group_desc(L, bs, groups, n, cls_out, code, gmax, params)
        _launch(cls.device, "match_cost (grouped)", lambda lib, stream: lib.bevmsda_match_cost_grouped_f32(
            _ptr(cls), _ptr(box), _ptr(gt), _ptr(label), _ptr(count), ctypes.byref(desc), _ptr(cost), stream), required=True)
        return cost
    cost = out if out is not None else torch.empty((L, bs, gmax, nq), dtype=torch.float32, device=cls.device)
    assert tuple(cost.shape) == (L, bs, gmax, nq) and cost.is_contiguous() and cost.dtype == torch.float32
    desc = _desc(L, bs, nq, cls_out, code, gmax, params)
    _launch(cls.device, "match_cost", lambda lib, stream: lib.bevmsda_match_cost_f32(
        _ptr(cls), _ptr(box), _ptr(gt), _ptr(label), _ptr(count), ctypes.byref(desc), _ptr(cost), stream), required=True)
    return cost


def lsap(cost, count, check=False):
    """``bevmsda_lsap_f32``: ``cost`` (P, Gmax, nq) fp32 (or (L, bs, Gmax, nq), P = L * bs; or the grouped
    (L, bs, groups, Gmax, n), P = L * bs * groups), ``count`` (P,) int32 rows of each
    problem -> ``(match (P, Gmax) int32, assigned (P, nq) int32, status (P,) int32)``: the column of each row (-1 on
    padding), the row of each column (-1: none) and 0 solved / 1 non-finite cost (nothing assigned) / 2 step bound.  The total
    is minimal; among equal totals the choice is the kernel's.  ``check=True`` reads ``status`` back — a synchronisation, for
    eager debugging — and raises ``ValueError`` on a non-zero one, as scipy does on a non-finite matrix."""
    cost, count = _need(cost, torch.float32, "cost"), _need(count, torch.int32, "count")
    if cost.dim() in (4, 5):
        cost = cost.view(-1, cost.shape[-2], cost.shape[-1])
    P, gmax, nq = cost.shape
    if tuple(count.shape) != (P,):
        raise ValueError(f"lsap: count {tuple(count.shape)} does not have one entry per problem ({P})")
    dev = cost.device
    match = torch.empty((P, gmax), dtype=torch.int32, device=dev)
    assigned = torch.empty((P, nq), dtype=torch.int32, device=dev)
    status = torch.empty((P,), dtype=torch.int32, device=dev)
    _launch(dev, "lsap", lambda lib, stream: lib.bevmsda_lsap_f32(
        _ptr(cost), _ptr(count), P, gmax, nq, _ptr(match), _ptr(assigned), _ptr(status), stream), required=True)
    if check and P:
        bad = status.nonzero().flatten().tolist()
        if bad:
            raise ValueError(f"lsap: problems {bad} have status {status[bad].tolist()} (1: cost matrix with a non-finite entry)")
    return match, assigned, status


def det_loss(cls, box, gt, label, count, assigned, code_weights, factors, params=LossParams(), groups=1, grouped_entry=False,
             return_group_losses=False):
    """``bevmsda_det_loss_f32``: predictions, packed gt, ``assigned`` (L, bs, nq) int32 (0-based gt of each query, -1
    background), ``code_weights`` (code_size,) and ``factors`` (2,) fp32 on the device (classification averaging factor,
    positive count) -> ``(losses (L, 2), grad_cls (L, bs, nq, cls_out), grad_box (L, bs, nq, code_size))``, the gradients of
    ``losses[l, 0]`` / ``losses[l, 1]`` with respect to the layer's logits / box codes.  ``groups > 1``
    (``bevmsda_det_loss_grouped_f32``; ``grouped_entry``: that entry point for one group too): ``factors`` are ONE group's,
    ``losses`` the mean over the groups of each group's pair (``return_group_losses``: also those, (L, groups, 2))."""
    cls, box = _need(cls, torch.float32, "cls"), _need(box, torch.float32, "box")
    gt, label, count = _need(gt, torch.float32, "gt"), _need(label, torch.int32, "label"), _need(count, torch.int32, "count")
    assigned = _need(assigned, torch.int32, "assigned")
    code_weights, factors = _need(code_weights, torch.float32, "code_weights"), _need(factors, torch.float32, "factors")
    L, bs, nq, cls_out, code, gmax = _shapes(cls, box, gt, label, count)
    if assigned.numel() != L * bs * nq or code_weights.numel() < code or factors.numel() != 2:
        raise ValueError("det_loss: assigned must be (L, bs, nq), code_weights (code_size,), factors (2,)")
    dev = cls.device
    losses = torch.zeros((L, 2), dtype=torch.float32, device=dev) if bs * nq == 0 else \
        torch.empty((L, 2), dtype=torch.float32, device=dev)
    grad_cls, grad_box = torch.empty_like(cls), torch.empty_like(box)
    groups, n = _per_group(nq, groups)
    if groups > 1 or grouped_entry:
        group_losses = torch.zeros((L, groups, 2), dtype=torch.float32, device=dev) if bs * nq == 0 else \
            torch.empty((L, groups, 2), dtype=torch.float32, device=dev)
        desc = _group_desc(L, bs, groups, n, cls_out, code, gmax, params)
        _launch(dev, "det_loss (grouped)", lambda lib, stream: lib.bevmsda_det_loss_grouped_f32(
            _ptr(cls), _ptr(box), _ptr(gt), _ptr(label), _ptr(count), _ptr(assigned), _ptr(code_weights), _ptr(factors),
            ctypes.byref(desc), _ptr(group_losses), _ptr(losses), _ptr(grad_cls), _ptr(grad_box), stream), required=True)
        return (losses, grad_cls, grad_box, group_losses) if return_group_losses else (losses, grad_cls, grad_box)
    if return_group_losses:
        raise ValueError("det_loss: return_group_losses needs the grouped entry point")
    desc = _desc(L, bs, nq, cls_out, code, gmax, params)
    _launch(dev, "det_loss", lambda lib, stream: lib.bevmsda_det_loss_f32(
        _ptr(cls), _ptr(box), _ptr(gt), _ptr(label), _ptr(count), _ptr(assigned), _ptr(code_weights), _ptr(factors),
        ctypes.byref(desc), _ptr(losses), _ptr(grad_cls), _ptr(grad_box), stream), required=True)
    return losses, grad_cls, grad_box


def loss_factors(count, nq, bs, bg_cls_weight=0.0, sync=False):
    """The two averaging factors of ``loss_single`` (bevformer_head.py:362-376) as a (2,) fp32 DEVICE tensor, from the device
    counts: ``max(num_pos + num_neg * bg_cls_weight, 1)`` — averaged over the ranks first when ``sync`` and
    ``torch.distributed`` is initialised — and ``max(mean over ranks of num_pos, 1)``.  No host read."""
    import torch.distributed as dist
    pos = count.clamp(min=0, max=nq).sum().to(torch.float32)
    f = torch.stack([pos + (float(bs * nq) - pos) * float(bg_cls_weight), pos])
    if dist.is_available() and dist.is_initialized():
        g = f / dist.get_world_size()
        dist.all_reduce(g)
        f = g if sync else torch.stack([f[0], g[1]])
    return f.clamp(min=1.0)


class _DetectionLoss(Function):
    @staticmethod
    def forward(ctx, cls, box, gt, label, count, count_rep, code_weights, factors, params, groups=1):
        cost = match_cost(cls, box, gt, label, count, params, groups=groups)
        _, assigned, status = lsap(cost, count_rep)
        losses, grad_cls, grad_box = det_loss(cls, box, gt, label, count, assigned, code_weights, factors, params, groups=groups)
        ctx.save_for_backward(grad_cls, grad_box)
        assigned = assigned.view(cls.shape[0], cls.shape[1], cls.shape[2])
        ctx.mark_non_differentiable(assigned, status)
        return losses, assigned, status

    @staticmethod
    @once_differentiable
    def backward(ctx, g_losses, _a, _s):
        grad_cls, grad_box = ctx.saved_tensors
        g = g_losses.to(torch.float32)
        return (grad_cls * g[:, 0].view(-1, 1, 1, 1), grad_box * g[:, 1].view(-1, 1, 1, 1), None, None, None, None, None, None,
                None, None)


def detection_loss(cls, box, gt, label, count, code_weights, factors=None, params=LossParams(), count_rep=None,
                   bg_cls_weight=0.0, sync_cls_avg_factor=False, return_assigned=False, groups=1):
    """The detection loss of all decoder layers: ``cls`` (L, bs, nq, cls_out), ``box`` (L, bs, nq, code_size), packed gt
    (``pack_gt``) -> ``losses`` (L, 2): (loss_cls, loss_bbox) per layer, differentiable with respect to ``cls`` and ``box``
    (the backward multiplies the saved unit gradients by the upstream (L, 2) gradient).  Three kernel launches — costs,
    assignment, loss — and no host read, so the call can be captured in a HIP graph; gt, label and count are read when the
    kernels run, a replay follows their contents.  ``factors``: the (2,) device averaging factors (default:
    ``loss_factors`` of the counts); ``count_rep``: ``count`` repeated per layer, (L * bs,).  ``return_assigned``: also the
    (L, bs, nq) int32 assignment (-1 background) and the solver's (L * bs,) status.  ``groups > 1``: Group-DETR (module
    docstring) — four launches, the factors are one group's (from ``nq // groups``), ``count_rep`` is per problem,
    (L * bs * groups,): ``count[(p // groups) % bs]``, and the status is (L * bs * groups,)."""
    L, bs, nq = cls.shape[:3]
    groups, n = _per_group(nq, groups)
    if factors is None:
        factors = loss_factors(count, n, bs, bg_cls_weight, sync_cls_avg_factor)
    if count_rep is None:
        count_rep = count.repeat(L) if groups == 1 else count.repeat_interleave(groups).repeat(L)
    losses, assigned, status = _DetectionLoss.apply(cls, box, gt, label, count, count_rep, code_weights, factors, params, groups)
    return (losses, assigned, status) if return_assigned else losses


def _is(m, name):
    return m is not None and type(m).__name__ == name


def detection_loss_reject(loss_cls, loss_bbox, assigner, code_size, cls_out):
    """Why the modules of a head are not what ``detection_loss`` computes (a short reason), or ``None`` when they are:
    ``FocalLoss`` (sigmoid, mean) + ``L1Loss`` (mean), an assigner with ``FocalLossCost`` + ``BBox3DL1Cost``, ``code_size``
    8 or 10, ``cls_out`` <= 32.  By class name and attributes: with mmdet installed the classes are its own."""
    if not _is(loss_cls, "FocalLoss") or not getattr(loss_cls, "use_sigmoid", False) or getattr(loss_cls, "reduction", "mean") != "mean":
        return "loss_cls is not a sigmoid FocalLoss with mean reduction"
    if not _is(loss_bbox, "L1Loss") or getattr(loss_bbox, "reduction", "mean") != "mean":
        return "loss_bbox is not an L1Loss with mean reduction"
    if not _is(getattr(assigner, "cls_cost", None), "FocalLossCost") or not _is(getattr(assigner, "reg_cost", None), "BBox3DL1Cost"):
        return "the assigner's costs are not FocalLossCost + BBox3DL1Cost"
    if code_size not in LOSS_CODE_SIZES:
        return f"code_size {code_size} is not 8 or 10"
    if not 1 <= cls_out <= LOSS_MAX_CLS_OUT:
        return f"cls_out {cls_out} is outside 1 .. {LOSS_MAX_CLS_OUT}"
    return None


def head_loss_params(head):
    """``LossParams`` of a head's assigner and loss modules."""
    cc, rc, lc, lb = head.assigner.cls_cost, head.assigner.reg_cost, head.loss_cls_fn, head.loss_bbox_fn
    return LossParams(cost_cls_weight=cc.weight, cost_reg_weight=rc.weight, cost_alpha=cc.alpha, cost_gamma=cc.gamma,
                      cost_eps=cc.eps, loss_alpha=lc.alpha, loss_gamma=lc.gamma, loss_cls_weight=lc.loss_weight,
                      loss_box_weight=lb.loss_weight)


def detection_loss_head(head, all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list, return_assigned=False):
    """``BEVFormerHead.loss`` through ``detection_loss``: packs the gt lists (host lengths -> the device count vector) and
    returns ``losses`` (L, 2).  A head with ``group_detr`` (``BEVFormerHead_GroupDETR``) gives the groups."""
    dev = all_cls_scores.device
    gt, label, count = pack_gt(gt_bboxes_list, gt_labels_list, dev)
    return detection_loss(all_cls_scores, all_bbox_preds, gt, label, count, head.code_weights.detach(),
                          params=head_loss_params(head), bg_cls_weight=head.bg_cls_weight,
                          sync_cls_avg_factor=head.sync_cls_avg_factor, return_assigned=return_assigned,
                          groups=getattr(head, "group_detr", 1))
