"""The detection loss's building blocks: box normalisation, match costs, the Hungarian assigner and the two loss modules.

``normalize_bbox`` is core/bbox/util.py:4-24 of the reference, ``BBox3DL1Cost`` core/bbox/match_costs/match_cost.py:6-28 and
``HungarianAssigner3D`` core/bbox/assigners/hungarian_assigner_3d.py:16-136, statement for statement.  ``FocalLossCost``,
``FocalLoss`` and ``L1Loss`` are mmdet's (third party, mmdet 2.14.0, docs/install.md:33; not in the reference tree): with
mmdet installed theirs are used and nothing below is registered.  Without it, these restatements — from the published
behaviour of the classes, NOT pinned against their source — let the reference's ``train_cfg`` and loss blocks build
stand-alone.  ``PseudoSampler`` is a ``nonzero`` of the assignment and has no class here.

This is the default path of ``BEVFormerHead.loss``; it runs on the CPU and the GPU and synchronises with the host once per
decoder layer and sample (scipy's ``linear_sum_assignment``).  The device-side path is ``ops.detection_loss`` (opt-in,
``modes.loss_fused``)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..registry import BBOX_ASSIGNERS, HAVE_MMDET, LOSSES, MATCH_COST, build_match_cost

try:
    from scipy.optimize import linear_sum_assignment
except ImportError:
    linear_sum_assignment = None


def normalize_bbox(bboxes, pc_range=None):
    """core/bbox/util.py:4-24: (cx, cy, cz, w, l, h, rot[, vx, vy]) -> (cx, cy, log w, log l, cz, log h, sin, cos[, vx, vy])."""
    cx = bboxes[..., 0:1]
    cy = bboxes[..., 1:2]
    cz = bboxes[..., 2:3]
    w = bboxes[..., 3:4].log()
    l = bboxes[..., 4:5].log()
    h = bboxes[..., 5:6].log()
    rot = bboxes[..., 6:7]
    if bboxes.size(-1) > 7:
        vx = bboxes[..., 7:8]
        vy = bboxes[..., 8:9]
        return torch.cat((cx, cy, w, l, cz, h, rot.sin(), rot.cos(), vx, vy), dim=-1)
    return torch.cat((cx, cy, w, l, cz, h, rot.sin(), rot.cos()), dim=-1)


class BBox3DL1Cost:
    """match_cost.py:6-28: ``cdist(p=1)`` of (num_query, k) predictions and (num_gt, k) targets, times ``weight``."""

    def __init__(self, weight=1.0):
        self.weight = weight

    def __call__(self, bbox_pred, gt_bboxes):
        bbox_cost = torch.cdist(bbox_pred, gt_bboxes, p=1)
        return bbox_cost * self.weight


class FocalLossCost:
    """mmdet's ``FocalLossCost`` [third party, restated from its published behaviour]: (num_query, num_class) logits and
    (num_gt,) labels -> (num_query, num_gt) ``(pos - neg)[:, gt_labels] * weight``."""

    def __init__(self, weight=1.0, alpha=0.25, gamma=2, eps=1e-12):
        self.weight = weight
        self.alpha = alpha
        self.gamma = gamma
        self.eps = eps

    def __call__(self, cls_pred, gt_labels):
        cls_pred = cls_pred.sigmoid()
        neg_cost = -(1 - cls_pred + self.eps).log() * (1 - self.alpha) * cls_pred.pow(self.gamma)
        pos_cost = -(cls_pred + self.eps).log() * self.alpha * (1 - cls_pred).pow(self.gamma)
        cls_cost = pos_cost[:, gt_labels] - neg_cost[:, gt_labels]
        return cls_cost * self.weight


class AssignResult:
    """What ``HungarianAssigner3D.assign`` returns (mmdet's ``AssignResult``, the fields this path reads): ``gt_inds`` is 0 for
    background and the 1-based gt index otherwise, ``labels`` the assigned gt's label, -1 for background."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts = num_gts
        self.gt_inds = gt_inds
        self.max_overlaps = max_overlaps
        self.labels = labels


class HungarianAssigner3D:
    """hungarian_assigner_3d.py:16-136.  ``iou_cost`` is accepted and unused, as in the reference (its config is a
    weight-0 placeholder).  scipy's ``ValueError`` on a cost matrix with a non-finite entry propagates."""

    def __init__(self, cls_cost=dict(type="ClassificationCost", weight=1.0), reg_cost=dict(type="BBoxL1Cost", weight=1.0),
                 iou_cost=dict(type="IoUCost", weight=0.0), pc_range=None):
        self.cls_cost = build_match_cost(cls_cost)
        self.reg_cost = build_match_cost(reg_cost)
        self.iou_cost_cfg = iou_cost
        self.pc_range = pc_range

    def cost(self, bbox_pred, cls_pred, gt_bboxes, gt_labels):
        """The (num_query, num_gt) cost matrix of :106-115."""
        cls_cost = self.cls_cost(cls_pred, gt_labels)
        normalized_gt_bboxes = normalize_bbox(gt_bboxes, self.pc_range)
        reg_cost = self.reg_cost(bbox_pred[:, :8], normalized_gt_bboxes[:, :8])
        return cls_cost + reg_cost

    def assign(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, gt_bboxes_ignore=None, eps=1e-7):
        assert gt_bboxes_ignore is None, "Only case when gt_bboxes_ignore is None is supported."
        num_gts, num_bboxes = gt_bboxes.size(0), bbox_pred.size(0)
        assigned_gt_inds = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        assigned_labels = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        if num_gts == 0 or num_bboxes == 0:
            if num_gts == 0:
                assigned_gt_inds[:] = 0
            return AssignResult(num_gts, assigned_gt_inds, None, labels=assigned_labels)
        cost = self.cost(bbox_pred, cls_pred, gt_bboxes, gt_labels)
        cost = cost.detach().cpu()
        if linear_sum_assignment is None:
            raise ImportError('Please run "pip install scipy" to install scipy first.')
        matched_row_inds, matched_col_inds = linear_sum_assignment(cost)
        matched_row_inds = torch.from_numpy(matched_row_inds).to(bbox_pred.device)
        matched_col_inds = torch.from_numpy(matched_col_inds).to(bbox_pred.device)
        assigned_gt_inds[:] = 0
        assigned_gt_inds[matched_row_inds] = matched_col_inds + 1
        assigned_labels[matched_row_inds] = gt_labels[matched_col_inds]
        return AssignResult(num_gts, assigned_gt_inds, None, labels=assigned_labels)


def sigmoid_focal_loss(pred, target, gamma=2.0, alpha=0.25):
    """Sigmoid focal loss per element: (N, C) logits, (N,) labels in [0, C] (C = background: an all-zero one-hot row)."""
    num_classes = pred.size(1)
    target = F.one_hot(target, num_classes=num_classes + 1)[:, :num_classes].type_as(pred)
    pred_sigmoid = pred.sigmoid()
    pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    return F.binary_cross_entropy_with_logits(pred, target, reduction="none") * focal_weight


class FocalLoss(nn.Module):
    """mmdet's ``FocalLoss`` [third party, restated from its published behaviour], the 'mean' reduction with an
    ``avg_factor``: ``loss_weight * sum(focal * weight[:, None]) / avg_factor``."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0):
        super().__init__()
        assert use_sigmoid is True, "Only sigmoid focal loss supported now."
        if reduction != "mean":
            raise NotImplementedError(f"FocalLoss: reduction {reduction!r} is not implemented (the head uses 'mean')")
        self.use_sigmoid = use_sigmoid
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        loss = sigmoid_focal_loss(pred, target, self.gamma, self.alpha)
        if weight is not None:
            loss = loss * weight.view(-1, 1)
        loss = loss.sum() / avg_factor if avg_factor is not None else loss.mean()
        return self.loss_weight * loss


class L1Loss(nn.Module):
    """mmdet's ``L1Loss`` [third party, restated]: ``loss_weight * sum(|pred - target| * weight) / avg_factor``; an empty
    target gives ``pred.sum() * 0``."""

    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError(f"L1Loss: reduction {reduction!r} is not implemented (the head uses 'mean')")
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        if target.numel() == 0:
            return self.loss_weight * (pred.sum() * 0)
        loss = torch.abs(pred - target)
        if weight is not None:
            loss = loss * weight
        loss = loss.sum() / avg_factor if avg_factor is not None else loss.mean()
        return self.loss_weight * loss


def reduce_mean(tensor):
    """mmdet's ``reduce_mean``: the mean over the ranks when ``torch.distributed`` is initialised, else the tensor."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return tensor
    tensor = tensor.clone()
    dist.all_reduce(tensor.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return tensor


if not HAVE_MMDET:      # with mmdet the assigner is the plugin's own class, the costs and losses are mmdet's
    BBOX_ASSIGNERS.register_module(name="HungarianAssigner3D", module=HungarianAssigner3D, force=True)
    MATCH_COST.register_module(name="BBox3DL1Cost", module=BBox3DL1Cost, force=True)
    MATCH_COST.register_module(name="FocalLossCost", module=FocalLossCost, force=True)
    LOSSES.register_module(name="FocalLoss", module=FocalLoss, force=True)
    LOSSES.register_module(name="L1Loss", module=L1Loss, force=True)
