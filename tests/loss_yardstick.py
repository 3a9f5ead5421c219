"""The yardstick of the detection-loss tests: a plain-torch restatement of the reference's loss
(dense_heads/bevformer_head.py:214-393, core/bbox/assigners/hungarian_assigner_3d.py:106-134, core/bbox/util.py:4-24) with
mmdet's focal cost, focal loss and L1 loss [third party, restated from their published behaviour].  It runs in whatever
dtype its inputs have (float32 or float64), on the CPU, uses scipy for the assignment and nothing of the product package."""
import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

CFG = dict(cost_cls_weight=2.0, cost_reg_weight=0.25, cost_alpha=0.25, cost_gamma=2.0, cost_eps=1e-12, loss_alpha=0.25,
           loss_gamma=2.0, loss_cls_weight=2.0, loss_box_weight=0.25)       # bevformer_base.py:139-160
CODE_WEIGHTS = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]


def normalize_bbox(b):
    parts = [b[..., 0:1], b[..., 1:2], b[..., 3:4].log(), b[..., 4:5].log(), b[..., 2:3], b[..., 5:6].log(),
             b[..., 6:7].sin(), b[..., 6:7].cos()]
    if b.size(-1) > 7:
        parts += [b[..., 7:8], b[..., 8:9]]
    return torch.cat(parts, dim=-1)


def focal_cost(cls_pred, gt_labels, cfg=CFG):
    p = cls_pred.sigmoid()
    neg = -(1 - p + cfg["cost_eps"]).log() * (1 - cfg["cost_alpha"]) * p.pow(cfg["cost_gamma"])
    pos = -(p + cfg["cost_eps"]).log() * cfg["cost_alpha"] * (1 - p).pow(cfg["cost_gamma"])
    return (pos[:, gt_labels] - neg[:, gt_labels]) * cfg["cost_cls_weight"]


def cost_matrix(bbox_pred, cls_pred, gt_bboxes, gt_labels, cfg=CFG):
    """(num_query, num_gt), as the assigner builds it."""
    cls_cost = focal_cost(cls_pred, gt_labels, cfg)
    reg_cost = torch.cdist(bbox_pred[:, :8], normalize_bbox(gt_bboxes)[:, :8], p=1) * cfg["cost_reg_weight"]
    return cls_cost + reg_cost


def assign_from_cost(cost):
    """(num_query, num_gt) cost -> gt_inds (num_query,) int64: 0 background, else the 1-based gt index."""
    gt_inds = torch.zeros(cost.shape[0], dtype=torch.long)
    if cost.shape[1] == 0 or cost.shape[0] == 0:
        return gt_inds
    rows, cols = linear_sum_assignment(cost.detach().cpu().numpy())
    gt_inds[torch.from_numpy(rows)] = torch.from_numpy(cols) + 1
    return gt_inds


def assign(bbox_pred, cls_pred, gt_bboxes, gt_labels, cfg=CFG):
    if gt_bboxes.shape[0] == 0:
        return torch.zeros(bbox_pred.shape[0], dtype=torch.long)
    return assign_from_cost(cost_matrix(bbox_pred, cls_pred, gt_bboxes, gt_labels, cfg))


def focal_loss(pred, labels, avg_factor, cfg=CFG):
    C = pred.size(1)
    target = F.one_hot(labels, num_classes=C + 1)[:, :C].type_as(pred)
    p = pred.sigmoid()
    pt = (1 - p) * target + p * (1 - target)
    fw = (cfg["loss_alpha"] * target + (1 - cfg["loss_alpha"]) * (1 - target)) * pt.pow(cfg["loss_gamma"])
    loss = F.binary_cross_entropy_with_logits(pred, target, reduction="none") * fw
    return cfg["loss_cls_weight"] * (loss.sum() / avg_factor)


def l1_loss(pred, target, weight, avg_factor, cfg=CFG):
    if target.numel() == 0:
        return cfg["loss_box_weight"] * (pred.sum() * 0)
    return cfg["loss_box_weight"] * ((torch.abs(pred - target) * weight).sum() / avg_factor)


def loss_single(cls_scores, bbox_preds, gt_bboxes_list, gt_labels_list, code_weights, cfg=CFG, gt_inds_list=None,
                factors=None):
    """One decoder layer: ``cls_scores`` (bs, nq, C), ``bbox_preds`` (bs, nq, code) -> (loss_cls, loss_bbox, gt_inds per
    sample).  ``gt_inds_list``: assignments to use instead of solving; ``factors``: (cls_avg_factor, num_total_pos) to use
    instead of ``max(num_pos, 1)``."""
    bs, nq, C = cls_scores.shape
    labels, targets, weights, inds = [], [], [], []
    num_pos = 0
    for i in range(bs):
        gt, lab = gt_bboxes_list[i].to(bbox_preds.dtype), gt_labels_list[i]
        gi = gt_inds_list[i] if gt_inds_list is not None else assign(bbox_preds[i].detach(), cls_scores[i].detach(), gt, lab, cfg)
        inds.append(gi)
        pos = torch.nonzero(gi > 0).squeeze(-1)
        num_pos += pos.numel()
        l = torch.full((nq,), C, dtype=torch.long)
        l[pos] = lab[gi[pos] - 1]
        t = torch.zeros_like(bbox_preds[i])[..., :gt.shape[-1]]
        w = torch.zeros_like(bbox_preds[i])
        w[pos] = 1.0
        if pos.numel():
            t[pos] = gt[gi[pos] - 1]
        labels.append(l)
        targets.append(t)
        weights.append(w)
    labels, targets, weights = torch.cat(labels), torch.cat(targets), torch.cat(weights)
    cls_avg, box_avg = factors if factors is not None else (max(num_pos * 1.0, 1), max(num_pos, 1))
    loss_cls = focal_loss(cls_scores.reshape(-1, C), labels, cls_avg, cfg)
    preds = bbox_preds.reshape(-1, bbox_preds.size(-1))
    nt = normalize_bbox(targets)
    ok = torch.isfinite(nt).all(dim=-1)
    weights = weights * code_weights.to(weights.dtype)
    loss_bbox = l1_loss(preds[ok, :10], nt[ok, :10], weights[ok, :10], box_avg, cfg)
    return torch.nan_to_num(loss_cls), torch.nan_to_num(loss_bbox), inds


def loss(all_cls, all_box, gt_bboxes_list, gt_labels_list, code_weights, cfg=CFG, gt_inds=None, factors=None):
    """All layers -> (dict with the reference's keys, [per layer [per sample gt_inds]])."""
    L = all_cls.shape[0]
    per = [loss_single(all_cls[l], all_box[l], gt_bboxes_list, gt_labels_list, code_weights, cfg,
                       None if gt_inds is None else gt_inds[l], factors) for l in range(L)]
    out = {"loss_cls": per[-1][0], "loss_bbox": per[-1][1]}
    for l in range(L - 1):
        out[f"d{l}.loss_cls"], out[f"d{l}.loss_bbox"] = per[l][0], per[l][1]
    return out, [p[2] for p in per]


def loss_with_grads(all_cls, all_box, gts, labels, code_weights, cfg=CFG, gt_inds=None, factors=None, dtype=torch.float64):
    """The yardstick in ``dtype`` on the given (fp32) inputs -> (losses (L, 2), grad of sum(losses) wrt all_cls, wrt all_box,
    gt_inds).  Each layer's losses depend on that layer's predictions only, so the gradient of the sum is also the per-layer
    unit gradient."""
    c = all_cls.detach().cpu().to(dtype).requires_grad_(True)
    b = all_box.detach().cpu().to(dtype).requires_grad_(True)
    g = [x.detach().cpu().to(dtype) for x in gts]
    lab = [x.detach().cpu().long() for x in labels]
    d, inds = loss(c, b, g, lab, torch.as_tensor(code_weights, dtype=dtype), cfg, gt_inds, factors)
    L = c.shape[0]
    keys = [(f"d{l}.loss_cls", f"d{l}.loss_bbox") for l in range(L - 1)] + [("loss_cls", "loss_bbox")]
    losses = torch.stack([torch.stack([d[k0], d[k1]]) for k0, k1 in keys])
    cls_total, box_total = losses[:, 0].sum(), losses[:, 1].sum()
    gc = torch.autograd.grad(cls_total, c, retain_graph=True)[0]
    gb = torch.autograd.grad(box_total, b, allow_unused=True)[0]
    gb = torch.zeros_like(b) if gb is None else gb
    return losses.detach(), gc, gb, inds


def make_preds(seed, L, bs, nq, cls_out=10, code_size=10, logit_scale=3.0, extremes=True):
    """Seeded predictions in the head's output format: logits (a few pushed out to +-30), box codes with centres in the base
    pc_range, log sizes, (sin, cos) and velocities."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(L, bs, nq, cls_out, generator=g) * logit_scale - 2.0
    if extremes and cls.numel() >= 8:
        flat = cls.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:max(4, flat.numel() // 50)]
        flat[idx] = torch.where(torch.arange(idx.numel()) % 2 == 0, 30.0, -30.0) * (0.5 + 0.5 * torch.rand(idx.numel(), generator=g))
        flat[idx[0]], flat[idx[1]] = 30.0, -30.0
    box = torch.randn(L, bs, nq, code_size, generator=g)
    box[..., 0:2] = (torch.rand(L, bs, nq, 2, generator=g) * 2 - 1) * 51.2
    box[..., 4] = torch.rand(L, bs, nq, generator=g) * 8 - 5
    return cls, box


def matching_total(cost_rows, match):
    """Sum in fp64, in column (query) order, of ``cost_rows[g, match[g]]`` for a (G, nq) fp32 matrix."""
    c = np.asarray(cost_rows, dtype=np.float64)
    total = 0.0
    for q, g in sorted((int(q), g) for g, q in enumerate(match)):
        total += c[g, q]
    return total
