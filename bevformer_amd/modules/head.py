"""The detection head: states of the decoder in, boxes out (inference).

``BEVFormerHead`` and ``NMSFreeCoder`` with the registry names, constructor arguments, ``state_dict`` keys and method
contracts of projects/mmdet3d_plugin/bevformer/dense_heads/bevformer_head.py:16-213,482-509 and
projects/mmdet3d_plugin/core/bbox/coders/nms_free_coder.py; ``denormalize_bbox`` of core/bbox/util.py:26-53.  ``loss``
follows bevformer_head.py:214-480 on the assigner, match costs and loss modules of modules/loss.py when the head is built with
a ``train_cfg`` that holds an ``assigner``; ``as_two_stage`` is not here.

``BEVFormerHead_GroupDETR`` (bevformer_head.py:512-683, the head of every bevformerv2 config): ``group_detr`` groups of
``num_query`` object queries in training — each group matched against the gt on its own, the loss their mean — and the first
group alone at inference.

With ``modes.head_fused`` (opt-in) and the stock branches, ``forward`` runs every layer's classification and regression
branch with the reference-point arithmetic in ONE launch (``ops.head_branches``, csrc/head_branch.h) and ``get_bboxes``
selects, denormalises and masks in one kernel (``ops.nms_free_decode``, csrc/head_decode.h); the only host synchronisation
left is the final variable-length slice, as in the reference.  With the switch off the statements below are the reference's.

With ``modes.loss_fused`` (opt-in) ``loss`` runs on the device in three launches without a host read
(``ops.detection_loss``: csrc/det_cost.h, match_lsap.h, det_loss.h) where ``loss_fused_reject`` finds the call covered;
the Group-DETR head's in four (``groups=group_detr``: every group's problems in the same launches, then the means).
"""
import copy
import math

import torch
import torch.nn as nn

from .. import ops
from ..registry import (BBOX_CODERS, HAVE_MMCV, HAVE_MMDET, HEADS, POSITIONAL_ENCODING, BaseModule, auto_fp16,
                        build_assigner, build_bbox_coder, build_loss, build_positional_encoding, build_transformer, force_fp32)
from .decoder import inverse_sigmoid
from .loss import normalize_bbox, reduce_mean


def denormalize_bbox(normalized_bboxes, pc_range=None):
    """core/bbox/util.py:26-53: (cx, cy, w, l, cz, h, sin, cos[, vx, vy]) -> (cx, cy, cz, exp w, exp l, exp h, rot[, vx, vy])."""
    rot = torch.atan2(normalized_bboxes[..., 6:7], normalized_bboxes[..., 7:8])
    cx, cy, cz = normalized_bboxes[..., 0:1], normalized_bboxes[..., 1:2], normalized_bboxes[..., 4:5]
    w, l, h = normalized_bboxes[..., 2:3].exp(), normalized_bboxes[..., 3:4].exp(), normalized_bboxes[..., 5:6].exp()
    if normalized_bboxes.size(-1) > 8:
        return torch.cat([cx, cy, cz, w, l, h, rot, normalized_bboxes[:, 8:9], normalized_bboxes[:, 9:10]], dim=-1)
    return torch.cat([cx, cy, cz, w, l, h, rot], dim=-1)


class NMSFreeCoder:
    """nms_free_coder.py:10-121.  ``decode_padded`` is the fixed-shape form on the HIP kernel."""

    def __init__(self, pc_range, voxel_size=None, post_center_range=None, max_num=100, score_threshold=None, num_classes=10):
        self.pc_range = pc_range
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.num_classes = num_classes
        self._range_tensor = None

    def encode(self):
        pass

    def decode_single(self, cls_scores, bbox_preds):
        """cls_scores (num_query, cls_out), bbox_preds (num_query, code_size) -> dict(bboxes, scores, labels)."""
        max_num = self.max_num
        cls_scores = cls_scores.sigmoid()
        scores, indexs = cls_scores.view(-1).topk(max_num)
        labels = indexs % self.num_classes
        bbox_index = indexs // self.num_classes
        bbox_preds = bbox_preds[bbox_index]
        final_box_preds = denormalize_bbox(bbox_preds, self.pc_range)
        final_scores = scores
        final_preds = labels
        if self.score_threshold is not None:
            thresh_mask = final_scores > self.score_threshold
            tmp_score = self.score_threshold
            while thresh_mask.sum() == 0:
                tmp_score *= 0.9
                if tmp_score < 0.01:
                    thresh_mask = final_scores > -1
                    break
                thresh_mask = final_scores >= tmp_score
        if self.post_center_range is None:
            raise NotImplementedError("Need to reorganize output as a batch, only support post_center_range is not None for now!")
        # (the reference replaces self.post_center_range by a tensor on first use; the list is kept here, the tensor beside it)
        post_center_range = self._range_tensor
        if post_center_range is None or post_center_range.device != scores.device:
            post_center_range = self._range_tensor = torch.tensor(self.post_center_range, device=scores.device)
        mask = (final_box_preds[..., :3] >= post_center_range[:3]).all(1)
        mask &= (final_box_preds[..., :3] <= post_center_range[3:]).all(1)
        if self.score_threshold:
            mask &= thresh_mask
        return {"bboxes": final_box_preds[mask], "scores": final_scores[mask], "labels": final_preds[mask]}

    def decode_padded(self, preds_dicts):
        """The last layer's predictions through ``ops.nms_free_decode``: ``(scores (bs, max_num), labels, boxes (bs, max_num,
        code_size - 1), keep (bs, max_num) bool, count (bs,) int32)`` — rank r is the r-th largest logit, ``keep`` the
        reference's mask; nothing is read back by the host.  ``None`` when the kernel does not cover the call."""
        if self.post_center_range is None:
            return None
        return ops.nms_free_decode(preds_dicts["all_cls_scores"][-1], preds_dicts["all_bbox_preds"][-1], max_num=self.max_num,
                                   post_center_range=[float(v) for v in self.post_center_range],
                                   score_threshold=self.score_threshold, num_classes=self.num_classes)

    def decode(self, preds_dicts):
        """-> list (one per batch entry) of dict(bboxes, scores, labels).  With ``modes.head_fused``: the kernel's padded result
        sliced by its mask — the one place that synchronises, as the reference's boolean slice does."""
        if ops.modes().head_fused:
            padded = self.decode_padded(preds_dicts)
            if padded is not None:
                scores, labels, boxes, keep, _ = padded
                return [{"bboxes": boxes[i][keep[i]], "scores": scores[i][keep[i]], "labels": labels[i][keep[i]]}
                        for i in range(scores.shape[0])]
        all_cls_scores = preds_dicts["all_cls_scores"][-1]
        all_bbox_preds = preds_dicts["all_bbox_preds"][-1]
        return [self.decode_single(all_cls_scores[i], all_bbox_preds[i]) for i in range(all_cls_scores.size()[0])]


# ---------------------------------------------------------------------------
# mmdet's ``LearnedPositionalEncoding`` (the configs' ``positional_encoding``, bevformer_base.py:135-140) is third-party and
# does not live in the reference tree (mmdet 2.14.0, docs/install.md:33); with mmcv / mmdet installed theirs is used and
# nothing below is registered.  Without them, this restatement — from the published behaviour of the class, NOT pinned
# against its source (third-party, absent) — lets the reference's head config build stand-alone.
# ---------------------------------------------------------------------------
class LearnedPositionalEncoding(BaseModule):
    """Row and column embeddings, concatenated per cell: mask (bs, h, w) -> (bs, 2 * num_feats, h, w); parameters
    ``row_embed.weight`` / ``col_embed.weight``, initialised uniform in [0, 1)."""

    def __init__(self, num_feats, row_num_embed=50, col_num_embed=50, init_cfg=dict(type="Uniform", layer="Embedding")):
        super().__init__(init_cfg)
        self.row_embed = nn.Embedding(row_num_embed, num_feats)
        self.col_embed = nn.Embedding(col_num_embed, num_feats)
        self.num_feats = num_feats
        self.row_num_embed = row_num_embed
        self.col_num_embed = col_num_embed

    def init_weights(self):
        nn.init.uniform_(self.row_embed.weight)
        nn.init.uniform_(self.col_embed.weight)
        self._is_init = True

    def forward(self, mask):
        h, w = mask.shape[-2:]
        x_embed = self.col_embed(torch.arange(w, device=mask.device))
        y_embed = self.row_embed(torch.arange(h, device=mask.device))
        pos = torch.cat((x_embed.unsqueeze(0).repeat(h, 1, 1), y_embed.unsqueeze(1).repeat(1, w, 1)), dim=-1)
        return pos.permute(2, 0, 1).unsqueeze(0).repeat(mask.shape[0], 1, 1, 1)


def bias_init_with_prob(prior_prob):
    """mmcv.cnn.bias_init_with_prob [third party, restated]: the bias whose sigmoid is ``prior_prob``."""
    return float(-math.log((1 - prior_prob) / prior_prob))


def _build_module(cfg, builder):
    return cfg if cfg is None or isinstance(cfg, nn.Module) or not isinstance(cfg, dict) else builder(cfg)


class BEVFormerHead(BaseModule):
    """bevformer_head.py:16-213 + :482-509, and ``loss`` (:214-480).  Arguments as the reference's (``DETRHead``'s that
    matter: ``num_classes``, ``in_channels``, ``num_query``, ``num_reg_fcs``, ``transformer``, ``positional_encoding``; the
    ``loss_*`` config dicts are kept under their names, ``loss_cls['use_sigmoid']`` gives ``cls_out_channels``).  A
    ``train_cfg`` with an ``assigner`` makes the head trainable: ``self.assigner`` and the loss modules ``loss_cls_fn``
    (``FocalLoss``) / ``loss_bbox_fn`` (``L1Loss``) are built from the configs; any other loss type raises."""

    def __init__(self, num_classes, in_channels, num_query=100, num_reg_fcs=2, transformer=None, sync_cls_avg_factor=False,
                 positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                 loss_cls=dict(type="CrossEntropyLoss", bg_cls_weight=0.1, use_sigmoid=False, loss_weight=1.0, class_weight=1.0),
                 loss_bbox=dict(type="L1Loss", loss_weight=5.0), loss_iou=dict(type="GIoULoss", loss_weight=2.0),
                 train_cfg=None, test_cfg=None, init_cfg=None, with_box_refine=False, as_two_stage=False, bbox_coder=None,
                 num_cls_fcs=2, code_weights=None, bev_h=30, bev_w=30, code_size=10, **kwargs):
        super().__init__(init_cfg)
        if as_two_stage:
            raise NotImplementedError("BEVFormerHead: as_two_stage=True is not implemented (no reference config uses it)")
        self.bev_h, self.bev_w = bev_h, bev_w
        self.fp16_enabled = False
        self.with_box_refine = with_box_refine
        self.as_two_stage = as_two_stage
        self.code_size = code_size
        code_weights = code_weights if code_weights is not None else [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]
        self.bbox_coder = bbox_coder if not isinstance(bbox_coder, dict) else build_bbox_coder(bbox_coder)
        self.pc_range = self.bbox_coder.pc_range
        self.real_w = self.pc_range[3] - self.pc_range[0]
        self.real_h = self.pc_range[4] - self.pc_range[1]
        self.num_cls_fcs = num_cls_fcs - 1
        self.num_query = num_query
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.num_reg_fcs = num_reg_fcs
        self.sync_cls_avg_factor = sync_cls_avg_factor
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.loss_cls, self.loss_bbox, self.loss_iou = loss_cls, loss_bbox, loss_iou       # (the config dicts)
        self.bg_cls_weight = 0          # (bevformer_head.py / DETRHead: 0 for sigmoid classification without class_weight)
        self.assigner = self.loss_cls_fn = self.loss_bbox_fn = None
        if isinstance(train_cfg, dict) and train_cfg.get("assigner") is not None:
            for cfg, want in ((loss_cls, "FocalLoss"), (loss_bbox, "L1Loss")):
                typ = (cfg or {}).get("type")
                if typ != want:
                    raise NotImplementedError(f"BEVFormerHead.loss: loss type {typ!r} is not implemented (only {want})")
            assert loss_cls.get("use_sigmoid", False), "FocalLoss: only the sigmoid form is supported"
            self.assigner = build_assigner(train_cfg["assigner"])
            self.loss_cls_fn = build_loss(loss_cls)
            self.loss_bbox_fn = build_loss(loss_bbox)
        self.use_sigmoid_cls = bool((loss_cls or {}).get("use_sigmoid", False))
        self.cls_out_channels = num_classes if self.use_sigmoid_cls else num_classes + 1
        self.positional_encoding = _build_module(positional_encoding, build_positional_encoding)
        self.transformer = _build_module(transformer, build_transformer)
        self.embed_dims = self.transformer.embed_dims
        num_feats = (positional_encoding or {}).get("num_feats") if isinstance(positional_encoding, dict) else None
        assert num_feats is None or num_feats * 2 == self.embed_dims, \
            f"embed_dims should be exactly 2 times of num_feats. Found {self.embed_dims} and {num_feats}."
        self._init_layers()
        self.code_weights = nn.Parameter(torch.tensor(code_weights, requires_grad=False), requires_grad=False)

    def _init_layers(self):
        """bevformer_head.py:69-107."""
        cls_branch = []
        for _ in range(self.num_reg_fcs):
            cls_branch.append(nn.Linear(self.embed_dims, self.embed_dims))
            cls_branch.append(nn.LayerNorm(self.embed_dims))
            cls_branch.append(nn.ReLU(inplace=True))
        cls_branch.append(nn.Linear(self.embed_dims, self.cls_out_channels))
        fc_cls = nn.Sequential(*cls_branch)
        reg_branch = []
        for _ in range(self.num_reg_fcs):
            reg_branch.append(nn.Linear(self.embed_dims, self.embed_dims))
            reg_branch.append(nn.ReLU())
        reg_branch.append(nn.Linear(self.embed_dims, self.code_size))
        reg_branch = nn.Sequential(*reg_branch)
        num_pred = self.transformer.decoder.num_layers
        if self.with_box_refine:
            self.cls_branches = nn.ModuleList([copy.deepcopy(fc_cls) for _ in range(num_pred)])
            self.reg_branches = nn.ModuleList([copy.deepcopy(reg_branch) for _ in range(num_pred)])
        else:
            self.cls_branches = nn.ModuleList([fc_cls for _ in range(num_pred)])
            self.reg_branches = nn.ModuleList([reg_branch for _ in range(num_pred)])
        self.bev_embedding = nn.Embedding(self.bev_h * self.bev_w, self.embed_dims)
        self.query_embedding = nn.Embedding(self.num_query, self.embed_dims * 2)

    def init_weights(self):
        """bevformer_head.py:109-115."""
        self.transformer.init_weights()
        if hasattr(self.positional_encoding, "init_weights"):
            self.positional_encoding.init_weights()
        if self.use_sigmoid_cls:
            bias_init = bias_init_with_prob(0.01)
            for m in self.cls_branches:
                nn.init.constant_(m[-1].bias, bias_init)
        self._is_init = True

    def head_fused_reject(self, hs=None):
        """Why ``forward`` does not take ``ops.head_branches`` (a short reason), or ``None`` when it does.  The switch itself
        (``modes.head_fused``) is the caller's to test."""
        for b in self.cls_branches:
            why = ops.head_branch_reject(b, "cls")
            if why is not None:
                return "cls branch: " + why
        for b in self.reg_branches:
            why = ops.head_branch_reject(b, "reg")
            if why is not None:
                return "reg branch: " + why
        if torch.is_grad_enabled():
            return "gradient mode is on"
        if self.training:
            return "train() mode"
        if ops.gemm_mode() not in ("split", "bf16"):
            return "GEMM mode is not split / bf16"
        if hs is not None and (not hs.is_cuda or hs.dtype != torch.float32):
            return "not CUDA fp32 tensors"
        return None

    def object_query_embeds(self, dtype):
        """The (num_query, 2 * embed_dims) query embeddings ``forward`` hands to the transformer."""
        return self.query_embedding.weight.to(dtype)

    @auto_fp16(apply_to=("mlvl_feats"))
    def forward(self, mlvl_feats, img_metas, prev_bev=None, only_bev=False):
        """mlvl_feats: list of (bs, Nc, C, h, w) -> dict(bev_embed, all_cls_scores (L, bs, num_query, cls_out),
        all_bbox_preds (L, bs, num_query, code_size), enc_cls_scores=None, enc_bbox_preds=None); ``only_bev``: the BEV."""
        bs = mlvl_feats[0].shape[0]
        dtype = mlvl_feats[0].dtype
        object_query_embeds = self.object_query_embeds(dtype)
        bev_queries = self.bev_embedding.weight.to(dtype)
        bev_mask = torch.zeros((bs, self.bev_h, self.bev_w), device=bev_queries.device).to(dtype)
        bev_pos = self.positional_encoding(bev_mask).to(dtype)
        grid_length = (self.real_h / self.bev_h, self.real_w / self.bev_w)
        if only_bev:
            return self.transformer.get_bev_features(mlvl_feats, bev_queries, self.bev_h, self.bev_w, grid_length=grid_length,
                                                     bev_pos=bev_pos, img_metas=img_metas, prev_bev=prev_bev)
        outputs = self.transformer(mlvl_feats, bev_queries, object_query_embeds, self.bev_h, self.bev_w,
                                   grid_length=grid_length, bev_pos=bev_pos,
                                   reg_branches=self.reg_branches if self.with_box_refine else None,
                                   cls_branches=None, img_metas=img_metas, prev_bev=prev_bev)
        bev_embed, hs, init_reference, inter_references = outputs
        outputs_classes, outputs_coords = self.predictions(hs, init_reference, inter_references)
        return {"bev_embed": bev_embed, "all_cls_scores": outputs_classes, "all_bbox_preds": outputs_coords,
                "enc_cls_scores": None, "enc_bbox_preds": None}

    def predictions(self, hs, init_reference, inter_references):
        """bevformer_head.py:171-203: ``hs`` (L, num_query, bs, C) the decoder's states, ``init_reference`` (bs, num_query,
        3), ``inter_references`` (L, bs, num_query, 3) -> (all_cls_scores, all_bbox_preds)."""
        if ops.modes().head_fused and self.head_fused_reject(hs) is None:
            refs = torch.cat([init_reference[None], inter_references[:-1]], 0) if hs.shape[0] > 1 else init_reference[None]
            out = ops.head_branches(hs, refs, self.cls_branches, self.reg_branches, self.pc_range)
            if out is not None:
                return out
        hs = hs.permute(0, 2, 1, 3)
        outputs_classes, outputs_coords = [], []
        for lvl in range(hs.shape[0]):
            reference = init_reference if lvl == 0 else inter_references[lvl - 1]
            reference = inverse_sigmoid(reference)
            outputs_class = _run_branch(self.cls_branches[lvl], hs[lvl], "head_cls")
            tmp = _run_branch(self.reg_branches[lvl], hs[lvl], "head_reg")
            assert reference.shape[-1] == 3
            tmp[..., 0:2] += reference[..., 0:2]
            tmp[..., 0:2] = tmp[..., 0:2].sigmoid()
            tmp[..., 4:5] += reference[..., 2:3]
            tmp[..., 4:5] = tmp[..., 4:5].sigmoid()
            tmp[..., 0:1] = (tmp[..., 0:1] * (self.pc_range[3] - self.pc_range[0]) + self.pc_range[0])
            tmp[..., 1:2] = (tmp[..., 1:2] * (self.pc_range[4] - self.pc_range[1]) + self.pc_range[1])
            tmp[..., 4:5] = (tmp[..., 4:5] * (self.pc_range[5] - self.pc_range[2]) + self.pc_range[2])
            outputs_classes.append(outputs_class)
            outputs_coords.append(tmp)
        return torch.stack(outputs_classes), torch.stack(outputs_coords)

    def _get_target_single(self, cls_score, bbox_pred, gt_labels, gt_bboxes, gt_bboxes_ignore=None):
        """bevformer_head.py:214-270 (the ``PseudoSampler`` is the two ``nonzero`` calls)."""
        num_bboxes = bbox_pred.size(0)
        gt_c = gt_bboxes.shape[-1]
        assign_result = self.assigner.assign(bbox_pred, cls_score, gt_bboxes, gt_labels, gt_bboxes_ignore)
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        labels = gt_bboxes.new_full((num_bboxes,), self.num_classes, dtype=torch.long)
        labels[pos_inds] = gt_labels[pos_assigned_gt_inds]
        label_weights = gt_bboxes.new_ones(num_bboxes)
        bbox_targets = torch.zeros_like(bbox_pred)[..., :gt_c]
        bbox_weights = torch.zeros_like(bbox_pred)
        bbox_weights[pos_inds] = 1.0
        bbox_targets[pos_inds] = gt_bboxes[pos_assigned_gt_inds, :] if gt_bboxes.numel() else gt_bboxes.view(-1, gt_c)
        return labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds

    def loss_single(self, cls_scores, bbox_preds, gt_bboxes_list, gt_labels_list, gt_bboxes_ignore_list=None):
        """bevformer_head.py:325-393: one decoder layer's (loss_cls, loss_bbox)."""
        assert gt_bboxes_ignore_list is None, "Only supports for gt_bboxes_ignore setting to None."
        num_imgs = cls_scores.size(0)
        targets = [self._get_target_single(cls_scores[i], bbox_preds[i], gt_labels_list[i], gt_bboxes_list[i])
                   for i in range(num_imgs)]
        labels = torch.cat([t[0] for t in targets], 0)
        label_weights = torch.cat([t[1] for t in targets], 0)
        bbox_targets = torch.cat([t[2] for t in targets], 0)
        bbox_weights = torch.cat([t[3] for t in targets], 0)
        num_total_pos = sum(t[4].numel() for t in targets)
        num_total_neg = sum(t[5].numel() for t in targets)
        cls_scores = cls_scores.reshape(-1, self.cls_out_channels)
        cls_avg_factor = num_total_pos * 1.0 + num_total_neg * self.bg_cls_weight
        if self.sync_cls_avg_factor:
            cls_avg_factor = reduce_mean(cls_scores.new_tensor([cls_avg_factor]))
        cls_avg_factor = max(cls_avg_factor, 1)
        loss_cls = self.loss_cls_fn(cls_scores, labels, label_weights, avg_factor=cls_avg_factor)
        num_total_pos = loss_cls.new_tensor([num_total_pos])
        num_total_pos = torch.clamp(reduce_mean(num_total_pos), min=1).item()
        bbox_preds = bbox_preds.reshape(-1, bbox_preds.size(-1))
        normalized_bbox_targets = normalize_bbox(bbox_targets, self.pc_range)
        isnotnan = torch.isfinite(normalized_bbox_targets).all(dim=-1)
        bbox_weights = bbox_weights * self.code_weights
        loss_bbox = self.loss_bbox_fn(bbox_preds[isnotnan, :10], normalized_bbox_targets[isnotnan, :10],
                                      bbox_weights[isnotnan, :10], avg_factor=num_total_pos)
        loss_cls = torch.nan_to_num(loss_cls)
        loss_bbox = torch.nan_to_num(loss_bbox)
        return loss_cls, loss_bbox

    def loss_fused_reject(self, preds_dicts=None, gt_bboxes_list=None):
        """Why ``loss`` does not take ``ops.detection_loss`` (a short reason), or ``None`` when it does.  The switch itself
        (``modes.loss_fused``) is the caller's to test."""
        if self.assigner is None:
            return "no assigner"
        why = ops.detection_loss_reject(self.loss_cls_fn, self.loss_bbox_fn, self.assigner, self.code_size, self.cls_out_channels)
        if why is not None:
            return why
        if preds_dicts is not None:
            cls, box = preds_dicts["all_cls_scores"], preds_dicts["all_bbox_preds"]
            if not (torch.is_tensor(cls) and torch.is_tensor(box) and cls.is_cuda and box.is_cuda
                    and cls.dtype == torch.float32 and box.dtype == torch.float32):
                return "not CUDA fp32 predictions"
            if cls.dim() != 4 or box.dim() != 4 or cls.shape[-1] != self.cls_out_channels or box.shape[-1] != self.code_size:
                return "prediction shapes are not (L, bs, nq, cls_out) / (L, bs, nq, code_size)"
            groups = getattr(self, "group_detr", 1)
            if groups < 1 or cls.shape[2] % groups:
                return f"{cls.shape[2]} queries do not split into {groups} groups"
            per_group = cls.shape[2] // groups
            if per_group > ops.LOSS_MAX_NQ:
                return f"num_query {per_group}" + (" per group" if groups > 1 else "") + f" is over {ops.LOSS_MAX_NQ}"
            if groups > 1 and cls.shape[0] * cls.shape[1] * groups > ops.LOSS_MAX_PROBLEMS:
                return f"more than {ops.LOSS_MAX_PROBLEMS} (layer, sample, group) problems"
            if gt_bboxes_list is not None:
                if any(g.shape[0] > min(ops.LOSS_MAX_GT, per_group) for g in gt_bboxes_list):
                    return f"more than {ops.LOSS_MAX_GT} (or num_query) gt boxes in a sample"
                if any(g.shape[-1] != self.code_size - 1 for g in gt_bboxes_list):
                    return "gt boxes are not code_size - 1 wide"
        return None

    @force_fp32(apply_to=("preds_dicts"))
    def loss(self, gt_bboxes_list=None, gt_labels_list=None, preds_dicts=None, gt_bboxes_ignore=None, img_metas=None):
        """bevformer_head.py:395-480 -> dict(loss_cls, loss_bbox, d{i}.loss_cls, d{i}.loss_bbox).  A gt box set is an object
        with ``.gravity_center`` and ``.tensor`` (mmdet3d's boxes) or a plain (G, code_size - 1) tensor already in
        gravity-centre form.  With ``modes.loss_fused`` and a covered call the values are views of one (L, 2) tensor."""
        if self.assigner is None:
            # (a head built without train_cfg['assigner']: as before this path existed)
            raise NotImplementedError("BEVFormerHead.loss: the detection loss and the Hungarian assigner are mmdet's "
                                      "(DETRHead, HungarianAssigner3D); this head is inference only")
        assert gt_bboxes_ignore is None, f"{self.__class__.__name__} only supports for gt_bboxes_ignore setting to None."
        all_cls_scores = preds_dicts["all_cls_scores"]
        all_bbox_preds = preds_dicts["all_bbox_preds"]
        if preds_dicts.get("enc_cls_scores") is not None:
            raise NotImplementedError("BEVFormerHead.loss: as_two_stage (enc_cls_scores) is not implemented")
        num_dec_layers = len(all_cls_scores)
        device = gt_labels_list[0].device
        gt_bboxes_list = [(torch.cat((g.gravity_center, g.tensor[:, 3:]), dim=1) if hasattr(g, "gravity_center") else g).to(device)
                          for g in gt_bboxes_list]
        losses = None
        if ops.modes().loss_fused and self.loss_fused_reject(preds_dicts, gt_bboxes_list) is None:
            losses = ops.detection_loss_head(self, all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list)
        if losses is not None:
            losses_cls, losses_bbox = losses[:, 0].unbind(0), losses[:, 1].unbind(0)
        else:
            per_layer = [self.loss_single(all_cls_scores[i], all_bbox_preds[i], gt_bboxes_list, gt_labels_list)
                         for i in range(num_dec_layers)]
            losses_cls, losses_bbox = [p[0] for p in per_layer], [p[1] for p in per_layer]
        loss_dict = dict()
        loss_dict["loss_cls"] = losses_cls[-1]
        loss_dict["loss_bbox"] = losses_bbox[-1]
        for num_dec_layer, (loss_cls_i, loss_bbox_i) in enumerate(zip(losses_cls[:-1], losses_bbox[:-1])):
            loss_dict[f"d{num_dec_layer}.loss_cls"] = loss_cls_i
            loss_dict[f"d{num_dec_layer}.loss_bbox"] = loss_bbox_i
        return loss_dict

    @force_fp32(apply_to=("preds_dicts"))
    def get_bboxes(self, preds_dicts, img_metas, rescale=False):
        """bevformer_head.py:482-509 -> list of [bboxes, scores, labels] per sample; bboxes wrapped in
        ``img_metas[i]['box_type_3d']`` when that key exists, else the (n, code_size - 1) tensor."""
        preds_dicts = self.bbox_coder.decode(preds_dicts)
        ret_list = []
        for i in range(len(preds_dicts)):
            preds = preds_dicts[i]
            bboxes = preds["bboxes"]
            bboxes[:, 2] = bboxes[:, 2] - bboxes[:, 5] * 0.5
            code_size = bboxes.shape[-1]
            if img_metas is not None and "box_type_3d" in img_metas[i]:
                bboxes = img_metas[i]["box_type_3d"](bboxes, code_size)
            ret_list.append([bboxes, preds["scores"], preds["labels"]])
        return ret_list


class BEVFormerHead_GroupDETR(BEVFormerHead):
    """bevformer_head.py:512-683.  ``num_query`` is ONE group's; the head holds ``group_detr * num_query`` query embeddings
    and predicts for all of them in ``train()`` mode, for the first group's otherwise."""

    def __init__(self, *args, group_detr=1, **kwargs):
        self.group_detr = group_detr
        assert "num_query" in kwargs
        kwargs["num_query"] = group_detr * kwargs["num_query"]
        super().__init__(*args, **kwargs)

    def object_query_embeds(self, dtype):
        object_query_embeds = self.query_embedding.weight.to(dtype)
        if not self.training:       # NOTE: Only difference to bevformer head  (bevformer_head.py:527-528)
            object_query_embeds = object_query_embeds[:self.num_query // self.group_detr]
        return object_query_embeds

    @force_fp32(apply_to=("preds_dicts"))
    def loss(self, gt_bboxes_list=None, gt_labels_list=None, preds_dicts=None, gt_bboxes_ignore=None, img_metas=None):
        """bevformer_head.py:603-683: every group's ``[g * n, (g + 1) * n)`` query slice through ``loss_single`` per layer,
        ``loss / group_detr`` added into the reference's keys.  With ``modes.loss_fused`` and a covered call: all groups on the
        device (``ops.detection_loss`` with ``groups=group_detr``), the values views of one (L, 2) tensor."""
        if self.assigner is None:
            raise NotImplementedError("BEVFormerHead_GroupDETR.loss: this head was built without train_cfg['assigner']; it is "
                                      "inference only")
        assert gt_bboxes_ignore is None, f"{self.__class__.__name__} only supports for gt_bboxes_ignore setting to None."
        all_cls_scores = preds_dicts["all_cls_scores"]
        all_bbox_preds = preds_dicts["all_bbox_preds"]
        assert preds_dicts.get("enc_cls_scores") is None and preds_dicts.get("enc_bbox_preds") is None
        num_dec_layers = len(all_cls_scores)
        device = gt_labels_list[0].device
        gt_bboxes_list = [(torch.cat((g.gravity_center, g.tensor[:, 3:]), dim=1) if hasattr(g, "gravity_center") else g).to(device)
                          for g in gt_bboxes_list]
        loss_dict = dict()
        if ops.modes().loss_fused and self.loss_fused_reject(preds_dicts, gt_bboxes_list) is None:
            losses = ops.detection_loss_head(self, all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list)
            loss_dict["loss_cls"], loss_dict["loss_bbox"] = losses[-1, 0], losses[-1, 1]
            for num_dec_layer in range(num_dec_layers - 1):
                loss_dict[f"d{num_dec_layer}.loss_cls"] = losses[num_dec_layer, 0]
                loss_dict[f"d{num_dec_layer}.loss_bbox"] = losses[num_dec_layer, 1]
            return loss_dict
        loss_dict["loss_cls"] = 0
        loss_dict["loss_bbox"] = 0
        for num_dec_layer in range(num_dec_layers - 1):
            loss_dict[f"d{num_dec_layer}.loss_cls"] = 0
            loss_dict[f"d{num_dec_layer}.loss_bbox"] = 0
        num_query_per_group = self.num_query // self.group_detr
        for group_index in range(self.group_detr):
            group_query_start = group_index * num_query_per_group
            group_query_end = (group_index + 1) * num_query_per_group
            group_cls_scores = all_cls_scores[:, :, group_query_start:group_query_end, :]
            group_bbox_preds = all_bbox_preds[:, :, group_query_start:group_query_end, :]
            per_layer = [self.loss_single(group_cls_scores[i], group_bbox_preds[i], gt_bboxes_list, gt_labels_list)
                         for i in range(num_dec_layers)]
            losses_cls, losses_bbox = [p[0] for p in per_layer], [p[1] for p in per_layer]
            loss_dict["loss_cls"] += losses_cls[-1] / self.group_detr
            loss_dict["loss_bbox"] += losses_bbox[-1] / self.group_detr
            for num_dec_layer, (loss_cls_i, loss_bbox_i) in enumerate(zip(losses_cls[:-1], losses_bbox[:-1])):
                loss_dict[f"d{num_dec_layer}.loss_cls"] += loss_cls_i / self.group_detr
                loss_dict[f"d{num_dec_layer}.loss_bbox"] += loss_bbox_i / self.group_detr
        return loss_dict


def _run_branch(branch, x, tag):
    """``branch(x)`` for an ``nn.Sequential`` of the head: its Linear layers go through the GEMM of the current mode on the
    GPU (``ops.linear_or_torch``, as every other Linear of the package; ``F.linear`` on the CPU), the rest are the modules."""
    if not isinstance(branch, nn.Sequential) or not x.is_cuda:
        return branch(x)
    for m in branch:
        x = ops.linear_or_torch(x, m.weight, m.bias, tag=tag) if isinstance(m, nn.Linear) else m(x)
    return x


HEADS.register_module(name="BEVFormerHead", module=BEVFormerHead, force=True)   # (takes over the plugin's name, as the other modules do)
HEADS.register_module(name="BEVFormerHead_GroupDETR", module=BEVFormerHead_GroupDETR, force=True)
if not HAVE_MMDET:      # with mmdet the coder is the plugin's own class
    BBOX_CODERS.register_module(name="NMSFreeCoder", module=NMSFreeCoder, force=True)
if not HAVE_MMCV:
    POSITIONAL_ENCODING.register_module(name="LearnedPositionalEncoding", module=LearnedPositionalEncoding, force=True)
