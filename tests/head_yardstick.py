"""The yardstick of the detection-head tests: a plain-torch restatement of the reference's head arithmetic
(dense_heads/bevformer_head.py:69-107,171-203,482-509; core/bbox/coders/nms_free_coder.py:40-100; core/bbox/util.py:26-53;
the decoder's refinement, modules/decoder.py:68-74 of the reference) that runs in whatever dtype its inputs have (float32 or
float64) and uses nothing of the product package."""
import math

import torch
import torch.nn.functional as F


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def branch_params(branch, dtype=torch.float64):
    """The parameters of an ``nn.Sequential`` branch as a list of (kind, weight, bias, eps) in ``dtype`` on the CPU."""
    out = []
    for m in branch:
        if isinstance(m, torch.nn.Linear):
            out.append(("linear", m.weight.detach().cpu().to(dtype), m.bias.detach().cpu().to(dtype), None))
        elif isinstance(m, torch.nn.LayerNorm):
            out.append(("norm", m.weight.detach().cpu().to(dtype), m.bias.detach().cpu().to(dtype), m.eps))
        elif isinstance(m, torch.nn.ReLU):
            out.append(("relu", None, None, None))
        else:
            raise TypeError(type(m))
    return out


def run_branch(params, x):
    for kind, w, b, eps in params:
        if kind == "linear":
            x = F.linear(x, w, b)
        elif kind == "norm":
            x = F.layer_norm(x, (x.shape[-1],), w, b, eps)
        else:
            x = torch.relu(x)
    return x


def head_post(tmp, reference, pc_range):
    """bevformer_head.py:180-195 on a copy of ``tmp`` (..., code_size); ``reference`` (..., 3) in (0, 1)."""
    tmp = tmp.clone()
    reference = inverse_sigmoid(reference)
    tmp[..., 0:2] += reference[..., 0:2]
    tmp[..., 0:2] = tmp[..., 0:2].sigmoid()
    tmp[..., 4:5] += reference[..., 2:3]
    tmp[..., 4:5] = tmp[..., 4:5].sigmoid()
    tmp[..., 0:1] = tmp[..., 0:1] * (pc_range[3] - pc_range[0]) + pc_range[0]
    tmp[..., 1:2] = tmp[..., 1:2] * (pc_range[4] - pc_range[1]) + pc_range[1]
    tmp[..., 4:5] = tmp[..., 4:5] * (pc_range[5] - pc_range[2]) + pc_range[2]
    return tmp


def head_outputs(hs, refs, cls_params, reg_params, pc_range):
    """``hs`` (L, nq, bs, C) decoder order, ``refs`` (L, bs, nq, 3) the reference each layer consumed, per-layer parameter
    lists -> (all_cls_scores (L, bs, nq, cls_out), all_bbox_preds (L, bs, nq, code_size))."""
    hs = hs.permute(0, 2, 1, 3)
    cls, box = [], []
    for lvl in range(hs.shape[0]):
        cls.append(run_branch(cls_params[lvl], hs[lvl]))
        box.append(head_post(run_branch(reg_params[lvl], hs[lvl]), refs[lvl], pc_range))
    return torch.stack(cls), torch.stack(box)


def refine(x, ref, reg_params):
    """decoder.py:68-74: ``x`` (nq, bs, C), ``ref`` (bs, nq, 3) -> new reference points (bs, nq, 3)."""
    tmp = run_branch(reg_params, x.permute(1, 0, 2))
    new = torch.zeros_like(ref)
    new[..., :2] = tmp[..., :2] + inverse_sigmoid(ref[..., :2])
    new[..., 2:3] = tmp[..., 4:5] + inverse_sigmoid(ref[..., 2:3])
    return new.sigmoid()


def denormalize_bbox(b):
    rot = torch.atan2(b[..., 6:7], b[..., 7:8])
    parts = [b[..., 0:1], b[..., 1:2], b[..., 4:5], b[..., 2:3].exp(), b[..., 3:4].exp(), b[..., 5:6].exp(), rot]
    if b.size(-1) > 8:
        parts += [b[..., 8:9], b[..., 9:10]]
    return torch.cat(parts, dim=-1)


def threshold_mask(scores, score_threshold):
    """nms_free_coder.py:65-73 (None: no mask)."""
    if score_threshold is None:
        return None
    mask = scores > score_threshold
    t = score_threshold
    while mask.sum() == 0:
        t *= 0.9
        if t < 0.01:
            return scores > -1
        mask = scores >= t
    return mask


def decode_padded(cls_scores, bbox_preds, max_num, num_classes, post_center_range, score_threshold=None, stable=False):
    """``decode_single`` before its boolean slice: (scores, indexs, labels, boxes, mask) over the ``max_num`` ranks.
    ``stable``: rank by a stable descending sort (ties: the lower flat index first) instead of ``topk``."""
    s = cls_scores.sigmoid().view(-1)
    if stable:
        order = torch.sort(cls_scores.reshape(-1), descending=True, stable=True)[1][:max_num]
        scores, indexs = s[order], order
    else:
        scores, indexs = s.topk(max_num)
    labels = indexs % num_classes
    boxes = denormalize_bbox(bbox_preds[indexs // num_classes])
    pcr = torch.tensor(post_center_range, dtype=boxes.dtype)
    mask = (boxes[..., :3] >= pcr[:3]).all(1) & (boxes[..., :3] <= pcr[3:]).all(1)
    tm = threshold_mask(scores, score_threshold)
    if score_threshold and tm is not None:
        mask = mask & tm
    return scores, indexs, labels, boxes, mask


def decode_single(cls_scores, bbox_preds, max_num, num_classes, post_center_range, score_threshold=None):
    scores, _, labels, boxes, mask = decode_padded(cls_scores, bbox_preds, max_num, num_classes, post_center_range, score_threshold)
    return {"bboxes": boxes[mask], "scores": scores[mask], "labels": labels[mask]}


def get_bboxes(decoded):
    """bevformer_head.py:496-507 without the box-type wrapper: the gravity-centre -> bottom shift."""
    out = []
    for d in decoded:
        b = d["bboxes"].clone()
        b[:, 2] = b[:, 2] - b[:, 5] * 0.5
        out.append([b, d["scores"], d["labels"]])
    return out


def trained_like_head_(module, seed=1):
    """Xavier-uniform Linear weights, small random biases, LayerNorm parameters perturbed around (1, 0) — in place, the
    regime of ``synthetic.trained_like_`` for the head's branches (whose LayerNorm keys that function does not know)."""
    g = torch.Generator().manual_seed(seed)
    seen = set()
    with torch.no_grad():
        for m in module.modules():
            if id(m) in seen:
                continue
            seen.add(id(m))
            if isinstance(m, torch.nn.Linear):
                bound = math.sqrt(6.0 / (m.weight.shape[0] + m.weight.shape[1]))
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * bound)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.02)
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + torch.randn(m.weight.shape, generator=g) * 0.05)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
    return module


def make_branches(L, code_size, cls_out, shared, seed=1):
    """(cls_branches, reg_branches) ModuleLists of the stock shape: ``shared`` = one module for every layer."""
    import copy
    nn = torch.nn
    cls = nn.Sequential(nn.Linear(256, 256), nn.LayerNorm(256), nn.ReLU(inplace=True), nn.Linear(256, 256), nn.LayerNorm(256),
                        nn.ReLU(inplace=True), nn.Linear(256, cls_out))
    reg = nn.Sequential(nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, code_size))
    if shared:
        c, r = nn.ModuleList([cls] * L), nn.ModuleList([reg] * L)
    else:
        c = nn.ModuleList([copy.deepcopy(cls) for _ in range(L)])
        r = nn.ModuleList([copy.deepcopy(reg) for _ in range(L)])
    trained_like_head_(c, seed)
    trained_like_head_(r, seed + 100)
    return c.eval(), r.eval()
