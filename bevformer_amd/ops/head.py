"""The detection head's kernels (csrc/head_branch.h, csrc/head_decode.h): the classification / regression branch chains of
every decoder layer in one launch (``head_branches``), the decoder's reference-point refinement (``reg_refine``) and the NMS-free
box decode (``nms_free_decode``).  Inference only; each returns ``None`` when the call is not covered and the caller runs its
modules."""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from ..ext import _ptr
from ._base import _TIMER, _gemm_ctx, _launch, _m, _precision
from .gemm import _rows2d
from .images import panel_weight

HEAD_CODE_SIZES = (8, 10)
HEAD_MAX_CLS_OUT = 32
DECODE_MAX_SCORES = 16384
DECODE_MAX_NUM = 1024


def _linear_is(m, n_in):
    return isinstance(m, nn.Linear) and m.weight.dim() == 2 and m.weight.shape[1] == n_in and m.bias is not None


def _norm_is(m):
    return isinstance(m, nn.LayerNorm) and tuple(m.normalized_shape) == (256,) and m.weight is not None and m.bias is not None


def head_branch_reject(branch, kind):
    """Why ``branch`` is not the stock branch of ``BEVFormerHead`` the kernel covers (a short reason), or ``None`` when it is.
    ``kind`` "reg": Linear(256, 256), ReLU, Linear(256, 256), ReLU, Linear(256, code_size in {8, 10}); "cls": Linear(256, 256),
    LayerNorm(256), ReLU, Linear(256, 256), LayerNorm(256), ReLU, Linear(256, 1 .. 32).  By attributes, not by class: with
    mmcv installed the Linear layers are its subclass and the container is whatever the head built."""
    try:
        mods = list(branch)
    except TypeError:
        return "not a sequence of layers"
    want = 5 if kind == "reg" else 7
    if len(mods) != want:
        return f"{len(mods)} layers, not {want}"
    step = 2 if kind == "reg" else 3
    for i in (0, step):
        if not _linear_is(mods[i], 256) or mods[i].weight.shape[0] != 256:
            return "hidden layer is not Linear(256, 256)"
        if kind == "cls" and not _norm_is(mods[i + 1]):
            return "no LayerNorm(256) with affine parameters behind a hidden layer"
        if not isinstance(mods[i + step - 1], nn.ReLU):
            return "activation is not ReLU"
    last = mods[-1]
    if not _linear_is(last, 256):
        return "last layer is not Linear(256, .)"
    n = last.weight.shape[0]
    if kind == "reg" and n not in HEAD_CODE_SIZES:
        return f"code_size {n} is not 8 or 10"
    if kind == "cls" and not 1 <= n <= HEAD_MAX_CLS_OUT:
        return f"cls_out {n} is outside 1 .. {HEAD_MAX_CLS_OUT}"
    return None


def _covered(*tensors):
    m = _m()
    if m.gemm not in ("split", "bf16") or not m.gemm_pack:
        return False
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            return False
    return True


def _wants_grad(tensors, modules):
    if not torch.is_grad_enabled():
        return False
    return any(t.requires_grad for t in tensors) or any(p.requires_grad for m in modules for p in m.parameters())


def _branch_entry(branch, kind, keep):
    """``_lib.HeadBranch`` of a stock branch (weight images through the cache of ``panel_weight``), or ``None``.  The kernel
    reads biases and LayerNorm parameters in place, and a captured graph keeps their addresses: a parameter that would need
    a copy (not contiguous) declines the call instead of handing the graph a temporary."""
    mods = list(branch)
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    norms = [m for m in mods if isinstance(m, nn.LayerNorm)]
    e = _lib.HeadBranch()
    for i, lin in enumerate(lins):
        w, b = lin.weight, lin.bias
        if not w.is_contiguous() or not b.is_contiguous():
            return None
        blob = panel_weight(w)
        if blob is None:
            return None
        keep.extend((blob, b))
        setattr(e, f"w{i + 1}", _ptr(blob))
        setattr(e, f"b{i + 1}", _ptr(b))
    if kind == "cls":
        for i, nm in enumerate(norms):
            g, be = nm.weight, nm.bias
            if not g.is_contiguous() or not be.is_contiguous():
                return None
            keep.extend((g, be))
            setattr(e, f"gamma{i + 1}", _ptr(g))
            setattr(e, f"beta{i + 1}", _ptr(be))
            setattr(e, f"eps{i + 1}", float(nm.eps))
    return e


def _table(branches, kind, keep):
    shared = all(b is branches[0] for b in branches)
    entries = []
    for b in (branches[:1] if shared else branches):
        e = _branch_entry(b, kind, keep)
        if e is None:
            return None, 0
        entries.append(e)
    return (_lib.HeadBranch * len(entries))(*entries), 0 if shared else 1


def _flops_bytes(rows, n_out):
    return 2.0 * rows * 256 * (512 + n_out), 4.0 * (rows * (256 + n_out) + 256 * (512 + n_out))


def head_branches(hs, refs, cls_branches, reg_branches, pc_range, *, tag="head_branches"):
    """``BEVFormerHead.forward``'s loop over the decoder layers (bevformer_head.py:175-203) in ONE launch
    (``bevmsda_head_branches_f32``): ``hs`` (L, num_query, bs, 256) the decoder's states in ITS order, ``refs`` (L, bs,
    num_query, 3) the reference point each layer consumed (``init_reference`` and ``inter_references[:-1]``), ``cls_branches``
    / ``reg_branches`` the head's module lists (one shared module, or one per layer) -> ``(all_cls_scores (L, bs, num_query,
    cls_out), all_bbox_preds (L, bs, num_query, code_size))``, or ``None`` when not covered: CPU or non-fp32 tensors, a
    gradient wanted, GEMM mode not split / bf16, a branch that is not the stock shape (``head_branch_reject``)."""
    if not _covered(hs, refs) or hs.dim() != 4 or hs.shape[-1] != 256 or refs.dim() != 4 or refs.shape[-1] != 3:
        return None
    L, nq, bs, _ = hs.shape
    if not 1 <= L <= _lib.HEAD_MAX_LAYERS or tuple(refs.shape) != (L, bs, nq, 3) or len(cls_branches) < L \
            or len(reg_branches) < L:
        return None
    cls_l, reg_l = list(cls_branches)[:L], list(reg_branches)[:L]
    if any(head_branch_reject(b, "cls") is not None for b in cls_l) or any(head_branch_reject(b, "reg") is not None for b in reg_l):
        return None
    code, nc = reg_l[0][-1].weight.shape[0], cls_l[0][-1].weight.shape[0]
    if any(b[-1].weight.shape[0] != code for b in reg_l) or any(b[-1].weight.shape[0] != nc for b in cls_l) \
            or all(b is reg_l[0] for b in reg_l) != all(b is cls_l[0] for b in cls_l):
        return None
    if _wants_grad((hs, refs), cls_l + reg_l):
        return None
    box = torch.empty((L, bs, nq, code), dtype=torch.float32, device=hs.device)
    cls = torch.empty((L, bs, nq, nc), dtype=torch.float32, device=hs.device)
    if nq == 0 or bs == 0:
        return cls, box
    x = hs if (hs.is_contiguous() and hs.data_ptr() % 16 == 0) else hs.contiguous()
    refs = refs.contiguous()
    keep = []
    with torch.cuda.device(hs.device):
        reg_t, stride = _table(reg_l, "reg", keep)
        cls_t, _ = _table(cls_l, "cls", keep)
    if reg_t is None or cls_t is None:
        return None
    desc = _lib.HeadDesc(ld_x=256, ld_layer=nq * bs * 256, mode=_lib.HEAD_MODE_HEAD, L=L, nq=nq, bs=bs, code_size=code,
                         cls_out=nc, precision=_precision(), layer_stride=stride)
    for i in range(6):
        desc.pc_range[i] = float(pc_range[i])
    f0, b0 = _flops_bytes(L * nq * bs, code)
    f1, b1 = _flops_bytes(L * nq * bs, nc)
    if not _launch(hs.device, "head_branches", lambda lib, stream: lib.bevmsda_head_branches_f32(
            _ptr(x), _ptr(refs), reg_t, cls_t, ctypes.byref(desc), _ptr(box), _ptr(cls), stream),
            timer=_gemm_ctx(tag, f0 + f1, b0 + b1)):
        return None
    return cls, box


def reg_refine(x, ref, reg_branch, *, tag="dec_refine"):
    """The decoder's reference-point refinement after a layer (modules/decoder.py:68-74) in one launch: ``x`` (num_query, bs,
    256) the layer's output in the decoder's order, ``ref`` (bs, num_query, 3) the reference points it consumed, ``reg_branch``
    the layer's stock regression branch -> ``sigmoid(reg_branch(x)[{0, 1, 4}] + inverse_sigmoid(ref))`` (bs, num_query, 3), or
    ``None`` when not covered (as ``head_branches``)."""
    if not _covered(x, ref) or x.dim() != 3 or x.shape[-1] != 256 or ref.dim() != 3 or ref.shape[-1] != 3:
        return None
    nq, bs, _ = x.shape
    if tuple(ref.shape) != (bs, nq, 3) or head_branch_reject(reg_branch, "reg") is not None or _wants_grad((x, ref), [reg_branch]):
        return None
    out = torch.empty((bs, nq, 3), dtype=torch.float32, device=x.device)
    if nq == 0 or bs == 0:
        return out
    x2, ldx = _rows2d(x, 256)
    ref = ref.contiguous()
    keep = []
    with torch.cuda.device(x.device):
        reg_t, _ = _table([reg_branch], "reg", keep)
    if reg_t is None:
        return None
    desc = _lib.HeadDesc(ld_x=ldx, ld_layer=0, mode=_lib.HEAD_MODE_REFINE, L=1, nq=nq, bs=bs,
                         code_size=reg_branch[-1].weight.shape[0], cls_out=0, precision=_precision(), layer_stride=0)
    desc.pc_range[3] = desc.pc_range[4] = desc.pc_range[5] = 1.0
    if not _launch(x.device, "reg_refine", lambda lib, stream: lib.bevmsda_head_branches_f32(
            _ptr(x2), _ptr(ref), reg_t, None, ctypes.byref(desc), _ptr(out), None, stream),
            timer=_gemm_ctx(tag, *_flops_bytes(nq * bs, reg_branch[-1].weight.shape[0]))):
        return None
    return out


def threshold_ladder(score_threshold):
    """The thresholds ``NMSFreeCoder.decode_single`` walks (nms_free_coder.py:65-73) as a list: ``thr``, then ``thr * 0.9 ** k``
    while it stays >= 0.01 (the same Python float products).  ``None`` / 0: no score test (the truthiness test at :83)."""
    if not score_threshold:
        return []
    out, t = [float(score_threshold)], float(score_threshold)
    while True:
        t *= 0.9
        if t < 0.01:
            return out
        out.append(t)


def nms_free_decode(cls, box, *, max_num, post_center_range, score_threshold=None, num_classes, tag="head_decode"):
    """``NMSFreeCoder.decode_single`` for every batch entry with fixed-shape outputs (``bevmsda_nms_free_decode_f32``): ``cls``
    (bs, num_query, num_classes) logits and ``box`` (bs, num_query, code_size) box codes of the last decoder layer ->
    ``(scores (bs, max_num), labels (bs, max_num) int64, boxes (bs, max_num, code_size - 1), keep (bs, max_num) bool, count
    (bs,) int32)``: rank r is the r-th largest LOGIT (ties: the lower flat index ``q * num_classes + c`` first), ``keep`` the
    reference's centre-range and score-threshold mask.  No device value is read by the host: capturable in a HIP graph.
    ``max_num`` > ``num_query * num_classes`` raises ``ValueError`` (as ``topk`` would).  Returns ``None`` when not covered
    (CPU or non-fp32 tensors, a gradient wanted, more than 16,384 scores, ``max_num`` > 1,024)."""
    if not torch.is_tensor(cls) or not torch.is_tensor(box) or cls.dim() != 3 or box.dim() != 3:
        return None
    bs, nq, C = cls.shape
    if max_num > nq * C:
        raise ValueError(f"nms_free_decode: max_num {max_num} is out of range for {nq} x {C} scores")
    if not cls.is_cuda or not box.is_cuda or cls.dtype != torch.float32 or box.dtype != torch.float32 \
            or C != num_classes or tuple(box.shape[:2]) != (bs, nq) or box.shape[-1] not in HEAD_CODE_SIZES \
            or nq * C > DECODE_MAX_SCORES or max_num > DECODE_MAX_NUM or max_num < 0 or post_center_range is None \
            or (torch.is_grad_enabled() and (cls.requires_grad or box.requires_grad)):
        return None
    ladder = threshold_ladder(score_threshold)
    if len(ladder) > 64:
        return None
    code = box.shape[-1]
    dev = cls.device
    scores = torch.empty((bs, max_num), dtype=torch.float32, device=dev)
    labels = torch.empty((bs, max_num), dtype=torch.int64, device=dev)
    boxes = torch.empty((bs, max_num, code - 1), dtype=torch.float32, device=dev)
    keep = torch.empty((bs, max_num), dtype=torch.bool, device=dev)
    count = torch.empty((bs,), dtype=torch.int32, device=dev)
    if bs == 0:
        return scores, labels, boxes, keep, count
    cls, box = cls.contiguous(), box.contiguous()
    desc = _lib.DecodeDesc(bs=bs, nq=nq, num_classes=C, code_size=code, max_num=max_num, n_ladder=len(ladder))
    for i in range(6):
        desc.post_center_range[i] = float(post_center_range[i])
    for i, t in enumerate(ladder):
        desc.ladder[i] = t
    cb = _TIMER["cb"]
    ctx = cb(tag, 4.0 * bs * (nq * (C + code) + max_num * (code + 3))) if cb is not None else None
    _launch(dev, "nms_free_decode", lambda lib, stream: lib.bevmsda_nms_free_decode_f32(
        _ptr(cls), _ptr(box), ctypes.byref(desc), _ptr(scores), _ptr(labels), _ptr(boxes), _ptr(keep), _ptr(count), stream),
        timer=ctx, required=True)
    return scores, labels, boxes, keep, count
