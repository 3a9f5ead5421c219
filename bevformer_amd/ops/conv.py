"""BEVFormerV2's temporal fusion on the channel-last 3 x 3 convolution kernel (csrc/conv3x3.h): ``conv3x3_bn`` (convolution +
inference BatchNorm + residual + ReLU over (bs, H W, C) rows), ``resnet_fusion`` (the blocks of a ``ResNetFusion`` and its
Linear + LayerNorm) and ``fusion_reject`` (why a module or call is not covered).  Inference only."""
import ctypes

import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm

from .. import _lib
from ..ext import _ptr
from ._base import _gemm_ctx, _launch, _m, _precision
from .gemm import _pkg, _rows2d
from .images import conv3x3_weight

CONV_GRAN = 32                      # channel counts (per segment, C_in, C_out) are multiples of this: both convolution kernels
CONV_MAX_SEGMENTS = _lib.CONV_MAX_SEGMENTS
CONV_MAX_ROWS = 1 << 24             # input rows of one call, both convolution kernels


def _conv_reject(conv):
    if not isinstance(conv, nn.Conv2d):
        return "not a Conv2d"
    if tuple(conv.kernel_size) != (3, 3):
        return "a convolution is not 3 x 3"
    if tuple(conv.stride) != (1, 1):
        return "a convolution has a stride"
    if conv.padding not in ((1, 1), 1) or getattr(conv, "padding_mode", "zeros") != "zeros":
        return "a convolution's padding is not 1 (zeros)"
    if tuple(conv.dilation) != (1, 1) or conv.groups != 1:
        return "a convolution is dilated or grouped"
    if conv.bias is not None:
        return "a convolution has a bias"
    if conv.in_channels % CONV_GRAN or conv.out_channels % CONV_GRAN:
        return f"channel counts are not multiples of {CONV_GRAN}"
    return None


def _norm_reject(norm):
    if not isinstance(norm, _BatchNorm):
        return "a norm is not BatchNorm"
    if norm.weight is None or norm.bias is None:
        return "a norm is not affine"
    if norm.running_mean is None or norm.running_var is None:
        return "a norm has no running statistics"
    return None


def _block_parts(block):
    """(conv1, norm1, conv2, norm2, downsample or None) of a ResNet basic block, by attribute: the in-tree block names its
    norms ``bn1`` / ``bn2``, mmdet's ``norm1`` / ``norm2``."""
    get = lambda *names: next((getattr(block, n) for n in names if hasattr(block, n)), None)
    return get("conv1"), get("bn1", "norm1"), get("conv2"), get("bn2", "norm2"), get("downsample")


def _block_reject(block):
    conv1, n1, conv2, n2, ds = _block_parts(block)
    if conv1 is None or conv2 is None or n1 is None or n2 is None:
        return "a block is not conv1 / norm1 / conv2 / norm2"
    if not isinstance(getattr(block, "relu", None), nn.ReLU):
        return "a block's activation is not ReLU"
    pairs = [(conv1, n1), (conv2, n2)]
    if ds is not None:
        try:
            mods = list(ds)
        except TypeError:
            return "a downsample is not conv + norm"
        if len(mods) != 2:
            return "a downsample is not conv + norm"
        pairs.append((mods[0], mods[1]))
    for conv, norm in pairs:
        why = _conv_reject(conv) or _norm_reject(norm)
        if why is not None:
            return why
        if norm.num_features != conv.out_channels:
            return "a norm does not match its convolution"
    if conv2.in_channels != conv1.out_channels or conv2.out_channels != conv1.out_channels:
        return "a block's convolutions do not chain"
    if ds is not None and (pairs[2][0].in_channels != conv1.in_channels or pairs[2][0].out_channels != conv2.out_channels):
        return "a downsample does not match its block"
    if ds is None and conv1.in_channels != conv2.out_channels:
        return "a block without downsample changes the channel count"
    return None


def fusion_reject(fusion, rows=None):
    """Why ``resnet_fusion`` does not cover ``fusion`` (a ``ResNetFusion``) on the BEV rows ``rows`` (a list of (bs, H W, C)
    tensors; ``None``: the module alone is judged) — a short reason — or ``None`` when it does.  The switch itself
    (``modes.bevfusion_fused``) is the caller's to test.  Structure first, then modes and tensors."""
    try:
        blocks = list(fusion.layers)
        lin, norm = fusion.layer_norm[0], fusion.layer_norm[1]
    except (AttributeError, TypeError, IndexError):
        return "not a ResNetFusion"
    if not blocks:
        return "no blocks"
    for blk in blocks:
        why = _block_reject(blk)
        if why is not None:
            return why
    for prev, blk in zip(blocks, blocks[1:]):
        if blk.conv1.in_channels != prev.conv2.out_channels:
            return "the blocks do not chain"
    if not isinstance(lin, nn.Linear) or not isinstance(norm, nn.LayerNorm) or lin.in_features != blocks[-1].conv2.out_channels:
        return "the output projection is not Linear + LayerNorm"
    if fusion.training:
        return "train() mode (batch statistics)"
    if torch.is_grad_enabled():
        return "grad mode is on"
    if _m().gemm not in ("split", "bf16"):
        return f"GEMM mode {_m().gemm}"
    params = [p for p in fusion.parameters()] + [b for b in fusion.buffers() if b.is_floating_point()]
    if not all(p.is_cuda and p.dtype == torch.float32 for p in params):
        return "not CUDA fp32 parameters"
    if rows is not None:
        rows = list(rows)
        if not rows or not all(torch.is_tensor(r) and r.is_cuda and r.dtype == torch.float32 and r.dim() == 3 for r in rows):
            return "not CUDA fp32 (bs, H W, C) rows"
        if any(r.shape != rows[0].shape for r in rows):
            return "the frames' rows differ in shape"
        if len(rows) * rows[0].shape[-1] != blocks[0].conv1.in_channels:
            return "the frames' channels do not add up to the first convolution's"
        if blocks[0].downsample is not None and (len(rows) > CONV_MAX_SEGMENTS or rows[0].shape[-1] % CONV_GRAN):
            return f"more than {CONV_MAX_SEGMENTS} frames, or frames off the channel granularity"
        if rows[0].shape[0] * rows[0].shape[1] > CONV_MAX_ROWS:
            return "more than 2^24 rows"
    return None


def conv3x3_bn(rows, hw, weight, bn, *, relu, res=None, tag="conv3x3_bn"):
    """``act(bn(conv3x3(x)) + res)`` over channel-last rows (``bevmsda_conv3x3_bn_f32``): ``rows`` is a (bs, H W, C) tensor or a
    list of up to 8 such segments of equal width whose concatenation along C is x (read in place; a segment may repeat),
    ``hw = (H, W)``, ``weight`` (C_out, C, 3, 3) of a stride-1, padding-1 convolution without bias, ``bn`` a BatchNorm module
    in eval mode (its four vectors and ``eps`` are read by the kernel, nothing is derived on the host), ``res`` an optional
    (bs, H W, C_out) tensor.  Returns (bs, H W, C_out), or ``None`` when the call is not covered."""
    segs = [rows] if torch.is_tensor(rows) else list(rows)
    mode = _m().gemm
    tensors = segs + [weight] + ([res] if res is not None else [])
    if mode not in ("split", "bf16") or not segs or len(segs) > CONV_MAX_SEGMENTS or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors) \
            or _norm_reject(bn) is not None or bn.training:
        return None
    H, W = int(hw[0]), int(hw[1])
    if any(s.dim() != 3 or s.shape != segs[0].shape for s in segs) or segs[0].shape[1] != H * W:
        return None
    bs, _, cseg = segs[0].shape
    N = weight.shape[0]
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (cseg * len(segs), 3, 3) or cseg % CONV_GRAN or N % CONV_GRAN \
            or bn.num_features != N or bs * H * W > CONV_MAX_ROWS:
        return None
    vecs = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if not all(v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == N for v in vecs):
        return None
    if res is not None and tuple(res.shape) != (bs, H * W, N):
        return None
    y = torch.empty((bs, H * W, N), dtype=torch.float32, device=segs[0].device)
    if y.numel() == 0:
        return y
    blob = conv3x3_weight(weight)
    if blob is None:
        return None
    desc = _lib.Conv3x3Desc(bs=bs, H=H, W=W, nseg=len(segs), c_seg=cseg, c_out=N, relu=int(bool(relu)),
                            precision=_precision(), eps=float(bn.eps), ld_y=N,
                            gamma=_ptr(bn.weight), beta=_ptr(bn.bias), mean=_ptr(bn.running_mean), var=_ptr(bn.running_var))
    keep = []
    for i, s in enumerate(segs):
        s2, ld = _rows2d(s, cseg)
        keep.append(s2)
        desc.seg[i], desc.ld_seg[i] = _ptr(s2), ld
    if res is not None:
        r2, ldres = _rows2d(res, N)
        keep.append(r2)
        desc.res, desc.ld_res = _ptr(r2), ldres
    M, K = bs * H * W, 9 * cseg * len(segs)
    timer = _gemm_ctx(tag, 2.0 * M * N * K, 4.0 * (M * K // 9 + N * K + M * N * (2 if res is not None else 1)))
    return y if _launch(y.device, "conv3x3_bn", lambda lib, stream: lib.bevmsda_conv3x3_bn_f32(
        ctypes.byref(desc), _ptr(blob), _ptr(y), stream), timer=timer) else None


def resnet_fusion(fusion, rows, bev_h, bev_w):
    """``ResNetFusion`` on the BEV rows of its frames, ``rows`` a list of (bs, H W, C): per block conv1-BN-ReLU, then
    conv2-BN + identity-ReLU, where the identity is the block's input or BN(downsample conv); then Linear + LayerNorm.
    The first block with a downsample reads the frames in place as segments of its two convolutions; without one the frames
    are concatenated once (the identity needs that tensor anyway).  The caller has asked ``fusion_reject`` first: a
    convolution the kernel then declines is an error, not a detour.  -> (bs, H W, out_channels)."""
    ops = _pkg()
    hw = (bev_h, bev_w)
    x = list(rows)

    def conv(x, conv_, norm_, relu, res=None):
        y = ops.conv3x3_bn(x, hw, conv_.weight, norm_, relu=relu, res=res)
        if y is None:
            raise RuntimeError("bevmsda: resnet_fusion: conv3x3_bn declined a call fusion_reject had accepted")
        return y

    for blk in fusion.layers:
        conv1, n1, conv2, n2, ds = _block_parts(blk)
        if ds is not None:
            identity = conv(x, ds[0], ds[1], False)
        else:
            if len(x) > 1:
                x = [torch.cat(x, -1)]
            identity = x[0]
        out = conv(x, conv1, n1, True)
        x = [conv([out], conv2, n2, True, res=identity)]
    x = x[0]
    lin, norm = fusion.layer_norm[0], fusion.layer_norm[1]
    y = ops.linear_layernorm(x, lin.weight, lin.bias, None, norm, tag="fusion_proj")
    if y is not None:
        return y
    y = ops.linear_or_torch(x, lin.weight, lin.bias, tag="fusion_proj")
    out = ops.add_layernorm(y, None, norm.weight, norm.bias, norm.eps) if not torch.is_grad_enabled() else None
    return out if out is not None else norm(y)
