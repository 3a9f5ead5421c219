"""The backbone's modulated deformable convolution (DCNv2) on the channel-last deformable kernel (csrc/deform_conv.h):
``deform_conv_rows`` (the bilinear-gather 3 x 3 convolution over (n_img H W, C) rows with bias or inference BatchNorm and ReLU in
the epilogue), ``dcn_offsets`` (the (M, 32) offset matrix of a pack's ``conv_offset`` from one row convolution), ``dcn`` (both
launches on an NCHW map) and ``dcn_reject`` (why a module or call is not covered).  Inference only.

The semantics restate mmcv 1.4.0's ``ModulatedDeformConv2dPack`` as published (``modules/backbone.py``).  The offset launch ALWAYS
runs in ``split`` precision, also under ``gemm="bf16"``: offsets are geometry — sample positions —, and this project keeps
geometry out of reduced precision (as the reference points and camera projections are); the deformable GEMM itself follows the
GEMM mode in force.

Layout as in ``ops.neck``: an input dense in ``torch.channels_last`` is read in place, any other layout costs one channels-last
copy; the result is the NCHW-shaped view of channel-last rows.  Nothing is read on the host: the path is capturable.

The plain convolutions of a bottleneck run on the row convolution + BatchNorm kernel (csrc/conv_bn_rows.h): ``conv_bn_rows``
(1 x 1 / 3 x 3 at stride 1 / 2 with the inference BatchNorm, the residual sum and the ReLU in the epilogue), ``bottleneck`` (the
schedule of one block on rows: 3 launches, 4 with a downsample, one more for a pack's offsets) and ``bottleneck_reject`` (why a
block or call is not covered).  A stage of covered blocks stays in rows: each block reads the view the one before it returned.

The stem runs on the stem kernel (csrc/stem_conv.h): ``stem_rows`` (7 x 7 stride-2 convolution + inference BatchNorm + ReLU + 3 x 3
stride-2 max pooling of an NCHW image batch, read in place, as channel-last rows in one launch), ``stem`` (that launch for a
ResNet's ``conv1`` / ``bn1`` / ``relu`` / ``maxpool``), ``stem_reject`` (why a module or call is not covered) and ``stem_hw`` (the output
size).

Training with frozen BatchNorms runs on the backward kernels of the row convolution (csrc/conv_bwd_rows.h):
``conv_bn_rows_backward`` (the weight gradient and the input gradient of one ``conv_bn_rows``, one launch each), ``conv_gz_rows`` (the
ReLU mask and norm scale on a gradient's rows), ``bottleneck_train`` (a whole block as one autograd Function) and
``bottleneck_train_reject`` (why a block or call is not covered).  With ``modes.dcn_train`` a block whose ``conv2`` is a DCNv2 pack
is covered too: ``deform_conv_rows_backward`` (csrc/deform_conv_bwd.h) is the gradient of ``deform_conv_rows`` with respect to its
input rows, its offset matrix and its weight.  With ``modes.bn_train`` a block whose norms are all in ``train()`` mode (batch
statistics) is covered as well, on the kernels of ``ops.norm`` (csrc/batchnorm_rows.h)."""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from ..ext import _ptr
from ._base import _forward_modes, _gemm_ctx, _launch, _m, _optr, _precision
from .conv import CONV_GRAN, CONV_MAX_ROWS, _norm_reject
from .gemm import _pkg, _rows2d
from .images import DCN_OFFSET_COLS, conv1x1_weight, conv3x3_weight, dcn_offset_padded_weight, dcn_offset_weight, stem_weight
from .neck import map_of_rows, rows_of_map


def _out_hw(hw, stride):
    return (int(hw[0]) - 1) // stride + 1, (int(hw[1]) - 1) // stride + 1


def deform_conv_rows(rows, n_img, hw, offs, weight, *, bias=None, bn=None, relu=False, stride=1, out=None, tag="deform_conv_rows"):
    """A modulated deformable 3 x 3 convolution over channel-last rows (``bevmsda_deform_conv_f32``): ``rows`` (n_img H W, C_in),
    ``hw = (H, W)``, ``offs`` the (n_img Ho Wo, >= 32) offset matrix (column 2 k = dy, 2 k + 1 = dx, 18 + k = mask logit of tap
    k; unit column stride), ``weight`` (C_out, C_in, 3, 3) — padding 1, dilation 1, ``stride`` 1 or 2 —, then ``+ bias`` (C_out)
    OR the inference BatchNorm ``bn`` (a module in eval mode: its four vectors and ``eps`` are read by the kernel), then ReLU when
    ``relu``.  ``out``: an optional (n_img Ho Wo, C_out) destination with unit column stride.  Returns (n_img Ho Wo, C_out) rows,
    or ``None`` when the call is not covered."""
    mode = _m().gemm
    tensors = [rows, offs, weight] + [t for t in (bias, out) if t is not None]
    if mode not in ("split", "bf16") or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return None
    if bias is not None and bn is not None:
        return None
    H, W, n_img = int(hw[0]), int(hw[1]), int(n_img)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or stride not in (1, 2):
        return None
    N, C = int(weight.shape[0]), int(weight.shape[1])
    if C % CONV_GRAN or N % CONV_GRAN or rows.shape[-1] != C or rows.numel() != n_img * H * W * C or n_img * H * W > CONV_MAX_ROWS:
        return None
    Ho, Wo = _out_hw((H, W), stride)
    M = n_img * Ho * Wo
    if offs.dim() != 2 or offs.shape[0] != M or offs.shape[1] < DCN_OFFSET_COLS or (M and offs.stride(1) != 1):
        return None
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        return None
    if bn is not None:
        if _norm_reject(bn) is not None or bn.training or bn.num_features != N:
            return None
        vecs = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        if not all(v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == N for v in vecs):
            return None
    if out is None:
        y = torch.empty((M, N), dtype=torch.float32, device=rows.device)
    else:
        y = out
        if y.dim() != 2 or tuple(y.shape) != (M, N) or y.stride(1) != 1:
            return None
    if M == 0 or N == 0:
        return y
    blob = conv3x3_weight(weight)
    if blob is None:
        return None
    x2, ldx = _rows2d(rows, C)
    o2 = offs if (M == 1 or offs.stride(0) % 4 == 0) and offs.data_ptr() % 16 == 0 else offs.contiguous()
    ld_offs = o2.stride(0) if M > 1 else o2.shape[1]
    desc = _lib.DeformConvDesc(x=_ptr(x2), ld_x=ldx, offs=_ptr(o2), ld_offs=ld_offs, n_img=n_img, H=H, W=W, c_in=C, c_out=N,
                               stride=stride, relu=int(bool(relu)), precision=_precision(), bias=_optr(bias))
    if bn is not None:
        desc.eps = float(bn.eps)
        for i, v in enumerate((bn.weight, bn.bias, bn.running_mean, bn.running_var)):
            desc.bn[i] = _ptr(v)
    K = 9 * C
    ld_y = y.stride(0) if M > 1 else N
    # algorithmic bytes: every input row once, the weight, the offset rows, the output
    timer = _gemm_ctx(tag, 2.0 * M * N * K, 4.0 * (n_img * H * W * C + N * K + M * DCN_OFFSET_COLS + M * N))
    return y if _launch(y.device, "deform_conv", lambda lib, stream: lib.bevmsda_deform_conv_f32(
        ctypes.byref(desc), _ptr(blob), _ptr(y), ld_y, stream), timer=timer) else None


def dcn_offsets(rows, n_img, hw, conv_offset, stride):
    """The (n_img Ho Wo, 32) offset matrix of a DCNv2 pack from ONE ``bevmsda_conv_rows_f32`` launch: ``conv_offset`` (a
    ``Conv2d(C_in, 27, 3, stride, padding=1)``) over the channel-last ``rows``, its weight zero-padded to 32 output channels
    (``dcn_offset_weight``: a cached image), its bias padded alike — columns 27 .. 31 are zeros.  Always in ``split`` precision
    (module docstring).  ``None`` when the call is not covered."""
    w, b = conv_offset.weight, conv_offset.bias
    tensors = [rows, w] + ([b] if b is not None else [])
    if _m().gemm not in ("split", "bf16") or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return None
    H, W, n_img = int(hw[0]), int(hw[1]), int(n_img)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != 27 or stride not in (1, 2):
        return None
    C = int(w.shape[1])
    if C % CONV_GRAN or rows.shape[-1] != C or rows.numel() != n_img * H * W * C or n_img * H * W > CONV_MAX_ROWS:
        return None
    Ho, Wo = _out_hw((H, W), stride)
    M, N = n_img * Ho * Wo, DCN_OFFSET_COLS
    y = torch.empty((M, N), dtype=torch.float32, device=rows.device)
    if M == 0:
        return y
    image = dcn_offset_weight(w, b)
    if image is None:
        return None
    blob, b32 = image
    x2, ldx = _rows2d(rows, C)
    desc = _lib.ConvRowsDesc(x=_ptr(x2), ld_x=ldx, n_img=n_img, H=H, W=W, c_in=C, c_out=N, taps=9, stride=stride, relu_in=0,
                             precision=0, bias=_ptr(b32))
    timer = _gemm_ctx("dcn_offsets", 2.0 * M * N * 9 * C, 4.0 * (n_img * H * W * C + N * 9 * C + M * N))
    return y if _launch(y.device, "conv_rows", lambda lib, stream: lib.bevmsda_conv_rows_f32(
        ctypes.byref(desc), _ptr(blob), _ptr(y), N, stream), timer=timer) else None


def _pack_reject(conv):
    """Why ``conv`` is not a covered DCNv2 pack (structure only), or ``None``."""
    off = getattr(conv, "conv_offset", None)
    w = getattr(conv, "weight", None)
    if not isinstance(off, nn.Conv2d) or not torch.is_tensor(w) or w.dim() != 4:
        return "not a ModulatedDeformConv2dPack"
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    try:
        k, s, p, d = pair(conv.kernel_size), pair(conv.stride), pair(conv.padding), pair(conv.dilation)
        groups, dg = int(conv.groups), int(conv.deform_groups)
    except (AttributeError, TypeError):
        return "not a ModulatedDeformConv2dPack"
    if k != (3, 3):
        return "the convolution is not 3 x 3"
    if s not in ((1, 1), (2, 2)):
        return "the stride is not 1 or 2"
    if d != (1, 1):
        return "the convolution is dilated"
    if p != (1, 1):
        return "the padding is not 1"
    if groups != 1 or dg != 1:
        return "groups or deform_groups above 1"
    if tuple(off.kernel_size) != k or tuple(off.stride) != s or pair(off.padding) != p or tuple(off.dilation) != d \
            or off.groups != 1 or off.out_channels != 27 or off.in_channels != w.shape[1] \
            or getattr(off, "padding_mode", "zeros") != "zeros":
        return "conv_offset does not match the convolution"
    if tuple(w.shape[2:]) != (3, 3) or w.shape[1] % CONV_GRAN or w.shape[0] % CONV_GRAN:
        return f"channel counts are not multiples of {CONV_GRAN}"
    return None


def dcn_reject(conv, x, norm=None):
    """Why ``dcn`` does not cover the DCNv2 pack ``conv`` (with the BatchNorm ``norm`` in its epilogue) on the map ``x`` (B, C, H,
    W; ``None``: the modules alone are judged) — a short reason — or ``None`` when it does.  The switch itself
    (``modes.dcn_fused``) is the caller's to test.  Structure first, then shapes, then modes, then devices and dtypes."""
    why = _pack_reject(conv)
    if why is not None:
        return why
    bias = getattr(conv, "bias", None)
    if norm is not None:
        why = _norm_reject(norm)
        if why is not None:
            return why
        if bias is not None:
            return "a bias and a norm (one epilogue)"
        if norm.num_features != conv.weight.shape[0]:
            return "the norm does not match the convolution"
        if norm.training:
            return "the norm is in train() mode (batch statistics)"
    if x is not None:
        if not torch.is_tensor(x) or x.dim() != 4:
            return "not a (B, C, H, W) tensor"
        if x.shape[1] != conv.weight.shape[1]:
            return "the input does not match the convolution"
        if x.shape[0] * x.shape[2] * x.shape[3] > CONV_MAX_ROWS:
            return "more than 2^24 rows"
    if torch.is_grad_enabled():
        return "grad mode is on"
    if _m().gemm not in ("split", "bf16"):
        return f"GEMM mode {_m().gemm}"
    params = [conv.weight, conv.conv_offset.weight] + [t for t in (bias, conv.conv_offset.bias) if t is not None]
    if norm is not None:
        params += [norm.weight, norm.bias, norm.running_mean, norm.running_var]
    if not all(p.is_cuda and p.dtype == torch.float32 for p in params):
        return "not CUDA fp32 parameters"
    if x is not None and not (x.is_cuda and x.dtype == torch.float32):
        return "not a CUDA fp32 input"
    return None


def dcn(conv, x, norm=None, relu=False):
    """A DCNv2 pack on the deformable kernel: ``relu?(norm?(conv(x)))`` for the NCHW map ``x`` in two launches — the offset
    matrix (``dcn_offsets``), then the deformable convolution with the bias or ``norm`` and the ReLU in its epilogue
    (``deform_conv_rows``) -> the (B, C_out, Ho, Wo)-shaped view of channel-last rows, or ``None`` when the call is not covered
    (``dcn_reject``).  A launch the kernels decline after ``dcn_reject`` has accepted the call is an error, not a detour."""
    if dcn_reject(conv, x, norm) is not None:
        return None
    ops = _pkg()
    B, _, H, W = x.shape
    stride = conv.stride[0] if isinstance(conv.stride, (tuple, list)) else int(conv.stride)
    rows = rows_of_map(x)
    offs = ops.dcn_offsets(rows, B, (H, W), conv.conv_offset, stride)
    y = None if offs is None else ops.deform_conv_rows(rows, B, (H, W), offs, conv.weight, bias=getattr(conv, "bias", None), bn=norm,
                                                       relu=relu, stride=stride, tag="dcn")
    if y is None:
        raise RuntimeError("bevmsda: dcn: a kernel declined a call dcn_reject had accepted")
    return map_of_rows(y, B, _out_hw((H, W), stride))


# ---- the plain convolutions of a bottleneck on the row convolution + BatchNorm kernel (csrc/conv_bn_rows.h)

def conv_bn_rows(rows, n_img, hw, weight, bn, *, stride=1, relu=False, res=None, out=None, tag="conv_bn_rows"):
    """``act(bn(conv(x)) + res)`` over channel-last rows (``bevmsda_conv_bn_rows_f32``): ``rows`` (n_img H W, C_in),
    ``hw = (H, W)``, ``weight`` (C_out, C_in, 1, 1) — padding 0 — or (C_out, C_in, 3, 3) — padding 1 — of a convolution without
    bias, ``stride`` 1 or 2 for both, ``bn`` a BatchNorm module in eval mode (its four vectors and ``eps`` are read by the kernel,
    nothing is derived on the host), ``res`` optional (n_img Ho Wo, C_out) rows added after the norm, then ReLU when ``relu``.
    ``out``: an optional (n_img Ho Wo, C_out) destination with unit column stride (its row stride may exceed its width).
    Returns (n_img Ho Wo, C_out) rows with Ho = (H - 1) // stride + 1, or ``None`` when the call is not covered."""
    mode = _m().gemm
    tensors = [rows, weight] + [t for t in (res, out) if t is not None]
    if mode not in ("split", "bf16") or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors) \
            or _norm_reject(bn) is not None or bn.training:
        return None
    H, W, n_img = int(hw[0]), int(hw[1]), int(n_img)
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (1, 3) or stride not in (1, 2):
        return None
    taps = int(weight.shape[2]) ** 2
    N, C = int(weight.shape[0]), int(weight.shape[1])
    if C % CONV_GRAN or N % CONV_GRAN or rows.shape[-1] != C or rows.numel() != n_img * H * W * C \
            or n_img * H * W > CONV_MAX_ROWS or bn.num_features != N:
        return None
    vecs = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if not all(v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == N for v in vecs):
        return None
    Ho, Wo = _out_hw((H, W), stride)
    M = n_img * Ho * Wo
    if res is not None and (res.shape[-1] != N or res.numel() != M * N):
        return None
    if out is None:
        y = torch.empty((M, N), dtype=torch.float32, device=rows.device)
    else:
        y = out
        if y.dim() != 2 or tuple(y.shape) != (M, N) or y.stride(1) != 1:
            return None
    if M == 0 or N == 0:
        return y
    blob = conv3x3_weight(weight) if taps == 9 else conv1x1_weight(weight)
    if blob is None:
        return None
    x2, ldx = _rows2d(rows, C)
    desc = _lib.ConvBnRowsDesc(x=_ptr(x2), ld_x=ldx, eps=float(bn.eps), n_img=n_img, H=H, W=W, c_in=C, c_out=N, taps=taps,
                               stride=stride, relu=int(bool(relu)), precision=_precision())
    for i, v in enumerate(vecs):
        desc.bn[i] = _ptr(v)
    keep = [x2]
    if res is not None:
        r2, ldres = _rows2d(res, N)
        keep.append(r2)
        desc.res, desc.ld_res = _ptr(r2), ldres
    K = taps * C
    ld_y = y.stride(0) if M > 1 else N
    # algorithmic bytes: every input row a tap can reach once (a 1 x 1 stride-2 convolution reads one pixel in four), the
    # weight, the four norm vectors, the residual, the output
    rows_read = M if taps == 1 else n_img * H * W
    timer = _gemm_ctx(tag, 2.0 * M * N * K, 4.0 * (rows_read * C + N * K + 4 * N + M * N * (2 if res is not None else 1)))
    return y if _launch(y.device, "conv_bn_rows", lambda lib, stream: lib.bevmsda_conv_bn_rows_f32(
        ctypes.byref(desc), _ptr(blob), _ptr(y), ld_y, stream), timer=timer) else None


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _bottleneck_parts(block):
    """(conv1, norm1, conv2, norm2, conv3, norm3, downsample or None) of a ResNet bottleneck, by attribute (``_block_parts``:
    the in-tree block names its norms ``bn1`` .., mmdet's ``norm1`` ..), or ``None`` when one is missing."""
    get = lambda *names: next((getattr(block, n) for n in names if hasattr(block, n)), None)
    parts = (get("conv1"), get("bn1", "norm1"), get("conv2"), get("bn2", "norm2"), get("conv3"), get("bn3", "norm3"))
    if any(p is None for p in parts) or not hasattr(block, "downsample"):
        return None
    return parts + (block.downsample,)


def _plain_conv_reject(conv, k):
    """Why ``conv`` is not a bare k x k ``nn.Conv2d`` the row kernel covers (padding k // 2, stride 1 or 2, no bias), or ``None``."""
    if not isinstance(conv, nn.Conv2d):
        return "a convolution is not a Conv2d"
    if tuple(conv.kernel_size) != (k, k):
        return f"a convolution is not {k} x {k}"
    if conv.bias is not None:
        return "a convolution has a bias"
    if tuple(conv.dilation) != (1, 1):
        return "a convolution is dilated"
    if conv.groups != 1:
        return "a convolution is grouped"
    if _pair(conv.padding) != (k // 2, k // 2) or getattr(conv, "padding_mode", "zeros") != "zeros":
        return f"a convolution's padding is not {k // 2} (zeros)"
    if tuple(conv.stride) not in ((1, 1), (2, 2)):
        return "a stride is not 1 or 2"
    if conv.in_channels % CONV_GRAN or conv.out_channels % CONV_GRAN:
        return f"channel counts are not multiples of {CONV_GRAN}"
    return None


def bottleneck_reject(block, x=None):
    """Why ``bottleneck`` does not cover ``block`` (a ResNet bottleneck: the in-tree class or mmdet's) on the map ``x`` (B, C, H,
    W; ``None``: the module alone is judged) — a short reason — or ``None`` when it does.  The switch itself
    (``modes.backbone_fused``) is the caller's to test.  Structure first, then shapes, then modes, then devices and dtypes."""
    why = _bottleneck_structure_reject(block, x)
    if why is not None:
        return why
    if torch.is_grad_enabled():
        return "grad mode is on"
    if _m().gemm not in ("split", "bf16"):
        return f"GEMM mode {_m().gemm}"
    params = list(block.parameters()) + [b for b in block.buffers() if b.is_floating_point()]
    if not all(p.is_cuda and p.dtype == torch.float32 for p in params):
        return "not CUDA fp32 parameters"
    if x is not None and not (x.is_cuda and x.dtype == torch.float32):
        return "not a CUDA fp32 input"
    conv2, n2 = _bottleneck_parts(block)[2:4]
    return dcn_reject(conv2, None, n2) if not isinstance(conv2, nn.Conv2d) else None


def _bottleneck_structure_reject(block, x=None, norm_modes=True, pack_bias="a convolution has a bias"):
    """``bottleneck_reject``'s rules on the block's structure and the input's shape, in its order; ``norm_modes=False`` leaves the
    norms' ``train()`` state to the caller; ``pack_bias``: the reason given for a DCNv2 ``conv2`` with a bias."""
    parts = _bottleneck_parts(block)
    if parts is None:
        return "not a bottleneck (conv1 / norm1 / conv2 / norm2 / conv3 / norm3 / downsample)"
    conv1, n1, conv2, n2, conv3, n3, ds = parts
    if not isinstance(getattr(block, "relu", None), nn.ReLU):
        return "a block's activation is not ReLU"
    if getattr(block, "with_plugins", False):
        return "a block has plugins"
    pairs = [(conv1, n1, 1), (conv3, n3, 1)]
    if ds is not None:
        try:
            mods = list(ds)
        except TypeError:
            return "a downsample is not conv + norm"
        if len(mods) != 2:
            return "a downsample is not conv + norm"
        pairs.append((mods[0], mods[1], 1))
    packed = not isinstance(conv2, nn.Conv2d)
    if packed:
        why = _pack_reject(conv2)
        if why is None and getattr(conv2, "bias", None) is not None:
            why = pack_bias
        if why is not None:
            return why
        c2_in, c2_out, s2 = int(conv2.weight.shape[1]), int(conv2.weight.shape[0]), _pair(conv2.stride)[0]
    else:
        pairs.insert(1, (conv2, n2, 3))
        c2_in, c2_out, s2 = conv2.in_channels, conv2.out_channels, conv2.stride[0]
    for conv, norm, k in pairs:
        why = _plain_conv_reject(conv, k)
        if why is not None:
            return why
    for conv, norm, k in pairs + ([(conv2, n2, 3)] if packed else []):
        why = _norm_reject(norm)
        if why is not None:
            return why
        if norm.num_features != (c2_out if conv is conv2 else conv.out_channels):
            return "a norm does not match its convolution"
        if norm_modes and norm.training:
            return "a norm is in train() mode (batch statistics)"
    if c2_in != conv1.out_channels or conv3.in_channels != c2_out:
        return "a block's convolutions do not chain"
    total = conv1.stride[0] * s2 * conv3.stride[0]
    if ds is None:
        if total != 1 or conv1.in_channels != conv3.out_channels:
            return "a block without downsample changes the shape"
    else:
        dconv = pairs[-1][0]
        if dconv.in_channels != conv1.in_channels or dconv.out_channels != conv3.out_channels or dconv.stride[0] != total:
            return "a downsample does not match its block"
    if x is not None:
        if not torch.is_tensor(x) or x.dim() != 4:
            return "not a (B, C, H, W) tensor"
        if x.shape[1] != conv1.in_channels:
            return "the input does not match the block"
        if x.shape[0] * x.shape[2] * x.shape[3] > CONV_MAX_ROWS:
            return "more than 2^24 rows"
    return None


def bottleneck(block, x):
    """A ResNet bottleneck on rows: ``relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + identity)`` for the NCHW map ``x``
    -> the NCHW-shaped view of channel-last rows, or ``None`` when the call is not covered (``bottleneck_reject``).

    Schedule on ``rows_of_map(x)``: conv1 + bn1 + ReLU; conv2 + bn2 + ReLU (``conv_bn_rows``, or for a DCNv2 pack ``dcn_offsets`` +
    ``deform_conv_rows`` directly on the rows, whatever ``modes.dcn_fused`` says); the identity (``downsample`` as one launch
    without ReLU, or the input rows); conv3 + bn3 + identity + ReLU in one launch.  3 launches per plain block, 4 with a
    downsample, one more for a pack's offsets; no ``contiguous()``, no permute, no add or ReLU launch.  A dense channels-last
    input is read in place, anything else costs the one copy of ``rows_of_map``.  A launch the kernels decline after
    ``bottleneck_reject`` has accepted the call is an error, not a detour."""
    if bottleneck_reject(block, x) is not None:
        return None
    ops = _pkg()
    conv1, n1, conv2, n2, conv3, n3, ds = _bottleneck_parts(block)
    B, _, H, W = x.shape
    rows = rows_of_map(x)

    def need(y):
        if y is None:
            raise RuntimeError("bevmsda: bottleneck: a kernel declined a call bottleneck_reject had accepted")
        return y

    def conv(r, hw, c, n, relu, tag, res=None):
        return need(ops.conv_bn_rows(r, B, hw, c.weight, n, stride=c.stride[0], relu=relu, res=res, tag=tag))

    hw = (int(H), int(W))
    out = conv(rows, hw, conv1, n1, True, "bottleneck_conv1")
    hw = _out_hw(hw, conv1.stride[0])
    if isinstance(conv2, nn.Conv2d):
        s2 = conv2.stride[0]
        out = conv(out, hw, conv2, n2, True, "bottleneck_conv2")
    else:
        s2 = _pair(conv2.stride)[0]
        offs = need(ops.dcn_offsets(out, B, hw, conv2.conv_offset, s2))
        out = need(ops.deform_conv_rows(out, B, hw, offs, conv2.weight, bn=n2, relu=True, stride=s2, tag="bottleneck_dcn"))
    hw = _out_hw(hw, s2)
    identity = rows if ds is None else conv(rows, (int(H), int(W)), ds[0], ds[1], False, "bottleneck_downsample")
    out = conv(out, hw, conv3, n3, True, "bottleneck_conv3", res=identity)
    return map_of_rows(out, B, _out_hw(hw, conv3.stride[0]))


# ---- training a backbone with frozen BatchNorms: the backward of ``conv_bn_rows`` on rows (csrc/conv_bwd_rows.h)

def _bn_scale_ok(bn, N):
    """Is ``bn`` a BatchNorm in eval mode whose scale the kernels can form (gamma and the running variance, contiguous CUDA fp32)?"""
    if _norm_reject(bn) is not None or bn.training or bn.num_features != N:
        return False
    return all(v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == N for v in (bn.weight, bn.running_var))


def conv_gz_rows(g, y=None, bn=None, *, out=None, tag="conv_gz_rows"):
    """``g * (y > 0) * scale`` over (M, C) rows in one launch (``bevmsda_conv_gz_rows_f32``): ``y`` the saved output of a
    convolution + norm + ReLU (``None``: no mask), ``bn`` its norm in eval mode (``None``: scale 1).  Without ``bn`` this is the
    gradient a block's last ReLU hands to both of its branches.  Returns the rows, or ``None`` when the call is not covered."""
    tensors = [g] + [t for t in (y, out) if t is not None]
    if torch.is_grad_enabled() or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return None
    C = int(g.shape[-1])
    if C % CONV_GRAN or (y is not None and tuple(y.shape) != tuple(g.shape)) or (bn is not None and not _bn_scale_ok(bn, C)):
        return None
    g2, ldg = _rows2d(g, C)
    M = g2.shape[0]
    if M > CONV_MAX_ROWS:
        return None
    gz = torch.empty((M, C), dtype=torch.float32, device=g.device) if out is None else out
    if gz.dim() != 2 or tuple(gz.shape) != (M, C) or gz.stride(1) != 1:
        return None
    if M == 0:
        return gz
    y2, ldy = _rows2d(y, C) if y is not None else (None, 0)
    ld_gz = gz.stride(0) if M > 1 else C
    timer = _gemm_ctx(tag, 2.0 * M * C, 4.0 * M * C * (3 if y is not None else 2))
    return gz if _launch(g.device, "conv_gz_rows", lambda lib, stream: lib.bevmsda_conv_gz_rows_f32(
        _ptr(g2), ldg, _optr(y2), ldy, _optr(bn.weight if bn is not None else None),
        _optr(bn.running_var if bn is not None else None), float(bn.eps) if bn is not None else 0.0, M, C, _ptr(gz), ld_gz, stream),
        timer=timer) else None


def conv_bn_rows_backward(g, y, rows, n_img, hw, weight, bn, *, stride=1, relu=False, add=None, need_dx=True, need_dw=True,
                          next_mask=None, next_bn=None, dx_out=None, dw_out=None, tag="conv_bn_rows_backward",
                          add_pool2=False, add_after_mask=False, relu_x=False, db_out=None):
    """The backward of ``conv_bn_rows`` with a frozen norm, one launch per gradient: ``g`` (n_img Ho Wo, C_out) the gradient
    w.r.t. the output ``y`` of ``act(bn(conv(x)) + res)``, ``rows`` the (n_img H W, C_in) input, ``hw = (H, W)`` the INPUT size.
    With ``gz = g * (y > 0 if relu) * scale`` (``y=None`` or ``relu=False``: no mask — ``g`` is masked already or there was no ReLU;
    ``bn=None``: scale 1 — ``g`` is a finished ``gz``; the residual's gradient is ``g * mask``, the caller's: ``conv_gz_rows``):

    * ``dx`` (``bevmsda_conv_dgrad_rows_f32``; ``need_dx``): ``conv_transpose(gz, weight) + add``, then with ``next_mask`` — the saved
      output of the convolution that produced ``rows`` — ``* (next_mask > 0) * scale(next_bn)``: the ``gz`` of that convolution.
      ``add``: (n_img H W, C_in) rows; ``dx_out``: an optional destination with unit column stride, which may be ``add`` itself.
      ``add_pool2``: ``add`` is the rows of the (n_img, 2H, 2W) map and its 2 x 2 sums are added (the transpose of ``conv_rows``'s
      ``res_up``; never ``dx_out`` itself); ``add_after_mask`` (with ``next_mask``): the mask and scale apply to the convolution
      path only, ``add`` joins afterwards.
    * ``dW`` (``bevmsda_conv_wgrad_rows_f32``; ``need_dw``): fp32, in ``weight``'s own shape, accumulated with atomics into
      ``dw_out`` (contiguous, the caller's to zero) or into fresh zeros.  ``relu_x``: the forward convolved ``relu(rows)``
      (``conv_rows``'s ``relu_in``).  ``db_out``: a contiguous (C_out) vector, the caller's to zero, into which the same launch
      accumulates the bias gradient ``gz.sum(0)`` (with ``need_dw`` only).

    Returns ``(dx, dW)`` (``None`` for one not asked for) — with ``db_out`` ``(dx, dW, db)`` —, or ``None`` when the call is not
    covered."""
    mode = _m().gemm
    tensors = [g, weight] + [t for t in (y, rows, add, next_mask, dx_out, dw_out, db_out) if t is not None]
    if mode not in ("split", "bf16") or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return None
    H, W, n_img = int(hw[0]), int(hw[1]), int(n_img)
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (1, 3) or stride not in (1, 2) \
            or not weight.is_contiguous():
        return None
    taps = int(weight.shape[2]) ** 2
    N, C = int(weight.shape[0]), int(weight.shape[1])
    Ho, Wo = _out_hw((H, W), stride)
    M_in, M = n_img * H * W, n_img * Ho * Wo
    if C % CONV_GRAN or N % CONV_GRAN or M_in > CONV_MAX_ROWS or M_in == 0 or g.shape[-1] != N or g.numel() != M * N:
        return None
    mask = y if relu else None
    if mask is not None and (mask.shape[-1] != N or mask.numel() != M * N):
        return None
    if (bn is not None and not _bn_scale_ok(bn, N)) or (next_bn is not None and (next_mask is None or not _bn_scale_ok(next_bn, C))):
        return None
    for t in (None if add_pool2 else add, next_mask) + ((rows,) if need_dw else ()):
        if t is not None and (t.shape[-1] != C or t.numel() != M_in * C):
            return None
    if need_dw and rows is None:
        return None
    if (add_pool2 or add_after_mask) and add is None or (add_after_mask and next_mask is None):
        return None
    if add_pool2 and (add.shape[-1] != C or add.numel() != 4 * M_in * C or 4 * M_in > CONV_MAX_ROWS or add is dx_out):
        return None
    if db_out is not None and (not need_dw or db_out.numel() != N or not db_out.is_contiguous()):
        return None
    g2, ldg = _rows2d(g, N)
    y2, ldy = _rows2d(mask, N) if mask is not None else (None, 0)
    gamma, var, eps = (bn.weight, bn.running_var, float(bn.eps)) if bn is not None else (None, None, 0.0)
    common = dict(g=_ptr(g2), ld_g=ldg, y=_optr(y2), ld_y=ldy, gamma=_optr(gamma), var=_optr(var), eps=eps, n_img=n_img, H=H, W=W,
                  c_in=C, c_out=N, taps=taps, stride=stride, precision=_precision())
    K = taps * N
    dx = dw = None
    if need_dw:
        dw = torch.zeros_like(weight) if dw_out is None else dw_out
        if tuple(dw.shape) != tuple(weight.shape) or not dw.is_contiguous():
            return None
        x2, ldx = _rows2d(rows, C)
        wdesc = _lib.ConvWgradRowsDesc(x=_ptr(x2), ld_x=ldx, relu_x=int(bool(relu_x)), dbias=_optr(db_out), **common)
        rows_read = M if taps == 1 else M_in
        timer = _gemm_ctx(tag + "_wgrad", 2.0 * M * N * taps * C, 4.0 * (M * N * (2 if mask is not None else 1) + rows_read * C + N * taps * C))
        if not _launch(g.device, "conv_wgrad_rows", lambda lib, stream: lib.bevmsda_conv_wgrad_rows_f32(
                ctypes.byref(wdesc), _ptr(dw), stream), timer=timer):
            return None
    if need_dx:
        dx = torch.empty((M_in, C), dtype=torch.float32, device=g.device) if dx_out is None else dx_out
        if dx.dim() != 2 or tuple(dx.shape) != (M_in, C) or dx.stride(1) != 1:
            return None
        blob = _pkg().conv_dgrad_weight(weight)
        if blob is None:
            return None
        ddesc = _lib.ConvDgradRowsDesc(add_mode=_lib.CONV_ADD_POOL2 if add_pool2 else _lib.CONV_ADD_SAME,
                                       add_after_mask=int(bool(add_after_mask)), **common)
        keep = []
        if add is not None:
            a2, ld_add = (dx, dx.stride(0) if M_in > 1 else C) if add is dx else _rows2d(add, C)
            keep.append(a2)
            ddesc.add, ddesc.ld_add = _ptr(a2), ld_add
        if next_mask is not None:
            m2, ld_m = _rows2d(next_mask, C)
            keep.append(m2)
            ddesc.next_mask, ddesc.ld_next_mask = _ptr(m2), ld_m
            if next_bn is not None:
                ddesc.next_gamma, ddesc.next_var, ddesc.next_eps = _ptr(next_bn.weight), _ptr(next_bn.running_var), float(next_bn.eps)
        ld_dx = dx.stride(0) if M_in > 1 else C
        extra = (add is not None) * (4 if add_pool2 else 1) + (next_mask is not None)
        timer = _gemm_ctx(tag + "_dgrad", 2.0 * M * N * taps * C, 4.0 * (M * N * (2 if mask is not None else 1) + C * K + M_in * C * (1 + extra)))
        if not _launch(g.device, "conv_dgrad_rows", lambda lib, stream: lib.bevmsda_conv_dgrad_rows_f32(
                ctypes.byref(ddesc), _ptr(blob), _ptr(dx), ld_dx, stream), timer=timer):
            return None
    return (dx, dw) if db_out is None else (dx, dw, db_out)


def deform_conv_rows_backward(g, y, rows, n_img, hw, offs, weight, bn, *, stride=1, relu=False, need_dx=True, need_doffs=True,
                              need_dw=True, dx_out=None, doffs_out=None, dw_out=None, tag="deform_conv_rows_backward"):
    """The backward of ``deform_conv_rows`` with a frozen norm: ``g`` (n_img Ho Wo, C_out) the gradient w.r.t. the output ``y`` of
    ``act(bn(deform_conv(x, offs, w)))``, ``rows`` the (n_img H W, C_in) input, ``hw = (H, W)`` the INPUT size, ``offs`` the
    (n_img Ho Wo, >= 32) offset matrix of the forward.  ``gz = g * (y > 0 if relu) * scale`` exactly as in ``conv_bn_rows_backward``
    (``y=None`` or ``relu=False``: no mask; ``bn=None``: ``g`` is a finished ``gz``).

    * ``dx`` (n_img H W, C_in) and ``doffs`` (n_img Ho Wo, 32) — the gradient w.r.t. ``offs`` in its own layout, columns 27 .. 31
      never written — come from ONE launch (``bevmsda_deform_conv_dgrad_f32``; ``need_dx`` / ``need_doffs`` leave either out).  Both
      are ACCUMULATED into with atomics: ``dx_out`` / ``doffs_out`` (unit column stride) are the caller's to zero; fresh zeros
      are used when absent.
    * ``dW`` (``bevmsda_deform_conv_wgrad_f32``; ``need_dw``): fp32, in ``weight``'s shape, accumulated into ``dw_out``
      (contiguous, the caller's to zero) or fresh zeros.

    GEMM timer tags: ``tag + "_dgrad"`` and ``tag + "_wgrad"``.  Returns ``(dx, doffs, dW)`` (``None`` for one not asked for), or
    ``None`` when the call is not covered."""
    mode = _m().gemm
    tensors = [g, rows, offs, weight] + [t for t in (y, dx_out, doffs_out, dw_out) if t is not None]
    if mode not in ("split", "bf16") or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return None
    H, W, n_img = int(hw[0]), int(hw[1]), int(n_img)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or stride not in (1, 2) or not weight.is_contiguous():
        return None
    N, C = int(weight.shape[0]), int(weight.shape[1])
    Ho, Wo = _out_hw((H, W), stride)
    M_in, M = n_img * H * W, n_img * Ho * Wo
    if C % CONV_GRAN or N % CONV_GRAN or M_in > CONV_MAX_ROWS or M_in == 0 or g.shape[-1] != N or g.numel() != M * N \
            or rows.shape[-1] != C or rows.numel() != M_in * C:
        return None
    if offs.dim() != 2 or offs.shape[0] != M or offs.shape[1] < DCN_OFFSET_COLS or (M > 1 and offs.stride(1) != 1):
        return None
    mask = y if relu else None
    if mask is not None and (mask.shape[-1] != N or mask.numel() != M * N):
        return None
    if bn is not None and not _bn_scale_ok(bn, N):
        return None
    g2, ldg = _rows2d(g, N)
    y2, ldy = _rows2d(mask, N) if mask is not None else (None, 0)
    x2, ldx = _rows2d(rows, C)
    o2 = offs if (M == 1 or offs.stride(0) % 4 == 0) and offs.data_ptr() % 16 == 0 else offs.contiguous()
    ld_offs = o2.stride(0) if M > 1 else o2.shape[1]
    gamma, var, eps = (bn.weight, bn.running_var, float(bn.eps)) if bn is not None else (None, None, 0.0)
    common = dict(g=_ptr(g2), ld_g=ldg, y=_optr(y2), ld_y=ldy, gamma=_optr(gamma), var=_optr(var), eps=eps, x=_ptr(x2), ld_x=ldx,
                  offs=_ptr(o2), ld_offs=ld_offs, n_img=n_img, H=H, W=W, c_in=C, c_out=N, stride=stride, precision=_precision())
    gbytes = M * N * (2 if mask is not None else 1)
    dx = doffs = dw = None
    if need_dx or need_doffs:
        if need_dx:
            dx = torch.zeros((M_in, C), dtype=torch.float32, device=g.device) if dx_out is None else dx_out
            if dx.dim() != 2 or tuple(dx.shape) != (M_in, C) or dx.stride(1) != 1:
                return None
        if need_doffs:
            doffs = torch.zeros((M, DCN_OFFSET_COLS), dtype=torch.float32, device=g.device) if doffs_out is None else doffs_out
            if doffs.dim() != 2 or tuple(doffs.shape) != (M, DCN_OFFSET_COLS) or doffs.stride(1) != 1:
                return None
        blob = _pkg().deform_dgrad_weight(weight)
        if blob is None:
            return None
        ddesc = _lib.DeformConvDgradDesc(need_dx=int(need_dx), need_doffs=int(need_doffs), **common)
        if need_dx:
            ddesc.dx, ddesc.ld_dx = _ptr(dx), dx.stride(0) if M_in > 1 else C
        if need_doffs:
            ddesc.doffs, ddesc.ld_doffs = _ptr(doffs), doffs.stride(0) if M > 1 else DCN_OFFSET_COLS
        # algorithmic bytes: gz, the weight, the offset rows; the corner rows read for doffs; the rows added to
        timer = _gemm_ctx(tag + "_dgrad", 2.0 * M * N * 9 * C, 4.0 * (gbytes + 9 * C * N + M * DCN_OFFSET_COLS
                          + (M_in * C + M * DCN_OFFSET_COLS if need_doffs else 0) + (M_in * C if need_dx else 0)))
        if not _launch(g.device, "deform_conv_dgrad", lambda lib, stream: lib.bevmsda_deform_conv_dgrad_f32(
                ctypes.byref(ddesc), _ptr(blob), stream), timer=timer):
            return None
    if need_dw:
        dw = torch.zeros_like(weight) if dw_out is None else dw_out
        if tuple(dw.shape) != tuple(weight.shape) or not dw.is_contiguous():
            return None
        wdesc = _lib.DeformConvWgradDesc(**common)
        timer = _gemm_ctx(tag + "_wgrad", 2.0 * M * N * 9 * C, 4.0 * (gbytes + M_in * C + M * DCN_OFFSET_COLS + N * 9 * C))
        if not _launch(g.device, "deform_conv_wgrad", lambda lib, stream: lib.bevmsda_deform_conv_wgrad_f32(
                ctypes.byref(wdesc), _ptr(dw), stream), timer=timer):
            return None
    return dx, doffs, dw


def _batch_stats_reject(block, x, norms):
    """``bottleneck_train_reject``'s rules for a block with a norm in ``train()`` mode under ``modes.bn_train``, in its order."""
    if not all(n.training for n in norms):
        return "norms in mixed modes"
    convs = _block_convs(block)
    if _is_pack(convs[1][0]):
        return "a deformable conv2 with batch statistics (not yet)"
    if getattr(block, "with_cp", False):
        return "with_cp with batch statistics (not yet)"
    if any(n.momentum is None for n in norms):
        return "a cumulative moving average (momentum=None)"
    if any(isinstance(n, nn.SyncBatchNorm) for n in norms):
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return "SyncBatchNorm across ranks (statistics are not all-reduced here)"
    if x is not None:
        hw = (int(x.shape[2]), int(x.shape[3]))
        hw1 = _out_hw(hw, convs[0][0].stride[0])
        hw2 = _out_hw(hw1, convs[1][0].stride[0])
        if int(x.shape[0]) * min(hw1[0] * hw1[1], hw2[0] * hw2[1]) < 2:      # (conv3 and the downsample keep conv2's output size)
            return "fewer than two values per channel"
    return None


def bottleneck_train_reject(block, x=None):
    """Why ``bottleneck_train`` does not cover ``block`` on the map ``x`` — a short reason — or ``None`` when it does: the rules of
    ``bottleneck_reject`` on the block's structure and the input's shape, then, in this order: a DCNv2 ``conv2`` (without
    ``modes.dcn_train``; with it a pack passes its structural rules and only one with a bias is turned away, in ``dcn_reject``'s
    words), a norm in ``train()`` mode, a norm whose affine parameters train, the GEMM mode, devices and dtypes.  Grad mode is NOT
    a reason.  The switch itself (``modes.backbone_train``) is the caller's to test.

    With ``modes.bn_train`` a block with a norm in ``train()`` mode takes other rules in place of the two on the norms (a block
    whose norms are all in eval mode keeps them): norms in mixed modes, a DCNv2 ``conv2``, ``with_cp``, ``momentum=None``, a
    ``SyncBatchNorm`` while ``torch.distributed`` runs more than one rank, fewer than two output rows for a norm — then the GEMM
    mode, devices and dtypes as above.  The affine parameters may train or be frozen."""
    dcn_train = bool(_m().dcn_train)
    # (with dcn_train a pack is judged by _pack_reject's structural rules, then its bias in dcn_reject's words)
    why = _bottleneck_structure_reject(block, x, norm_modes=False,
                                       **(dict(pack_bias="a bias and a norm (one epilogue)") if dcn_train else {}))
    if why is not None:
        return why
    conv1, n1, conv2, n2, conv3, n3, ds = _bottleneck_parts(block)
    if not isinstance(conv2, nn.Conv2d) and not dcn_train:
        return "a deformable conv2 (no backward yet)"
    norms = [n1, n2, n3] + ([ds[1]] if ds is not None else [])
    if _m().bn_train and any(n.training for n in norms):
        why = _batch_stats_reject(block, x, norms)
        if why is not None:
            return why
    else:
        if any(n.training for n in norms):
            return "a norm is in train() mode (batch statistics)"
        if any(p.requires_grad for n in norms for p in (n.weight, n.bias)):
            return "a norm's affine parameters require a gradient"
    if _m().gemm not in ("split", "bf16"):
        return f"GEMM mode {_m().gemm}"
    params = list(block.parameters()) + [b for b in block.buffers() if b.is_floating_point()]
    if not all(p.is_cuda and p.dtype == torch.float32 for p in params):
        return "not CUDA fp32 parameters"
    if x is not None and not (x.is_cuda and x.dtype == torch.float32):
        return "not a CUDA fp32 input"
    return None


def _need(y, what="bottleneck_train"):
    if y is None:
        raise RuntimeError(f"bevmsda: {what}: a kernel declined a call bottleneck_train_reject had accepted")
    return y


def _block_convs(block):
    """[(conv, norm)] of conv1, conv2, conv3 and, when there is one, the downsample."""
    conv1, n1, conv2, n2, conv3, n3, ds = _bottleneck_parts(block)
    return [(conv1, n1), (conv2, n2), (conv3, n3)] + ([(ds[0], ds[1])] if ds is not None else [])


def _is_pack(conv):
    return not isinstance(conv, nn.Conv2d)


def _block_inner(ops, block, rows, B, hw):
    """conv1 + bn1 + ReLU and conv2 + bn2 + ReLU of a block on rows -> (o1, hw1, offs, o2, hw2); ``offs``: the offset matrix of a
    DCNv2 ``conv2`` (``dcn_offsets`` + ``deform_conv_rows``, as at inference), ``None`` for a plain one."""
    (c1, n1), (c2, n2) = _block_convs(block)[:2]
    o1 = _need(ops.conv_bn_rows(rows, B, hw, c1.weight, n1, stride=c1.stride[0], relu=True, tag="bottleneck_conv1"))
    hw1 = _out_hw(hw, c1.stride[0])
    s2 = _pair(c2.stride)[0]
    if _is_pack(c2):
        offs = _need(ops.dcn_offsets(o1, B, hw1, c2.conv_offset, s2))
        o2 = _need(ops.deform_conv_rows(o1, B, hw1, offs, c2.weight, bn=n2, relu=True, stride=s2, tag="bottleneck_dcn"))
    else:
        offs = None
        o2 = _need(ops.conv_bn_rows(o1, B, hw1, c2.weight, n2, stride=s2, relu=True, tag="bottleneck_conv2"))
    return o1, hw1, offs, o2, _out_hw(hw1, s2)


class _BottleneckTrain(torch.autograd.Function):
    """A whole bottleneck with frozen norms as one node: ``bottleneck``'s launches forward; backward one mask launch, then per
    convolution one weight-gradient and one input-gradient launch, each input gradient's epilogue writing the ``gz`` of the
    convolution before it (``bottleneck_train``).  ``weights``: the block's convolution weights in ``_block_convs``'s order, then
    for a DCNv2 ``conv2`` its ``conv_offset``'s weight and bias."""

    @staticmethod
    def forward(ctx, x, block, *weights):
        ops = _pkg()
        B, _, H, W = x.shape
        hw = (int(H), int(W))
        rows = rows_of_map(x)
        convs = _block_convs(block)
        o1, hw1, offs, o2, hw2 = _block_inner(ops, block, rows, B, hw)
        idt = rows
        if len(convs) == 4:
            dc, dn = convs[3]
            idt = _need(ops.conv_bn_rows(rows, B, hw, dc.weight, dn, stride=dc.stride[0], relu=False, tag="bottleneck_downsample"))
        c3, n3 = convs[2]
        out = map_of_rows(_need(ops.conv_bn_rows(o2, B, hw2, c3.weight, n3, relu=True, res=idt, tag="bottleneck_conv3")), B, hw2)
        ctx.block, ctx.modes, ctx.geom = block, _m().snapshot(), (B, hw, hw1, hw2)
        ctx.recompute = bool(getattr(block, "with_cp", False))
        inner = () if ctx.recompute else ((o1, o2) if offs is None else (o1, offs, o2))
        ctx.save_for_backward(rows, out, *inner, *weights)
        return out

    @staticmethod
    @_forward_modes
    def backward(ctx, g):
        ops, block = _pkg(), ctx.block
        B, hw, hw1, hw2 = ctx.geom
        saved = ctx.saved_tensors
        rows, out = saved[0], rows_of_map(saved[1])
        convs = _block_convs(block)
        (c1, n1), (c2, n2), (c3, n3) = convs[:3]
        pack = _is_pack(c2)
        if ctx.recompute:
            o1, _, offs, o2, _ = _block_inner(ops, block, rows, B, hw)
        elif pack:
            o1, offs, o2 = saved[2:5]
        else:
            (o1, o2), offs = saved[2:4], None
        need_w = ctx.needs_input_grad[2:2 + len(convs)]
        need_x = ctx.needs_input_grad[0]
        need1 = need_x or need_w[0]                     # does anything ahead of conv2 want a gradient?
        need_ow, need_ob = ctx.needs_input_grad[2 + len(convs):] if pack else (False, False)
        # the offsets are a function of o1: their gradient is wanted by conv_offset's parameters and by whatever is ahead of conv2
        need_doffs = pack and (need_ow or need_ob or need1)
        # one zero fill for every weight gradient of the block and, for a pack, for what its atomics add to: dx1, doffs and the
        # offset convolution's weight gradient in its padded (32, C, 3, 3) shape
        sizes = [c.weight.numel() if nw else 0 for (c, _), nw in zip(convs, need_w)]
        C2 = int(c2.weight.shape[1])
        M1, M2 = B * hw1[0] * hw1[1], B * hw2[0] * hw2[1]
        extra = [M1 * C2 if pack and need1 else 0, M2 * DCN_OFFSET_COLS if need_doffs else 0,
                 DCN_OFFSET_COLS * C2 * 9 if need_ow else 0]
        total = sum(sizes) + sum(extra)
        flat = torch.zeros(total, dtype=torch.float32, device=rows.device) if total else None
        dws, o = [], 0
        for (c, _), n in zip(convs, sizes):
            dws.append(flat[o:o + n].view(c.weight.shape) if n else None)
            o += n
        dx1 = doffs = dow = None
        if extra[0]:
            dx1 = flat[o:o + extra[0]].view(M1, C2)
            o += extra[0]
        if extra[1]:
            doffs = flat[o:o + extra[1]].view(M2, DCN_OFFSET_COLS)
            o += extra[1]
        if extra[2]:
            dow = flat[o:o + extra[2]].view(DCN_OFFSET_COLS, C2, 3, 3)
        ds = convs[3] if len(convs) == 4 else None
        bwd = lambda *a, **k: _need(ops.conv_bn_rows_backward(*a, **k))

        gid = _need(ops.conv_gz_rows(rows_of_map(g), out, tag="bottleneck_mask"))       # the identity's gradient, too
        gz2, _ = bwd(gid, None, o2, B, hw2, c3.weight, n3, need_dw=need_w[2], dw_out=dws[2], next_mask=o2, next_bn=n2,
                     tag="bottleneck_conv3")
        s2 = _pair(c2.stride)[0]
        g_ow = g_ob = None
        if not pack:
            gz1, _ = bwd(gz2, None, o1, B, hw1, c2.weight, None, stride=s2, need_dx=need1, need_dw=need_w[1], dw_out=dws[1],
                         next_mask=o1, next_bn=n1, tag="bottleneck_conv2")
        else:
            gz1 = None
            if need1 or need_doffs or need_w[1]:
                _need(ops.deform_conv_rows_backward(gz2, None, o1, B, hw1, offs, c2.weight, None, stride=s2, need_dx=need1,
                                                    need_doffs=need_doffs, need_dw=need_w[1], dx_out=dx1, doffs_out=doffs,
                                                    dw_out=dws[1], tag="bottleneck_dcn"))
            if need1 or need_ow:
                # conv_offset's gradients on the row kernels: g = doffs, no mask, no norm, the weight zero-padded to 32 output
                # channels; always in split precision, as the forward's offset launch.  The input gradient adds to dx1 in place
                # and its epilogue finishes gz1
                w32 = _need(dcn_offset_padded_weight(c2.conv_offset.weight))
                with ops.using(gemm="split"):
                    gz1, _ = bwd(doffs, None, o1, B, hw1, w32, None, stride=s2, need_dx=need1, need_dw=need_ow, dw_out=dow,
                                 add=dx1, dx_out=dx1, next_mask=o1, next_bn=n1, tag="bottleneck_dcn_offset")
            if need_ow:
                g_ow = dow[:27]
            if need_ob:
                g_ob = doffs[:, :27].sum(0)             # one torch reduction: the bias gradient is the column sum of doffs
        dx = None
        if need1:
            dx, _ = bwd(gz1, None, rows, B, hw, c1.weight, None, stride=c1.stride[0], need_dx=need_x, need_dw=need_w[0],
                        dw_out=dws[0], add=gid if ds is None else None, tag="bottleneck_conv1")
        if ds is not None and (need_x or need_w[3]):
            dx, _ = bwd(gid, None, rows, B, hw, ds[0].weight, ds[1], stride=ds[0].stride[0], need_dx=need_x, need_dw=need_w[3],
                        dw_out=dws[3], add=dx, dx_out=dx, tag="bottleneck_downsample")
        return (map_of_rows(dx, B, hw) if need_x else None, None, *dws, *((g_ow, g_ob) if pack else ()))


def bottleneck_train(block, x):
    """``bottleneck`` under autograd for a block whose norms are frozen (eval mode, affine parameters without gradients): ONE
    autograd Function for the whole block -> the NCHW-shaped view of channel-last rows, or ``None`` when the call is not covered
    (``bottleneck_train_reject``).

    Forward: ``bottleneck``'s ``conv_bn_rows`` launches; the input rows, the two inner activations and the output are saved
    (``block.with_cp``: input and output only — the backward recomputes the inner activations with two forward launches).
    Backward: one mask launch ``g * (out > 0)`` (``conv_gz_rows``: the identity's gradient and, scaled by ``bn3`` on the way into
    the kernels, conv3's ``gz``); conv3's weight gradient and its input gradient, whose epilogue writes conv2's ``gz``; the same
    for conv2; conv1's weight gradient and its input gradient with the identity's gradient as ``add``; with a downsample its
    weight gradient and an input gradient that accumulates into the same ``dx`` — 7 launches per plain block, 9 with a downsample,
    one zero fill for all weight gradients; no torch convolution, add or ReLU backward.  An input that needs no gradient (the
    first trainable block after a frozen stage) skips the two input gradients that feed it, a frozen weight its weight gradient.

    With ``modes.dcn_train`` a DCNv2 ``conv2`` is covered.  Forward: ``conv1``, ``dcn_offsets`` (always ``split``), then
    ``deform_conv_rows`` with ``bn2`` and the ReLU, ``conv3``; the offset matrix is saved too (``with_cp``: recomputed, three forward
    launches).  Backward, after conv3's: the deformable input + offset gradient into zeroed ``dx1`` and ``doffs`` (ONE launch) and
    the deformable weight gradient (``deform_conv_rows_backward``); then ``conv_offset``'s weight gradient and its input gradient
    through ``conv_bn_rows_backward`` on ``doffs`` with the weight zero-padded to 32 output channels (always ``split``) — the input
    gradient adds to ``dx1`` in place and its epilogue finishes conv1's ``gz`` —; ``conv_offset.bias``'s gradient is the column
    sum of ``doffs[:, :27]``, one torch reduction.  The block's one zero fill also covers ``dx1``, ``doffs`` and the padded offset
    weight gradient.  Skipped: the deformable weight gradient of a frozen ``conv2.weight``, ``conv_offset``'s weight gradient when
    it is frozen, and the deformable input + offset gradient when nothing ahead of ``conv2`` nor ``conv_offset`` wants one (the
    offsets are a function of conv1's output, so ``doffs`` is formed whenever anything ahead of ``conv2`` wants a gradient).
    ``dx`` is the NCHW-shaped view of channel-last rows: between covered blocks the gradient stays in rows.

    With ``modes.bn_train`` a block whose norms are all in ``train()`` mode (batch statistics; affine parameters trainable or not)
    is one Function on the kernels of ``ops.norm`` (csrc/batchnorm_rows.h).  Forward, per convolution: the raw convolution
    (``conv_raw_rows``), the statistics (``bn_stats_rows``, which also advance the running statistics and ``num_batches_tracked``)
    and the apply (``bn_apply_rows``; conv3's with the identity and the ReLU) — 9 launches per block, 12 with a downsample; saved:
    the input rows, the output and per convolution ``z``, its activated output and ``(mean, var)``.  Backward, per convolution:
    ``bn_rows_backward``'s reduce and apply, then ``conv_bn_rows_backward`` on the finished ``dz`` for ``dW`` and for ``dx`` — 12
    launches, 16 with a downsample, less what nobody asked for; conv3's backward apply writes the identity's gradient, which
    conv1's input gradient adds (or the downsample's norm backward reads unmasked); the Function returns every norm's ``dgamma`` /
    ``dbeta``."""
    if bottleneck_train_reject(block, x) is not None:
        return None
    convs = _block_convs(block)
    if _m().bn_train and any(n.training for _, n in convs):
        from .norm import _bottleneck_train_bn
        return _bottleneck_train_bn(block, x)
    off = convs[1][0].conv_offset if _is_pack(convs[1][0]) else None
    return _BottleneckTrain.apply(x, block, *(c.weight for c, _ in convs), *((off.weight, off.bias) if off is not None else ()))


# ---- the stem (conv1 + bn1 + ReLU + max pooling) as one launch on an NCHW image batch (csrc/stem_conv.h)

STEM_CIN, STEM_COUT = 3, 64


def stem_hw(H, W, pool=True):
    """The stem's output size: the 7 x 7 stride-2 padding-3 convolution's ``(Hc, Wc) = ((H - 1) // 2 + 1, ...)``, and with ``pool``
    the 3 x 3 stride-2 padding-1 max pooling's ``(Hp, Wp) = ((Hc - 1) // 2 + 1, ...)`` of it."""
    hw = _out_hw((H, W), 2)
    return _out_hw(hw, 2) if pool else hw


def _image_strides(x):
    """``(tensor, ld_img, ld_ch, ld_row)`` of a (B, 3, H, W) batch the kernel reads in place: ``x`` itself when its columns are
    contiguous, its rows lie inside its channels and its channels inside its images without overlap (a crop, a slice of a larger
    batch), else one ``contiguous()`` copy.  Strides of size-1 dimensions are free in torch and are taken as dense."""
    B, C, H, W = x.shape
    s = list(x.stride())
    if W == 1:
        s[3] = 1
    if H == 1:
        s[2] = W
    row_ext = (H - 1) * s[2] + W
    if B == 1:
        s[0] = (C - 1) * s[1] + row_ext
    ok = s[3] == 1 and s[2] >= W and s[1] >= row_ext and s[0] >= (C - 1) * s[1] + row_ext and x.data_ptr() % 4 == 0
    if not ok:
        x = x.contiguous()
        s = [C * H * W, H * W, W, 1]
    return x, s[0], s[1], s[2]


def stem_rows(x, weight, bn, *, pool=True, out=None, tag="stem"):
    """``max_pool2d(relu(bn(conv2d(x, weight, stride=2, padding=3))), 3, 2, 1)`` of an NCHW image batch as channel-last rows in ONE
    launch (``bevmsda_stem_f32``): ``x`` (B, 3, H, W), ``weight`` (64, 3, 7, 7) of a convolution without bias, ``bn`` a BatchNorm
    module in eval mode (its four vectors and ``eps`` are read by the kernel).  ``pool=False``: the (B Hc Wc, 64) rows of the
    normed, rectified convolution instead of the (B Hp Wp, 64) pooled rows (``stem_hw``).  ``x`` of any strides with unit column
    stride and non-overlapping rows, channels and images is read in place; anything else costs one ``contiguous()``.  ``out``: an
    optional destination of that shape with unit column stride (its row stride may exceed 64).  Returns the rows, or ``None``
    when the call is not covered."""
    mode = _m().gemm
    tensors = [x, weight] + ([out] if out is not None else [])
    if mode not in ("split", "bf16") or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors) \
            or _norm_reject(bn) is not None or bn.training:
        return None
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape) != (STEM_COUT, STEM_CIN, 7, 7) or x.shape[1] != STEM_CIN \
            or bn.num_features != STEM_COUT:
        return None
    vecs = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if not all(v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == STEM_COUT for v in vecs):
        return None
    B, C, H, W = (int(v) for v in x.shape)
    Hc, Wc = stem_hw(H, W, pool=False) if H and W else (0, 0)
    if B * Hc * Wc > CONV_MAX_ROWS:
        return None
    Ho, Wo = stem_hw(H, W, pool=pool) if H and W else (0, 0)
    M, N = B * Ho * Wo, STEM_COUT
    if out is None:
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    else:
        y = out
        if y.dim() != 2 or tuple(y.shape) != (M, N) or y.stride(1) != 1:
            return None
    if M == 0:
        return y
    blob = stem_weight(weight)
    if blob is None:
        return None
    x4, ld_img, ld_ch, ld_row = _image_strides(x)
    desc = _lib.StemDesc(x=_ptr(x4), ld_img=ld_img, ld_ch=ld_ch, ld_row=ld_row, eps=float(bn.eps), n_img=B, H=H, W=W, c_in=C,
                         c_out=N, pool=int(bool(pool)), precision=_precision())
    for i, v in enumerate(vecs):
        desc.bn[i] = _ptr(v)
    ld_y = y.stride(0) if M > 1 else N
    # algorithmic: the convolution's products; the image in, the rows out, the weight and the four norm vectors
    timer = _gemm_ctx(tag, 2.0 * B * Hc * Wc * N * C * 49, 4.0 * (B * C * H * W + M * N + N * C * 49 + 4 * N))
    return y if _launch(y.device, "stem", lambda lib, stream: lib.bevmsda_stem_f32(
        ctypes.byref(desc), _ptr(blob), _ptr(y), ld_y, stream), timer=timer) else None


def _stem_parts(net):
    """(conv1, norm1, relu, maxpool) of a ResNet, by attribute (the in-tree class names its norm ``bn1``, mmdet's ``norm1``), or
    ``None`` when one is missing."""
    get = lambda *names: next((getattr(net, n) for n in names if hasattr(net, n)), None)
    parts = (get("conv1"), get("bn1", "norm1"), get("relu"), get("maxpool"))
    return None if any(p is None for p in parts) else parts


def stem_reject(net, x=None):
    """Why ``stem`` does not cover the stem of ``net`` (a ResNet: the in-tree class or mmdet's) on the image batch ``x`` (B, 3, H,
    W; ``None``: the module alone is judged) — a short reason — or ``None`` when it does.  The switch itself
    (``modes.stem_fused``) is the caller's to test.  Structure first, then shapes, then modes, then devices and dtypes."""
    if getattr(net, "deep_stem", False):
        return "a deep stem (three 3 x 3 convolutions)"
    parts = _stem_parts(net)
    if parts is None:
        return "not a stem (conv1 / norm1 / relu / maxpool)"
    conv, norm, relu, pool = parts
    if not isinstance(conv, nn.Conv2d):
        return "the convolution is not a Conv2d"
    if conv.in_channels != STEM_CIN or conv.out_channels != STEM_COUT:
        return f"the convolution is not {STEM_CIN} -> {STEM_COUT} channels"
    if tuple(conv.kernel_size) != (7, 7):
        return "the convolution is not 7 x 7"
    if tuple(conv.stride) != (2, 2):
        return "the convolution's stride is not 2"
    if conv.bias is not None:
        return "the convolution has a bias"
    if tuple(conv.dilation) != (1, 1):
        return "the convolution is dilated"
    if conv.groups != 1:
        return "the convolution is grouped"
    if _pair(conv.padding) != (3, 3) or getattr(conv, "padding_mode", "zeros") != "zeros":
        return "the convolution's padding is not 3 (zeros)"
    why = _norm_reject(norm)
    if why is not None:
        return why
    if norm.num_features != STEM_COUT:
        return "the norm does not match the convolution"
    if norm.training:
        return "the norm is in train() mode (batch statistics)"
    if not isinstance(relu, nn.ReLU):
        return "the activation is not ReLU"
    if not isinstance(pool, nn.MaxPool2d):
        return "the pooling is not a MaxPool2d"
    if _pair(pool.kernel_size) != (3, 3) or _pair(pool.stride) != (2, 2) or _pair(pool.padding) != (1, 1) \
            or _pair(pool.dilation) != (1, 1):
        return "the pooling is not 3 x 3, stride 2, padding 1"
    if pool.ceil_mode:
        return "the pooling rounds up (ceil_mode)"
    if pool.return_indices:
        return "the pooling returns indices"
    if x is not None:
        if not torch.is_tensor(x) or x.dim() != 4:
            return "not a (B, C, H, W) tensor"
        if x.shape[1] != STEM_CIN:
            return "the input does not match the convolution"
        if x.shape[0] * x.shape[2] * x.shape[3] == 0:
            return "an empty batch"
        Hc, Wc = stem_hw(int(x.shape[2]), int(x.shape[3]), pool=False)
        if x.shape[0] * Hc * Wc > CONV_MAX_ROWS:
            return "more than 2^24 conv pixels"
    if torch.is_grad_enabled():
        return "grad mode is on"
    if _m().gemm not in ("split", "bf16"):
        return f"GEMM mode {_m().gemm}"
    params = [conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var]
    if not all(p.is_cuda and p.dtype == torch.float32 for p in params):
        return "not CUDA fp32 parameters"
    if x is not None and not (x.is_cuda and x.dtype == torch.float32):
        return "not a CUDA fp32 input"
    return None


def stem(net, x):
    """A ResNet's stem on the stem kernel: ``maxpool(relu(norm1(conv1(x))))`` for the NCHW image batch ``x`` in one launch -> the
    (B, 64, Hp, Wp)-shaped view of channel-last rows (``rows_of_map`` of it is a view: the first bottleneck of ``backbone_fused``
    reads it in place), or ``None`` when the call is not covered (``stem_reject``).  A launch the kernel declines after
    ``stem_reject`` has accepted the call is an error, not a detour."""
    if stem_reject(net, x) is not None:
        return None
    conv, norm, _, _ = _stem_parts(net)
    B, _, H, W = x.shape
    y = _pkg().stem_rows(x, conv.weight, norm, pool=True, tag="stem")
    if y is None:
        raise RuntimeError("bevmsda: stem: the kernel declined a call stem_reject had accepted")
    return map_of_rows(y, B, stem_hw(int(H), int(W)))
