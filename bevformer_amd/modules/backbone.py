"""The image backbone of the reference configs: ``img_backbone=dict(type='ResNet', depth=101, style='caffe', dcn=dict(type='DCNv2',
...), stage_with_dcn=(False, False, True, True))`` (bevformer_base.py:43-53, bevformer_small.py:50-61) and the ResNet-50 of
bevformer_tiny.py:55-63.

``ResNet`` / ``Bottleneck`` (mmdet ``models/backbones/resnet.py``) and ``ModulatedDeformConv2dPack`` (mmcv 1.4.0 ``ops/
modulated_deform_conv.py``, whose operator is native code of mmcv) are third-party classes that are not on disk here.  With a
real mmdet its own registries and classes are used and nothing below is registered.  Without it, this restatement — from the
published behaviour of the classes, NOT pinned against their source — lets the reference's backbone config build stand-alone,
with the constructor arguments the reference configs use and mmdet's ``state_dict`` keys (``conv1``, ``bn1``,
``layer{s}.{i}.conv{1,2,3}``, ``bn{1,2,3}``, ``downsample.{0,1}``, ``conv2.conv_offset.{weight,bias}``), so that
``r101_dcn_fcos3d_pretrain.pth`` loads.

Everything but the deformable convolution stays on torch.  With ``modes.dcn_fused`` a covered pack (``ops.dcn_reject``) runs on
the deformable kernel (``ops.dcn``); a bottleneck whose ``bn2`` is in eval mode hands ``bn2`` + ReLU to that launch.  With
``modes.backbone_fused`` a covered bottleneck (``ops.bottleneck_reject``) runs whole on channel-last rows (``ops.bottleneck``): every
convolution with its norm, the residual sum and the ReLUs in 3 to 5 launches.  With ``modes.stem_fused`` a covered stem
(``ops.stem_reject``) — ``conv1``, ``bn1``, the ReLU and the max pooling — is ONE launch on the NCHW image batch (``ops.stem``) that
writes the channel-last rows the first bottleneck reads; the two switches are independent, and with both on no torch convolution,
norm, pooling or layout copy is left on the inference path.  With ``stem_fused`` off the stem and the max pooling stay on torch.
With ``modes.backbone_train`` and grad mode on, a block in which nothing needs a gradient (a frozen stage behind a frozen stem) and
a frozen stem run on those inference kernels under ``no_grad``, and a covered trainable block (``ops.bottleneck_train_reject``: a
plain ``conv2``, frozen norms) runs as one autograd Function on the row kernels (``ops.bottleneck_train``); with ``modes.dcn_train``
as well, so does a block whose ``conv2`` is a DCNv2 pack (the deformable backward kernels of ``ops.deform_conv_rows_backward``)."""
import torch
import torch.nn as nn
import torch.utils.checkpoint as cp
from torch.nn.modules.batchnorm import _BatchNorm

from .. import ops
from ..registry import BACKBONES, CONV_LAYERS, HAVE_MMDET_BACKBONES, BaseModule


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class ModulatedDeformConv2dPack(nn.Module):
    """Modulated deformable convolution (DCNv2) with its own offset / mask convolution, mmcv's constructor arguments and keys
    (``weight``, optional ``bias``, ``conv_offset.weight``, ``conv_offset.bias``; the ``..._offset.*`` keys of version < 2
    checkpoints are accepted on load).  ``conv_offset`` is a plain convolution of the same kernel, stride, padding and dilation
    with ``3 * kh * kw`` output channels, zero-initialised; for tap ``k = kw * i + j`` its channel ``2 k`` is the y offset,
    ``2 k + 1`` the x offset and ``2 kh kw + k`` the mask logit (mmcv's ``chunk(3)`` + ``cat(o1, o2)`` with the operator's
    interleaved offset layout).  The output is

        y[co, oy, ox] = bias[co] + sum_k sigmoid(logit_k) sum_ci w[co, ci, i, j] bilin(x[ci], S oy - pad + dil i + dy_k,
                                                                                     S ox - pad + dil j + dx_k)

    with bilinear interpolation in pixel coordinates whose corners outside the image count zero; a position that is not finite or
    outside (-1, H) x (-1, W) counts zero.  ``groups`` and ``deform_groups`` above 1 are not restated."""

    _version = 2

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deform_groups=1,
                 bias=True):
        super().__init__()
        if groups != 1 or deform_groups != 1:
            raise NotImplementedError(f"ModulatedDeformConv2dPack: groups={groups}, deform_groups={deform_groups} are not restated here")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
        self.groups, self.deform_groups = groups, deform_groups
        self.transposed, self.output_padding = False, (0, 0)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.conv_offset = nn.Conv2d(in_channels, deform_groups * 3 * self.kernel_size[0] * self.kernel_size[1], self.kernel_size,
                                     stride=self.stride, padding=self.padding, dilation=self.dilation, bias=True)
        self.init_weights()

    def init_weights(self):
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        stdv = 1.0 / n ** 0.5
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.zero_()
            self.conv_offset.weight.zero_()
            self.conv_offset.bias.zero_()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:     # the offset convolution was a sibling of the pack: ``conv2_offset`` next to ``conv2``
            for leaf in ("weight", "bias"):
                new, old = f"{prefix}conv_offset.{leaf}", f"{prefix[:-1]}_offset.{leaf}"
                if new not in state_dict and old in state_dict:
                    state_dict[new] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x):
        if ops.modes().dcn_fused and ops.dcn_reject(self, x) is None:
            return ops.dcn(self, x)
        return self.forward_torch(x)

    def forward_torch(self, x):
        """The module path: torch statements only (explicit corner gathers; CPU and GPU, fp32 and fp64, differentiable)."""
        B, C, H, W = x.shape
        kh, kw = self.kernel_size
        K = kh * kw
        raw = self.conv_offset(x)                               # (B, 3 K, Ho, Wo)
        Ho, Wo = raw.shape[2:]
        dy, dx = raw[:, 0:2 * K:2], raw[:, 1:2 * K:2]           # (B, K, Ho, Wo)
        mask = torch.sigmoid(raw[:, 2 * K:])
        ar = lambda n, s, p: torch.arange(n, device=x.device, dtype=x.dtype) * s - p
        tap = torch.arange(K, device=x.device)
        ty = (torch.div(tap, kw, rounding_mode="floor") * self.dilation[0]).to(x.dtype)
        tx = ((tap % kw) * self.dilation[1]).to(x.dtype)
        py = ar(Ho, self.stride[0], self.padding[0]).view(1, 1, Ho, 1) + ty.view(1, K, 1, 1) + dy
        px = ar(Wo, self.stride[1], self.padding[1]).view(1, 1, 1, Wo) + tx.view(1, K, 1, 1) + dx
        valid = (py > -1) & (py < H) & (px > -1) & (px < W)     # NaN fails every compare
        py, px = torch.where(valid, py, torch.zeros_like(py)), torch.where(valid, px, torch.zeros_like(px))
        y0, x0 = py.detach().floor(), px.detach().floor()
        ly, lx = py - y0, px - x0
        y0, x0 = y0.long(), x0.long()
        flat = x.reshape(B, C, H * W)
        cols = x.new_zeros(B, C, K, Ho, Wo)
        for cy, cx, wgt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx),
                            (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
            inside = valid & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
            idx = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).reshape(B, 1, -1).expand(B, C, -1)
            val = flat.gather(2, idx).reshape(B, C, K, Ho, Wo)
            coef = torch.where(inside, wgt * mask, torch.zeros_like(wgt))
            cols = cols + torch.where(inside.unsqueeze(1), val, torch.zeros_like(val)) * coef.unsqueeze(1)
        y = torch.einsum("bckhw,ock->bohw", cols, self.weight.reshape(self.out_channels, C, K))
        return y if self.bias is None else y + self.bias.view(1, -1, 1, 1)


def build_conv_layer(cfg, *args, **kwargs):
    """mmcv's ``build_conv_layer``: ``None`` / ``Conv2d`` / ``Conv`` -> ``nn.Conv2d``; ``DCNv2`` / ``ModulatedDeformConv2dPack`` ->
    the pack.  Anything else raises by name."""
    cfg = dict(cfg) if cfg is not None else dict(type="Conv2d")
    typ = cfg.pop("type")
    if typ in ("Conv2d", "Conv"):
        return nn.Conv2d(*args, **kwargs, **cfg)
    cls = CONV_LAYERS.get(typ)
    if cls is None:
        raise NotImplementedError(f"conv layer type {typ!r} is not restated here")
    return cls(*args, **kwargs, **cfg)


def _build_norm(norm_cfg, num_features):
    cfg = dict(norm_cfg)
    typ = cfg.pop("type")
    requires_grad = cfg.pop("requires_grad", True)
    if typ not in ("BN", "BN2d", "SyncBN"):
        raise NotImplementedError(f"norm_cfg type {typ!r} is not restated here")
    cfg.setdefault("eps", 1e-5)
    # (SyncBN: torch's SyncBatchNorm — BatchNorm2d's parameters, buffers and state_dict keys; on one rank the same arithmetic)
    norm = (nn.SyncBatchNorm if typ == "SyncBN" else nn.BatchNorm2d)(num_features, **cfg)
    for p in norm.parameters():
        p.requires_grad = requires_grad
    return norm


def _bottleneck_train_path(block, x):
    """``modes.backbone_train`` with grad mode on, for the in-tree block or mmdet's (the parts are found by attribute): a block in
    which nothing needs a gradient — a frozen stage behind a frozen stem — runs ``ops.bottleneck`` under ``no_grad``, any other
    covered block ``ops.bottleneck_train``.  ``None``: the module path."""
    if not torch.is_tensor(x):
        return None
    if not x.requires_grad and not any(p.requires_grad for p in block.parameters()):
        with torch.no_grad():
            return ops.bottleneck(block, x)         # (None when bottleneck_reject has another reason than grad mode)
    return ops.bottleneck_train(block, x)           # (None when bottleneck_train_reject has a reason)


def _stem_train_path(net, x):
    """``modes.backbone_train`` with grad mode on: a stem in which nothing needs a gradient runs ``ops.stem`` under ``no_grad``.
    ``None``: the module path."""
    parts = ops._stem_parts(net)
    if parts is None or not torch.is_tensor(x) or x.requires_grad \
            or any(p.requires_grad for m in parts[:2] for p in m.parameters()):
        return None
    with torch.no_grad():
        return ops.stem(net, x)


class Bottleneck(BaseModule):
    """mmdet's ResNet bottleneck: 1 x 1 -> 3 x 3 -> 1 x 1 (4 x ``planes``) with BatchNorm after each, the residual sum and a
    ReLU; ``style='caffe'`` puts the stride on ``conv1``, ``'pytorch'`` on ``conv2``; ``dcn``: ``conv2`` is that layer (unless
    ``fallback_on_stride`` and the block has a stride).  Plugins are not restated."""

    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style="pytorch", with_cp=False, conv_cfg=None,
                 norm_cfg=dict(type="BN"), dcn=None, plugins=None, init_cfg=None):
        super().__init__(init_cfg)
        if style not in ("pytorch", "caffe"):
            raise NotImplementedError(f"Bottleneck: style={style!r}")
        if plugins is not None:
            raise NotImplementedError("Bottleneck: plugins are not restated here")
        if conv_cfg is not None:
            raise NotImplementedError(f"Bottleneck: conv_cfg {conv_cfg!r} is not restated here")
        self.inplanes, self.planes, self.stride, self.dilation = inplanes, planes, stride, dilation
        self.style, self.with_cp, self.dcn, self.with_dcn = style, with_cp, dcn, dcn is not None
        self.conv1_stride, self.conv2_stride = (1, stride) if style == "pytorch" else (stride, 1)
        self.conv1 = nn.Conv2d(inplanes, planes, 1, stride=self.conv1_stride, bias=False)
        self.bn1 = _build_norm(norm_cfg, planes)
        fallback_on_stride = False
        if self.with_dcn:
            dcn = dict(dcn)
            fallback_on_stride = dcn.pop("fallback_on_stride", False)
        if not self.with_dcn or (fallback_on_stride and stride > 1):
            self.conv2 = nn.Conv2d(planes, planes, 3, stride=self.conv2_stride, padding=dilation, dilation=dilation, bias=False)
        else:
            self.conv2 = build_conv_layer(dcn, planes, planes, 3, stride=self.conv2_stride, padding=dilation, dilation=dilation,
                                          bias=False)
        self.bn2 = _build_norm(norm_cfg, planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = _build_norm(norm_cfg, planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    norm1 = property(lambda self: self.bn1)
    norm2 = property(lambda self: self.bn2)
    norm3 = property(lambda self: self.bn3)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # version < 2 checkpoints keep the pack's offset convolution as ``conv2_offset`` next to ``conv2``: renamed here, where
        # the keys are in view (torch hands a child only the keys under its own prefix)
        if isinstance(self.conv2, ModulatedDeformConv2dPack):
            for leaf in ("weight", "bias"):
                new, old = f"{prefix}conv2.conv_offset.{leaf}", f"{prefix}conv2_offset.{leaf}"
                if new not in state_dict and old in state_dict:
                    state_dict[new] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _conv2(self, out):
        """relu(bn2(conv2(out))): ONE launch after the offset convolution's when conv2 is a covered pack and bn2 is in eval mode."""
        if ops.modes().dcn_fused and isinstance(self.conv2, ModulatedDeformConv2dPack) and not self.bn2.training \
                and ops.dcn_reject(self.conv2, out, self.bn2) is None:
            return ops.dcn(self.conv2, out, self.bn2, relu=True)
        return self.relu(self.bn2(self.conv2(out)))

    def _inner(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self._conv2(out)
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return out + identity

    def forward(self, x):
        # (the dispatch sits here, not in _inner: the final ReLU is inside the fast path's last launch; with_cp only matters
        # with gradients, which the fast path rejects)
        if ops.modes().backbone_fused and ops.bottleneck_reject(self, x) is None:
            return ops.bottleneck(self, x)
        if ops.modes().backbone_train and torch.is_grad_enabled():
            y = _bottleneck_train_path(self, x)
            if y is not None:
                return y
        if self.with_cp and x.requires_grad:
            out = cp.checkpoint(self._inner, x)
        else:
            out = self._inner(x)
        return self.relu(out)

    def forward_torch(self, x):
        """The module path: torch statements only."""
        out = self.relu(self.bn1(self.conv1(x)))
        conv2 = self.conv2.forward_torch if isinstance(self.conv2, ModulatedDeformConv2dPack) else self.conv2
        out = self.relu(self.bn2(conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class ResNet(BaseModule):
    """mmdet's ResNet of bottlenecks as the reference configs build it: ``depth`` 50 / 101, the 7 x 7 stride-2 stem + 3 x 3
    stride-2 max pooling, ``num_stages`` stages of width 64 * 2^s with the stage stride on the first block (whose shortcut is
    1 x 1 convolution + BatchNorm); ``out_indices``: the stages returned; ``frozen_stages``: the stem and that many stages in eval
    mode without gradients; ``norm_eval``: every BatchNorm stays in eval mode under ``train()``; ``dcn`` / ``stage_with_dcn``: the
    stages whose ``conv2`` is that layer.  Arguments the reference configs do not use raise by name."""

    arch_settings = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style="pytorch", deep_stem=False, avg_down=False,
                 frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True,
                 pretrained=None, init_cfg=None):
        super().__init__(init_cfg)
        if depth not in self.arch_settings:
            raise NotImplementedError(f"ResNet: depth={depth} is not restated here (50, 101)")
        for name, value, default in (("deep_stem", deep_stem, False), ("avg_down", avg_down, False), ("conv_cfg", conv_cfg, None),
                                     ("plugins", plugins, None), ("pretrained", pretrained, None),
                                     ("dilations", tuple(dilations), (1, 1, 1, 1)), ("strides", tuple(strides), (1, 2, 2, 2))):
            if value != default:
                raise NotImplementedError(f"ResNet: {name}={value!r} is not restated here")
        assert 1 <= num_stages <= 4 and max(out_indices) < num_stages
        if dcn is not None:
            assert len(stage_with_dcn) == num_stages
        self.depth, self.num_stages, self.out_indices, self.style = depth, num_stages, tuple(out_indices), style
        self.frozen_stages, self.norm_eval, self.with_cp, self.zero_init_residual = frozen_stages, norm_eval, with_cp, zero_init_residual
        self.dcn, self.stage_with_dcn = dcn, tuple(stage_with_dcn)
        stem_channels = stem_channels or base_channels
        self.conv1 = nn.Conv2d(in_channels, stem_channels, 7, stride=2, padding=3, bias=False)
        self.bn1 = _build_norm(norm_cfg, stem_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers = []
        inplanes = stem_channels
        for s, blocks in enumerate(self.arch_settings[depth][:num_stages]):
            planes = base_channels * 2 ** s
            stage_dcn = dcn if dcn is not None and self.stage_with_dcn[s] else None
            layers = []
            for i in range(blocks):
                stride = strides[s] if i == 0 else 1
                downsample = None
                if i == 0 and (stride != 1 or inplanes != planes * Bottleneck.expansion):
                    downsample = nn.Sequential(nn.Conv2d(inplanes, planes * Bottleneck.expansion, 1, stride=stride, bias=False),
                                               _build_norm(norm_cfg, planes * Bottleneck.expansion))
                layers.append(Bottleneck(inplanes, planes, stride=stride, downsample=downsample, style=style, with_cp=with_cp,
                                         norm_cfg=norm_cfg, dcn=stage_dcn))
                inplanes = planes * Bottleneck.expansion
            name = f"layer{s + 1}"
            self.add_module(name, nn.Sequential(*layers))
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self.init_weights()
        self._freeze_stages()

    norm1 = property(lambda self: self.bn1)

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, _BatchNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        for m in self.modules():
            if isinstance(m, ModulatedDeformConv2dPack):        # (the offset convolution starts at zero: the plain convolution)
                nn.init.zeros_(m.conv_offset.weight)
                nn.init.zeros_(m.conv_offset.bias)
            if isinstance(m, Bottleneck) and self.zero_init_residual:
                nn.init.zeros_(m.bn3.weight)
        self._is_init = True

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.bn1.eval()
            for m in (self.conv1, self.bn1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, f"layer{i}")
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def forward(self, x):
        y = ops.stem(self, x) if ops.modes().stem_fused else None       # (None: not covered — the module path below)
        if y is None and ops.modes().backbone_train and torch.is_grad_enabled():
            y = _stem_train_path(self, x)
        x = self.maxpool(self.relu(self.bn1(self.conv1(x)))) if y is None else y
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self


if not HAVE_MMDET_BACKBONES:        # a real mmdet / mmcv keep their own ResNet and DCNv2 under those names
    CONV_LAYERS.register_module(name="DCNv2", force=True, module=ModulatedDeformConv2dPack)
    CONV_LAYERS.register_module(name="ModulatedDeformConv2dPack", force=True, module=ModulatedDeformConv2dPack)
    BACKBONES.register_module(name="ResNet", force=True, module=ResNet)
