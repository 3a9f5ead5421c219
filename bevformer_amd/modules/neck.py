"""The image neck of the reference configs: ``img_neck=dict(type='FPN', ...)`` (bevformer_base.py:54-61, bevformer_small.py,
bevformer_tiny.py, every bevformerv2 config).

``FPN`` and the ``ConvModule`` it is made of are third-party classes (mmdet ``models/necks/fpn.py``, mmcv ``cnn/bricks/
conv_module.py``) that are not on disk here.  With a real mmdet its own registry and class are used and nothing below is
registered.  Without it, this restatement — from the published behaviour of the classes, NOT pinned against their source —
lets the reference's neck config build stand-alone, with mmdet's constructor arguments and ``state_dict`` keys
(``lateral_convs.{i}.conv.{weight,bias}``, ``fpn_convs.{i}.conv.{weight,bias}``)."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..registry import NECKS, HAVE_MMDET_NECKS, BaseModule, xavier_uniform_


class ConvModule(nn.Module):
    """conv -> norm -> activation with mmcv's attribute names (``conv``, ``with_norm``, ``with_activation``); the bias is on
    unless a norm follows (mmcv's ``bias='auto'``).  Norms: ``BN``, ``GN``; activation: ``ReLU``."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None,
                 act_cfg=None, inplace=False):
        super().__init__()
        if conv_cfg is not None and conv_cfg.get("type", "Conv2d") not in ("Conv2d", "Conv"):
            raise NotImplementedError(f"conv_cfg {conv_cfg!r} is not restated here")
        self.with_norm = norm_cfg is not None
        self.with_activation = act_cfg is not None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=not self.with_norm)
        if self.with_norm:
            cfg = dict(norm_cfg)
            typ = cfg.pop("type")
            requires_grad = cfg.pop("requires_grad", True)
            if typ in ("BN", "BN2d"):
                self.bn = nn.BatchNorm2d(out_channels, **cfg)
            elif typ == "GN":
                self.gn = nn.GroupNorm(num_channels=out_channels, **cfg)
            else:
                raise NotImplementedError(f"norm_cfg type {typ!r} is not restated here")
            for p in self.norm.parameters():
                p.requires_grad = requires_grad
        if self.with_activation:
            if act_cfg.get("type") != "ReLU":
                raise NotImplementedError(f"act_cfg {act_cfg!r} is not restated here")
            self.activate = nn.ReLU(inplace=inplace)

    @property
    def norm(self):
        return getattr(self, "bn", None) or getattr(self, "gn", None)

    def forward(self, x):
        x = self.conv(x)
        if self.with_norm:
            x = self.norm(x)
        if self.with_activation:
            x = self.activate(x)
        return x


class FPN(BaseModule):
    """Feature pyramid: 1 x 1 laterals on the input levels ``start_level .. end_level``, top-down sums with the nearest-
    upsampled coarser lateral, a 3 x 3 convolution per level; ``num_outs`` beyond the used levels are stride-2 3 x 3
    convolutions (``add_extra_convs``: on the input, the top lateral or the previous output; ``True`` means ``'on_input'``;
    ``relu_before_extra_convs``: a ReLU in front of the second and later ones) or, without extra convolutions,
    ``max_pool2d(1, stride=2)`` subsamples.  inputs: one (B, C_i, H_i, W_i) per entry of ``in_channels`` -> tuple of
    ``num_outs`` maps (B, out_channels, h, w).

    With ``modes.fpn_fused`` and a covered module and call (``ops.fpn_reject``) the forward runs on the channel-last row
    convolution kernel (``ops.fpn``) and returns NCHW-shaped views of channel-last storage; otherwise the torch statements.
    Under grad mode with ``modes.fpn_train`` a covered module and call (``ops.fpn_train_reject``) runs as one autograd Function
    on the same kernels and their backward (``ops.fpn_train``)."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode="nearest"), init_cfg=dict(type="Xavier", layer="Conv2d", distribution="uniform")):
        super().__init__(init_cfg)
        assert isinstance(in_channels, (list, tuple))
        self.in_channels = list(in_channels)
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.relu_before_extra_convs = relu_before_extra_convs
        self.no_norm_on_lateral = no_norm_on_lateral
        self.fp16_enabled = False
        self.upsample_cfg = copy.deepcopy(upsample_cfg)
        if end_level == -1:
            self.backbone_end_level = self.num_ins
            assert num_outs >= self.num_ins - start_level
        else:
            self.backbone_end_level = end_level
            assert end_level <= self.num_ins
            assert num_outs == end_level - start_level
        self.start_level = start_level
        self.end_level = end_level
        assert isinstance(add_extra_convs, (str, bool))
        if isinstance(add_extra_convs, str):
            assert add_extra_convs in ("on_input", "on_lateral", "on_output")
        elif add_extra_convs:
            add_extra_convs = "on_input"
        self.add_extra_convs = add_extra_convs

        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(ConvModule(self.in_channels[i], out_channels, 1, conv_cfg=conv_cfg,
                                                 norm_cfg=norm_cfg if not no_norm_on_lateral else None, act_cfg=act_cfg))
            self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1, conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                                             act_cfg=act_cfg))
        extra_levels = num_outs - self.backbone_end_level + self.start_level
        if self.add_extra_convs and extra_levels >= 1:
            for i in range(extra_levels):
                c_in = self.in_channels[self.backbone_end_level - 1] if i == 0 and self.add_extra_convs == "on_input" \
                    else out_channels
                self.fpn_convs.append(ConvModule(c_in, out_channels, 3, stride=2, padding=1, conv_cfg=conv_cfg,
                                                 norm_cfg=norm_cfg, act_cfg=act_cfg))
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                xavier_uniform_(m)
        self._is_init = True

    def forward(self, inputs):
        assert len(inputs) == len(self.in_channels)
        if torch.is_grad_enabled() and ops.modes().fpn_train and ops.fpn_train_reject(self, inputs) is None:
            return ops.fpn_train(self, inputs)
        if ops.modes().fpn_fused and ops.fpn_reject(self, inputs) is None:
            return tuple(ops.fpn(self, inputs))
        return self.forward_torch(inputs)

    def forward_torch(self, inputs):
        """The module path: torch statements only."""
        laterals = [conv(inputs[i + self.start_level]) for i, conv in enumerate(self.lateral_convs)]
        used = len(laterals)
        for i in range(used - 1, 0, -1):
            if "scale_factor" in self.upsample_cfg:
                laterals[i - 1] = laterals[i - 1] + F.interpolate(laterals[i], **self.upsample_cfg)
            else:
                laterals[i - 1] = laterals[i - 1] + F.interpolate(laterals[i], size=laterals[i - 1].shape[2:], **self.upsample_cfg)
        outs = [self.fpn_convs[i](laterals[i]) for i in range(used)]
        if self.num_outs > len(outs):
            if not self.add_extra_convs:
                for _ in range(self.num_outs - used):
                    outs.append(F.max_pool2d(outs[-1], 1, stride=2))
            else:
                if self.add_extra_convs == "on_input":
                    source = inputs[self.backbone_end_level - 1]
                elif self.add_extra_convs == "on_lateral":
                    source = laterals[-1]
                else:
                    source = outs[-1]
                outs.append(self.fpn_convs[used](source))
                for i in range(used + 1, self.num_outs):
                    outs.append(self.fpn_convs[i](F.relu(outs[-1]) if self.relu_before_extra_convs else outs[-1]))
        return tuple(outs)


if not HAVE_MMDET_NECKS:        # a real mmdet keeps its own FPN under that name
    NECKS.register_module(name="FPN", force=True, module=FPN)
