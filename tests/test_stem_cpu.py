"""No GPU: the ``stem_fused`` switch is off by default, ``ops.stem_reject`` names why a stem or a call is not covered by the fast
path — structure first, then shapes, then modes, then devices —, a rejected call runs the module path unchanged, and the op's
size helper agrees with torch's output shapes."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from bevformer_amd import modes, ops
from bevformer_amd.modules import ResNet


def _net():
    return ResNet(depth=50, num_stages=1, out_indices=(0,)).eval()


def test_switch_is_off_by_default_and_using_toggles_it():
    assert "stem_fused" in modes.Modes.__slots__ and modes.process_defaults().stem_fused is False
    assert ops.modes().stem_fused is False
    with ops.using(stem_fused=True):
        assert ops.modes().stem_fused is True and ops.modes().backbone_fused is False     # independent of the other switch
        assert ops.modes().snapshot().stem_fused is True
        with ops.using(stem_fused=False):
            assert ops.modes().stem_fused is False
    assert ops.modes().stem_fused is False


def test_the_environment_variable_sets_the_default(monkeypatch):
    monkeypatch.setenv("BEVMSDA_STEM_FUSED", "1")
    assert modes.Modes().stem_fused is True
    monkeypatch.delenv("BEVMSDA_STEM_FUSED")
    assert modes.Modes().stem_fused is False


def test_the_names_are_exported():
    import bevformer_amd
    for name in ("stem_rows", "stem", "stem_reject", "stem_hw", "stem_weight"):
        assert callable(getattr(ops, name)) and getattr(bevformer_amd.ops, name) is getattr(ops, name)
    assert "_bevmsda_stem" in ops.images.IMAGE_ATTRS


def test_stem_reject_names_the_first_uncovered_condition():
    def edited(**kw):
        net = _net()
        for k, v in kw.items():
            setattr(net, k, v)
        return net

    conv = lambda *a, **kw: nn.Conv2d(*a, **{"stride": 2, "padding": 3, "bias": False, **kw})
    with torch.no_grad():
        cases = [
            (edited(conv1=conv(3, 64, 7, bias=True)), "the convolution has a bias"),
            (edited(conv1=conv(3, 64, 5, padding=2)), "the convolution is not 7 x 7"),
            (edited(conv1=conv(3, 64, 7, stride=1)), "the convolution's stride is not 2"),
            (edited(conv1=conv(4, 64, 7)), "the convolution is not 3 -> 64 channels"),
            (edited(conv1=conv(3, 32, 7), bn1=nn.BatchNorm2d(32).eval()), "the convolution is not 3 -> 64 channels"),
            (edited(conv1=conv(3, 64, 7, dilation=2)), "the convolution is dilated"),
            (edited(conv1=conv(3, 64, 7, padding=2)), "the convolution's padding is not 3 (zeros)"),
            (edited(conv1=conv(3, 64, 7, padding_mode="reflect")), "the convolution's padding is not 3 (zeros)"),
            (edited(deep_stem=True), "a deep stem (three 3 x 3 convolutions)"),
            (edited(maxpool=nn.MaxPool2d(3, 2, 1, ceil_mode=True)), "the pooling rounds up (ceil_mode)"),
            (edited(maxpool=nn.MaxPool2d(3, 2, 1, return_indices=True)), "the pooling returns indices"),
            (edited(maxpool=nn.MaxPool2d(2, 2)), "the pooling is not 3 x 3, stride 2, padding 1"),
            (edited(maxpool=nn.MaxPool2d(3, 2, 1, dilation=2)), "the pooling is not 3 x 3, stride 2, padding 1"),
            (edited(maxpool=nn.AvgPool2d(3, 2, 1)), "the pooling is not a MaxPool2d"),
            (edited(relu=nn.LeakyReLU()), "the activation is not ReLU"),
            (edited(bn1=nn.BatchNorm2d(64, affine=False).eval()), "a norm is not affine"),
            (edited(bn1=nn.BatchNorm2d(64, track_running_stats=False).eval()), "a norm has no running statistics"),
            (edited(bn1=nn.GroupNorm(8, 64)), "a norm is not BatchNorm"),
            (edited(bn1=nn.BatchNorm2d(64).train()), "the norm is in train() mode (batch statistics)"),
        ]
        for net, why in cases:
            assert ops.stem_reject(net) == why, why
        assert ops.stem_reject(nn.Linear(3, 3)) == "not a stem (conv1 / norm1 / relu / maxpool)"
        # structure passes; then shapes, then modes, then devices
        net = _net()
        assert ops.stem_reject(net, torch.zeros(3, 8, 8)) == "not a (B, C, H, W) tensor"
        assert ops.stem_reject(net, torch.zeros(1, 4, 8, 8)) == "the input does not match the convolution"
        with ops.using(gemm="native"):
            assert ops.stem_reject(net) == "GEMM mode native"
        with ops.using(gemm="split"):
            assert ops.stem_reject(net) == "not CUDA fp32 parameters"
    with ops.using(gemm="split"):
        assert ops.stem_reject(_net()) == "grad mode is on"
        assert ops.stem_reject(edited(maxpool=nn.MaxPool2d(3, 2, 1, ceil_mode=True))) == "the pooling rounds up (ceil_mode)"     # structure first


def test_mmdet_style_attribute_names_are_read():
    class Other(nn.Module):             # mmdet's ResNet: ``norm1`` is a property of the module the config names
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
            self.add_module("bn_stem", nn.BatchNorm2d(64))
            self.relu, self.maxpool, self.deep_stem = nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1), False

        norm1 = property(lambda self: self.bn_stem)

    with torch.no_grad(), ops.using(gemm="split"):
        assert ops.stem_reject(Other().eval()) == "not CUDA fp32 parameters"            # everything structural passed
        assert ops.stem_reject(Other().train()) == "the norm is in train() mode (batch statistics)"


def test_cpu_tensors_and_grad_mode_run_the_module_path_unchanged():
    g = torch.Generator().manual_seed(3)
    net = _net()
    with torch.no_grad():
        for m in net.layer1:
            m.bn3.weight.fill_(0.5)             # (zero_init_residual would hide the stem behind the blocks' shortcuts)
    x = torch.randn(2, 3, 33, 47, generator=g)
    ref = copy.deepcopy(net)
    with torch.no_grad():
        want = ref.layer1(ref.maxpool(ref.relu(ref.bn1(ref.conv1(x)))))             # today's statement
        with ops.using(stem_fused=True):        # CPU tensors: rejected
            assert ops.stem(net, x) is None and ops.stem_rows(x, net.conv1.weight, net.bn1) is None
            got = net(x)
    assert len(got) == 1 and torch.equal(got[0], want) and float(want.abs().max()) > 0.1
    with ops.using(stem_fused=True):            # grad mode on: rejected too, and differentiable as before
        xg = x.clone().requires_grad_(True)
        out = net(xg)[0]
        assert out.requires_grad and torch.equal(out.detach(), want)
        out.sum().backward()
        assert xg.grad is not None and float(xg.grad.abs().max()) > 0 and net.conv1.weight.grad is not None


def test_stem_hw_is_torchs_output_shape():
    w = torch.zeros(1, 1, 7, 7)
    for H in range(1, 41):
        for W in (H, 41 - H):
            c = F.conv2d(torch.zeros(1, 1, H, W), w, None, stride=2, padding=3)
            p = F.max_pool2d(c, 3, 2, 1)
            assert ops.stem_hw(H, W, pool=False) == tuple(c.shape[2:]), (H, W)
            assert ops.stem_hw(H, W) == tuple(p.shape[2:]), (H, W)


def test_image_strides_keeps_crops_and_copies_what_the_kernel_cannot_read():
    from bevformer_amd.ops.backbone import _image_strides
    big = torch.zeros(3, 4, 20, 30)
    crop = big[1:, :3, 2:12, 5:25]
    t, ld_img, ld_ch, ld_row = _image_strides(crop)
    assert t is crop and (ld_img, ld_ch, ld_row) == (2400, 600, 30)
    dense = torch.zeros(2, 3, 10, 20)
    assert _image_strides(dense)[0] is dense and _image_strides(dense)[1:] == (600, 200, 20)
    nhwc = dense.contiguous(memory_format=torch.channels_last)
    t, *ld = _image_strides(nhwc)                                   # unit CHANNEL stride: one copy
    assert t is not nhwc and t.is_contiguous() and tuple(ld) == (600, 200, 20)
    expanded = torch.zeros(1, 1, 10, 20).expand(2, 3, 10, 20)       # channels that overlap: one copy
    assert _image_strides(expanded)[0] is not expanded
    one = torch.zeros(1, 3, 1, 1)
    assert _image_strides(one)[0] is one and _image_strides(one)[1:] == (3, 1, 1)
