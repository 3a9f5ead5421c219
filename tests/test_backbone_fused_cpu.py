"""No GPU: the ``backbone_fused`` switch is off by default, ``ops.bottleneck_reject`` names why a block or a call is not covered by
the fast path — structure first, then shapes, then modes, then devices —, and a rejected call runs the module path unchanged."""
import torch

from bevformer_amd import ops
from bevformer_amd.modules import Bottleneck, ResNet

DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)


def _downsample(cin, cout, stride=1):
    return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(cout))


def test_switch_is_off_by_default_and_using_toggles_it():
    assert ops.modes().backbone_fused is False
    with ops.using(backbone_fused=True):
        assert ops.modes().backbone_fused is True
        with ops.using(backbone_fused=False):
            assert ops.modes().backbone_fused is False
    assert ops.modes().backbone_fused is False


def test_the_names_are_exported():
    import bevformer_amd
    for name in ("conv_bn_rows", "bottleneck", "bottleneck_reject"):
        assert callable(getattr(ops, name)) and getattr(bevformer_amd.ops, name) is getattr(ops, name)


def test_bottleneck_reject_names_the_first_uncovered_condition():
    x = torch.randn(1, 256, 4, 5)
    ok = lambda **kw: Bottleneck(256, 64, **kw).eval()
    with torch.no_grad(), ops.using(gemm="split"):
        # structure
        assert ops.bottleneck_reject(torch.nn.Conv2d(64, 64, 3)) == "not a bottleneck (conv1 / norm1 / conv2 / norm2 / conv3 / norm3 / downsample)"
        for name, k in (("conv1", 1), ("conv2", 3), ("conv3", 1)):                  # a conv with a bias
            blk = ok()
            old = getattr(blk, name)
            setattr(blk, name, torch.nn.Conv2d(old.in_channels, old.out_channels, k, padding=k // 2, bias=True))
            assert ops.bottleneck_reject(blk, x) == "a convolution has a bias", name
        assert ops.bottleneck_reject(Bottleneck(192, 48).eval()) == "channel counts are not multiples of 32"    # planes = 48
        assert ops.bottleneck_reject(ok(dilation=2), x) == "a convolution is dilated"
        assert ops.bottleneck_reject(ok(dcn=DCN, dilation=2), x) == "the convolution is dilated"       # (the pack's own words)
        blk = ok()
        blk.bn2.train()
        assert ops.bottleneck_reject(blk, x) == "a norm is in train() mode (batch statistics)"
        ds3 = torch.nn.Sequential(torch.nn.AvgPool2d(1), torch.nn.Conv2d(64, 256, 1, bias=False), torch.nn.BatchNorm2d(256))
        assert ops.bottleneck_reject(Bottleneck(64, 64, downsample=ds3).eval()) == "a downsample is not conv + norm"
        blk = ok()
        blk.bn3 = torch.nn.GroupNorm(32, 256)
        assert ops.bottleneck_reject(blk, x) == "a norm is not BatchNorm"
        blk = ok()
        blk.bn1 = torch.nn.BatchNorm2d(64, affine=False).eval()
        assert ops.bottleneck_reject(blk, x) == "a norm is not affine"
        blk = ok()
        blk.bn1 = torch.nn.BatchNorm2d(64, track_running_stats=False).eval()
        assert ops.bottleneck_reject(blk, x) == "a norm has no running statistics"
        blk = ok()
        blk.conv2 = torch.nn.Conv2d(64, 64, 3, padding=1, groups=2, bias=False)
        assert ops.bottleneck_reject(blk, x) == "a convolution is grouped"
        blk = ok()
        blk.conv3 = torch.nn.Conv2d(64, 256, 1, stride=4, bias=False)
        assert ops.bottleneck_reject(blk, x) == "a stride is not 1 or 2"
        # strides and channels that chain
        assert ops.bottleneck_reject(Bottleneck(256, 64, stride=2).eval()) == "a block without downsample changes the shape"
        assert ops.bottleneck_reject(Bottleneck(128, 64).eval()) == "a block without downsample changes the shape"
        assert ops.bottleneck_reject(Bottleneck(256, 128, stride=2, downsample=_downsample(256, 512, 1)).eval()) \
            == "a downsample does not match its block"
        assert ops.bottleneck_reject(Bottleneck(256, 128, stride=2, downsample=_downsample(256, 256, 2)).eval()) \
            == "a downsample does not match its block"
        # shapes
        assert ops.bottleneck_reject(ok(), x[0]) == "not a (B, C, H, W) tensor"
        assert ops.bottleneck_reject(ok(), torch.randn(1, 64, 4, 5)) == "the input does not match the block"
        # covered structures get as far as the devices: the block's tensors are on the CPU
        for blk in (ok(), ok(style="caffe"), ok(dcn=DCN), Bottleneck(64, 64, downsample=_downsample(64, 256)).eval(),
                    Bottleneck(256, 128, stride=2, style="caffe", downsample=_downsample(256, 512, 2)).eval(),
                    Bottleneck(256, 128, stride=2, style="pytorch", downsample=_downsample(256, 512, 2)).eval()):
            assert ops.bottleneck_reject(blk) == "not CUDA fp32 parameters"
    # modes before devices
    with ops.using(gemm="split"):
        assert ops.bottleneck_reject(ok(), x) == "grad mode is on"
    with torch.no_grad(), ops.using(gemm="native"):
        assert ops.bottleneck_reject(ok(), x) == "GEMM mode native"
    with torch.no_grad(), ops.using(gemm="bf16"):
        assert ops.bottleneck_reject(ok(), x) == "not CUDA fp32 parameters"
        assert ops.bottleneck(ok(), x) is None
        assert ops.conv_bn_rows(torch.randn(20, 64), 1, (4, 5), torch.randn(64, 64, 1, 1), torch.nn.BatchNorm2d(64).eval()) is None


def test_rejected_calls_run_the_module_path_bit_for_bit():
    g = torch.Generator().manual_seed(0)
    blk = Bottleneck(256, 64).eval()
    net = ResNet(depth=50).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, Bottleneck):
                m.bn3.weight.fill_(0.5)            # (zero_init_residual would hide conv1 .. conv3 of every block)
    xb = torch.randn(2, 256, 6, 10, generator=g)
    xn = torch.randn(2, 3, 32, 32, generator=g)
    with torch.no_grad():
        want_b, want_n = blk.forward_torch(xb), net(xn)
        with ops.using(backbone_fused=True):        # CPU tensors: rejected, so forward IS forward_torch
            got_b, got_n = blk(xb), net(xn)
            assert ops.bottleneck(blk, xb) is None
    assert torch.equal(got_b, want_b) and float(want_b.abs().max()) > 0.1
    assert len(got_n) == len(want_n) == 4
    for a, b in zip(got_n, want_n):
        assert torch.equal(a, b) and float(b.abs().max()) > 0
    with ops.using(backbone_fused=True):            # grad mode on: rejected too, and differentiable as before
        xg = xb.clone().requires_grad_(True)
        out = blk(xg)
        assert out.requires_grad and torch.equal(out.detach(), want_b)


def test_state_dict_keys_are_unchanged_by_the_switch():
    keys = list(ResNet(depth=50, style="caffe", dcn=DCN, stage_with_dcn=(False, False, True, True)).state_dict())
    with ops.using(backbone_fused=True):
        net = ResNet(depth=50, style="caffe", dcn=DCN, stage_with_dcn=(False, False, True, True)).eval()
        with torch.no_grad():
            net(torch.randn(1, 3, 32, 32))
        assert list(net.state_dict()) == keys
    assert "layer3.0.conv2.conv_offset.weight" in keys and "layer1.0.downsample.1.running_var" in keys
