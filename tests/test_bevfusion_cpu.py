"""No GPU: what ``ops.fusion_reject`` says about modules the temporal-fusion fast path does not cover, and that the switch
(``modes.bevfusion_fused``) changes nothing where the path does not apply."""
import pytest
import torch
import torch.nn as nn

from bevformer_amd import modes, ops, synthetic as S
from bevformer_amd.modules.transformer import ResNetFusion

import fusion_yardstick as Y


def _fusion(inc=128, outc=64, inter=128, n=2):
    torch.manual_seed(0)
    return Y.randomize_bn(ResNetFusion(inc, outc, inter, n)).eval()


def _replace_conv(block, name, **kw):
    old = getattr(block, name)
    args = dict(kernel_size=3, stride=1, padding=1, bias=False)
    args.update(kw)
    setattr(block, name, nn.Conv2d(old.in_channels, old.out_channels, **args))


def test_switch_defaults_off_and_is_a_mode():
    assert modes.Modes().bevfusion_fused is False
    with ops.using(bevfusion_fused=True) as m:
        assert m.bevfusion_fused and ops.modes().bevfusion_fused
    assert not ops.modes().bevfusion_fused


def test_fusion_reject_names_the_reason():
    with torch.no_grad():
        f = _fusion()
        assert ops.fusion_reject(f) == "not CUDA fp32 parameters"       # a covered structure: only the device is wrong here
        _replace_conv(f.layers[1], "conv2", stride=2)
        assert "stride" in ops.fusion_reject(f)

        f = _fusion()
        _replace_conv(f.layers[0], "conv1", bias=True)
        assert "bias" in ops.fusion_reject(f)

        f = _fusion(inc=128, inter=64)                                   # with a downsample
        f.layers[0].downsample[1] = nn.BatchNorm2d(64, track_running_stats=False)
        assert "running statistics" in ops.fusion_reject(f)

        f = _fusion()
        f.layers[0].bn1 = nn.BatchNorm2d(128, affine=False)
        assert "affine" in ops.fusion_reject(f)

        f = _fusion()
        f.layers[0].bn2 = nn.GroupNorm(4, 128)
        assert "BatchNorm" in ops.fusion_reject(f)

        f = _fusion(inc=96, inter=48)                                    # 48 channels: off the 32-channel granularity
        assert "multiples of 32" in ops.fusion_reject(f)

        f = _fusion(inc=128, inter=64)
        _replace_conv(f.layers[0].downsample, "0", dilation=2, padding=2)
        assert ops.fusion_reject(f) is not None

        f = _fusion().train()
        assert "train()" in ops.fusion_reject(f)
        assert ops.fusion_reject(object()) == "not a ResNetFusion"


def test_fusion_reject_reports_grad_mode_before_the_device():
    f = _fusion()
    with torch.enable_grad():
        assert "grad mode" in ops.fusion_reject(f)
    with torch.no_grad(), ops.using(gemm="native"):
        assert "native" in ops.fusion_reject(f)


def test_forward_rows_on_the_module_path_equals_forward_of_the_permuted_maps():
    H, W = 5, 7
    for inter in (128, 64):
        f = _fusion(inter=inter)
        rows = [torch.randn(2, H * W, 64), torch.randn(2, H * W, 64)]
        maps = [Y.rows_to_maps(r, H, W).contiguous() for r in rows]
        with torch.no_grad():
            want = f(maps)
            assert torch.equal(f.forward_rows(rows, H, W), want)
            with ops.using(bevfusion_fused=True):                        # CPU tensors: rejected, the module path as it is
                assert torch.equal(f.forward_rows(rows, H, W), want)
            err = Y.max_err(want, Y.fusion64(f.state_dict(), rows, H, W))
        assert err < 1e-4                                                # (the yardstick restates the module)


def test_fuse_frames_with_the_switch_on_is_bit_equal_on_cpu():
    import bevformer_amd
    cfg = S.transformer_cfg("micro")
    kw = dict(num_feature_levels=cfg["num_feature_levels"], encoder=cfg["encoder"], frames=(-1, 0, 1), num_fusion=1,
              inter_channels=64)
    torch.manual_seed(1)
    t = bevformer_amd.build_transformer(dict(type="PerceptionTransformerV2", **kw)).eval()
    t.init_weights()
    Y.randomize_bn(t.fusion)
    H, W = 4, 6
    bev, later = torch.randn(1, H * W, 256), torch.randn(1, H * W, 256)
    with torch.no_grad():
        prev_off = [None, None, later.clone()]
        off = t.fuse_frames(bev, prev_off, H, W)
        with ops.using(bevfusion_fused=True):
            prev_on = [None, None, later.clone()]
            on = t.fuse_frames(bev, prev_on, H, W)
    assert torch.equal(on, off)
    assert len(prev_on) == 3 and all(torch.equal(a, b) for a, b in zip(prev_on, prev_off))
    assert prev_on[0] is not None and torch.equal(prev_on[0], bev) and prev_on[1] is bev
