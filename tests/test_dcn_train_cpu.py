"""No GPU: the ``dcn_train`` switch (default, environment, per-thread override, the slot), ``ops.bottleneck_train_reject``'s reason
for a DCNv2 ``conv2`` with the switch off and the order of its reasons with it on, and on CPU tensors the module path with
gradients bit-equal to the switches-off run."""
import torch

from bevformer_amd import modes, ops
from bevformer_amd.modules import Bottleneck, ResNet

FROZEN_BN = dict(type="BN", requires_grad=False)
DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)
OLD_REASON = "a deformable conv2 (no backward yet)"


def test_mode_default_environment_override_and_slot(monkeypatch):
    assert "dcn_train" in modes.Modes.__slots__
    assert modes.process_defaults().dcn_train is False and ops.modes().dcn_train is False
    monkeypatch.delenv("BEVMSDA_DCN_TRAIN", raising=False)
    assert modes.Modes().dcn_train is False
    for value, want in (("1", True), ("0", False), ("", False), ("true", False)):
        monkeypatch.setenv("BEVMSDA_DCN_TRAIN", value)
        assert modes.Modes().dcn_train is want, value
        assert modes.Modes().backbone_train is False                # (the switch does not turn the other on)
    with ops.using(dcn_train=True):
        assert ops.modes().dcn_train is True and modes.process_defaults().dcn_train is False
        assert ops.modes().snapshot().dcn_train is True             # (what an autograd Function carries to its backward)
    assert ops.modes().dcn_train is False
    assert "_bevmsda_ddgrad" in ops.IMAGE_ATTRS and "_bevmsda_dcnoff32" in ops.IMAGE_ATTRS


def _ds():
    ds = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, bias=False), torch.nn.BatchNorm2d(128))
    for p in ds[1].parameters():
        p.requires_grad = False
    return ds


def _block(**kw):
    kw.setdefault("norm_cfg", FROZEN_BN)
    kw.setdefault("dcn", DCN)
    return Bottleneck(64, 32, downsample=_ds(), **kw).eval()


def test_a_pack_keeps_the_old_reason_with_the_switch_off():
    x = torch.zeros(1, 64, 4, 4)
    with ops.using(gemm="split"):
        assert ops.bottleneck_train_reject(_block(), x) == OLD_REASON
        with ops.using(backbone_train=True):
            assert ops.bottleneck_train_reject(_block(), x) == OLD_REASON
            assert ops.bottleneck_train(_block(), x) is None


def test_reject_reasons_in_order_with_the_switch_on():
    x = torch.zeros(1, 64, 4, 4)
    reason = lambda b, xx=x: ops.bottleneck_train_reject(b, xx)
    with ops.using(gemm="split", backbone_train=True, dcn_train=True):
        # the pack's structural rules first (with bottleneck_reject's words)
        b = _block()
        b.conv2.dilation = (2, 2)
        assert reason(b) == "the convolution is dilated"
        b = _block()
        b.conv2.deform_groups = 2
        assert reason(b) == "groups or deform_groups above 1"
        b = _block()
        b.conv2.conv_offset = torch.nn.Conv2d(32, 27, 3, padding=1, stride=2)
        assert reason(b) == "conv_offset does not match the convolution"
        b = _block()
        b.conv2.bias = torch.nn.Parameter(torch.zeros(32))
        assert reason(b) == "a bias and a norm (one epilogue)"          # (dcn_reject's words)
        with ops.using(dcn_train=False):
            assert reason(b) == "a convolution has a bias"              # (as before)
        assert reason(_block(), torch.zeros(1, 32, 4, 4)) == "the input does not match the block"
        # then the rest of the order, unchanged: a norm in train(), trainable norms, the GEMM mode, devices
        everything = _block(norm_cfg=dict(type="BN"))
        everything.bn2.train()
        with ops.using(gemm="native"):
            assert reason(everything) == "a norm is in train() mode (batch statistics)"
            everything.bn2.eval()
            assert reason(everything) == "a norm's affine parameters require a gradient"
            assert reason(_block()) == "GEMM mode native"
        assert reason(_block()) == "not CUDA fp32 parameters"
        assert reason(_block(), None) == "not CUDA fp32 parameters"
        assert ops.bottleneck_train(_block(), x) is None
        # the inference paths keep their own rule
        assert torch.is_grad_enabled() and ops.bottleneck_reject(_block(), x) == "grad mode is on"
        assert ops.dcn_reject(_block().conv2, torch.zeros(1, 32, 4, 4)) == "grad mode is on"
    # the switch alone (without backbone_train) changes the reason, not the dispatch: modules test backbone_train first
    with ops.using(gemm="split", dcn_train=True):
        assert reason(_block()) == "not CUDA fp32 parameters"


def test_cpu_tensors_take_the_module_path_with_both_switches_on():
    gen = torch.Generator().manual_seed(3)
    net = ResNet(depth=50, base_channels=32, stem_channels=64, num_stages=2, out_indices=(0, 1), frozen_stages=0, norm_eval=True,
                 norm_cfg=FROZEN_BN, dcn=DCN, stage_with_dcn=(False, True)).train()
    with torch.no_grad():               # (conv_offset starts at zero: give the offsets something to do)
        for m in net.modules():
            if hasattr(m, "conv_offset"):
                m.conv_offset.weight.copy_(torch.randn(m.conv_offset.weight.shape, generator=gen) * 0.02)
                m.conv_offset.bias.copy_(torch.randn(27, generator=gen) * 0.3)
    x = torch.randn(1, 3, 32, 32, generator=gen)

    def grads():
        for p in net.parameters():
            p.grad = None
        outs = net(x)
        sum(o.sum() for o in outs).backward()
        return [o.detach() for o in outs], {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    outs_off, g_off = grads()
    with ops.using(backbone_train=True, dcn_train=True):
        outs_on, g_on = grads()
    assert any("conv_offset" in n for n in g_off) and sorted(g_on) == sorted(g_off)
    assert all(torch.equal(a, b) for a, b in zip(outs_on, outs_off))
    assert all(torch.equal(g_on[n], g_off[n]) for n in g_off)
