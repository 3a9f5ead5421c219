"""No GPU: the ``backbone_train`` switch (default, environment, per-thread override), the order and wording of
``ops.bottleneck_train_reject``'s reasons, and on CPU tensors the module path with gradients bit-equal to the switch-off run."""
import torch

from bevformer_amd import modes, ops
from bevformer_amd.modules import Bottleneck, ResNet

FROZEN_BN = dict(type="BN", requires_grad=False)
DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)


def test_mode_default_environment_and_override(monkeypatch):
    assert modes.process_defaults().backbone_train is False and ops.modes().backbone_train is False
    monkeypatch.delenv("BEVMSDA_BACKBONE_TRAIN", raising=False)
    assert modes.Modes().backbone_train is False
    for value, want in (("1", True), ("0", False), ("", False), ("true", False)):
        monkeypatch.setenv("BEVMSDA_BACKBONE_TRAIN", value)
        assert modes.Modes().backbone_train is want, value
    with ops.using(backbone_train=True):
        assert ops.modes().backbone_train is True and modes.process_defaults().backbone_train is False
    assert ops.modes().backbone_train is False
    assert "_bevmsda_dgrad" in ops.IMAGE_ATTRS


def _block(**kw):
    kw.setdefault("norm_cfg", FROZEN_BN)
    return Bottleneck(64, 16 if kw.pop("narrow", False) else 32, downsample=None if kw.pop("same", False) else _ds(), **kw).eval()


def _ds():
    ds = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, bias=False), torch.nn.BatchNorm2d(128))
    for p in ds[1].parameters():
        p.requires_grad = False
    return ds


def test_reject_reasons_in_order():
    x = torch.zeros(1, 64, 4, 4)
    reason = lambda b, xx=x: ops.bottleneck_train_reject(b, xx)
    with ops.using(gemm="split"):
        # structure first, with bottleneck_reject's words
        assert reason(torch.nn.Identity()) == "not a bottleneck (conv1 / norm1 / conv2 / norm2 / conv3 / norm3 / downsample)"
        assert reason(_block(narrow=True)) == "channel counts are not multiples of 32"
        assert reason(_block(), torch.zeros(1, 32, 4, 4)) == "the input does not match the block"
        # then, in this order: a pack, a norm in train(), trainable norms, the GEMM mode, devices
        everything = _block(dcn=DCN, norm_cfg=dict(type="BN"))
        everything.bn2.train()
        with ops.using(gemm="native"):
            assert reason(everything) == "a deformable conv2 (no backward yet)"
            b = _block(norm_cfg=dict(type="BN"))
            b.bn2.train()
            assert reason(b) == "a norm is in train() mode (batch statistics)"
            b.bn2.eval()
            assert reason(b) == "a norm's affine parameters require a gradient"
            assert reason(_block()) == "GEMM mode native"
        assert reason(_block()) == "not CUDA fp32 parameters"
        assert reason(_block(), None) == "not CUDA fp32 parameters"
        # grad mode is no reason here, and stays one for the inference path
        assert torch.is_grad_enabled() and ops.bottleneck_reject(_block(), x) == "grad mode is on"
        with torch.no_grad():
            assert reason(_block()) == "not CUDA fp32 parameters" and ops.bottleneck_reject(_block(), x) == "not CUDA fp32 parameters"
        b = _block()
        b.downsample[1].train()
        assert reason(b) == "a norm is in train() mode (batch statistics)"
        assert ops.bottleneck_train(_block(), x) is None


def test_cpu_tensors_take_the_module_path_with_the_switch_on():
    gen = torch.Generator().manual_seed(3)
    net = ResNet(depth=50, base_channels=32, stem_channels=64, num_stages=2, out_indices=(0, 1), frozen_stages=1, norm_eval=True,
                 norm_cfg=FROZEN_BN, with_cp=True).train()
    x = torch.randn(1, 3, 32, 32, generator=gen)

    def grads():
        for p in net.parameters():
            p.grad = None
        outs = net(x)
        sum(o.sum() for o in outs).backward()
        return [o.detach() for o in outs], {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    outs_off, g_off = grads()
    with ops.using(backbone_train=True):
        outs_on, g_on = grads()
    assert g_off and sorted(g_on) == sorted(g_off) and all(n.startswith("layer2.") for n in g_off)
    assert all(torch.equal(a, b) for a, b in zip(outs_on, outs_off))
    assert all(torch.equal(g_on[n], g_off[n]) for n in g_off)
