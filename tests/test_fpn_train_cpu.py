"""No GPU: ``ops.fpn_train_reject`` names why a neck or a call is not covered by the training fast path, in its documented order
(``fpn_reject``'s structural and shape rules, subsampled extra levels, the GEMM mode, devices and dtypes — grad mode is no reason);
``ops.fpn_reject`` answers word for word what it did; ``modes.fpn_train`` follows the environment and ``ops.using``; and
``FPN.forward`` on the CPU stays on the torch statements with the switch on."""
import pytest
import torch

import bevformer_amd
from bevformer_amd import ops

import fpn_yardstick as Y


def _neck(in_channels=(64, 96, 128), out_channels=160, num_outs=4, **kw):
    cfg = dict(type="FPN", in_channels=list(in_channels), out_channels=out_channels, start_level=0,
               add_extra_convs="on_output", num_outs=num_outs, relu_before_extra_convs=True)
    cfg.update(kw)
    return bevformer_amd.build_neck(cfg)


def _inputs(in_channels=(64, 96, 128), hw=(12, 20), n_img=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n_img, c, hw[0] >> i, hw[1] >> i, generator=g) for i, c in enumerate(in_channels)]


def _train_reject(neck, xs=None, gemm="split", grad=True):
    with torch.set_grad_enabled(grad), ops.using(gemm=gemm):
        return ops.fpn_train_reject(neck, xs)


def _reject(neck, xs=None, gemm="split", grad=False):
    with torch.set_grad_enabled(grad), ops.using(gemm=gemm):
        return ops.fpn_reject(neck, xs)


# one case per rule, in fpn_reject's order; what fpn_reject says with grad mode off, fpn_train_reject says under grad mode too
STRUCTURE = [
    (lambda: (torch.nn.Linear(4, 4), None), "not an FPN"),
    (lambda: (_neck(add_extra_convs="on_input"), None), "add_extra_convs='on_input'"),
    (lambda: (_neck(add_extra_convs="on_lateral"), None), "add_extra_convs='on_lateral'"),
    (lambda: (_neck(upsample_cfg=dict(mode="bilinear")), None), "upsample_cfg is not nearest by size"),
    (lambda: (_neck(norm_cfg=dict(type="BN")), None), "a ConvModule has a norm or an activation"),
    (lambda: (_neck(in_channels=(64, 80, 128)), None), "channel counts are not multiples of 32"),
    (lambda: (_neck(), _inputs()[:2]), "not one (B, C, H, W) tensor per input level"),
    (lambda: (_neck(), _inputs(in_channels=(64, 64, 128))), "the inputs do not match the lateral convolutions"),
    (lambda: (_neck(), [torch.randn(2, 64, 13, 20), torch.randn(2, 96, 7, 10), torch.randn(2, 128, 4, 5)]),
     "adjacent levels are not exact 2x of each other"),
]


@pytest.mark.parametrize("case", range(len(STRUCTURE)))
def test_structural_and_shape_rules_are_fpn_rejects(case):
    make, why = STRUCTURE[case]
    neck, xs = make()
    assert _reject(neck, xs) == why
    assert _train_reject(neck, xs, grad=True) == why and _train_reject(neck, xs, grad=False) == why
    # (they come before everything else: a native GEMM mode and CPU parameters do not change the answer)
    assert _train_reject(neck, xs, gemm="native") == why and _reject(neck, xs, gemm="native", grad=True) == why


def test_train_reasons_in_order():
    xs = _inputs()
    sub = _neck(add_extra_convs=False)                          # num_outs 4 on three levels: one max_pool2d subsample
    # 1. subsampled extra levels: after structure and shapes, before the GEMM mode
    assert _train_reject(sub, xs, gemm="native") == "subsampled extra levels (no backward yet)"
    assert _train_reject(sub) == "subsampled extra levels (no backward yet)"
    bad = list(xs)
    bad[1] = torch.randn(2, 96, 6, 11)
    assert _train_reject(sub, bad) == "adjacent levels are not exact 2x of each other"
    assert _train_reject(_neck(add_extra_convs=False, num_outs=3), xs, gemm="native") == "GEMM mode native"   # (no extra level)
    # 2. the GEMM mode, before devices
    assert _train_reject(_neck(), xs, gemm="native") == "GEMM mode native"
    # 3. devices and dtypes
    assert _train_reject(_neck(), xs) == "not CUDA fp32 parameters"
    assert _train_reject(_neck()) == "not CUDA fp32 parameters"
    # grad mode is not a reason: the answer is the same either way
    assert _train_reject(_neck(), xs, grad=False) == "not CUDA fp32 parameters"
    assert ops.fpn_train(_neck(), xs) is None


def test_fpn_rejects_answers_are_unchanged():
    xs = _inputs()
    assert _reject(_neck(), xs) == "not CUDA fp32 parameters" and _reject(_neck()) == "not CUDA fp32 parameters"
    assert _reject(_neck(), xs, grad=True) == "grad mode is on"
    assert _reject(_neck(), xs, grad=True, gemm="native") == "grad mode is on"          # grad mode before the GEMM mode
    assert _reject(_neck(), xs, gemm="native") == "GEMM mode native"
    assert _reject(_neck(add_extra_convs=False), xs) == "not CUDA fp32 parameters"      # subsamples are covered at inference
    assert _reject(_neck(add_extra_convs=False), xs, grad=True) == "grad mode is on"


def test_the_switch_follows_the_environment_and_using(monkeypatch):
    from bevformer_amd import modes
    monkeypatch.delenv("BEVMSDA_FPN_TRAIN", raising=False)
    assert modes.Modes().fpn_train is False and ops.modes().fpn_train is False
    monkeypatch.setenv("BEVMSDA_FPN_TRAIN", "1")
    assert modes.Modes().fpn_train is True and modes.Modes().fpn_fused is False         # independent of fpn_fused
    with ops.using(fpn_train=True):
        assert ops.modes().fpn_train is True and ops.modes().fpn_fused is False
        with ops.using(fpn_train=False):
            assert ops.modes().fpn_train is False
    assert ops.modes().fpn_train is False


def test_forward_on_the_cpu_stays_on_the_torch_statements(monkeypatch):
    neck = Y.randomize_neck_(_neck(), seed=6)
    xs = [x.requires_grad_() for x in _inputs(seed=7)]
    want = neck.forward_torch(xs)
    gw = torch.autograd.grad(sum(o.sum() for o in want), [neck.lateral_convs[0].conv.weight, xs[0]])
    calls = []
    real = type(neck).forward_torch
    monkeypatch.setattr(type(neck), "forward_torch", lambda self, inputs: (calls.append(1), real(self, inputs))[1])
    monkeypatch.setattr(ops, "fpn_train", lambda *a, **k: pytest.fail("the fast path ran on CPU tensors"))
    with ops.using(fpn_train=True, fpn_fused=True):
        assert ops.fpn_train_reject(neck, xs) == "not CUDA fp32 parameters"
        got = neck(xs)
    assert calls == [1] and all(torch.equal(g, w) for g, w in zip(got, want))
    gg = torch.autograd.grad(sum(o.sum() for o in got), [neck.lateral_convs[0].conv.weight, xs[0]])
    assert all(torch.equal(a, b) for a, b in zip(gg, gw))
