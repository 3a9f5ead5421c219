"""No GPU: the image neck builds from the reference's config (``build_neck(synthetic.neck_cfg(...))``), its module path agrees
with the float64 restatement of mmdet's FPN forward (tests/fpn_yardstick.py), and ``ops.fpn_reject`` names why a module or a
call is not covered by the fast path — after which ``forward`` is the module path bit for bit."""
import pytest
import torch

import bevformer_amd
from bevformer_amd import ops, synthetic as S

import fpn_yardstick as Y


def _neck(in_channels=(64, 96, 128), out_channels=160, num_outs=4, **kw):
    cfg = dict(type="FPN", in_channels=list(in_channels), out_channels=out_channels, start_level=0,
               add_extra_convs="on_output", num_outs=num_outs, relu_before_extra_convs=True)
    cfg.update(kw)
    return bevformer_amd.build_neck(cfg)


def _inputs(in_channels=(64, 96, 128), hw=(12, 20), n_img=2, seed=0, lattice=False):
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *s: Y.lattice(s, -4, 4, g)) if lattice else (lambda *s: torch.randn(*s, generator=g))
    return [draw(n_img, c, hw[0] >> i, hw[1] >> i) for i, c in enumerate(in_channels)]


def test_base_neck_builds_with_the_reference_keys_and_shapes():
    neck = bevformer_amd.build_neck(S.neck_cfg("base"))
    want = {f"lateral_convs.{i}.conv.{p}" for i in range(3) for p in ("weight", "bias")} \
        | {f"fpn_convs.{i}.conv.{p}" for i in range(4) for p in ("weight", "bias")}
    assert set(neck.state_dict()) == want
    assert neck.lateral_convs[2].conv.weight.shape == (256, 2048, 1, 1)
    assert neck.fpn_convs[3].conv.stride == (2, 2) and neck.fpn_convs[3].conv.weight.shape == (256, 256, 3, 3)
    H, W = 10, 12                                   # (the base image's 116 x 200 halves the same way)
    xs = S.make_neck_inputs("base", n_img=1, hw=(H * 4, W * 4))
    assert [tuple(x.shape) for x in xs] == [(1, 512, 4 * H, 4 * W), (1, 1024, 2 * H, 2 * W), (1, 2048, H, W)]
    with torch.no_grad():
        outs = neck(xs)
    assert [tuple(o.shape) for o in outs] == [(1, 256, 4 * H, 4 * W), (1, 256, 2 * H, 2 * W), (1, 256, H, W),
                                              (1, 256, (H - 1) // 2 + 1, (W - 1) // 2 + 1)]
    # the base workload's four levels are this pyramid of the base image
    h0, w0 = S.NECKS["base"][2]
    assert [(h0, w0), (h0 // 2, w0 // 2), (h0 // 4, w0 // 4), ((h0 // 4 - 1) // 2 + 1, (w0 // 4 - 1) // 2 + 1)] \
        == S.WORKLOADS["base"]["shapes"]


def test_tiny_neck_builds_one_level():
    neck = bevformer_amd.build_neck(S.neck_cfg("tiny"))
    assert set(neck.state_dict()) == {f"{n}.0.conv.{p}" for n in ("lateral_convs", "fpn_convs") for p in ("weight", "bias")}
    xs = S.make_neck_inputs("tiny", n_img=2, hw=(3, 5))
    with torch.no_grad():
        outs = neck(xs)
    assert len(outs) == 1 and tuple(outs[0].shape) == (2, 256, 3, 5)
    assert S.NECKS["tiny"][2] == S.WORKLOADS["tiny"]["shapes"][0] and S.NECKS["small"][2] == S.WORKLOADS["small"]["shapes"][0]
    assert len(bevformer_amd.build_neck(S.neck_cfg("v2")).fpn_convs) == 5


def test_init_is_xavier_uniform_with_zero_bias():
    neck = _neck()
    w = neck.lateral_convs[0].conv.weight.detach()
    bound = (6.0 / (w.shape[1] + w.shape[0])) ** 0.5
    assert w.abs().max().item() <= bound and w.abs().max().item() > 0.9 * bound
    assert all(float(m.conv.bias.detach().abs().max()) == 0.0 for m in list(neck.lateral_convs) + list(neck.fpn_convs))


def test_module_forward_equals_the_yardstick_on_the_lattice():
    neck = Y.lattice_neck_(_neck(num_outs=5), seed=1)
    xs = _inputs(lattice=True)
    want = Y.fpn64(neck.state_dict(), Y.spec_of(neck), xs, check_lattice=True)
    with torch.no_grad():
        got = neck(xs)
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        assert torch.equal(g.double(), w)


def test_module_forward_agrees_with_the_yardstick_on_random_inputs():
    neck = Y.randomize_neck_(_neck(), seed=2)
    xs = _inputs(seed=3)
    want = Y.fpn64(neck.state_dict(), Y.spec_of(neck), xs)
    with torch.no_grad():
        got = neck(xs)
    for g, w in zip(got, want):
        # fp32 rounding of sums of <= 9 * 160 products of O(1 / sqrt(K)) terms at O(1) results: a few 1e-6
        assert Y.max_err(g, w) <= 1e-4 * max(1.0, w.abs().max().item())


def test_relu_only_before_the_second_extra_level():
    """``num_outs = ins + 2``: the first extra level reads the last output as it is, the second its ReLU."""
    neck = Y.randomize_neck_(_neck(num_outs=5), seed=4)
    xs = _inputs(seed=5)
    sd = {k: v.double() for k, v in neck.state_dict().items()}
    with torch.no_grad():
        outs = neck(xs)
    assert (outs[2] < 0).any() and (outs[3] < 0).any()
    conv = lambda x, i, relu: Y.conv64(x, sd[f"fpn_convs.{i}.conv.weight"], sd[f"fpn_convs.{i}.conv.bias"], 2, relu)
    tol = lambda w: 1e-4 * max(1.0, w.abs().max().item())
    assert Y.max_err(outs[3], conv(outs[2], 3, False)) <= tol(outs[3])
    assert Y.max_err(outs[3], conv(outs[2], 3, True)) > 100 * tol(outs[3])
    assert Y.max_err(outs[4], conv(outs[3], 4, True)) <= tol(outs[4])
    assert Y.max_err(outs[4], conv(outs[3], 4, False)) > 100 * tol(outs[4])
    off = _neck(num_outs=5, relu_before_extra_convs=False)
    off.load_state_dict(neck.state_dict())
    with torch.no_grad():
        assert Y.max_err(off(xs)[4], conv(outs[3], 4, False)) <= tol(outs[4])


def _reject(neck, xs=None, gemm="split", grad=False):
    with torch.set_grad_enabled(grad), ops.using(gemm=gemm):
        return ops.fpn_reject(neck, xs)


def test_reject_cpu_tensors():
    assert _reject(_neck(), _inputs()) == "not CUDA fp32 parameters"
    assert _reject(_neck()) == "not CUDA fp32 parameters"


def test_reject_grad_mode():
    assert _reject(_neck(), _inputs(), grad=True) == "grad mode is on"


def test_reject_native_gemm():
    assert _reject(_neck(), _inputs(), gemm="native") == "GEMM mode native"


def test_reject_a_norm_inside_a_conv_module():
    assert _reject(_neck(norm_cfg=dict(type="BN"))) == "a ConvModule has a norm or an activation"
    assert _reject(_neck(act_cfg=dict(type="ReLU"))) == "a ConvModule has a norm or an activation"
    assert _reject(_neck(norm_cfg=dict(type="BN"), no_norm_on_lateral=True)) == "a ConvModule has a norm or an activation"


def test_reject_extra_convs_on_input():
    assert _reject(_neck(add_extra_convs="on_input")) == "add_extra_convs='on_input'"
    assert _reject(_neck(add_extra_convs=True)) == "add_extra_convs='on_input'"
    assert _reject(_neck(add_extra_convs="on_lateral")) == "add_extra_convs='on_lateral'"
    assert _reject(_neck(add_extra_convs=False)) == "not CUDA fp32 parameters"          # covered as far as a CPU can tell


def test_reject_a_level_pair_that_is_not_2x():
    xs = _inputs()
    xs[1] = torch.randn(2, 96, 6, 11)
    assert _reject(_neck(), xs) == "adjacent levels are not exact 2x of each other"
    odd = [torch.randn(2, 64, 13, 20), torch.randn(2, 96, 7, 10), torch.randn(2, 128, 4, 5)]
    assert _reject(_neck(), odd) == "adjacent levels are not exact 2x of each other"


def test_reject_a_channel_count_off_the_granularity():
    assert _reject(_neck(in_channels=(64, 80, 128))) == "channel counts are not multiples of 32"
    assert _reject(_neck(out_channels=144)) == "channel counts are not multiples of 32"


def test_reject_other_structures():
    assert _reject(torch.nn.Linear(4, 4)) == "not an FPN"
    assert _reject(_neck(upsample_cfg=dict(mode="bilinear"))) == "upsample_cfg is not nearest by size"
    assert _reject(_neck(upsample_cfg=dict(mode="nearest", scale_factor=2))) == "upsample_cfg is not nearest by size"
    assert _reject(_neck(), _inputs()[:2]) == "not one (B, C, H, W) tensor per input level"


def test_forward_with_the_mode_set_but_rejected_is_the_module_path():
    neck = Y.randomize_neck_(_neck(), seed=6)
    xs = _inputs(seed=7)
    with torch.no_grad():
        want = neck(xs)
        with ops.using(fpn_fused=True):
            assert ops.fpn_reject(neck, xs) is not None and ops.fpn(neck, xs) is None
            got = neck(xs)
    assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


def test_the_switch_is_off_by_default(monkeypatch):
    from bevformer_amd import modes
    monkeypatch.delenv("BEVMSDA_FPN_FUSED", raising=False)
    assert modes.Modes().fpn_fused is False
    monkeypatch.setenv("BEVMSDA_FPN_FUSED", "1")
    assert modes.Modes().fpn_fused is True
