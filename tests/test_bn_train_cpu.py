"""No GPU: the C ABI of BatchNorm with batch statistics on rows (csrc/batchnorm_rows.h) — symbols, argument checks in the order
include/bevmsda.h documents, the workspace size —, the ``bn_train`` switch and ``bottleneck_train_reject``'s rules under it, the
``SyncBN`` norm and the bevformerv2 backbone's build, and the kink condition of the GPU block and net cases from float64 alone."""
import copy
import ctypes

import pytest
import torch

import bn_train_yardstick as N

from bevformer_amd import _lib

OK, NULLP, SHAPE, LARGE, MISAL, OPT, UNSUP = 0, -1, -2, -3, -4, -6, -7
# far apart: nothing overlaps by accident
Z, G, YM, RES, OUT, GY, WS, V = 0x1000000, 0x2000000, 0x3000000, 0x4000000, 0x5000000, 0x6000000, 0x7000000, 0x8000000
MEAN, VAR, GAMMA, BETA, RM, RV, NBT, SUMS = (V + i * 0x10000 for i in range(8))
NAMES = ("bevmsda_bn_rows_workspace_bytes", "bevmsda_bn_stats_rows_f32", "bevmsda_bn_apply_rows_f32",
         "bevmsda_bn_bwd_reduce_rows_f32", "bevmsda_bn_bwd_apply_rows_f32")


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    """Building a module draws its initial weights from torch's global generator, and other test files build their networks from
    that generator's state: every test here hands it back as it found it, so that those files draw the same numbers whether
    this one ran before them or not.  (Everything random HERE comes from seeded generators of its own.)"""
    state = torch.get_rng_state()
    yield
    torch.set_rng_state(state)


@pytest.fixture(scope="module")
def lib():
    from bevformer_amd import build
    if build.is_stale():
        build.build_library()
    return _lib.load(build.LIB_PATH)


def _p(v):
    return ctypes.c_void_p(v) if v else None


def test_signatures_are_listed_and_the_abi_version_stays():
    assert _lib.ABI_VERSION == 7
    for name in NAMES:
        assert name in _lib.SIGNATURES


def test_header_declares_the_entry_points():
    from bevformer_amd import build
    text = open(build.PUBLIC_HEADER).read()
    assert "#define BEVMSDA_ABI_VERSION 7" in text
    assert "int64_t bevmsda_bn_rows_workspace_bytes(int64_t M, int32_t C);" in text
    for name in NAMES[1:]:
        assert f"int {name}(const float *" in text


def test_workspace_size(lib):
    size = lib.bevmsda_bn_rows_workspace_bytes
    assert size(2, 32) == 2 * 32 * 4 and size(1024, 64) == 2 * 64 * 4          # one chunk of rows
    assert size(1025, 64) == 2 * 2 * 64 * 4 and size(40000, 64) == 40 * 2 * 64 * 4
    assert size(1 << 24, 32) == 2048 * 2 * 32 * 4                                # at most 2048 chunks
    for M, C in ((1, 32), (0, 32), (-1, 32), (100, 48), (100, 0), (100, -32), ((1 << 24) + 1, 32), (100, 65536 + 32)):
        assert size(M, C) == 0, (M, C)


def _common(call, strides, pointers, required):
    """The checks the four entry points share behind their options: ``call(**kw)`` with ``M``, ``C``, the stride and pointer names."""
    assert call(M=-1) == SHAPE and call(C=-1) == SHAPE
    assert call(M=-1, C=48) == SHAPE                                    # (before the granularity)
    assert call(M=(1 << 24) + 1) == LARGE and call(C=65536 + 32, **{s: 1 << 17 for s in strides}) == LARGE
    assert call(M=(1 << 24) + 1, C=48) == LARGE
    assert call(M=1) == UNSUP and call(M=0) == UNSUP and call(C=48) == UNSUP and call(C=16) == UNSUP
    assert call(M=1, **{required[0]: 0}) == UNSUP                       # (before the pointers)
    assert call(C=0, **{n: 0 for n in required}) == OK                  # an empty problem, whatever the pointers
    for n in required:
        assert call(**{n: 0}) == NULLP, n
    assert call(**{required[0]: 0, strides[0]: 32}) == NULLP            # (before the strides)
    for s in strides:
        assert call(**{s: 32}) == SHAPE, s
    assert call(**{strides[0]: 32, pointers[0][0]: pointers[0][1] + 4}) == SHAPE    # (before the alignment)
    for s in strides:
        assert call(**{s: 66}) == MISAL, s
    for n, v in pointers:
        assert call(**{n: v + 4}) == MISAL, n


def test_stats_rejects_bad_arguments_in_the_documented_order(lib):
    def call(z=Z, ld_z=64, M=100, C=64, mean=MEAN, var=VAR, rm=RM, rv=RV, nbt=NBT, momentum=0.1, ws=WS):
        return lib.bevmsda_bn_stats_rows_f32(_p(z), ld_z, M, C, _p(mean), _p(var), _p(rm), _p(rv), _p(nbt), momentum, _p(ws), None)
    # (every call here is turned away or empty: a complete call would launch on fake pointers)
    # options first, whatever else is wrong
    assert call(rm=0, M=-1) == OPT and call(rv=0, C=48) == OPT
    assert call(momentum=-0.5, M=-1) == OPT and call(momentum=1.5) == OPT and call(momentum=float("nan")) == OPT
    assert call(rm=0, rv=0, momentum=7.0, M=-1) == SHAPE                 # (no running statistics: the momentum is not looked at)
    _common(call, ["ld_z"], [("z", Z), ("mean", MEAN), ("var", VAR), ("rm", RM), ("rv", RV), ("ws", WS)], ["z", "mean", "var", "ws"])
    assert call(nbt=NBT + 4) == MISAL
    assert call(nbt=NBT + 8, ws=Z) == OPT                                # (the counter: 8 bytes are enough)
    assert call(z=Z + 4, ws=Z) == MISAL                                  # (before the overlap)
    assert call(ws=Z) == OPT and call(mean=Z + 64 * 4) == OPT and call(var=Z + (99 * 64 + 60) * 4) == OPT
    assert call(rm=Z) == OPT and call(rv=Z + 16) == OPT


def test_apply_rejects_bad_arguments_in_the_documented_order(lib):
    def call(z=Z, ld_z=64, mean=MEAN, var=VAR, gamma=GAMMA, beta=BETA, res=RES, ld_res=64, relu=1, M=100, C=64, y=OUT, ld_y=64):
        return lib.bevmsda_bn_apply_rows_f32(_p(z), ld_z, _p(mean), _p(var), _p(gamma), _p(beta), 1e-5, _p(res), ld_res, relu, M, C,
                                             _p(y), ld_y, None)
    assert call(relu=2, M=-1) == OPT and call(relu=-1, C=48) == OPT
    _common(call, ["ld_z", "ld_y", "ld_res"],
            [("z", Z), ("mean", MEAN), ("var", VAR), ("gamma", GAMMA), ("beta", BETA), ("res", RES), ("y", OUT)],
            ["z", "mean", "var", "gamma", "beta", "y"])
    assert call(res=0, ld_res=2, y=Z + 64 * 4) == OPT                    # (no residual: its stride is not looked at)
    assert call(z=Z + 4, y=Z + 64 * 4) == MISAL                          # (before the overlap)
    assert call(y=Z + 64 * 4) == OPT                                     # one row into z
    assert call(y=Z, ld_y=128) == OPT                                    # at z with another stride
    assert call(y=RES) == OPT and call(y=MEAN) == OPT and call(y=BETA - 99 * 64 * 4) == OPT


def test_bwd_reduce_rejects_bad_arguments_in_the_documented_order(lib):
    def call(g=G, ld_g=64, y=YM, ld_y=64, z=Z, ld_z=64, mean=MEAN, var=VAR, M=100, C=64, sums=SUMS, ws=WS):
        return lib.bevmsda_bn_bwd_reduce_rows_f32(_p(g), ld_g, _p(y), ld_y, _p(z), ld_z, _p(mean), _p(var), 1e-5, M, C, _p(sums), _p(ws), None)
    _common(call, ["ld_g", "ld_z", "ld_y"], [("g", G), ("y", YM), ("z", Z), ("mean", MEAN), ("var", VAR), ("sums", SUMS), ("ws", WS)],
            ["g", "z", "mean", "var", "sums", "ws"])
    assert call(g=G + 4, sums=G) == MISAL                                # (before the overlap)
    assert call(sums=G) == OPT and call(ws=Z + 16) == OPT and call(sums=YM + 99 * 64 * 4) == OPT and call(sums=MEAN) == OPT
    assert call(sums=WS) == OPT


def test_bwd_apply_rejects_bad_arguments_in_the_documented_order(lib):
    def call(g=G, ld_g=64, y=YM, ld_y=64, z=Z, ld_z=64, mean=MEAN, var=VAR, gamma=GAMMA, sums=SUMS, M=100, C=64, dz=OUT, ld_dz=64,
             gy=GY, ld_gy=64):
        return lib.bevmsda_bn_bwd_apply_rows_f32(_p(g), ld_g, _p(y), ld_y, _p(z), ld_z, _p(mean), _p(var), _p(gamma), 1e-5, _p(sums), M, C,
                                                 _p(dz), ld_dz, _p(gy), ld_gy, None)
    _common(call, ["ld_g", "ld_z", "ld_dz", "ld_y", "ld_gy"],
            [("g", G), ("y", YM), ("z", Z), ("mean", MEAN), ("var", VAR), ("gamma", GAMMA), ("sums", SUMS), ("dz", OUT), ("gy", GY)],
            ["g", "z", "mean", "var", "gamma", "sums", "dz"])
    assert call(g=G + 4, dz=G + 64 * 4) == MISAL                         # (before the overlap)
    assert call(dz=G + 64 * 4) == OPT and call(dz=G, ld_dz=128) == OPT   # one row into g; at g with another stride
    assert call(dz=Z) == OPT and call(dz=YM) == OPT and call(gy=G) == OPT and call(gy=Z) == OPT and call(gy=OUT) == OPT
    assert call(dz=SUMS - 99 * 64 * 4) == OPT


# ---- the switch and the reject rules

def _block(**kw):
    from bevformer_amd.modules import Bottleneck
    return Bottleneck(128, 32, **kw)


def test_the_switch_exists_and_defaults_off(monkeypatch):
    from bevformer_amd import modes, ops
    assert ops.modes().bn_train is False
    with ops.using(backbone_train=True, bn_train=True) as m:
        assert m.bn_train is True and ops.modes().bn_train is True
    assert ops.modes().bn_train is False
    monkeypatch.setenv("BEVMSDA_BN_TRAIN", "1")
    assert modes.Modes().bn_train is True
    monkeypatch.delenv("BEVMSDA_BN_TRAIN")
    assert modes.Modes().bn_train is False
    for name in ("bn_stats_rows", "bn_apply_rows", "bn_rows_backward", "conv_raw_rows"):
        assert callable(getattr(ops, name))


def test_switch_off_keeps_the_old_reasons():
    from bevformer_amd import ops
    blk = _block().train()
    with ops.using(backbone_train=True):
        assert ops.bottleneck_train_reject(blk) == "a norm is in train() mode (batch statistics)"
        assert ops.bottleneck_train_reject(blk.eval()) == "a norm's affine parameters require a gradient"


def test_switch_on_gives_the_new_reasons_in_order(monkeypatch):
    from bevformer_amd import ops
    from bevformer_amd.modules.backbone import ModulatedDeformConv2dPack
    dcn = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)
    with ops.using(backbone_train=True, bn_train=True, dcn_train=True):
        # every norm in eval mode: the two old rules, unchanged
        assert ops.bottleneck_train_reject(_block().eval()) == "a norm's affine parameters require a gradient"
        frozen = _block(norm_cfg=dict(type="BN", requires_grad=False)).eval()
        assert ops.bottleneck_train_reject(frozen) == "not CUDA fp32 parameters"           # (a frozen block: its present path's next rule)
        # one block that breaks every new rule at once loses them one by one, in the documented order
        blk = _block(dcn=dcn, with_cp=True, norm_cfg=dict(type="SyncBN", momentum=None)).train()
        assert isinstance(blk.conv2, ModulatedDeformConv2dPack)
        monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
        monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
        x1 = torch.zeros(1, 128, 1, 1)
        blk.bn2.eval()
        assert ops.bottleneck_train_reject(blk, x1) == "norms in mixed modes"
        blk.bn2.train()
        assert ops.bottleneck_train_reject(blk, x1) == "a deformable conv2 with batch statistics (not yet)"
        blk = _block(with_cp=True, norm_cfg=dict(type="SyncBN", momentum=None)).train()
        assert ops.bottleneck_train_reject(blk, x1) == "with_cp with batch statistics (not yet)"
        blk.with_cp = False
        assert ops.bottleneck_train_reject(blk, x1) == "a cumulative moving average (momentum=None)"
        for m in (blk.bn1, blk.bn2, blk.bn3):
            m.momentum = 0.1
        assert ops.bottleneck_train_reject(blk, x1) == "SyncBatchNorm across ranks (statistics are not all-reduced here)"
        monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 1)             # one rank: an ordinary BatchNorm
        assert ops.bottleneck_train_reject(blk, x1) == "fewer than two values per channel"
        assert ops.bottleneck_train_reject(blk, torch.zeros(2, 128, 1, 1)) == "not CUDA fp32 parameters"
        assert ops.bottleneck_train_reject(blk) == "not CUDA fp32 parameters"
        with ops.using(gemm="native"):
            assert ops.bottleneck_train_reject(blk) == "GEMM mode native"
        # a stride-2 block whose input has two pixels but whose norms see one
        ds = N._downsample(128, 128, 2, N.BN)
        blk = _block(stride=2, downsample=ds).train()
        assert ops.bottleneck_train_reject(blk, torch.zeros(1, 128, 1, 2)) == "fewer than two values per channel"
    # without dcn_train the pack rule comes first, as before
    with ops.using(backbone_train=True, bn_train=True):
        assert ops.bottleneck_train_reject(_block(dcn=dcn).train()) == "a deformable conv2 (no backward yet)"


def test_cpu_tensors_take_the_module_path_with_the_same_gradients():
    from bevformer_amd import ops
    blk, x, g = N.block_case("stride2_caffe")
    blk = copy.deepcopy(blk)

    def step(**modes):
        b = copy.deepcopy(blk)
        xi = x.clone().requires_grad_()
        with ops.using(**modes):
            out = b(xi)
        (out * g).sum().backward()
        return [out.detach(), xi.grad] + [p.grad for p in b.parameters()] + list(N.running_of(b).values())

    off, on = step(), step(backbone_train=True, bn_train=True)
    assert len(off) == len(on) and all(torch.equal(a, b) for a, b in zip(off, on))
    assert torch.equal(blk.bn1.num_batches_tracked, torch.tensor(0))


# ---- the SyncBN norm and the bevformerv2 backbone

# img_backbone of the reference's projects/configs/bevformerv2/bevformerv2-r50-t1-24ep.py, typed in: values only
V2_IMG_BACKBONE = dict(type="ResNet", depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=-1,
                       norm_cfg=dict(type="SyncBN"), norm_eval=False, style="caffe")


def test_syncbn_builds_a_sync_batch_norm():
    from bevformer_amd.modules.backbone import _build_norm
    n = _build_norm(dict(type="SyncBN"), 64)
    assert isinstance(n, torch.nn.SyncBatchNorm) and n.num_features == 64 and n.eps == 1e-5
    assert list(n.state_dict()) == list(torch.nn.BatchNorm2d(64).state_dict())
    frozen = _build_norm(dict(type="SyncBN", requires_grad=False), 32)
    assert not any(p.requires_grad for p in frozen.parameters())
    with pytest.raises(NotImplementedError):
        _build_norm(dict(type="GN", num_groups=2), 64)


def test_the_bevformerv2_backbone_builds_and_loads_a_bn_state_dict():
    from bevformer_amd.modules import ResNet
    from bevformer_amd.registry import build_backbone
    net = build_backbone(dict(V2_IMG_BACKBONE))
    assert isinstance(net, ResNet)
    norms = [m for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert len(norms) == 1 + 16 * 3 + 4 and all(isinstance(m, torch.nn.SyncBatchNorm) for m in norms)
    net.train()
    assert all(m.training for m in norms) and all(p.requires_grad for p in net.parameters())
    bn = build_backbone(dict(V2_IMG_BACKBONE, norm_cfg=dict(type="BN")))
    assert list(bn.state_dict()) == list(net.state_dict())
    result = net.load_state_dict(bn.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), bn.state_dict().values()))


# ---- the kink condition of the GPU cases, from float64 alone

@pytest.mark.parametrize("name", N.BLOCKS)
def test_the_block_cases_keep_every_relu_off_its_kink(name):
    blk, x, g = N.block_case(name)
    assert all(m.training for m in blk.modules() if isinstance(m, torch.nn.BatchNorm2d))
    margin = N.margin_of(N.pre_activations64(blk, x))
    print(f"block {name}: closest ReLU input {margin:.3e} of its tensor's maximum")
    assert margin >= N.BLOCK_MARGIN
    # both sides of the ReLU are taken: some channels pass, some do not
    out = copy.deepcopy(blk).forward_torch(x).detach()
    assert 0.2 < float((out > 0).float().mean()) < 0.8


def test_the_net_case_keeps_every_relu_off_its_kink():
    net, x, gs = N.make_net()
    assert all(isinstance(m, torch.nn.SyncBatchNorm) and m.training for m in net.modules()
               if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    margin = N.net_margin64(net, x)
    print(f"net: closest ReLU input {margin:.3e} of its tensor's maximum")
    assert margin >= N.NET_MARGIN
