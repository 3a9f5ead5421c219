"""GPU: the backbone's bottlenecks on channel-last rows (``ops.bottleneck``, ``modes.backbone_fused``) against the module's own
``forward_torch`` in float64 (tests/backbone_yardstick.py).  Bound: error <= 3 x the error of the parent — every plain
convolution as im2col + ``ops.linear``, a pack as the deformable im2col, BatchNorm / add / ReLU in torch fp32 — on the same inputs
in the same GEMM mode; on the sparse integer lattice a block EQUALS the yardstick.  Then the seams: a whole ResNet-50 under the
switch (views all the way into the neck, determinism, graph capture), the per-block fallback, and the switch left off.

torch's own convolutions (the stem; the module path of a rejected block) are not bit-reproducible on an MI355X unless asked to
be, so the tests that compare bits ask (``_deterministic``): what is left to differ is this package's code."""
import contextlib
import functools

import pytest
import torch

import bevformer_amd
import backbone_yardstick as Y
import fpn_yardstick as FY

pytestmark = pytest.mark.gpu

MODES = ["split", "bf16"]
DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)


@contextlib.contextmanager
def _deterministic():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = det


def _downsample(cin, cout, stride):
    return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(cout))


def _make_block(name):
    from bevformer_amd.modules import Bottleneck
    return {
        "plain": lambda: Bottleneck(256, 64, style="caffe"),
        "stage1_first": lambda: Bottleneck(64, 64, downsample=_downsample(64, 256, 1)),
        "stride2_caffe": lambda: Bottleneck(256, 128, stride=2, style="caffe", downsample=_downsample(256, 512, 2)),
        "stride2_pytorch": lambda: Bottleneck(256, 128, stride=2, style="pytorch", downsample=_downsample(256, 512, 2)),
        "dcn": lambda: Bottleneck(256, 64, dcn=DCN, style="caffe"),
        "lattice_downsample": lambda: Bottleneck(64, 64, stride=2, style="caffe", downsample=_downsample(64, 256, 2)),
    }[name]()


BLOCKS = ["plain", "stage1_first", "stride2_caffe", "stride2_pytorch", "dcn"]
LAUNCHES = {"plain": 3, "stage1_first": 4, "stride2_caffe": 4, "stride2_pytorch": 4, "dcn": 4}


@functools.lru_cache(maxsize=None)
def _block_case(name):
    """(block on the GPU in eval mode, input on the GPU, float64 result): made once and shared; nobody writes to it."""
    g = torch.Generator().manual_seed(5 + BLOCKS.index(name))
    blk = Y.randomize_norms_(Y.randomize_convs_(_make_block(name), g), g).eval()
    x = torch.randn(2, blk.conv1.in_channels, 6, 10, generator=g)
    want = Y.block64(blk, x)
    return blk.cuda(), x.cuda(), want


# ---- 1. a block's error bound

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BLOCKS)
def test_bottleneck_within_three_parent_errors(name, mode):
    from bevformer_amd import ops
    blk, x, want = _block_case(name)
    launches = []
    ops.set_gemm_timer(lambda tag, flops, nbytes: (launches.append(tag), contextlib.nullcontext())[1])
    try:
        with torch.no_grad(), ops.using(gemm=mode, backbone_fused=True):
            assert ops.bottleneck_reject(blk, x) is None
            got = blk(x)
    finally:
        ops.set_gemm_timer(None)
    with torch.no_grad(), ops.using(gemm=mode, backbone_fused=False):
        off = blk(x)
        parent = Y.parent_block(blk, x)
    assert tuple(got.shape) == tuple(want.shape) and ops.rows_of_map(got).data_ptr() == got.data_ptr()
    assert len(launches) == LAUNCHES[name], launches        # 3 per plain block, 4 with a downsample or with a pack's offsets
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"{name} {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent
    assert not torch.equal(got, off)                        # the switch did choose another path


# ---- 2. lattice exactness of a block

@functools.lru_cache(maxsize=None)
def _lattice_case(name):
    """A block with sparse lattice parameters and a lattice input, the seed picked on the CPU so that the float64 truth alone
    meets both conditions: every tensor a later convolution reads an integer of magnitude <= 256, more than a quarter of
    the outputs nonzero."""
    for seed in range(32):
        blk = Y.lattice_block_(_make_block(name), seed).eval()
        x = Y.lattice((2, blk.conv1.in_channels, 6, 10), -4, 4, torch.Generator().manual_seed(100 + seed))
        o1, o2, idt, out = Y.block64_intermediates(blk, x)
        ok = all(torch.equal(t, t.round()) and t.abs().max().item() <= Y.BF16_EXACT for t in (o1, o2, idt, out))
        if ok and (out != 0).double().mean().item() > 0.25 and (o1 != 0).double().mean().item() > 0.25 \
                and (o2 != 0).double().mean().item() > 0.25:
            break
    else:
        raise AssertionError("no seed gives a lattice block whose truth is exact and mostly nonzero")
    for t in (o1, o2, idt, out):
        Y.assert_lattice(t, Y.BF16_EXACT)
    assert o1.abs().max() <= 20 and o2.abs().max() <= 64 and out.abs().max() <= 144
    assert (out != 0).double().mean().item() > 0.25
    assert torch.equal(out, Y.block64(blk, x))
    return blk.cuda(), x.cuda(), out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["plain", "lattice_downsample"])
def test_bottleneck_exact_on_the_lattice(name, mode):
    from bevformer_amd import ops
    blk, x, want = _lattice_case(name)
    with torch.no_grad(), ops.using(gemm=mode, backbone_fused=True):
        assert ops.bottleneck_reject(blk, x) is None
        got = blk(x)
    assert torch.equal(got.double().cpu(), want)


# ---- 3. a whole ResNet-50

@functools.lru_cache(maxsize=None)
def _net_case(style):
    """(ResNet-50 on the GPU in eval mode, input on the GPU, float64 outputs): made once per module and shared."""
    from bevformer_amd.modules import ResNet
    g = torch.Generator().manual_seed(21)
    kw = dict(dcn=DCN, stage_with_dcn=(False, False, True, True)) if style == "caffe" else {}
    net = Y.randomize_norms_(ResNet(depth=50, style=style, out_indices=(1, 2, 3), **kw), g).eval()
    x = torch.randn(2, 3, 64, 64, generator=g)
    want = Y.resnet64(net, x)
    return net.cuda(), x.cuda(), want


@functools.lru_cache(maxsize=None)
def _neck():
    neck = bevformer_amd.build_neck(dict(type="FPN", in_channels=[512, 1024, 2048], out_channels=256, start_level=0,
                                         add_extra_convs="on_output", num_outs=4, relu_before_extra_convs=True))
    return FY.randomize_neck_(neck, seed=3).cuda().eval()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("style", ["pytorch", "caffe"])
def test_resnet50_within_three_parent_errors_views_into_the_neck(style, mode):
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck
    net, x, want = _net_case(style)
    neck = _neck()
    with torch.no_grad(), ops.using(gemm=mode, backbone_fused=True), _deterministic():
        assert all(ops.bottleneck_reject(m) is None for m in net.modules() if isinstance(m, Bottleneck))
        got = net(x)
        again = net(x)
        with ops.using(fpn_fused=True):
            assert ops.fpn_reject(neck, list(got)) is None
            got_neck = neck(list(got))
    with torch.no_grad(), ops.using(gemm=mode):
        parent = Y.parent_resnet(net, x)
        parent_neck = FY.parent_fpn(neck.state_dict(), FY.spec_of(neck), parent)
    assert [tuple(o.shape) for o in got] == [(2, 512, 8, 8), (2, 1024, 4, 4), (2, 2048, 2, 2)]
    for lvl, (o, a, p, w) in enumerate(zip(got, again, parent, want)):
        assert ops.rows_of_map(o).data_ptr() == o.data_ptr()            # no copy between backbone and neck
        assert torch.equal(o, a)                                        # two runs are bit-equal
        e_parent, e_fused = Y.max_err(p, w), Y.max_err(o, w)
        print(f"resnet50 {style} {mode} out {lvl}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        assert float(w.abs().max()) > 0.1 and e_fused <= 3 * e_parent
    want_neck = FY.fpn64(neck.state_dict(), FY.spec_of(neck), want)
    for lvl, (o, p, w) in enumerate(zip(got_neck, parent_neck, want_neck)):
        e_parent, e_fused = Y.max_err(p, w), Y.max_err(o, w)
        print(f"resnet50 {style} {mode} neck {lvl}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        assert e_fused <= 3 * e_parent


# ---- 4. graph capture

def test_backbone_is_capturable():
    from bevformer_amd import ops
    net, x, _ = _net_case("caffe")
    with torch.no_grad(), ops.using(gemm="split", backbone_fused=True), _deterministic():
        eager = [o.clone() for o in net(x)]                 # (also builds the weight images outside the capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ys = net(x)
        for _ in range(3):
            for y in ys:
                y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for y, e in zip(ys, eager):
                assert torch.equal(y, e)


# ---- 5. the fallback, block by block

def test_a_backbone_off_the_granularity_runs_the_module_path():
    """``base_channels=48``: the stem and stage 1 are 48 channels wide, off the kernel's granularity, so every block of a one-stage
    backbone is rejected and its output is the switch-off output.  (In a four-stage backbone stages 2 .. 4 are 96 / 192 / 384
    wide — multiples of 32 — and covered: the rejection is per block, which the reasons show.)"""
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck, ResNet
    g = torch.Generator().manual_seed(31)
    net = Y.randomize_norms_(ResNet(depth=50, base_channels=48, num_stages=1, out_indices=(0,)), g).cuda().eval()
    x = torch.randn(2, 3, 64, 64, generator=g).cuda()
    with torch.no_grad(), ops.using(gemm="split"), _deterministic():
        off = net(x)
        with ops.using(backbone_fused=True):
            assert all(ops.bottleneck_reject(b) == "channel counts are not multiples of 32" for b in net.layer1)
            on = net(x)
    assert len(on) == 1 and torch.equal(on[0], off[0]) and float(off[0].abs().max()) > 0.1
    full = ResNet(depth=50, base_channels=48).cuda().eval()
    with torch.no_grad(), ops.using(gemm="split"):
        why = {name: ops.bottleneck_reject(m) for name, m in full.named_modules() if isinstance(m, Bottleneck)}
    assert all((r is not None) == name.startswith("layer1.") for name, r in why.items()), why


@pytest.mark.parametrize("mode", MODES)
def test_a_block_with_a_norm_in_train_mode_falls_back_alone(mode):
    """``layer2[0].bn1`` in ``train()``: that block runs the module path (batch statistics), every other block the fast path; the
    truth and the parent are computed with the same norm states."""
    import copy
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck
    net0, x, _ = _net_case("pytorch")
    net = copy.deepcopy(net0)
    net.layer2[0].bn1.train()
    want = Y.resnet64(net, x)
    with torch.no_grad(), ops.using(gemm=mode, backbone_fused=True):
        why = {name: ops.bottleneck_reject(m) for name, m in net.named_modules() if isinstance(m, Bottleneck)}
        assert why.pop("layer2.0") == "a norm is in train() mode (batch statistics)" and not any(why.values())
        got = net(x)
    with torch.no_grad(), ops.using(gemm=mode):
        off = net(x)
        parent = Y.parent_resnet(net, x)
    for lvl, (o, f, p, w) in enumerate(zip(got, off, parent, want)):
        e_parent, e_fused = Y.max_err(p, w), Y.max_err(o, w)
        print(f"bn1 in train() {mode} out {lvl}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        assert e_fused <= 3 * e_parent
        assert not torch.equal(o, f)                        # the other blocks did take the fast path
    assert not torch.equal(want[0], _net_case("pytorch")[2][0])        # and the norm's state does change the truth


# ---- 6. the switch left off

@pytest.mark.parametrize("name", ["stride2_caffe", "dcn"])
def test_switch_off_is_the_module_path_bit_for_bit(name):
    from bevformer_amd import ops
    blk, x, _ = _block_case(name)
    assert ops.modes().backbone_fused is False
    with torch.no_grad(), ops.using(gemm="split"), _deterministic():
        assert torch.equal(blk(x), blk.forward_torch(x))
    with ops.using(gemm="split", backbone_fused=True), _deterministic():        # grad mode on: rejected, the module path again
        assert ops.bottleneck(blk, x) is None
        assert torch.equal(blk(x), blk.forward_torch(x))
