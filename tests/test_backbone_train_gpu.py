"""GPU: training a backbone with frozen BatchNorms on channel-last rows (``ops.bottleneck_train``, ``modes.backbone_train``) against
float64 autograd through the module's own ``forward_torch`` (tests/backbone_train_yardstick.py).  On the sparse integer lattice
of ``backbone_yardstick.lattice_block_`` with an integer output gradient every pre-activation is an integer — a kink is an exact
zero in every precision — and every gradient EQUALS float64.  On random inputs: error <= 3 x the error of the parent (im2col +
``ops.linear``'s autograd path, BatchNorm / add / ReLU in torch fp32) on the same inputs in the same GEMM mode.  Then the seams: a
ResNet-50 under ``train()`` with a frozen stage, DCN stages on the module path, a captured training step whose weights change
between replays, and the switch left off."""
import contextlib
import copy
import functools

import pytest
import torch

import backbone_train_yardstick as T
import backbone_yardstick as Y

pytestmark = pytest.mark.gpu

MODES = ["split", "bf16"]
FROZEN_BN = dict(type="BN", requires_grad=False)
DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)


def _downsample(cin, cout, stride):
    ds = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(cout))
    for p in ds[1].parameters():
        p.requires_grad = False
    return ds


def _make_block(name):
    from bevformer_amd.modules import Bottleneck
    kw = dict(norm_cfg=FROZEN_BN)
    blk = {
        "plain": lambda: Bottleneck(256, 64, style="caffe", **kw),
        "stride2_pytorch": lambda: Bottleneck(64, 64, stride=2, style="pytorch", downsample=_downsample(64, 256, 2), **kw),
        "stride2_caffe": lambda: Bottleneck(64, 64, stride=2, style="caffe", downsample=_downsample(64, 256, 2), **kw),
        "with_cp": lambda: Bottleneck(256, 64, style="caffe", with_cp=True, **kw),
        "input_without_grad": lambda: Bottleneck(64, 64, stride=2, style="pytorch", downsample=_downsample(64, 256, 2), **kw),
        "frozen_conv2": lambda: Bottleneck(256, 64, style="caffe", **kw),
        "random": lambda: Bottleneck(32, 32, downsample=_downsample(32, 128, 1), **kw),
    }[name]()
    if name == "frozen_conv2":
        blk.conv2.weight.requires_grad = False
    return blk


@contextlib.contextmanager
def _launch_tags():
    from bevformer_amd import ops
    tags = []
    ops.set_gemm_timer(lambda tag, flops, nbytes: (tags.append(tag), contextlib.nullcontext())[1])
    try:
        yield tags
    finally:
        ops.set_gemm_timer(None)


def _step(blk, x, g, need_x=True):
    """(out, dx or None, {name: dW}) of ``sum(g * blk(x))`` through the module's ``forward`` in the modes in force."""
    from bevformer_amd import ops
    x = x.detach().clone().requires_grad_(need_x)
    for p in blk.parameters():
        p.grad = None
    _step.dx_in_rows = None
    if need_x:      # (the leaf's accumulation re-lays the gradient out as the leaf: look at what the block's node handed over)
        x.register_hook(lambda gx: setattr(_step, "dx_in_rows", ops.rows_of_map(gx).data_ptr() == gx.data_ptr()))
    out = blk(x)
    (out * g).sum().backward()
    return out.detach(), x.grad, {n: p.grad for n, p in blk.named_parameters() if p.requires_grad}


# ---- 1. lattice blocks: every gradient equals float64

LATTICE = ["plain", "stride2_pytorch", "stride2_caffe", "with_cp", "input_without_grad", "frozen_conv2"]
# kernel launches of one forward + backward (tags of the GEMM timer): 3 (+ 1 downsample) forward; backward 1 mask + a weight
# gradient and an input gradient per convolution, less what nobody asked for, plus with_cp's two recomputing launches
N_LAUNCHES = {"plain": 3 + 7, "stride2_pytorch": 4 + 9, "stride2_caffe": 4 + 9, "with_cp": 3 + 2 + 7, "input_without_grad": 4 + 7,
              "frozen_conv2": 3 + 6}


@functools.lru_cache(maxsize=None)
def _lattice_case(name):
    """A block with sparse lattice parameters, a lattice input and an integer output gradient, the seed picked on the CPU so
    that the float64 truth alone meets the conditions: every tensor a kernel reads — activations and the three ``gz`` — an
    integer of magnitude <= 256 (exactly a bf16 number), every gradient an integer below 2^24, and the gradients not trivial."""
    need_x = name != "input_without_grad"
    for seed in range(32):
        blk = Y.lattice_block_(_make_block(name), seed).eval()
        gen = torch.Generator().manual_seed(200 + seed)
        x = Y.lattice((2, blk.conv1.in_channels, 6, 10), -4, 4, gen)
        o1, o2, idt, out = Y.block64_intermediates(blk, x)
        g = Y.lattice(tuple(out.shape), -2, 2, gen)
        gz = T.block_gz64(blk, x, g)
        out64, dx64, gw64 = T.block_grads64(blk, x, g, need_x)
        exact = lambda t, bound: torch.equal(t, t.round()) and t.abs().max().item() <= bound
        ok = all(exact(t, Y.BF16_EXACT) for t in (o1, o2, idt, out) + gz) and all(exact(t, float(1 << 24)) for t in gw64.values()) \
            and (dx64 is None or exact(dx64, float(1 << 24)))
        busy = all((t != 0).double().mean().item() > 0.02 for t in gz) and all(t.abs().max().item() > 0 for t in gw64.values())
        if ok and busy:
            break
    else:
        raise AssertionError("no seed gives a lattice block whose truth is exact and not trivial")
    for t in (o1, o2, idt, out) + gz:
        Y.assert_lattice(t, Y.BF16_EXACT)
    for t in list(gw64.values()) + ([dx64] if need_x else []):
        Y.assert_lattice(t)
    assert torch.equal(out64, out)
    return blk.cuda(), x.cuda(), g.cuda(), (out64, dx64, gw64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", LATTICE)
def test_block_gradients_equal_float64_on_the_lattice(name, mode):
    from bevformer_amd import ops
    blk, x, g, (out64, dx64, gw64) = _lattice_case(name)
    need_x = name != "input_without_grad"
    with ops.using(gemm=mode, backbone_train=True), _launch_tags() as tags:
        assert ops.bottleneck_train_reject(blk, x) is None
        out, dx, gw = _step(blk, x, g, need_x)
    assert len(tags) == N_LAUNCHES[name], tags
    assert torch.equal(out.double().cpu(), out64)
    assert (dx is None) == (not need_x) and (not need_x or torch.equal(dx.double().cpu(), dx64))
    assert need_x or not any(t in tags for t in ("bottleneck_conv1_dgrad", "bottleneck_downsample_dgrad"))
    assert sorted(gw) == sorted(gw64) and ("conv2.weight" in gw) == (name != "frozen_conv2")
    for n, want in gw64.items():
        assert torch.equal(gw[n].double().cpu(), want), n
    assert _step.dx_in_rows is (True if need_x else None)               # the gradient stays in rows between covered blocks


# ---- 2. a random block in split mode: within three parent errors, no ReLU within delta of its kink

# seed 50973: of the seeds 0 .. 59999 the one whose float64 pre-activations keep the largest distance from zero, 4.633e-3 (the
# expected closest of 3072 unit-scale values is 4e-4).  delta, measured on the GPU when this was written: the parent's forward
# error 3.218e-5 (outputs up to 6.6), so delta = 100 x that = 3.218e-3, below what the seed gives
RANDOM_SEED, RANDOM_MARGIN = 50973, 4.5e-3


@functools.lru_cache(maxsize=None)
def _random_case():
    gen = torch.Generator().manual_seed(RANDOM_SEED)
    blk = Y.randomize_norms_(Y.randomize_convs_(_make_block("random"), gen), gen).eval()
    x = torch.randn(1, 32, 4, 4, generator=gen)
    g = torch.randn(1, 128, 4, 4, generator=gen)
    return blk, x, g


def test_the_recorded_seed_keeps_every_relu_off_its_kink():
    """CPU arithmetic only (float64): the condition the seed was chosen for."""
    blk, x, g = _random_case()
    closest = min(p.abs().min().item() for p in T.pre_activations64(blk, x))
    print(f"closest pre-activation to zero: {closest:.3e}")
    assert closest >= RANDOM_MARGIN


def test_random_block_within_three_parent_errors():
    from bevformer_amd import ops
    blk, x, g = _random_case()
    out64, dx64, gw64 = T.block_grads64(blk, x, g)
    closest = min(p.abs().min().item() for p in T.pre_activations64(blk, x))
    blk, x, g = copy.deepcopy(blk).cuda(), x.cuda(), g.cuda()
    with ops.using(gemm="split", backbone_train=True):
        pout, pdx, pgw = T.parent_block_grads(blk, x, g)
        delta = 100 * T.max_err(pout, out64)
        print(f"seed {RANDOM_SEED}: parent forward error {delta / 100:.3e}, delta {delta:.3e}, closest pre-activation {closest:.3e}")
        assert closest >= delta                                 # no mask can flip between the precisions
        out, dx, gw = _step(blk, x, g)
    pairs = [("dx", dx, pdx, dx64)] + [(n, gw[n], pgw[n], gw64[n]) for n in gw64]
    for what, got, parent, want in pairs:
        e_parent, e = T.max_err(parent, want), T.max_err(got, want)
        print(f"random block {what}: E_parent {e_parent:.3e}  fused {e:.3e}  bound {3 * e_parent:.3e}")
        assert float(want.abs().max()) > 1e-3 and e <= 3 * e_parent, what


# ---- 3. a ResNet-50 under train()

# A random ResNet-50 would put a few of its 400,000 ReLU inputs within the forward's rounding error of their kinks, and one flipped
# mask drowns every rounding error below it: backbone_train_yardstick.keep_kinks_away_ moves the kinks away from the data, from
# float64 alone, and the tests assert that the closest ReLU input keeps NET_MARGIN_FACTOR x the parent's relative forward error.
NET_MARGIN_FACTOR = 100


def _net(style, dcn=False):
    from bevformer_amd.modules import ResNet
    gen = torch.Generator().manual_seed(41)
    kw = dict(dcn=DCN, stage_with_dcn=(False, False, True, True)) if dcn else {}
    # (stem_channels=64: the stem kernel's width; base_channels=32 keeps the stages small)
    net = ResNet(depth=50, base_channels=32, stem_channels=64, frozen_stages=1, norm_eval=True, norm_cfg=FROZEN_BN, style=style,
                 out_indices=(1, 2, 3), zero_init_residual=False, **kw)
    # (packs=False: a pack's conv_offset keeps its zero initialisation, so every sample position is an exact integer in every
    # precision — a bilinear sample's slope in its offset jumps at pixel boundaries, and positions that the arms round to different
    # sides of one would take different slopes: the same argument as for the ReLUs, settled the same way, from the inputs alone)
    Y.randomize_norms_(net, gen, packs=False).train()
    x = torch.randn(2, 3, 64, 64, generator=gen)
    T.keep_kinks_away_(net, x, gen, k=10.0)
    gs = [torch.randn(2, c, s, s, generator=gen) for c, s in ((256, 8), (512, 4), (1024, 2))]
    return net, x, gs


def _parent_net_grads(net, x, gs):
    """The backbone with the parent's operators: the frozen stem and stage on torch without gradients, every trainable block with
    a plain conv2 as ``parent_block_diff``, a DCN block as its own ``forward_torch`` in fp32."""
    def block(b, y):
        if not any(p.requires_grad for p in b.parameters()):
            with torch.no_grad():
                return b.forward_torch(y)
        return b.forward_torch(y) if hasattr(b.conv2, "conv_offset") else T.parent_block_diff(b, y)
    with torch.enable_grad():
        with torch.no_grad():
            y = net.maxpool(net.relu(net.bn1(net.conv1(x))))
        outs = []
        for i, name in enumerate(net.res_layers):
            for b in getattr(net, name):
                y = block(b, y)
            if i in net.out_indices:
                outs.append(y)
        loss = sum((o * g).sum() for o, g in zip(outs, gs))
        return [o.detach() for o in outs], T._grads_of(net, loss)


@contextlib.contextmanager
def _spy(monkeypatch):
    """Count what ran: ``ops.stem`` / ``ops.bottleneck`` / ``ops.bottleneck_train`` calls that returned a map, and torch convolutions."""
    from bevformer_amd import ops
    seen = dict(stem=0, bottleneck=0, bottleneck_train=0, conv2d=0)

    def wrap(name):
        fn = getattr(ops, name)

        def spy(*a, **k):
            y = fn(*a, **k)
            seen[name] += y is not None
            return y
        monkeypatch.setattr(ops, name, spy)
    for name in ("stem", "bottleneck", "bottleneck_train"):
        wrap(name)
    conv_forward = torch.nn.Conv2d.forward

    def counting(self, x):
        seen["conv2d"] += 1
        return conv_forward(self, x)
    monkeypatch.setattr(torch.nn.Conv2d, "forward", counting)
    yield seen
    monkeypatch.undo()


def _assert_margin(tag, net, x, parent_outs, outs64):
    """No ReLU of a trainable block within NET_MARGIN_FACTOR forward errors of its kink (both relative to their tensors' maxima)."""
    margin = T.relu_margin64(net, x)
    e_fwd = max(T.max_err(p, w) / float(w.abs().max()) for p, w in zip(parent_outs, outs64))
    print(f"{tag}: closest ReLU input {margin:.3e} of its tensor's maximum, parent's relative forward error {e_fwd:.3e}")
    assert margin >= NET_MARGIN_FACTOR * e_fwd


def _compare(tag, got, parent, want):
    worst = 0.0
    for n, w in want.items():
        e_parent, e = T.max_err(parent[n], w), T.max_err(got[n], w)
        worst = max(worst, e / max(e_parent, 1e-30))
        assert e <= 3 * e_parent, f"{tag} {n}: E_parent {e_parent:.3e} fused {e:.3e}"
    print(f"{tag}: {len(want)} parameter gradients, worst error ratio to the parent {worst:.2f}")


@pytest.mark.parametrize("style", ["pytorch", "caffe"])
def test_resnet50_train_gradients_and_dispatch(style, monkeypatch):
    from bevformer_amd import ops
    net, x, gs = _net(style)
    outs64, gw64 = T.net_grads64(net, x, gs)
    frozen = [n for n, p in net.named_parameters() if not p.requires_grad]
    assert any(n.startswith("layer1.") for n in frozen) and "conv1.weight" in frozen and not any(n in gw64 for n in frozen)
    net, x, gs = net.cuda(), x.cuda(), [g.cuda() for g in gs]
    with ops.using(gemm="split", backbone_train=True):
        with _spy(monkeypatch) as seen:
            _, gw = T.net_grads(net, x, gs)
        assert seen == dict(stem=1, bottleneck=3, bottleneck_train=4 + 6 + 3, conv2d=0), seen
        parent_outs, parent = _parent_net_grads(net, x, gs)
    _assert_margin(f"resnet50 {style}", net, x, parent_outs, outs64)
    assert sorted(gw) == sorted(gw64) and all(g is not None for g in gw.values())
    assert all(p.grad is None for n, p in net.named_parameters() if n in frozen)
    _compare(f"resnet50 {style}", gw, parent, gw64)


def test_resnet50_with_dcn_stages_keeps_them_on_the_module_path(monkeypatch):
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck
    net, x, gs = _net("caffe", dcn=True)
    outs64, gw64 = T.net_grads64(net, x, gs)
    net, x, gs = net.cuda(), x.cuda(), [g.cuda() for g in gs]
    with ops.using(gemm="split", backbone_train=True):
        why = {n: ops.bottleneck_train_reject(m) for n, m in net.named_modules() if isinstance(m, Bottleneck)}
        assert all((r == "a deformable conv2 (no backward yet)") == n.startswith(("layer3.", "layer4.")) for n, r in why.items()), why
        assert not any(r for n, r in why.items() if n.startswith(("layer1.", "layer2.")))
        with _spy(monkeypatch) as seen:
            _, gw = T.net_grads(net, x, gs)
        assert seen["stem"] == 1 and seen["bottleneck"] == 3 and seen["bottleneck_train"] == 4 and seen["conv2d"] > 0, seen
        parent_outs, parent = _parent_net_grads(net, x, gs)
    # (the forward error of the stage that runs on the kernels: stages 3 and 4 are the module path's fp32 code in both arms)
    _assert_margin("resnet50 dcn", net, x, parent_outs[:1], outs64[:1])
    _compare("resnet50 dcn", gw, parent, gw64)


# ---- 4. a captured training step replays the weights of its time

def test_captured_step_follows_in_place_weight_updates():
    from bevformer_amd import ops
    gen = torch.Generator().manual_seed(77)
    blk = Y.randomize_norms_(Y.randomize_convs_(_make_block("stride2_pytorch"), gen), gen).eval().cuda()
    x = torch.randn(2, 64, 6, 10, generator=gen).cuda().requires_grad_()
    g = torch.randn(2, 256, 3, 5, generator=gen).cuda()
    params = [p for p in blk.parameters() if p.requires_grad]

    def step():
        out = blk(x)
        return out, torch.autograd.grad((out * g).sum(), [x] + params)

    with ops.using(gemm="split", backbone_train=True):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()                                              # (warm-up: packs the images outside the capture)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, grads = step()
        graph.replay()
        torch.cuda.synchronize()
        first = [t.clone() for t in (out,) + tuple(grads)]
        with torch.no_grad():
            for p in params:
                p.mul_(1.25).add_(0.01)
        graph.replay()
        torch.cuda.synchronize()
        second = [t.clone() for t in (out,) + tuple(grads)]
        eager_out, eager = step()
        pout, pdx, pgw = T.parent_block_grads(blk, x, g)
    assert not torch.equal(first[0], second[0])                 # the update did reach the replay
    assert torch.equal(second[0], eager_out)                    # forward: bit for bit
    out64, dx64, gw64 = T.block_grads64(blk, x, g)
    names = [n for n, p in blk.named_parameters() if p.requires_grad]
    for what, got, eag, parent, want in zip(["dx"] + names, second[1:], eager, [pdx] + [pgw[n] for n in names], [dx64] + [gw64[n] for n in names]):
        e_parent, e, e_eager = T.max_err(parent, want), T.max_err(got, want), T.max_err(eag, want)
        print(f"captured step {what}: E_parent {e_parent:.3e}  replay {e:.3e}  eager {e_eager:.3e}  bound {3 * e_parent:.3e}")
        assert e <= 3 * e_parent, what


# ---- 5. the switch left off

def test_switch_off_rejects_grad_mode_and_runs_the_module_path(monkeypatch):
    from bevformer_amd import ops
    blk, x, g, _ = _lattice_case("plain")
    assert ops.modes().backbone_train is False
    with ops.using(gemm="split"):
        assert ops.bottleneck_reject(blk, x) == "grad mode is on"
        with ops.using(backbone_fused=True):
            assert ops.bottleneck_reject(blk, x) == "grad mode is on" and ops.bottleneck(blk, x) is None
        with _spy(monkeypatch) as seen, _launch_tags() as tags:
            out, dx, gw = _step(blk, x, g)
        assert seen["bottleneck_train"] == 0 and seen["bottleneck"] == 0 and seen["conv2d"] == 3 and not tags
        assert dx is not None and all(v is not None for v in gw.values())
