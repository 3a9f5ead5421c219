"""GPU: training a bottleneck whose ``conv2`` is a DCNv2 pack on channel-last rows (``modes.dcn_train`` with ``modes.backbone_train``:
``ops.bottleneck_train`` over ``ops.deform_conv_rows_backward``) against float64 autograd through the module's own
``forward_torch`` (tests/dcn_train_yardstick.py).  On the lattice — ``backbone_yardstick.lattice_block_``'s sparse integer
parameters, a ``conv_offset`` whose output lands on half-integer offsets and logits in {-inf, 0, 64} — every tensor a kernel
reads is exact in its number format and every gradient EQUALS float64.  On random inputs: error <= 3 x the error of the parent
(im2col / deformable im2col + ``ops.linear``'s autograd path, everything else in torch fp32) in the same GEMM mode.  Then a
ResNet-50 with DCN stages, a captured training step whose weights change between replays, and the switch left off."""
import contextlib
import copy
import functools

import pytest
import torch

import backbone_train_yardstick as T
import backbone_yardstick as Y
import dcn_train_yardstick as DT

pytestmark = pytest.mark.gpu

FROZEN_BN = dict(type="BN", requires_grad=False)
DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)
OLD_REASON = "a deformable conv2 (no backward yet)"


def _downsample(cin, cout, stride):
    ds = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(cout))
    for p in ds[1].parameters():
        p.requires_grad = False
    return ds


def _make_block(name):
    from bevformer_amd.modules import Bottleneck
    kw = dict(norm_cfg=FROZEN_BN, dcn=DCN)
    blk = {
        "plain": lambda: Bottleneck(256, 64, style="caffe", **kw),
        "stride2_pytorch": lambda: Bottleneck(64, 64, stride=2, style="pytorch", downsample=_downsample(64, 256, 2), **kw),
        "stride2_caffe": lambda: Bottleneck(64, 64, stride=2, style="caffe", downsample=_downsample(64, 256, 2), **kw),
        "with_cp": lambda: Bottleneck(256, 64, style="caffe", with_cp=True, **kw),
        "input_without_grad": lambda: Bottleneck(64, 64, stride=2, style="pytorch", downsample=_downsample(64, 256, 2), **kw),
        "frozen_conv_offset": lambda: Bottleneck(256, 64, style="caffe", **kw),
        "frozen_conv2": lambda: Bottleneck(256, 64, style="caffe", **kw),
        "random": lambda: Bottleneck(32, 32, downsample=_downsample(32, 128, 1), **kw),
    }[name]()
    if name == "frozen_conv2":
        blk.conv2.weight.requires_grad = False
    if name == "frozen_conv_offset":
        for p in blk.conv2.conv_offset.parameters():
            p.requires_grad = False
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


# ---- 1. lattice DCN blocks: every gradient equals float64

LATTICE = ["plain", "stride2_pytorch", "stride2_caffe", "with_cp", "input_without_grad", "frozen_conv_offset", "frozen_conv2"]


def _expected_tags(name):
    """The launch list of ``ops.bottleneck_train``'s docstring for a pack, as GEMM-timer tags in launch order."""
    ds = name in ("stride2_pytorch", "stride2_caffe", "input_without_grad")
    inner = ["bottleneck_conv1", "dcn_offsets", "bottleneck_dcn"]
    fwd = inner + (["bottleneck_downsample"] if ds else []) + ["bottleneck_conv3"]
    bwd = (inner if name == "with_cp" else []) + ["bottleneck_mask", "bottleneck_conv3_wgrad", "bottleneck_conv3_dgrad",
                                                   "bottleneck_dcn_dgrad"]
    if name != "frozen_conv2":
        bwd.append("bottleneck_dcn_wgrad")
    if name != "frozen_conv_offset":
        bwd.append("bottleneck_dcn_offset_wgrad")
    bwd += ["bottleneck_dcn_offset_dgrad", "bottleneck_conv1_wgrad"]
    need_x = name != "input_without_grad"
    if need_x:
        bwd.append("bottleneck_conv1_dgrad")
    if ds:
        bwd += ["bottleneck_downsample_wgrad"] + (["bottleneck_downsample_dgrad"] if need_x else [])
    return fwd + bwd


def _multiple_of(t, q, bound):
    """Is every element of ``t`` (float64) a finite multiple of 1 / q whose q-fold is at most ``bound``?"""
    return bool(torch.isfinite(t).all()) and torch.equal(q * t, (q * t).round()) and float((q * t).abs().max()) <= bound


@functools.lru_cache(maxsize=None)
def _lattice_case(name):
    """A DCN block with sparse lattice parameters, a lattice input and an integer output gradient, the seed picked on the CPU so
    that the float64 truth alone meets the conditions.  What a kernel reads as a bf16 operand is exactly a bf16 number (integers
    of magnitude <= 256: conv1's output, the identity, conv3's and conv2's ``gz``); what it reads through the split (16
    significant bits) next to such an operand fits it (conv2's output, multiples of 1/8; ``doffs``, multiples of 1/16; conv1's
    ``gz``, multiples of 1/32); ``raw`` lies on the backward's lattice (half-integer offsets, logits in {-inf, 0, 64}); every
    gradient is a multiple of 1/32 below 2^24 / 32; and nothing is trivial.  The offsets are NOT confined to [-3, 3]: conv1's
    integer outputs reach 20 — a far tap is dead or samples far, and is exact either way."""
    need_x = name != "input_without_grad"
    for seed in range(48):
        blk = Y.lattice_block_(_make_block(name), seed).eval()
        DT.lattice_offsets_(blk.conv2, seed)
        gen = torch.Generator().manual_seed(300 + seed)
        x = Y.lattice((2, blk.conv1.in_channels, 6, 10), -4, 4, gen)
        o1, o2, idt, out = Y.block64_intermediates(blk, x)
        g = Y.lattice(tuple(out.shape), -2, 2, gen)
        gz1, gz2, gz3 = T.block_gz64(blk, x, g)
        out64, dx64, gw64, raw, draw = DT.block_truth64(blk, x, g, need_x)
        offs, logit = raw[:, :18], raw[:, 18:]
        ok = all(_multiple_of(t, 1, Y.BF16_EXACT) for t in (o1, idt, gz2, gz3)) \
            and _multiple_of(o2, 8, 65535.0) and _multiple_of(out, 8, float(1 << 24)) and _multiple_of(gz1, 32, 65535.0) \
            and _multiple_of(draw, 16, 65535.0) and _multiple_of(offs, 2, 64.0) \
            and bool(((logit == float("-inf")) | (logit == 0) | (logit == 64)).all()) \
            and all(_multiple_of(t, 32, float(1 << 24)) for t in gw64.values()) \
            and (dx64 is None or _multiple_of(dx64, 32, float(1 << 24)))
        busy = all((t != 0).double().mean().item() > 0.02 for t in (gz1, gz2, gz3)) \
            and all(t.abs().max().item() > 0 for t in gw64.values()) \
            and (draw[:, :18] != 0).double().mean().item() > 0.02 and (draw[:, 18:] != 0).double().mean().item() > 0.02
        if ok and busy:
            break
    else:
        raise AssertionError("no seed gives a lattice DCN block whose truth is exact and not trivial")
    assert torch.equal(out64, out)
    return blk.cuda(), x.cuda(), g.cuda(), (out64, dx64, gw64)


def test_lattice_cases_exist_on_the_cpu():
    """CPU arithmetic only (float64): the seed search of every variant succeeds."""
    for name in LATTICE:
        _lattice_case(name)


@pytest.mark.parametrize("name", LATTICE)
def test_dcn_block_gradients_equal_float64_on_the_lattice(name):
    from bevformer_amd import ops
    blk, x, g, (out64, dx64, gw64) = _lattice_case(name)
    need_x = name != "input_without_grad"
    with ops.using(gemm="split", backbone_train=True, dcn_train=True), _launch_tags() as tags:
        assert ops.bottleneck_train_reject(blk, x) is None
        out, dx, gw = _step(blk, x, g, need_x)
    assert tags == _expected_tags(name), tags
    assert torch.equal(out.double().cpu(), out64)
    assert (dx is None) == (not need_x) and (not need_x or torch.equal(dx.double().cpu(), dx64))
    assert sorted(gw) == sorted(gw64)
    assert ("conv2.weight" in gw) == (name != "frozen_conv2")
    assert ("conv2.conv_offset.weight" in gw) == ("conv2.conv_offset.bias" in gw) == (name != "frozen_conv_offset")
    for n, want in gw64.items():
        assert gw[n] is not None and torch.equal(gw[n].double().cpu(), want), f"{n}: {T.max_err(gw[n], want):.3e}"
    assert _step.dx_in_rows is (True if need_x else None)               # the gradient stays in rows between covered blocks


# ---- 2. a random DCN block in split mode: within three parent errors, no ReLU near its kink, no sample near a cell boundary

NET_MARGIN_FACTOR = 100


def _pre_activations64(blk, x):
    b = copy.deepcopy(blk).double().cpu()
    x = x.detach().double().cpu()
    with torch.no_grad():
        p1 = b.bn1(b.conv1(x))
        o1 = torch.relu(p1)
        raw = b.conv2.conv_offset(o1)
        p2 = b.bn2(b.conv2.forward_torch(o1))
        idt = x if b.downsample is None else b.downsample(x)
        p3 = b.bn3(b.conv3(torch.relu(p2))) + idt
    return (p1, p2, p3), o1, raw


def _random_block(seed):
    gen = torch.Generator().manual_seed(seed)
    blk = Y.randomize_norms_(Y.randomize_convs_(_make_block("random"), gen), gen).eval()
    x = torch.randn(1, 32, 4, 4, generator=gen)
    g = torch.randn(1, 128, 4, 4, generator=gen)
    return blk, x, g


def _margins64(blk, x):
    pre, o1, raw = _pre_activations64(blk, x)
    return min(p.abs().min().item() for p in pre), DT.position_margin64(tuple(o1.shape), raw, blk.conv2.stride[0])


# seed 312: of the seeds 0 .. 39999 the one with the largest min(ReLU margin, position margin) in float64 on the CPU: the closest
# pre-activation to zero is 2.935e-3, the closest sample coordinate to an integer or a border 7.102e-3.  Measured on the GPU when
# this was written: the parent's forward error 2.538e-5 (100 x = 2.538e-3) and its error in raw 1.030e-5 (100 x = 1.030e-3)
RANDOM_SEED, RANDOM_RELU_MARGIN, RANDOM_POSITION_MARGIN = 312, 2.9e-3, 7.1e-3


@functools.lru_cache(maxsize=None)
def _random_case():
    return (RANDOM_SEED,) + _random_block(RANDOM_SEED)


def test_the_recorded_seed_keeps_relus_and_positions_off_their_kinks():
    """CPU arithmetic only (float64): the conditions the seed was chosen for."""
    seed, blk, x, g = _random_case()
    relu_margin, pos_margin = _margins64(blk, x)
    print(f"seed {seed}: closest pre-activation to zero {relu_margin:.3e}, closest sample coordinate to a cell boundary {pos_margin:.3e}")
    assert relu_margin >= RANDOM_RELU_MARGIN and pos_margin >= RANDOM_POSITION_MARGIN


def test_random_dcn_block_within_three_parent_errors():
    from bevformer_amd import ops
    seed, blk, x, g = _random_case()
    out64, dx64, gw64, raw64, _ = DT.block_truth64(blk, x, g)
    relu_margin, pos_margin = _margins64(blk, x)
    blk, x, g = copy.deepcopy(blk).cuda(), x.cuda(), g.cuda()
    with ops.using(gemm="split", backbone_train=True, dcn_train=True):
        pout, pdx, pgw, praw = DT.parent_dcn_block_grads(blk, x, g)
        e_out, e_raw = T.max_err(pout, out64), T.max_err(praw, raw64)
        print(f"seed {seed}: parent forward error {e_out:.3e} (ReLU margin {relu_margin:.3e}), parent raw error {e_raw:.3e} "
              f"(position margin {pos_margin:.3e})")
        assert relu_margin >= NET_MARGIN_FACTOR * e_out             # no mask can flip between the precisions
        assert pos_margin >= NET_MARGIN_FACTOR * e_raw              # no sample can change its cell or go dead
        assert ops.bottleneck_train_reject(blk, x) is None
        out, dx, gw = _step(blk, x, g)
    pairs = [("dx", dx, pdx, dx64)] + [(n, gw[n], pgw[n], gw64[n]) for n in gw64]
    assert any("conv_offset" in n for n in gw64)
    for what, got, parent, want in pairs:
        e_parent, e = T.max_err(parent, want), T.max_err(got, want)
        print(f"random DCN block {what}: E_parent {e_parent:.3e}  fused {e:.3e}  bound {3 * e_parent:.3e}")
        assert float(want.abs().max()) > 1e-3 and e <= 3 * e_parent, what


# ---- 3. a ResNet-50 with DCN stages under train(), both switches on

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
    """The backbone with the parent's operators: the frozen stem and stage on torch without gradients, a trainable block with a
    plain conv2 as ``parent_block_diff``, a DCN block as ``parent_dcn_block_diff``."""
    def block(b, y):
        if not any(p.requires_grad for p in b.parameters()):
            with torch.no_grad():
                return b.forward_torch(y)
        return DT.parent_dcn_block_diff(b, y)[0] if hasattr(b.conv2, "conv_offset") else T.parent_block_diff(b, y)
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


def test_resnet50_with_dcn_stages_runs_every_trainable_block_on_the_kernels(monkeypatch):
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck
    net, x, gs = _net("caffe", dcn=True)
    outs64, gw64 = T.net_grads64(net, x, gs)
    assert any("conv_offset.weight" in n for n in gw64)
    net, x, gs = net.cuda(), x.cuda(), [g.cuda() for g in gs]
    with ops.using(gemm="split", backbone_train=True, dcn_train=True):
        why = {n: ops.bottleneck_train_reject(m) for n, m in net.named_modules() if isinstance(m, Bottleneck)}
        assert not any(why.values()), why
        with _spy(monkeypatch) as seen:
            _, gw = T.net_grads(net, x, gs)
        assert seen == dict(stem=1, bottleneck=3, bottleneck_train=4 + 6 + 3, conv2d=0), seen
        parent_outs, parent = _parent_net_grads(net, x, gs)
    margin = T.relu_margin64(net, x)
    e_fwd = max(T.max_err(p, w) / float(w.abs().max()) for p, w in zip(parent_outs, outs64))
    print(f"resnet50 dcn: closest ReLU input {margin:.3e} of its tensor's maximum, parent's relative forward error {e_fwd:.3e}")
    assert margin >= NET_MARGIN_FACTOR * e_fwd
    assert sorted(gw) == sorted(gw64) and all(v is not None for v in gw.values())
    worst = 0.0
    for n, w in gw64.items():
        e_parent, e = T.max_err(parent[n], w), T.max_err(gw[n], w)
        worst = max(worst, e / max(e_parent, 1e-30))
        assert e <= 3 * e_parent, f"resnet50 dcn {n}: E_parent {e_parent:.3e} fused {e:.3e}"
    print(f"resnet50 dcn: {len(gw64)} parameter gradients, worst error ratio to the parent {worst:.2f}")


# ---- 4. a captured training step replays the weights of its time, conv_offset's included

def test_captured_dcn_step_follows_in_place_weight_updates():
    from bevformer_amd import ops
    seed, blk, x, g = _random_case()
    blk, x, g = copy.deepcopy(blk).cuda(), x.cuda().requires_grad_(), g.cuda()
    params = [p for p in blk.parameters() if p.requires_grad]
    names = [n for n, p in blk.named_parameters() if p.requires_grad]
    assert "conv2.conv_offset.weight" in names and "conv2.conv_offset.bias" in names

    def step():
        out = blk(x)
        return out, torch.autograd.grad((out * g).sum(), [x] + params)

    with ops.using(gemm="split", backbone_train=True, dcn_train=True):
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
        # (a small update: the recorded seed's margins must survive it — float64 on the CPU gives 3.02e-3 / 7.00e-3 after it, against
        # 2.12e-3 / 5.53e-3 after a factor of 1 + 2^-10, which is below 100 parent errors; both are asserted again below)
        with torch.no_grad():
            for p in params:
                p.mul_(1.0 + 2.0 ** -14)
        graph.replay()
        torch.cuda.synchronize()
        second = [t.clone() for t in (out,) + tuple(grads)]
        eager_out, eager = step()
        pout, pdx, pgw, praw = DT.parent_dcn_block_grads(blk, x.detach(), g)
    assert not torch.equal(first[0], second[0])                 # the update did reach the replay
    assert not torch.equal(first[1 + 1 + names.index("conv2.conv_offset.weight")],
                           second[1 + 1 + names.index("conv2.conv_offset.weight")])
    assert torch.equal(second[0], eager_out)                    # forward: bit for bit
    out64, dx64, gw64, raw64, _ = DT.block_truth64(blk, x.detach(), g)
    relu_margin, pos_margin = _margins64(blk, x.detach())
    print(f"after the update: ReLU margin {relu_margin:.3e} (parent forward error {T.max_err(pout, out64):.3e}), position margin "
          f"{pos_margin:.3e} (parent raw error {T.max_err(praw, raw64):.3e})")
    assert relu_margin >= NET_MARGIN_FACTOR * T.max_err(pout, out64) and pos_margin >= NET_MARGIN_FACTOR * T.max_err(praw, raw64)
    for what, got, eag, parent, want in zip(["dx"] + names, second[1:], eager, [pdx] + [pgw[n] for n in names],
                                            [dx64] + [gw64[n] for n in names]):
        e_parent, e, e_eager = T.max_err(parent, want), T.max_err(got, want), T.max_err(eag, want)
        print(f"captured DCN step {what}: E_parent {e_parent:.3e}  replay {e:.3e}  eager {e_eager:.3e}  bound {3 * e_parent:.3e}")
        assert e <= 3 * e_parent, what


# ---- 5. dcn_train left off

def test_dcn_train_off_keeps_a_dcn_block_on_the_module_path(monkeypatch):
    from bevformer_amd import ops
    blk, x, g, _ = _lattice_case("plain")
    assert ops.modes().dcn_train is False
    with ops.using(gemm="split", backbone_train=True):
        assert ops.bottleneck_train_reject(blk, x) == OLD_REASON
        with _spy(monkeypatch) as seen, _launch_tags() as tags:
            out, dx, gw = _step(blk, x, g)
        assert seen["bottleneck_train"] == 0 and seen["bottleneck"] == 0 and seen["conv2d"] == 3 and not tags, (seen, tags)
        assert dx is not None and all(v is not None for v in gw.values())
