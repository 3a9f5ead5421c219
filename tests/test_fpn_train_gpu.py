"""GPU: training the image neck on channel-last rows (``ops.fpn_train``, ``modes.fpn_train``) against float64 autograd through the
module's own ``forward_torch`` (tests/fpn_train_yardstick.py).  On the sparse integer lattice of ``fpn_yardstick.lattice_neck_`` with
lattice inputs and integer output gradients every tensor a kernel reads is an integer of magnitude <= 256 and every gradient an
integer below 2^24: outputs and gradients EQUAL float64 in ``split`` and in ``bf16``.  On a random neck in ``split``: error <= 3 x
the error of the parent (im2col + ``ops.linear``'s autograd path, bias / add / upsampling / ReLU in torch fp32) on the same inputs.
Then the seams: the forward against ``ops.fpn``, a bottleneck in front of the neck, a captured training step whose weights change
between replays, and the switch left off."""
import contextlib
import copy
import functools

import pytest
import torch

import backbone_yardstick as BY
import fpn_train_yardstick as T
import fpn_yardstick as Y

pytestmark = pytest.mark.gpu

MODES = ["split", "bf16"]
N_IMG = 2
# name: (in_channels, out_channels, num_outs, finest size, inputs need a gradient, frozen lateral)
NECKS = {
    "relu5": ((32, 64, 64), 32, 5, (8, 12), True, None),           # extras of 1 x 2 and 1 x 1; the second reads a ReLU
    "single": ((64,), 64, 1, (4, 6), True, None),
    "base_like": ((32, 64, 96), 64, 4, (8, 12), True, None),       # three levels and one extra, as the base config
    "input_without_grad": ((32, 64, 64), 32, 5, (8, 12), False, None),
    "frozen_lateral": ((32, 64, 64), 32, 5, (8, 12), True, 1),
}
# kernel launches (tags of the GEMM timer): one per convolution forward; backward a weight gradient and an input gradient per
# convolution, less the laterals' input gradients nobody asked for and the weight gradient of a frozen convolution
N_FORWARD = {"relu5": 8, "single": 2, "base_like": 7, "input_without_grad": 8, "frozen_lateral": 8}
N_BACKWARD = {"relu5": 16, "single": 4, "base_like": 14, "input_without_grad": 16 - 3, "frozen_lateral": 16 - 1}


def _build(name):
    from bevformer_amd.modules.neck import FPN
    cin, cout, num_outs, _, _, frozen = NECKS[name]
    neck = FPN(list(cin), cout, num_outs=num_outs, add_extra_convs="on_output", relu_before_extra_convs=True)
    if frozen is not None:
        for p in neck.lateral_convs[frozen].conv.parameters():
            p.requires_grad = False
    return neck


@contextlib.contextmanager
def _launch_tags():
    from bevformer_amd import ops
    tags = []
    ops.set_gemm_timer(lambda tag, flops, nbytes: (tags.append(tag), contextlib.nullcontext())[1])
    try:
        yield tags
    finally:
        ops.set_gemm_timer(None)


def _step(neck, xs, gs, need_x=True):
    """(outs, [dx], {name: gradient}, [was the gradient handed to input i a row view?]) of ``sum_i sum(gs[i] * neck(xs)[i])``
    through the module's ``forward`` in the modes in force."""
    from bevformer_amd import ops
    xs = [x.detach().clone().requires_grad_(need_x) for x in xs]
    for p in neck.parameters():
        p.grad = None
    in_rows = [None] * len(xs)
    if need_x:      # (the leaf's accumulation re-lays the gradient out as the leaf: look at what the neck's node handed over)
        for i, x in enumerate(xs):
            x.register_hook(lambda gx, i=i: in_rows.__setitem__(i, ops.rows_of_map(gx).data_ptr() == gx.data_ptr()))
    outs = neck(xs)
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    return [o.detach() for o in outs], [x.grad for x in xs], {n: p.grad for n, p in neck.named_parameters() if p.requires_grad}, in_rows


# ---- 1. lattice necks: outputs and every gradient equal float64

@functools.lru_cache(maxsize=None)
def _lattice_case(name):
    """A neck with sparse lattice parameters, lattice inputs in {-4..4} and output gradients in {-2..2}, the seed picked on the CPU so
    that the float64 truth alone meets the conditions: every tensor a kernel reads — the levels, the laterals' gradients and the
    levels' summed gradients — an integer of magnitude <= 256 (exactly a bf16 number), every parameter and input gradient an integer
    below 2^24, and no parameter gradient all zero."""
    cin, cout, num_outs, (H, W), need_x, _ = NECKS[name]
    exact = lambda t, bound: torch.equal(t, t.round()) and t.abs().max().item() <= bound
    for seed in range(32):
        neck = Y.lattice_neck_(_build(name), seed)
        gen = torch.Generator().manual_seed(300 + seed)
        xs = [Y.lattice((N_IMG, c, H >> i, W >> i), -4, 4, gen) for i, c in enumerate(cin)]
        outs64 = Y.fpn64(neck.state_dict(), Y.spec_of(neck), xs)
        gs = [Y.lattice(tuple(o.shape), -2, 2, gen) for o in outs64]
        levels, glat, glev = T.neck_reads64(neck, xs, gs)
        truth = T.neck_grads64(neck, xs, gs, need_x)
        grads = list(truth[2].values()) + [d for d in truth[1] if d is not None]
        ok = all(exact(t, Y.BF16_EXACT) for t in levels + glat + glev) and all(exact(t, float(1 << 24)) for t in grads)
        if ok and all(t.abs().max().item() > 0 for t in truth[2].values()):
            break
    else:
        raise AssertionError("no seed gives a lattice neck whose truth is exact and not trivial")
    for t in levels + glat + glev:
        Y.assert_lattice(t, Y.BF16_EXACT)
    for t in grads:
        Y.assert_lattice(t)
    assert all(torch.equal(a, b) for a, b in zip(truth[0], outs64))
    return neck.cuda(), [x.cuda() for x in xs], [g.cuda() for g in gs], truth


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(NECKS))
def test_neck_gradients_equal_float64_on_the_lattice(name, mode):
    from bevformer_amd import ops
    neck, xs, gs, (outs64, dxs64, gw64) = _lattice_case(name)
    need_x, frozen = NECKS[name][4], NECKS[name][5]
    with ops.using(gemm=mode, fpn_train=True), _launch_tags() as tags:
        assert ops.fpn_train_reject(neck, xs) is None
        outs, dxs, gw, in_rows = _step(neck, xs, gs, need_x)
    fwd, bwd = tags[:N_FORWARD[name]], tags[N_FORWARD[name]:]
    assert len(tags) == N_FORWARD[name] + N_BACKWARD[name], tags
    assert all(t in ("fpn_lateral", "fpn_out", "fpn_extra") for t in fwd) and all(t.endswith(("_wgrad", "_dgrad")) for t in bwd), tags
    assert bwd.count("fpn_lateral_dgrad") == (len(xs) if need_x else 0)        # no input gradient nobody asked for
    assert bwd.count("fpn_lateral_wgrad") == len(xs) - (frozen is not None)     # no weight gradient of a frozen convolution
    n_extra = NECKS[name][2] - len(xs)
    assert bwd.count("fpn_out_wgrad") == bwd.count("fpn_out_dgrad") == len(xs)
    assert bwd.count("fpn_extra_wgrad") == bwd.count("fpn_extra_dgrad") == n_extra
    assert len(outs) == len(outs64) and all(torch.equal(o.double().cpu(), w) for o, w in zip(outs, outs64))
    for i, (d, want) in enumerate(zip(dxs, dxs64)):
        assert (d is None) == (not need_x)
        if need_x:
            assert torch.equal(d.double().cpu(), want), f"dx{i}"
            assert in_rows[i] is True                                           # the gradient leaves the neck in rows
    assert sorted(gw) == sorted(gw64) and len(gw) == 2 * (NECKS[name][2] + len(xs) - (frozen is not None))
    assert frozen is None or f"lateral_convs.{frozen}.conv.weight" not in gw
    for n, want in gw64.items():
        assert torch.equal(gw[n].double().cpu(), want), n


# ---- 2. a random neck in split mode: within three parent errors, the one ReLU input off its kink

# seed and margin: test_the_recorded_seed_keeps_the_relu_off_its_kink (CPU, float64) asserts them; the seed is the one of 0 .. 1999
# whose first extra level (128 values, the only tensor a ReLU of this neck reads) stays farthest from zero: 3.555e-2 (the expected
# closest of 128 unit-scale values is about 1e-2).  The GPU test asserts that this is at least 100 parent forward errors
RANDOM_SEED, RANDOM_MARGIN = 400, 3.5e-2


@functools.lru_cache(maxsize=None)
def _random_case():
    neck = Y.randomize_neck_(_build("relu5"), seed=RANDOM_SEED)
    gen = torch.Generator().manual_seed(RANDOM_SEED + 1)
    cin, _, _, (H, W), _, _ = NECKS["relu5"]
    xs = [torch.randn(N_IMG, c, H >> i, W >> i, generator=gen) for i, c in enumerate(cin)]
    shapes = [tuple(o.shape) for o in Y.fpn64(neck.state_dict(), Y.spec_of(neck), xs)]
    gs = [torch.randn(s, generator=gen) for s in shapes]
    return neck, xs, gs


def test_the_recorded_seed_keeps_the_relu_off_its_kink():
    """CPU arithmetic only (float64): the condition the seed was chosen for."""
    neck, xs, gs = _random_case()
    closest = T.first_extra_pre_relu64(neck, xs).abs().min().item()
    print(f"closest pre-ReLU value of the first extra level: {closest:.3e}")
    assert closest >= RANDOM_MARGIN


def test_random_neck_within_three_parent_errors():
    from bevformer_amd import ops
    neck, xs, gs = _random_case()
    outs64, dxs64, gw64 = T.neck_grads64(neck, xs, gs)
    closest = T.first_extra_pre_relu64(neck, xs).abs().min().item()
    assert closest >= RANDOM_MARGIN
    neck, xs, gs = copy.deepcopy(neck).cuda(), [x.cuda() for x in xs], [g.cuda() for g in gs]
    with ops.using(gemm="split", fpn_train=True):
        pouts, pdxs, pgw = T.parent_neck_grads(neck, xs, gs)
        forward_error = max(T.max_err(p, w) for p, w in zip(pouts, outs64))
        print(f"seed {RANDOM_SEED}: parent forward error {forward_error:.3e}, margin {RANDOM_MARGIN:.3e}, closest {closest:.3e}")
        assert RANDOM_MARGIN >= 100 * forward_error                             # the mask cannot flip between the precisions
        outs, dxs, gw, _ = _step(neck, xs, gs)
    pairs = [(f"dx{i}", dxs[i], pdxs[i], dxs64[i]) for i in range(len(xs))] + [(n, gw[n], pgw[n], gw64[n]) for n in gw64]
    for what, got, parent, want in pairs:
        e_parent, e = T.max_err(parent, want), T.max_err(got, want)
        print(f"random neck {what}: E_parent {e_parent:.3e}  fused {e:.3e}  bound {3 * e_parent:.3e}")
        assert float(want.abs().max()) > 1e-3 and e <= 3 * e_parent, what


# ---- 3. the forward is ops.fpn's

@pytest.mark.parametrize("mode", MODES)
def test_forward_is_bit_equal_to_the_inference_path(mode):
    from bevformer_amd import ops
    neck, xs, gs = _random_case()
    neck, xs = copy.deepcopy(neck).cuda(), [x.cuda() for x in xs]
    with ops.using(gemm=mode, fpn_train=True):
        with torch.no_grad():
            want = ops.fpn(neck, xs)
        got = neck(xs)
    assert want is not None and len(got) == len(want) == 5
    assert all(o.grad_fn is not None and "_FpnTrain" in type(o.grad_fn).__name__ for o in got)
    assert all(torch.equal(g, w) and g.stride() == w.stride() for g, w in zip(got, want))


# ---- 4. a bottleneck in front of the neck: the gradient reaches it in rows

def test_a_bottleneck_receives_the_necks_gradient_in_rows():
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck
    from bevformer_amd.modules.neck import FPN
    gen = torch.Generator().manual_seed(5)
    blk = Bottleneck(256, 64, style="caffe", norm_cfg=dict(type="BN", requires_grad=False))     # a stage-4-like block at tiny size
    blk = BY.randomize_norms_(BY.randomize_convs_(blk, gen), gen).eval().cuda()
    neck = Y.randomize_neck_(FPN([256], 64, num_outs=1), seed=6).cuda()
    x = torch.randn(N_IMG, 256, 4, 6, generator=gen).cuda()
    g = torch.randn(N_IMG, 64, 4, 6, generator=gen).cuda()
    seen = {}
    with ops.using(gemm="split", backbone_train=True, fpn_train=True), _launch_tags() as tags:
        feat = blk(x)
        assert "_BottleneckTrain" in type(feat.grad_fn).__name__
        feat.register_hook(lambda gf: seen.update(rows=ops.rows_of_map(gf).data_ptr() == gf.data_ptr()))
        out, = neck([feat])
        (out * g).sum().backward()
    assert seen == dict(rows=True)
    assert "fpn_lateral_dgrad" in tags and "bottleneck_conv3_wgrad" in tags
    # the same step on the module path, in float64: the block's first weight sees the neck's gradient
    b64, n64 = copy.deepcopy(blk).double().cpu(), copy.deepcopy(neck).double().cpu()
    o64, = n64.forward_torch([b64.forward_torch(x.double().cpu())])
    want, = torch.autograd.grad((o64 * g.double().cpu()).sum(), [b64.conv1.weight])
    assert T.max_err(blk.conv1.weight.grad, want) <= 1e-3 * want.abs().max().item()             # (split: about 1e-5 relative)


# ---- 5. a captured training step replays the weights of its time

def test_captured_step_follows_in_place_weight_updates():
    from bevformer_amd import ops
    neck, xs, gs = _random_case()
    neck = copy.deepcopy(neck).cuda()
    xs, gs = [x.cuda().requires_grad_() for x in xs], [g.cuda() for g in gs]
    params = list(neck.parameters())

    def step():
        outs = neck(xs)
        return outs, torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, gs)), xs + params)

    with ops.using(gemm="split", fpn_train=True):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()                                              # (warm-up: packs the images outside the capture)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs, grads = step()
        graph.replay()
        torch.cuda.synchronize()
        first = [t.clone() for t in tuple(outs) + tuple(grads)]
        with torch.no_grad():
            for p in params:
                p.mul_(1.25).add_(0.01)
        graph.replay()
        torch.cuda.synchronize()
        second = [t.clone() for t in tuple(outs) + tuple(grads)]
        eager_outs, eager = step()
    n = len(eager_outs)
    assert not torch.equal(first[0], second[0])                 # the update did reach the replay
    for got, want in zip(second[:n], eager_outs):
        assert torch.equal(got, want)                           # forward: bit for bit
    # the gradients follow the new weights: what the replay gives is what an eager step on the updated weights gives, up to the
    # order of the atomics (a few fp32 roundings), and is far from the gradients of the old weights
    for i, (got, want, old) in enumerate(zip(second[n:], eager, first[n:])):
        scale = want.abs().max().item()
        assert T.max_err(got, want.double().cpu()) <= 1e-5 * scale, i
        if i < len(xs):                                         # (input gradients are linear in the weights: they all moved)
            assert T.max_err(got, old.double().cpu()) > 1e-2 * scale, i


# ---- 6. the switch left off

def test_switch_off_runs_the_module_path(monkeypatch):
    from bevformer_amd import ops
    neck, xs, gs, _ = _lattice_case("relu5")
    assert ops.modes().fpn_train is False
    calls = []
    real = type(neck).forward_torch
    monkeypatch.setattr(type(neck), "forward_torch", lambda self, inputs: (calls.append(1), real(self, inputs))[1])
    fast = []
    real_train = ops.fpn_train
    monkeypatch.setattr(ops, "fpn_train", lambda *a, **k: (fast.append(1), real_train(*a, **k))[1])
    with ops.using(gemm="split"):
        assert ops.fpn_reject(neck, xs) == "grad mode is on" and ops.fpn_train_reject(neck, xs) is None
        for fused in (False, True):
            with ops.using(fpn_fused=fused), _launch_tags() as tags:
                outs, dxs, gw, in_rows = _step(neck, xs, gs)
            assert not tags and not fast and all(d is not None for d in dxs) and all(v is not None for v in gw.values())
        assert calls == [1, 1]
        with ops.using(fpn_train=True), _launch_tags() as tags:
            _step(neck, xs, gs)
        assert fast == [1] and calls == [1, 1] and len(tags) == N_FORWARD["relu5"] + N_BACKWARD["relu5"]
