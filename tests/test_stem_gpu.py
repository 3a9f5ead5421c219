"""GPU: the backbone's stem in one launch (``ops.stem_rows``, ``ops.stem``, ``modes.stem_fused``; csrc/stem_conv.h) against the
float64 yardstick of tests/stem_yardstick.py.  Bound: error <= 3 x the error of the parent — im2col + ``ops.linear``, BatchNorm /
ReLU / max pooling in torch fp32 — on the same inputs in the same GEMM mode.  On the integer lattice the result must EQUAL the
yardstick.  A workgroup owns 7 x 8 pooled pixels (14 x 16 conv pixels, 28 x 32 input pixels): the shapes are the smallest that are
below one tile, odd, and more than two tiles plus a remainder in both directions."""
import contextlib
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import backbone_yardstick as BY
import stem_yardstick as Y

pytestmark = pytest.mark.gpu

MODES = ["split", "bf16"]
# (B, H, W): one pixel; smaller than the filter; odd conv (19 x 26) and pooled (10 x 13) sizes, two images; Hp = 18 = 2 tiles + 4,
# Wp = 38 = 4 tiles + 6, three images
LATTICE_SHAPES = [(1, 1, 1), (1, 5, 3), (2, 37, 51), (3, 70, 150)]
RANDOM_SHAPES = [(2, 37, 51), (6, 64, 96)]


@contextlib.contextmanager
def _deterministic():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = det


@functools.lru_cache(maxsize=None)
def _case(shape, kind="random", gamma="mixed", beta=None):
    """(x, w, bn, (pooled, un-pooled) float64 truth) on the CPU, made once and shared; nobody writes to it."""
    g = torch.Generator().manual_seed(sum(shape) + 7 * len(kind))
    x, w, bn = Y.lattice_case(shape, g, gamma, beta) if kind == "lattice" else Y.random_case(shape, g)
    want = Y.stem64(x, w, bn)
    if kind == "lattice":
        Y.assert_lattice(want[0]), Y.assert_lattice(want[1])
    return x, w, bn, want


def _rows_map(rows, B, hw):
    return rows.reshape(B, hw[0], hw[1], -1).permute(0, 3, 1, 2)


def _run(x, w, bn, mode, pool, out=None):
    """-> the (B, 64, Ho, Wo) map of ``ops.stem_rows`` on GPU tensors ``x``, ``w`` and the CPU norm tuple ``bn``"""
    from bevformer_amd import ops
    B, _, H, W = x.shape
    with torch.no_grad(), ops.using(gemm=mode):
        y = ops.stem_rows(x, w, Y.bn_module(bn), pool=pool, out=out)
    assert y is not None
    hw = Y.out_hw(H, W)[1 if pool else 0]
    assert tuple(y.shape) == (B * hw[0] * hw[1], 64) and ops.stem_hw(H, W, pool=pool) == hw
    return _rows_map(y, B, hw)


# ---- 1. lattice exactness

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_exact_on_the_lattice(shape, pool, mode):
    """x in {-4..4}, w in {-2..2}, a norm of scale exactly +-1 with integer beta and mean: every product is exact in bf16, every sum
    exact in fp32 — the result EQUALS the yardstick, no element excluded."""
    x, w, bn, want = _case(shape, "lattice")
    if shape[1] > 8:
        assert (want[0] != 0).double().mean().item() > 0.4          # equality is not equality of zeros
    got = _run(x.cuda(), w.cuda(), bn, mode, pool)
    assert torch.equal(got.double().cpu(), want[0 if pool else 1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", [0, 1])
def test_stem_norms_before_it_pools(pool, mode):
    """Every gamma = -1: the maximum of the normed values is the norm of the MINIMUM — pooling first gives other integers."""
    x, w, bn, want = _case((2, 37, 51), "lattice", -1)
    wrong = torch.relu(Y._bn(F.max_pool2d(F.conv2d(x.double(), w.double(), None, stride=2, padding=3), 3, 2, 1),
                             tuple(t.double() for t in bn[:4]) + (bn[4],)))
    assert not torch.equal(wrong, want[0])                          # the case can tell the two orders apart
    got = _run(x.cuda(), w.cuda(), bn, mode, pool)
    assert torch.equal(got.double().cpu(), want[0 if pool else 1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", [0, 1])
def test_stem_of_negative_values_is_exactly_zero(pool, mode):
    """beta = -2000: every value before the ReLU is negative, so every output is exactly 0 — also at the borders, where a window
    has taps outside the conv map: no padding value leaks into the maximum."""
    x, w, bn, want = _case((2, 37, 51), "lattice", "mixed", -2000)
    assert not want[0].any() and not want[1].any()
    got = _run(x.cuda(), w.cuda(), bn, mode, pool)
    assert torch.equal(got, torch.zeros_like(got))


# ---- 2. the error bound on random values

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_within_three_parent_errors(shape, pool, mode):
    from bevformer_amd import ops
    x, w, bn, want = _case(shape)
    xd, wd = x.cuda(), w.cuda()
    got = _run(xd, wd, bn, mode, pool)
    with torch.no_grad(), ops.using(gemm=mode):
        parent = Y.parent_stem(xd, wd, tuple(t.cuda() for t in bn[:4]) + (bn[4],))
    k = 0 if pool else 1
    e_parent, e_fused = Y.max_err(parent[k], want[k]), Y.max_err(got, want[k])
    print(f"{shape} pool {pool} {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert float(want[k].abs().max()) > 0.1 and e_fused <= 3 * e_parent


# ---- 3. a strided input is read in place, and nothing outside the image is read

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", [0, 1])
def test_a_crop_is_read_in_place_and_its_surround_is_never_read(pool, mode):
    from bevformer_amd.ops import backbone as B
    x, w, bn, _ = _case((2, 37, 51))
    big = torch.full((2, 4, 37 + 9, 51 + 12), float("nan"), device="cuda")          # image and channel strides are not dense
    crop = big[:, :3, 3:3 + 37, 5:5 + 51]
    crop.copy_(x)
    assert not crop.is_contiguous() and B._image_strides(crop)[0] is crop           # no copy
    got = _run(crop, w.cuda(), bn, mode, pool)
    dense = _run(crop.contiguous(), w.cuda(), bn, mode, pool)
    assert not torch.isnan(got).any() and torch.equal(got, dense)


# ---- 4. output bounds

@pytest.mark.parametrize("pool", [0, 1])
def test_columns_beyond_64_and_guard_rows_are_never_written(pool):
    x, w, bn, _ = _case((2, 37, 51))
    hw = Y.out_hw(37, 51)[1 if pool else 0]
    M, guard, sentinel = 2 * hw[0] * hw[1], 3, -7.5
    buf = torch.full((M + 2 * guard, 80), sentinel, device="cuda")
    out = buf[guard:guard + M, :64]
    got = _run(x.cuda(), w.cuda(), bn, "split", pool, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got, _run(x.cuda(), w.cuda(), bn, "split", pool))
    keep = torch.full_like(buf, sentinel)
    assert torch.equal(buf[:, 64:], keep[:, 64:]) and torch.equal(buf[:guard], keep[:guard]) and torch.equal(buf[-guard:], keep[-guard:])


# ---- 5. NaN

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", [0, 1])
def test_a_nan_pixel_reaches_the_outputs_the_module_path_gives_it(pool, mode):
    """The module path's statements are evaluated on the CPU: there the NaN reaches exactly the conv pixels whose 7 x 7 window holds
    the pixel (4 columns of the conv map here), the float64 truth's set.  torch's convolution on the GPU is free to pick an
    algorithm that works on tiles of outputs and spreads the NaN over 6 columns (measured on an MI355X: 1152 NaN elements of the
    conv map against 768) — a property of that algorithm, not of the operator —, so on the GPU the module path's set is asserted
    to CONTAIN the kernel's."""
    x, w, bn, _ = _case((2, 37, 51))
    x = x.clone()
    x[1, 2, 20, 33] = float("nan")
    xd, wd = x.cuda(), w.cuda()
    got = _run(xd, wd, bn, mode, pool)

    def module_path(x, w, norm):
        with torch.no_grad():
            c = torch.relu(norm(F.conv2d(x, w, None, stride=2, padding=3)))
            return F.max_pool2d(c, 3, 2, 1) if pool else c

    module = module_path(x, w, Y.bn_module(bn, device="cpu"))
    assert torch.isnan(module).any() and not torch.isnan(module).all()
    assert torch.equal(torch.isnan(module), torch.isnan(Y.stem64(x, w, bn)[0 if pool else 1]))
    print(f"NaN outputs, pool {pool} {mode}: kernel {int(torch.isnan(got).sum())}, module path {int(torch.isnan(module).sum())}")
    assert torch.equal(torch.isnan(got).cpu(), torch.isnan(module))
    on_gpu = torch.isnan(module_path(xd, wd, Y.bn_module(bn)))
    assert bool((on_gpu | ~torch.isnan(got)).all())


# ---- 6. module level

@functools.lru_cache(maxsize=None)
def _net_case():
    """(one-stage ResNet-50 on the GPU in eval mode, input on the GPU, float64 output): made once and shared."""
    from bevformer_amd.modules import ResNet
    g = torch.Generator().manual_seed(41)
    net = BY.randomize_norms_(ResNet(depth=50, num_stages=1, out_indices=(0,)), g)
    with torch.no_grad():                                           # mixed-sign gamma in the stem
        net.bn1.weight.mul_((torch.randint(0, 2, (64,), generator=g) * 2 - 1).float())
    net = net.eval()
    x = torch.randn(2, 3, 45, 77, generator=g)
    want = BY.resnet64(net, x)[0]
    return net.cuda(), x.cuda(), want


def _parent_net(net, x, blockfn):
    y = Y.parent_stem(x, net.conv1.weight, Y.norm_of(net.bn1))[0]
    for blk in net.layer1:
        y = blockfn(blk, y)
    return y


@pytest.mark.parametrize("mode", MODES)
def test_resnet_with_both_switches_within_three_parent_errors_and_no_copy(mode):
    from bevformer_amd import ops
    net, x, want = _net_case()
    with torch.no_grad(), ops.using(gemm=mode, stem_fused=True, backbone_fused=True):
        assert ops.stem_reject(net, x) is None
        s = ops.stem(net, x)
        assert tuple(s.shape) == (2, 64, 12, 20) and ops.rows_of_map(s).data_ptr() == s.data_ptr()      # a view: no copy
        got = net(x)[0]
    with torch.no_grad(), ops.using(gemm=mode, backbone_fused=True):
        parent = _parent_net(net, x, lambda b, y: b(y))             # the parent's stem, then the same fused blocks
        off = net(x)[0]
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"stem + blocks {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert float(want.abs().max()) > 0.1 and e_fused <= 3 * e_parent
    assert not torch.equal(got, off)                                # the switch did choose another path


@pytest.mark.parametrize("mode", MODES)
def test_resnet_with_the_stem_switch_alone_within_three_parent_errors(mode):
    from bevformer_amd import ops
    net, x, want = _net_case()
    with torch.no_grad(), ops.using(gemm=mode, stem_fused=True):
        got = net(x)[0]
    with torch.no_grad(), ops.using(gemm=mode):
        parent = _parent_net(net, x, lambda b, y: b.forward_torch(y))       # the parent's stem, then torch blocks
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"stem alone {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent


def test_switch_off_is_the_module_path_bit_for_bit():
    from bevformer_amd import ops
    net, x, _ = _net_case()
    assert ops.modes().stem_fused is False
    with torch.no_grad(), ops.using(gemm="split"), _deterministic():
        y = net.maxpool(net.relu(net.bn1(net.conv1(x))))
        assert torch.equal(net(x)[0], net.layer1(y))


# ---- 7. capture

def _capture(net, x):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(x)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = net(x)
    return graph, ys


def test_the_backbone_with_the_stem_is_capturable_and_follows_the_image_cache_rule():
    """The captured step is bit-equal to the eager one.  A weight written in place after the capture: an inference graph freezes
    its weight images and ``graph_weights_stale`` names the stem's weight (capture again); under ``graph_repack`` the pack launch of
    a trainable weight is part of the graph, and the next replay computes with the new values."""
    from bevformer_amd import ops
    net0, x, _ = _net_case()
    net = copy.deepcopy(net0)
    assert net.conv1.weight.requires_grad
    ops.release_captured_images()                                   # (the registry is the process's: other tests' graphs are gone)
    try:
        with torch.no_grad(), ops.using(gemm="split", stem_fused=True, backbone_fused=True):
            eager = net(x)[0].clone()
            graph, ys = _capture(net, x)
            ys[0].zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(ys[0], eager) and not ops.graph_weights_stale()
            net.conv1.weight.mul_(0.5)
            assert any(shape == (64, 3, 7, 7) for shape, _ in ops.graph_weights_stale())     # frozen, and said so
            eager_new = net(x)[0].clone()
            assert not torch.equal(eager_new, eager)
            del graph, ys
            ops.release_captured_images()
            with ops.using(graph_repack=True):
                graph, ys = _capture(net, x)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(ys[0], eager_new)
                net.conv1.weight.mul_(2.0)                          # back to the first values, in place
                graph.replay()                                      # the second replay packs the weight it finds
                torch.cuda.synchronize()
                assert torch.equal(ys[0], eager)
            del graph, ys
    finally:
        ops.release_captured_images()


# ---- 8. rejections fall back

def test_rejected_calls_run_the_module_path():
    from bevformer_amd import ops
    net0, x, _ = _net_case()

    def same_as_module(net, x):
        y = net.maxpool(net.relu(net.bn1(net.conv1(x))))
        return torch.equal(net(x)[0], net.layer1(y))

    with _deterministic():
        with torch.no_grad(), ops.using(gemm="native", stem_fused=True):
            assert ops.stem_reject(net0, x) == "GEMM mode native" and ops.stem(net0, x) is None and same_as_module(net0, x)
        with ops.using(gemm="split", stem_fused=True):              # grad mode on
            assert ops.stem_reject(net0, x) == "grad mode is on" and ops.stem(net0, x) is None and same_as_module(net0, x)
        with torch.no_grad(), ops.using(gemm="split", stem_fused=True):
            net = copy.deepcopy(net0)
            net.bn1.train()
            assert ops.stem_reject(net, x) == "the norm is in train() mode (batch statistics)" and ops.stem(net, x) is None
            net.bn1.momentum = 0.0                                  # (two forwards: the running statistics must not move)
            assert same_as_module(net, x)
            net64, x64 = copy.deepcopy(net0).double(), x.double()
            assert ops.stem_reject(net64, x64) == "not CUDA fp32 parameters" and ops.stem(net64, x64) is None
            assert ops.stem_reject(net0, x64) == "not a CUDA fp32 input" and ops.stem(net0, x64) is None
            assert same_as_module(net64, x64)
            assert ops.stem(net0, x) is not None                    # the covered call does run
