"""GPU: ``ops.conv_bn_rows`` (csrc/conv_bn_rows.h) against the float64 yardstick of tests/backbone_yardstick.py.  Bound: error
<= 3 x the error of the parent — the same convolution as im2col + ``ops.linear``, BatchNorm / add / ReLU in torch fp32 — on the
same inputs in the same GEMM mode.  On the integer lattice the result must EQUAL the yardstick, and where another kernel of the
library computes the same problem the bits must agree.  Shapes are the smallest at which the kernel can go wrong."""
import functools

import pytest
import torch

import backbone_yardstick as Y

pytestmark = pytest.mark.gpu

# (n_img, H, W, C_in, C_out, taps, stride, res, relu)
CASES = {
    "single_pixel": (1, 1, 1, 32, 128, 1, 1, False, True),         # one output row
    "odd_sizes": (2, 5, 7, 64, 160, 1, 2, False, False),           # odd sizes at 1 x 1 stride 2, an image boundary inside a tile, a column tail
    "long_row": (1, 3, 130, 32, 128, 1, 1, True, True),            # three tiles and a row tail, residual
    "half_tile": (2, 6, 10, 96, 64, 9, 2, False, True),            # pytorch-style conv2, half a column tile
    "3x3_stride1": (2, 6, 10, 96, 160, 9, 1, True, True),          # the fusion kernel's form
    "downsample": (2, 4, 6, 64, 256, 1, 2, False, False),          # a downsample, two column tiles
    "stage4": (1, 2, 3, 512, 2048, 1, 1, True, True),              # the stage-4 conv3 channel shape
}
IDS = list(CASES)
MODES = ["split", "bf16"]


@functools.lru_cache(maxsize=None)
def _case(name, kind="random"):
    """Inputs of a case (CPU fp32) and the float64 result, made once and shared by every test: (x, w, bn, res, want)."""
    n_img, H, W, C, N, taps, stride, has_res, relu = CASES[name]
    g = torch.Generator().manual_seed(IDS.index(name))
    k = 3 if taps == 9 else 1
    Ho, Wo = Y.out_hw(H, W, stride)
    if kind == "lattice":
        x, w = Y.lattice((n_img, C, H, W), -4, 4, g), Y.lattice((N, C, k, k), -2, 2, g)
        bn = (torch.ones(N), Y.lattice((N,), -4, 4, g), Y.lattice((N,), -4, 4, g), torch.ones(N), 0.0)      # scale exactly 1
        res = Y.lattice((n_img, N, Ho, Wo), -4, 4, g) if has_res else None
    else:
        x, w = torch.randn(n_img, C, H, W, generator=g), torch.randn(N, C, k, k, generator=g) / (taps * C) ** 0.5
        bn = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2, torch.randn(N, generator=g) * 0.2,
              torch.rand(N, generator=g) + 0.5, 1e-5)
        res = torch.randn(n_img, N, Ho, Wo, generator=g) if has_res else None
    want = Y.conv_bn64(x, w, bn, stride, res, relu)
    if kind == "lattice":
        Y.assert_lattice(want)
        if relu:                                        # equality is not equality of zeros
            assert (want != 0).double().mean().item() > 0.4
    return x, w, bn, res, want


def _bn_module(bn, training=False):
    N = bn[0].numel()
    m = torch.nn.BatchNorm2d(N, eps=bn[4]).cuda().train(training)
    with torch.no_grad():
        m.weight.copy_(bn[0]), m.bias.copy_(bn[1]), m.running_mean.copy_(bn[2]), m.running_var.copy_(bn[3])
    return m


def _rows(t):
    """(B, C, H, W) -> contiguous (B H W, C) rows"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _map(rows, n_img, hw):
    return rows.reshape(n_img, hw[0], hw[1], -1).permute(0, 3, 1, 2)


def _run(name, mode, kind="random", x_map=None, out=None):
    """-> (result as a (n_img, C_out, Ho, Wo) map, the case's tensors on the GPU, float64 result)"""
    from bevformer_amd import ops
    n_img, H, W, C, N, taps, stride, has_res, relu = CASES[name]
    x, w, bn, res, want = _case(name, kind)
    dev = torch.device("cuda")
    xd = x.to(dev) if x_map is None else x_map
    wd, resd = w.to(dev), (None if res is None else res.to(dev))
    with torch.no_grad(), ops.using(gemm=mode):
        y = ops.conv_bn_rows(ops.rows_of_map(xd), n_img, (H, W), wd, _bn_module(bn), stride=stride, relu=relu,
                             res=None if resd is None else _rows(resd), out=out)
    assert y is not None
    Ho, Wo = Y.out_hw(H, W, stride)
    assert tuple(y.shape) == (n_img * Ho * Wo, N)
    bnd = tuple(t.to(dev) for t in bn[:4]) + (bn[4],)
    return _map(y, n_img, (Ho, Wo)), (xd, wd, bnd, resd), want


# ---- 1. the operator's error bound

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IDS)
def test_conv_bn_rows_within_three_parent_errors(name, mode):
    from bevformer_amd import ops
    n_img, H, W, C, N, taps, stride, has_res, relu = CASES[name]
    got, (xd, wd, bnd, resd), want = _run(name, mode)
    with torch.no_grad(), ops.using(gemm=mode):
        parent = Y.parent_conv_bn(xd, wd, bnd, stride, resd, relu)
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"{name} {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent


# ---- 2. lattice exactness

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IDS)
def test_conv_bn_rows_exact_on_the_lattice(name, mode):
    """x, res in {-4..4}, w in {-2..2}, a norm of scale exactly 1 with integer mean and beta: every product is exact in bf16, every
    sum exact in fp32 — the result EQUALS the yardstick, no element excluded: a tap leaking across a row end or an image
    boundary, or a stride-2 pixel taken from the wrong row, cannot hide in a tolerance."""
    got, _, want = _run(name, mode, kind="lattice")
    assert torch.equal(got.double().cpu(), want)


# ---- 3. the bits of the kernels that compute the same problem

@pytest.mark.parametrize("mode", MODES)
def test_3x3_stride1_is_conv3x3_bn_bit_for_bit(mode):
    from bevformer_amd import ops
    name = "3x3_stride1"
    n_img, H, W, C, N, taps, stride, has_res, relu = CASES[name]
    got, (xd, wd, bnd, resd), _ = _run(name, mode)
    x, w, bn, res, _ = _case(name)
    with torch.no_grad(), ops.using(gemm=mode):
        other = ops.conv3x3_bn(_rows(xd).view(n_img, H * W, C), (H, W), wd, _bn_module(bn), relu=relu,
                               res=_rows(resd).view(n_img, H * W, N))
    assert other is not None and float(other.abs().max()) > 0.1
    assert torch.equal(got, _map(other.reshape(-1, N), n_img, (H, W)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["single_pixel", "long_row", "stage4"])
def test_1x1_with_the_identity_norm_is_conv_rows_with_a_bias_bit_for_bit(name, mode):
    """gamma 1, var 1, eps 0, mean 0, beta = b: scale is exactly 1 and shift exactly b, so v * 1 + b is conv_rows' v + b."""
    from bevformer_amd import ops
    n_img, H, W, C, N, taps, stride, has_res, relu = CASES[name]
    x, w, bn, res, _ = _case(name)
    b = bn[1]
    ident = _bn_module((torch.ones(N), b, torch.zeros(N), torch.ones(N), 0.0))
    xd, wd = x.cuda(), w.cuda()
    rows = ops.rows_of_map(xd)
    with torch.no_grad(), ops.using(gemm=mode):
        got = ops.conv_bn_rows(rows, n_img, (H, W), wd, ident)
        other = ops.conv_rows(rows, n_img, (H, W), wd, b.cuda())
    assert got is not None and other is not None and float(other.abs().max()) > 0.1
    assert torch.equal(got, other)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["odd_sizes", "downsample"])
def test_1x1_stride2_is_stride1_on_the_subsampled_map_bit_for_bit(name, mode):
    from bevformer_amd import ops
    n_img, H, W, C, N, taps, stride, has_res, relu = CASES[name]
    assert (taps, stride) == (1, 2)
    got, (xd, wd, _, _), _ = _run(name, mode)
    x, w, bn, res, _ = _case(name)
    sub = xd[:, :, ::2, ::2].contiguous()
    Ho, Wo = Y.out_hw(H, W, 2)
    assert tuple(sub.shape[2:]) == (Ho, Wo)
    with torch.no_grad(), ops.using(gemm=mode):
        other = ops.conv_bn_rows(ops.rows_of_map(sub), n_img, (Ho, Wo), wd, _bn_module(bn), stride=1, relu=relu)
    assert other is not None and float(other.abs().max()) > 0.1
    assert torch.equal(got, _map(other, n_img, (Ho, Wo)))


# ---- 4. determinism and the output stride

def test_two_runs_are_bit_equal_and_a_wider_output_stride_is_respected():
    for name in ("odd_sizes", "long_row", "half_tile"):
        n_img, H, W, C, N, taps, stride, has_res, relu = CASES[name]
        a, _, _ = _run(name, "split")
        b, _, _ = _run(name, "split")
        assert torch.equal(a, b)
        M = a.shape[0] * a.shape[2] * a.shape[3]
        buf = torch.full((M, N + 32), -7.5, device="cuda")
        got, _, _ = _run(name, "split", out=buf[:, :N])
        assert torch.equal(got, a)
        assert (buf[:, N:] == -7.5).all()                   # nothing beyond the row's width is touched


# ---- 5. layout

def test_a_channels_last_input_is_read_in_place():
    from bevformer_amd import ops
    for name in ("3x3_stride1", "odd_sizes"):
        x = _case(name)[0].cuda()
        x_cl = x.contiguous(memory_format=torch.channels_last)
        assert ops.rows_of_map(x_cl).data_ptr() == x_cl.data_ptr()
        assert ops.rows_of_map(x).data_ptr() != x.data_ptr()
        a, _, _ = _run(name, "split", x_map=x)
        b, _, _ = _run(name, "split", x_map=x_cl)
        assert torch.equal(a, b)


# ---- 6. declined calls

def test_declined_calls_return_none():
    from bevformer_amd import ops
    x, w, bn, _, _ = _case("downsample")
    rows, wd = _rows(x.cuda()), w.cuda()
    norm = _bn_module(bn)
    with ops.using(gemm="split"):
        assert ops.conv_bn_rows(rows, 2, (4, 6), wd, norm, stride=2) is None                # grad mode on
    with torch.no_grad(), ops.using(gemm="native"):
        assert ops.conv_bn_rows(rows, 2, (4, 6), wd, norm, stride=2) is None
    with torch.no_grad(), ops.using(gemm="split"):
        r48, w48 = torch.randn(48, 48, device="cuda"), torch.randn(64, 48, 1, 1, device="cuda")
        assert ops.conv_bn_rows(r48, 2, (4, 6), w48, torch.nn.BatchNorm2d(64).cuda().eval()) is None      # 48 channels
        w_48 = torch.randn(48, 64, 1, 1, device="cuda")
        assert ops.conv_bn_rows(rows, 2, (4, 6), w_48, torch.nn.BatchNorm2d(48).cuda().eval()) is None
        assert ops.conv_bn_rows(rows, 2, (4, 6), wd, _bn_module(bn, training=True), stride=2) is None     # bn.training
        assert ops.conv_bn_rows(rows, 2, (4, 6), wd, torch.nn.BatchNorm2d(256, affine=False).cuda().eval(), stride=2) is None
        assert ops.conv_bn_rows(rows, 2, (4, 6), wd, torch.nn.BatchNorm2d(256, track_running_stats=False).cuda().eval(), stride=2) is None
        assert ops.conv_bn_rows(rows, 2, (4, 6), wd, norm, stride=3) is None
        assert ops.conv_bn_rows(rows, 2, (4, 6), wd, norm, stride=2) is not None            # the covered call does run
