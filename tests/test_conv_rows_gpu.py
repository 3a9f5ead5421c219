"""GPU: ``ops.conv_rows`` (csrc/conv_rows.h) against the float64 yardstick of tests/fpn_yardstick.py.  Bound: error <= 3 x the
error of the parent — the same convolution as an im2col matrix (``F.unfold``) through ``ops.linear``, bias in that GEMM,
residual in torch fp32 — on the same inputs in the same GEMM mode: the arithmetic is the projections', not IEEE fp32.  On the
integer lattice the result must EQUAL the yardstick.  Shapes are the smallest at which the kernel can go wrong."""
import functools

import pytest
import torch

import fpn_yardstick as Y

pytestmark = pytest.mark.gpu

# (n_img, H, W, C_in, C_out, kernel, stride, bias, residual: None / "same" / "up", relu_in)
CASES = {
    "1x1px_3x3": (1, 1, 1, 32, 128, 3, 1, False, None, False),           # only the centre tap is live
    "6x10_3x3_96to160": (2, 6, 10, 96, 160, 3, 1, False, None, False),    # image boundary inside a tile, 27 K chunks, N tail
    "6x10_3x3_same_res": (2, 6, 10, 96, 160, 3, 1, True, "same", False),  # ... with bias and a same-shape residual
    "5x7_3x3_s2": (2, 5, 7, 64, 128, 3, 2, False, None, False),           # odd sizes -> 3 x 4, taps off the right / bottom edge
    "3x130_3x3_s2": (1, 3, 130, 32, 128, 3, 2, False, None, False),       # a row longer than a tile
    "12x20_1x1_2048_bias": (2, 12, 20, 2048, 256, 1, 1, True, None, False),   # deepest K; M = 480: a tail tile
    "12x20_1x1_up_res": (2, 12, 20, 64, 160, 1, 1, True, "up", False),    # the gather crosses the image boundary inside a tile
    "6x10_3x3_s2_relu_bias": (2, 6, 10, 64, 128, 3, 2, True, None, True),     # input ReLU
    "6x10_3x3_s2_relu": (2, 6, 10, 64, 128, 3, 2, False, None, True),
}
IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def _case(name, lattice=False):
    """Inputs of a case (CPU fp32 maps) and the float64 result, made once and shared by every test."""
    n_img, H, W, C, N, k, stride, bias, res, relu_in = CASES[name]
    g = torch.Generator().manual_seed(IDS.index(name))
    if lattice:
        x, w = Y.lattice((n_img, C, H, W), -4, 4, g), Y.lattice((N, C, k, k), -2, 2, g)
    else:
        x, w = torch.randn(n_img, C, H, W, generator=g), torch.randn(N, C, k, k, generator=g) / (k * k * C) ** 0.5
    b = None if not bias else (Y.lattice((N,), -4, 4, g) if lattice else torch.randn(N, generator=g) * 0.2)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = None
    if res is not None:
        rs = (n_img, N, Ho // 2, Wo // 2) if res == "up" else (n_img, N, Ho, Wo)
        r = Y.lattice(rs, -4, 4, g) if lattice else torch.randn(*rs, generator=g)
    want = Y.conv64(x, w, b, stride, relu_in, r, res == "up")
    if lattice:
        Y.assert_lattice(want)                                            # integers below 2^24: exact in bf16 x bf16 -> fp32
        Y.assert_lattice(Y.conv64(x.abs(), w.abs(), None if b is None else b.abs(), stride, False,
                                  None if r is None else r.abs(), res == "up"))      # ... and so is every partial sum
    return x, w, b, r, want


def _run(name, mode, lattice=False, x_map=None, out=None):
    """-> (result as a (n_img, C_out, Ho, Wo) map, the case's tensors on the GPU, float64 result)"""
    from bevformer_amd import ops
    n_img, H, W, C, N, k, stride, bias, res, relu_in = CASES[name]
    x, w, b, r, want = _case(name, lattice)
    dev = torch.device("cuda")
    xd = x.to(dev) if x_map is None else x_map
    wd, bd, rd = w.to(dev), (None if b is None else b.to(dev)), (None if r is None else r.to(dev))
    with torch.no_grad(), ops.using(gemm=mode):
        y = ops.conv_rows(ops.rows_of_map(xd), n_img, (H, W), wd, bd, stride=stride, relu_in=relu_in,
                          res=None if rd is None else ops.rows_of_map(rd), res_up=res == "up", out=out)
    assert y is not None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert tuple(y.shape) == (n_img * Ho * Wo, N)
    return y.reshape(n_img, Ho, Wo, N).permute(0, 3, 1, 2), (xd, wd, bd, rd), want


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("name", IDS)
def test_conv_rows_within_three_parent_errors(name, mode):
    from bevformer_amd import ops
    n_img, H, W, C, N, k, stride, bias, res, relu_in = CASES[name]
    got, (xd, wd, bd, rd), want = _run(name, mode)
    with torch.no_grad(), ops.using(gemm=mode):
        parent = Y.parent_conv(xd, wd, bd, stride, relu_in, rd, res == "up")
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"{name} {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("name", IDS)
def test_conv_rows_exact_on_the_integer_lattice(name, mode):
    """Inputs, bias and residual in {-4..4}, weights in {-2..2}: every product and sum is exact in both modes
    (|sum| <= 9 * 2048 * 8 < 2^24), so the result EQUALS the yardstick, no element excluded — a tap leaking across a row end,
    an image boundary or a stride cannot hide in a tolerance."""
    got, _, want = _run(name, mode, lattice=True)
    assert torch.equal(got.double().cpu(), want)


def test_conv_rows_two_runs_are_bit_equal():
    for name in ("12x20_1x1_up_res", "5x7_3x3_s2"):
        a, _, _ = _run(name, "split")
        b, _, _ = _run(name, "split")
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_conv_rows_relu_in_keeps_nan(mode):
    """max(x, 0) as torch.relu: a NaN input stays NaN, so exactly the outputs whose taps read it are NaN."""
    name = "6x10_3x3_s2_relu_bias"
    x, w, b, r, _ = _case(name)
    x = x.clone()
    x[1, 5, 3, 4] = float("nan")
    x[0, 0, 0, 0] = float("nan")
    want = Y.conv64(x, w, b, 2, True)
    got, _, _ = _run(name, mode, x_map=x.cuda())
    nan = torch.isnan(want)
    assert nan.any() and not nan.all()
    assert torch.equal(torch.isnan(got).cpu(), nan)
    # NaN poisons every output channel of the pixels that read it and nothing else: (1, :, 1..2, 1..2) reads input (3, 4)
    assert nan[1, :, 1:3, 2].all() and nan[0, :, 0, 0].all() and not nan[0, :, 2, 4].any()


@pytest.mark.parametrize("name", ["12x20_1x1_up_res", "5x7_3x3_s2"])
def test_conv_rows_writes_an_output_with_a_wider_row_stride(name):
    n_img, H, W, C, N, k, stride, *_ = CASES[name]
    M = n_img * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    plain, _, _ = _run(name, "split")
    buf = torch.full((M, N + 32), -7.5, device="cuda")
    got, _, _ = _run(name, "split", out=buf[:, :N])
    assert torch.equal(got, plain)
    assert torch.equal(buf[:, :N].reshape(plain.shape[0], plain.shape[2], plain.shape[3], N).permute(0, 3, 1, 2), plain)
    assert (buf[:, N:] == -7.5).all()                    # nothing beyond the row's width is touched


@pytest.mark.parametrize("name", ["6x10_3x3_96to160", "12x20_1x1_2048_bias", "5x7_3x3_s2"])
def test_conv_rows_reads_a_channels_last_view_in_place(name):
    """A map that is dense in ``torch.channels_last`` IS the kernel's row matrix: no copy, and the same bits as the same values
    passed as NCHW."""
    from bevformer_amd import ops
    x = _case(name)[0].cuda()
    x_cl = x.contiguous(memory_format=torch.channels_last)
    assert ops.rows_of_map(x_cl).data_ptr() == x_cl.data_ptr()
    assert ops.rows_of_map(x).data_ptr() != x.data_ptr()
    a, _, _ = _run(name, "split", x_map=x)
    b, _, _ = _run(name, "split", x_map=x_cl)
    assert torch.equal(a, b)


def test_conv_rows_declines_what_it_does_not_cover():
    from bevformer_amd import ops
    x = torch.randn(2 * 6 * 10, 64, device="cuda")
    w3, w1 = torch.randn(128, 64, 3, 3, device="cuda"), torch.randn(128, 64, 1, 1, device="cuda")
    with torch.no_grad(), ops.using(gemm="split"):
        assert ops.conv_rows(x, 2, (6, 10), w1, None, stride=2) is None                  # 1 x 1 has no stride
        assert ops.conv_rows(x, 2, (6, 10), torch.randn(100, 64, 3, 3, device="cuda"), None) is None
        assert ops.conv_rows(x, 2, (6, 10), w3, None, stride=2, res=torch.randn(2 * 1 * 2, 128, device="cuda"), res_up=True) is None
        assert ops.conv_rows(x, 2, (6, 11), w3, None) is None                            # rows do not match n_img H W
    with torch.no_grad(), ops.using(gemm="native"):
        assert ops.conv_rows(x, 2, (6, 10), w3, None) is None
    with ops.using(gemm="split"):
        assert ops.conv_rows(x, 2, (6, 10), w3, None) is None                            # grad mode on


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("bs,H,W,C,N", [(2, 5, 7, 64, 96),        # one ragged tile: M = 70
                                        (2, 9, 11, 96, 160)])     # two row tiles and two column tiles, both ragged: M = 198
def test_conv_rows_and_conv3x3_bn_are_the_same_gemm(bs, H, W, C, N, mode):
    """The two kernels share one main loop (csrc/conv_mfma.h); they differ in the fetch of a row and in the epilogue.  Under an
    identity BatchNorm (eps 0, weight 1, bias 0, mean 0, var 1: scale exactly 1, shift exactly 0) and without ReLU,
    ``conv3x3_bn`` IS ``conv_rows`` at 3 x 3, stride 1, no bias: the results must be bit-equal."""
    from bevformer_amd import ops
    g = torch.Generator().manual_seed(15)
    rows = torch.randn(bs, H * W, C, generator=g).cuda()
    w = (torch.randn(N, C, 3, 3, generator=g) / (9 * C) ** 0.5).cuda()
    bn = torch.nn.BatchNorm2d(N, eps=0.0).cuda().eval()
    with torch.no_grad(), ops.using(gemm=mode):
        a = ops.conv3x3_bn(rows, (H, W), w, bn, relu=False)
        b = ops.conv_rows(rows.reshape(bs * H * W, C), bs, (H, W), w, None)
    assert a is not None and b is not None
    assert float(a.abs().max()) > 0.1
    assert torch.equal(a.reshape(bs * H * W, N), b)
