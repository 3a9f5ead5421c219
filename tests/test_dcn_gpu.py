"""GPU: ``ops.deform_conv_rows`` / ``ops.dcn_offsets`` / ``ops.dcn`` (csrc/deform_conv.h) against the float64 yardstick of
tests/dcn_yardstick.py.  Bound: error <= 3 x the error of the parent — the same operator as a deformable im2col in torch fp32
put through ``ops.linear``, bias / BatchNorm / ReLU in torch — on the same inputs in the same GEMM mode.  On the lattice the
result must EQUAL the yardstick.  Shapes are the smallest at which the kernel can go wrong."""
import functools

import pytest
import torch

import dcn_yardstick as Y

pytestmark = pytest.mark.gpu

# (n_img, H, W, C_in, C_out, stride, epilogue)
CASES = {
    "1x1px": (1, 1, 1, 32, 128, 1, "none"),                    # a single pixel
    "6x10_96to160_bias": (2, 6, 10, 96, 160, 1, "bias"),       # image boundary inside a tile, a tap change every 3 chunks, N tail
    "5x7_s2": (2, 5, 7, 64, 128, 2, "none"),                   # odd sizes at stride 2
    "3x130_bn_relu": (1, 3, 130, 32, 128, 1, "bn+relu"),       # a row longer than a tile, M tail
    "6x10_256_bn_relu": (2, 6, 10, 256, 256, 1, "bn+relu"),    # the stage-3 channel shape
    "4x5_512_bn_relu": (1, 4, 5, 512, 512, 1, "bn+relu"),      # the stage-4 channel shape
}
IDS = list(CASES)
MODES = ["split", "bf16"]


@functools.lru_cache(maxsize=None)
def _case(name, kind="random"):
    """Inputs of a case (CPU fp32) and the float64 result, made once and shared by every test.  ``kind``: ``random``,
    ``lattice`` (module docstring of the yardstick) or ``plain`` (zero offsets, logits + 64: the plain convolution)."""
    n_img, H, W, C, N, stride, ep = CASES[name]
    g = torch.Generator().manual_seed(IDS.index(name))
    Ho, Wo = Y.out_hw(H, W, stride)
    lat = kind == "lattice"
    if lat:
        x, w = Y.lattice((n_img, C, H, W), -4, 4, g), Y.lattice((N, C, 3, 3), -2, 2, g)
        raw = Y.lattice_raw((n_img, Ho, Wo), g)
    else:
        x, w = torch.randn(n_img, C, H, W, generator=g), torch.randn(N, C, 3, 3, generator=g) / (9 * C) ** 0.5
        raw = Y.random_raw((n_img, Ho, Wo), g)
        if kind == "plain":
            raw = torch.cat([torch.zeros(n_img, 18, Ho, Wo), torch.full((n_img, 9, Ho, Wo), 64.0)], 1)
    bias = bn = None
    if ep == "bias":
        bias = Y.lattice((N,), -4, 4, g) if lat else torch.randn(N, generator=g) * 0.2
    elif ep == "bn+relu":
        if lat:     # scale exactly 1 (gamma 1, var 1, eps 0), integer shift
            bn = (torch.ones(N), Y.lattice((N,), -4, 4, g), Y.lattice((N,), -4, 4, g), torch.ones(N), 0.0)
        else:
            bn = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2, torch.randn(N, generator=g) * 0.2,
                  torch.rand(N, generator=g) + 0.5, 1e-5)
    want = Y.dcn64(x, raw, w, stride, bias, bn, ep == "bn+relu")
    if lat:
        Y.assert_lattice(4 * want)                      # multiples of 1/4 below 2^22: exact in bf16 x bf16 -> fp32
        if H * W > 1:                                   # (a single pixel: most lattice offsets leave the image)
            assert (want != 0).double().mean().item() > (0.4 if ep == "bn+relu" else 0.9)
    return x, raw, w, bias, bn, want


def _bn_module(bn):
    N = bn[0].numel()
    m = torch.nn.BatchNorm2d(N, eps=bn[4]).cuda().eval()
    with torch.no_grad():
        m.weight.copy_(bn[0]), m.bias.copy_(bn[1]), m.running_mean.copy_(bn[2]), m.running_var.copy_(bn[3])
    return m


def _run(name, mode, kind="random", x_map=None, raw=None, out=None):
    """-> (result as a (n_img, C_out, Ho, Wo) map, the case's tensors on the GPU, float64 result)"""
    from bevformer_amd import ops
    n_img, H, W, C, N, stride, ep = CASES[name]
    x, raw0, w, bias, bn, want = _case(name, kind)
    dev = torch.device("cuda")
    xd = x.to(dev) if x_map is None else x_map
    rawd = (raw0 if raw is None else raw).to(dev)
    wd, bd = w.to(dev), (None if bias is None else bias.to(dev))
    with torch.no_grad(), ops.using(gemm=mode):
        y = ops.deform_conv_rows(ops.rows_of_map(xd), n_img, (H, W), Y.rows_of_raw(rawd), wd, bias=bd,
                                 bn=None if bn is None else _bn_module(bn), relu=ep == "bn+relu", stride=stride, out=out)
    assert y is not None
    Ho, Wo = Y.out_hw(H, W, stride)
    assert tuple(y.shape) == (n_img * Ho * Wo, N)
    bnd = None if bn is None else tuple(t.to(dev) for t in bn[:4]) + (bn[4],)
    return y.reshape(n_img, Ho, Wo, N).permute(0, 3, 1, 2), (xd, rawd, wd, bd, bnd), want


# ---- 1. the operator's error bound

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IDS)
def test_deform_conv_within_three_parent_errors(name, mode):
    from bevformer_amd import ops
    n_img, H, W, C, N, stride, ep = CASES[name]
    got, (xd, rawd, wd, bd, bnd), want = _run(name, mode)
    with torch.no_grad(), ops.using(gemm=mode):
        parent = Y.parent_dcn(xd, rawd, wd, stride, bd, bnd, ep == "bn+relu")
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"{name} {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent


# ---- 2. lattice exactness

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IDS)
def test_deform_conv_exact_on_the_lattice(name, mode):
    """x in {-4..4}, weights in {-2..2}, half-integer offsets, masks exactly 0 / 1: every coefficient is a multiple of 1/4, every
    blended operand exact in bf16, every sum exact in fp32 — the result EQUALS the yardstick, no element excluded: a corner
    leaking across a row end or an image boundary cannot hide in a tolerance."""
    got, _, want = _run(name, mode, kind="lattice")
    assert torch.equal(got.double().cpu(), want)


# ---- 3. the same GEMM as ops.conv_rows

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["6x10_96to160_bias", "5x7_s2", "1x1px"])
def test_zero_offsets_are_the_plain_row_convolution(name, mode):
    from bevformer_amd import ops
    n_img, H, W, C, N, stride, ep = CASES[name]
    got, (xd, _, wd, bd, _), _ = _run(name, mode, kind="plain")
    with torch.no_grad(), ops.using(gemm=mode):
        plain = ops.conv_rows(ops.rows_of_map(xd), n_img, (H, W), wd, bd, stride=stride)
    assert plain is not None and float(plain.abs().max()) > 0.1
    Ho, Wo = Y.out_hw(H, W, stride)
    assert torch.equal(got, plain.reshape(n_img, Ho, Wo, N).permute(0, 3, 1, 2))


# ---- 4. dead taps

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["6x10_96to160_bias", "5x7_s2"])
def test_non_finite_positions_are_dead_taps(name, mode):
    """NaN, +-inf and +-1e30 offsets on chosen taps against the same taps switched off by their mask (logit -inf, offset 0): bit
    equal and finite — such a position is range-checked before it is converted, contributes zero and addresses nothing."""
    raw = _case(name)[1]
    bad, off = raw.clone(), raw.clone()
    vals = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]
    g = torch.Generator().manual_seed(7)
    B, _, Ho, Wo = raw.shape
    hit = torch.rand(B, 9, Ho, Wo, generator=g) < 0.3
    which = torch.randint(0, len(vals), (B, 9, Ho, Wo), generator=g)
    on_x = torch.rand(B, 9, Ho, Wo, generator=g) < 0.5              # the bad value sits on dx, else on dy
    v = torch.tensor(vals)[which]
    for k in range(9):
        h = hit[:, k]
        bad[:, 2 * k] = torch.where(h & ~on_x[:, k], v[:, k], bad[:, 2 * k])
        bad[:, 2 * k + 1] = torch.where(h & on_x[:, k], v[:, k], bad[:, 2 * k + 1])
        off[:, 2 * k] = torch.where(h, torch.zeros(()), off[:, 2 * k])
        off[:, 2 * k + 1] = torch.where(h, torch.zeros(()), off[:, 2 * k + 1])
        off[:, 18 + k] = torch.where(h, torch.full((), float("-inf")), off[:, 18 + k])
    assert hit.any() and not torch.isfinite(bad).all()
    a, _, _ = _run(name, mode, raw=bad)
    b, _, _ = _run(name, mode, raw=off)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert Y.max_err(b, Y.dcn64(_case(name)[0], off, _case(name)[2], CASES[name][5], _case(name)[3])) < 0.05


# ---- 5. determinism and the output stride

def test_two_runs_are_bit_equal_and_a_wider_output_stride_is_respected():
    for name in ("6x10_96to160_bias", "3x130_bn_relu"):
        n_img, H, W, C, N, stride, ep = CASES[name]
        a, _, _ = _run(name, "split")
        b, _, _ = _run(name, "split")
        assert torch.equal(a, b)
        M = a.shape[0] * a.shape[2] * a.shape[3]
        buf = torch.full((M, N + 32), -7.5, device="cuda")
        got, _, _ = _run(name, "split", out=buf[:, :N])
        assert torch.equal(got, a)
        assert (buf[:, N:] == -7.5).all()                   # nothing beyond the row's width is touched


# ---- 6. layout

def test_a_channels_last_input_is_read_in_place():
    from bevformer_amd import ops
    name = "6x10_96to160_bias"
    x = _case(name)[0].cuda()
    x_cl = x.contiguous(memory_format=torch.channels_last)
    assert ops.rows_of_map(x_cl).data_ptr() == x_cl.data_ptr()
    a, _, _ = _run(name, "split", x_map=x)
    b, _, _ = _run(name, "split", x_map=x_cl)
    assert torch.equal(a, b)


# ---- 7. the pack module

def _pack(C, N, stride, seed=0):
    from bevformer_amd.modules import ModulatedDeformConv2dPack
    g = torch.Generator().manual_seed(seed)
    p = ModulatedDeformConv2dPack(C, N, 3, stride=stride, padding=1, bias=False)
    with torch.no_grad():
        p.weight.copy_(torch.randn(p.weight.shape, generator=g) / (9 * C) ** 0.5)
        p.conv_offset.weight.copy_(torch.randn(p.conv_offset.weight.shape, generator=g) * (0.8 / (9 * C) ** 0.5))
        p.conv_offset.bias.copy_(torch.randn(27, generator=g) * 0.5)
    return p


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stride", [1, 2])
def test_pack_within_three_parent_errors(stride, mode):
    import copy
    from bevformer_amd import ops
    p = _pack(64, 64, stride)
    x = torch.randn(2, 64, 6, 10, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = copy.deepcopy(p).double().forward_torch(x.double())
    pd, xd = p.cuda(), x.cuda()
    with torch.no_grad(), ops.using(gemm=mode):
        assert ops.dcn_reject(pd, xd) is None
        got = ops.dcn(pd, xd)
        parent = Y.parent_pack(pd, xd)
        offs = ops.dcn_offsets(ops.rows_of_map(xd), 2, (6, 10), pd.conv_offset, stride)
    with torch.no_grad(), ops.using(gemm="split"):
        offs_split = ops.dcn_offsets(ops.rows_of_map(xd), 2, (6, 10), pd.conv_offset, stride)
    assert tuple(got.shape) == tuple(want.shape)
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"pack stride {stride} {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent
    # offsets are geometry: the same bits whatever the GEMM mode, 27 channels + zero padding
    assert tuple(offs.shape) == (want.shape[0] * want.shape[2] * want.shape[3], 32)
    assert torch.equal(offs, offs_split) and not offs[:, 27:].any() and offs[:, :18].abs().max() > 0.5


# ---- 8. the bottleneck

@pytest.mark.parametrize("mode", MODES)
def test_bottleneck_with_dcn_within_three_parent_errors(mode):
    import copy
    from bevformer_amd import ops
    from bevformer_amd.modules import Bottleneck
    g = torch.Generator().manual_seed(5)
    blk = Bottleneck(256, 64, dcn=dict(type="DCNv2", deform_groups=1, fallback_on_stride=False), style="caffe")
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5), m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.2), m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
        blk.conv2.conv_offset.weight.copy_(torch.randn(27, 64, 3, 3, generator=g) * (0.8 / 24))
        blk.conv2.conv_offset.bias.copy_(torch.randn(27, generator=g) * 0.5)
    blk.eval()
    x = torch.randn(2, 256, 6, 10, generator=g)
    with torch.no_grad():
        want = copy.deepcopy(blk).double().forward_torch(x.double())
    blk, xd = blk.cuda(), x.cuda()

    def parent(x):          # the block with its conv2 + bn2 + ReLU as the parent's operator
        out = blk.relu(blk.bn1(blk.conv1(x)))
        out = Y.parent_pack(blk.conv2, out, blk.bn2, relu=True)
        return blk.relu(blk.bn3(blk.conv3(out)) + x)

    with torch.no_grad(), ops.using(gemm=mode, dcn_fused=True):
        assert ops.dcn_reject(blk.conv2, blk.bn1(blk.conv1(xd)), blk.bn2) is None
        got = blk(xd)
        par = parent(xd)
    # two runs of torch's own 1 x 1 convolutions are not bit-equal on an MI355X unless asked to be (conv3: 1.5e-8 between two
    # calls); with deterministic algorithms what is left to differ is this package's code
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad(), ops.using(gemm=mode, dcn_fused=False):
            off = blk(xd)
            assert torch.equal(off, blk.forward_torch(xd))
    finally:
        torch.backends.cudnn.deterministic = det
    e_parent, e_fused = Y.max_err(par, want), Y.max_err(got, want)
    print(f"bottleneck {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent
    assert not torch.equal(got, off)                        # the switch did choose another path


# ---- 9. graph capture

def test_dcn_is_capturable():
    from bevformer_amd import ops
    p = _pack(64, 64, 1).cuda()
    bn = torch.nn.BatchNorm2d(64).cuda().eval()
    x = torch.randn(2, 64, 6, 10, device="cuda")
    with torch.no_grad(), ops.using(gemm="split"):
        eager = ops.dcn(p, x, bn, relu=True).clone()        # (also builds the weight images outside the capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.dcn(p, x, bn, relu=True)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = ops.dcn(p, x, bn, relu=True)
        for _ in range(3):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)


# ---- 10. declined calls

def test_declined_calls_run_the_module_path():
    from bevformer_amd import ops
    from bevformer_amd.modules import ModulatedDeformConv2dPack
    p = _pack(64, 64, 1).cuda()
    x = torch.randn(1, 64, 4, 5, device="cuda")
    rows, offs = x.permute(0, 2, 3, 1).reshape(20, 64).contiguous(), torch.zeros(20, 32, device="cuda")
    with ops.using(gemm="split", dcn_fused=True):
        assert ops.dcn(p, x) is None and ops.deform_conv_rows(rows, 1, (4, 5), offs, p.weight) is None          # grad mode on
        assert torch.equal(p(x), p.forward_torch(x))
    with torch.no_grad(), ops.using(gemm="native", dcn_fused=True):
        assert ops.dcn(p, x) is None and ops.deform_conv_rows(rows, 1, (4, 5), offs, p.weight) is None
        assert ops.dcn_offsets(rows, 1, (4, 5), p.conv_offset, 1) is None
        assert torch.equal(p(x), p.forward_torch(x))
    with torch.no_grad(), ops.using(gemm="split", dcn_fused=True):
        p48 = ModulatedDeformConv2dPack(48, 64, 3, padding=1, bias=False).cuda()
        x48 = torch.randn(1, 48, 4, 5, device="cuda")
        assert ops.dcn(p48, x48) is None
        assert ops.deform_conv_rows(x48.permute(0, 2, 3, 1).reshape(20, 48).contiguous(), 1, (4, 5), offs, p48.weight) is None
        assert torch.equal(p48(x48), p48.forward_torch(x48))
        pd = ModulatedDeformConv2dPack(64, 64, 3, padding=2, dilation=2, bias=False).cuda()
        assert ops.dcn_reject(pd, x) == "the convolution is dilated" and ops.dcn(pd, x) is None
        assert torch.equal(pd(x), pd.forward_torch(x)) and tuple(pd(x).shape) == (1, 64, 4, 5)
        assert ops.dcn(p, x) is not None                    # the covered call does run
