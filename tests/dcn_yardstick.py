"""Yardstick of the backbone's deformable convolution (``ops.deform_conv_rows``, ``ops.dcn``): the modulated deformable 3 x 3
convolution (mmcv 1.4.0's ``ModulatedDeformConv2dPack`` as published: DCNv2, ``groups = deform_groups = 1``) in float64 on the
CPU by explicit gathers (``dcn64``), and the PARENT the error bound is measured from — the same operator as a deformable
im2col written in torch fp32 statements on the GPU, an (M, 9 C) matrix put through ``ops.linear`` in the GEMM mode in force,
bias / BatchNorm / ReLU in torch: the arithmetic of the commit before the kernel, using nothing that came with it.  The bound
of every test: error against the float64 yardstick <= 3 x the parent's error on the same inputs in the same mode.

The raw offset tensor has 27 channels per output pixel: for tap k = 3 i + j channel 2 k is dy, 2 k + 1 is dx, 18 + k the mask
logit.  The sample of tap k at output pixel (oy, ox) lies at (S oy - 1 + i + dy, S ox - 1 + j + dx); a position that is not
finite or outside (-1, H) x (-1, W) contributes zero, a corner outside the image contributes zero.

The lattice: x in {-4..4}, weights in {-2..2}, offsets half-integers in [-3, 3], mask logits in {-inf, +64} (sigmoid exactly
0 / 1 in fp32 and fp64).  Every bilinear coefficient is then a multiple of 1/4, every blended A operand a multiple of 1/4 of
magnitude <= 4 (exact in bf16), and 4 y an integer below 2^24: a kernel must EQUAL the float64 result
(``fpn_yardstick.assert_lattice(4 * want)`` guards it)."""
import torch
import torch.nn.functional as F

from fpn_yardstick import assert_lattice, lattice, max_err, parent_conv  # noqa: F401  (re-exported for the tests)


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _epilogue(y, bias, bn, relu):
    """``bn``: (gamma, beta, mean, var, eps) or None, on a (B, C_out, Ho, Wo) map in its own dtype."""
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if bn is not None:
        ga, be, mu, va, eps = bn
        y = (y - mu.view(1, -1, 1, 1)) / torch.sqrt(va.view(1, -1, 1, 1) + eps) * ga.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def _cols(x, raw, stride):
    """The deformable im2col in ``x``'s dtype on its device: (B, Ho, Wo, 9, C), tap-major."""
    B, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, stride)
    assert tuple(raw.shape) == (B, 27, Ho, Wo)
    xl = x.permute(0, 2, 3, 1).reshape(B, H * W, C)                 # rows of channels
    oy = torch.arange(Ho, device=x.device, dtype=x.dtype).view(1, Ho, 1) * stride
    ox = torch.arange(Wo, device=x.device, dtype=x.dtype).view(1, 1, Wo) * stride
    taps = []
    for k in range(9):
        i, j = k // 3, k % 3
        py = oy - 1 + i + raw[:, 2 * k]
        px = ox - 1 + j + raw[:, 2 * k + 1]
        m = torch.sigmoid(raw[:, 18 + k])
        ok = (py > -1) & (py < H) & (px > -1) & (px < W)            # False for NaN
        py = torch.where(ok, py, torch.zeros_like(py))
        px = torch.where(ok, px, torch.zeros_like(px))
        y0, x0 = torch.floor(py), torch.floor(px)
        ly, lx = py - y0, px - x0
        y0, x0 = y0.long(), x0.long()
        acc = torch.zeros(B, Ho, Wo, C, dtype=x.dtype, device=x.device)
        for ddy, ddx, cw in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
            cy, cx = y0 + ddy, x0 + ddx
            live = ok & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
            idx = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).reshape(B, Ho * Wo, 1).expand(B, Ho * Wo, C)
            v = torch.gather(xl, 1, idx).reshape(B, Ho, Wo, C)
            coef = torch.where(live, cw * m, torch.zeros_like(cw)).unsqueeze(-1)
            acc = acc + torch.where(live.unsqueeze(-1), v, torch.zeros_like(v)) * coef
        taps.append(acc)
    return torch.stack(taps, 3)


def dcn64(x, raw, w, stride=1, bias=None, bn=None, relu=False):
    """The operator in float64 on the CPU: ``x`` (B, C, H, W), ``raw`` (B, 27, Ho, Wo), ``w`` (C_out, C, 3, 3) -> (B, C_out, Ho, Wo)."""
    d = lambda t: None if t is None else t.detach().double().cpu()
    x, raw, w = d(x), d(raw), d(w)
    cols = _cols(x, raw, stride)                                    # (B, Ho, Wo, 9, C)
    y = torch.einsum("bhwkc,ock->bohw", cols, w.reshape(w.shape[0], w.shape[1], 9))
    return _epilogue(y, d(bias), None if bn is None else tuple(d(t) for t in bn[:4]) + (bn[4],), relu)


def dcn64_grid_sample(x, raw, w, stride=1):
    """The same operator through ``F.grid_sample(align_corners=True, padding_mode='zeros')`` in float64 (H, W >= 2): an
    independent formulation of the bilinear gather.  Positions outside (-1, H) x (-1, W) sample zeros there too."""
    x, raw, w = x.double(), raw.double(), w.double()
    B, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, stride)
    oy = torch.arange(Ho, dtype=torch.float64).view(1, Ho, 1) * stride
    ox = torch.arange(Wo, dtype=torch.float64).view(1, 1, Wo) * stride
    y = torch.zeros(B, w.shape[0], Ho, Wo, dtype=torch.float64)
    for k in range(9):
        py = oy - 1 + k // 3 + raw[:, 2 * k]
        px = ox - 1 + k % 3 + raw[:, 2 * k + 1]
        grid = torch.stack([px / (W - 1) * 2 - 1, py / (H - 1) * 2 - 1], -1)
        s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)      # (B, C, Ho, Wo)
        y = y + torch.einsum("bchw,oc->bohw", s * torch.sigmoid(raw[:, 18 + k]).unsqueeze(1), w[:, :, k // 3, k % 3])
    return y


def parent_dcn(x, raw, w, stride=1, bias=None, bn=None, relu=False):
    """``dcn64``'s operator on fp32 GPU maps in the GEMM mode in force: the deformable im2col in torch fp32 -> (M, 9 C) ->
    ``ops.linear``; bias / BatchNorm / ReLU in torch fp32."""
    from bevformer_amd import ops
    B, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, stride)
    cols = _cols(x, raw, stride).reshape(B * Ho * Wo, 9 * C).contiguous()
    wm = w.reshape(w.shape[0], C, 9).permute(0, 2, 1).reshape(w.shape[0], 9 * C).contiguous()       # k = tap * C + ci
    y = ops.linear(cols, wm, None)
    assert y is not None, "ops.linear declined the im2col GEMM"
    y = y.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)
    return _epilogue(y, bias, bn, relu)


def parent_pack(pack, x, norm=None, relu=False):
    """The module-level parent: the offset convolution as ``fpn_yardstick.parent_conv`` under ``gemm="split"``, then
    ``parent_dcn`` in the mode in force."""
    from bevformer_amd import ops
    off = pack.conv_offset
    with ops.using(gemm="split"):
        raw = parent_conv(x, off.weight, off.bias, off.stride[0])
    bn = None if norm is None else (norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.eps)
    return parent_dcn(x, raw, pack.weight, pack.stride[0], pack.bias, bn, relu)


def rows_of_raw(raw, pad_to=32):
    """(B, 27, Ho, Wo) -> the kernel's (B Ho Wo, 32) offset matrix (zero padding)."""
    B, c, Ho, Wo = raw.shape
    rows = raw.permute(0, 2, 3, 1).reshape(B * Ho * Wo, c)
    return torch.cat([rows, rows.new_zeros(rows.shape[0], pad_to - c)], 1).contiguous()


def lattice_raw(shape_bhw, g):
    """Lattice offsets: half-integers in [-3, 3], logits in {-inf, +64} -> (B, 27, Ho, Wo)."""
    B, Ho, Wo = shape_bhw
    off = torch.randint(-6, 7, (B, 18, Ho, Wo), generator=g).float() / 2
    on = torch.randint(0, 4, (B, 9, Ho, Wo), generator=g) > 0              # three taps in four are on
    logit = torch.where(on, torch.full((B, 9, Ho, Wo), 64.0), torch.full((B, 9, Ho, Wo), float("-inf")))
    return torch.cat([off, logit], 1)


def random_raw(shape_bhw, g, scale=1.5):
    B, Ho, Wo = shape_bhw
    return torch.cat([torch.randn(B, 18, Ho, Wo, generator=g) * scale, torch.randn(B, 9, Ho, Wo, generator=g)], 1)
