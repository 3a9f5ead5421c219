"""Yardstick of the deformable convolution's backward (``ops.deform_conv_rows_backward``, ``modes.dcn_train``): the float64 truth of
the gradients with respect to the input, the raw offset tensor and the weight, and the PARENT the error bound is measured from.

The operator is ``dcn_yardstick``'s: ``z = einsum(_cols(x, raw), w)``, ``y = act(bn(z))`` with an inference BatchNorm.  The truth is
torch's autograd through those statements in float64 on the CPU; the ReLU's mask is NOT recomputed but taken from the ``y`` the
test supplies (``y > 0``), as in ``backbone_train_yardstick.conv_bwd64``.  ``floor`` has zero slope there, so at an integer
position the slope is the one of the cell ``floor`` selects; a dead position (``torch.where`` on ``ok``) passes no gradient.

The parent is float32 autograd of the same statements on the GPU with the code of the commit before the kernels: ``_cols`` in torch
fp32, the (M, 9 C) matrix through ``ops.linear_or_torch`` (``_LinearFunction``, asserted) in the GEMM mode in force, BatchNorm and
mask as torch statements.  The bound of every error test: error against float64 <= 3 x the parent's error.

The lattice of the backward (``lattice_raw3``): half-integer offsets in [-3, 3], logits drawn from {-inf, 0, +64}: m is in
{0, 1/2, 1} and m (1 - m) in {0, 1/4}, every bilinear coefficient a multiple of 1/4 — with integer x, w and g every gradient is
a multiple of 1/16."""
import torch

import backbone_train_yardstick as T
import backbone_yardstick as B
import dcn_yardstick as D
from dcn_yardstick import max_err  # noqa: F401  (re-exported for the tests)

_d = T._d


def _z(x, raw, w, stride):
    cols = D._cols(x, raw, stride)                                  # (B, Ho, Wo, 9, C)
    return torch.einsum("bhwkc,ock->bohw", cols, w.reshape(w.shape[0], w.shape[1], 9))


def dcn_bwd64(g, y, x, raw, w, bn, stride=1, relu=False):
    """(dx, draw, dW) in float64 on the CPU of ``sum(g * act(bn(deform_conv(x, raw, w))))`` with the ReLU's mask taken from ``y``:
    maps ``g``, ``y`` (B, C_out, Ho, Wo), ``x`` (B, C_in, H, W), ``raw`` (B, 27, Ho, Wo), ``w`` (C_out, C_in, 3, 3), ``bn``
    (gamma, beta, mean, var, eps) or ``None``."""
    x64, r64, w64 = _d(x).requires_grad_(), _d(raw).requires_grad_(), _d(w).requires_grad_()
    z = _z(x64, r64, w64, stride)
    if bn is not None:
        z = B._bn(z, tuple(_d(t) for t in bn[:4]) + (bn[4],))
    gm = _d(g) * (_d(y) > 0).double() if relu else _d(g)
    return torch.autograd.grad((z * gm).sum(), (x64, r64, w64))


def parent_dcn_grads(g, y, x, raw, w, bn, stride=1, relu=False):
    """``dcn_bwd64``'s gradients on fp32 GPU maps with the parent's arithmetic in the GEMM mode in force."""
    from bevformer_amd import ops
    x32, r32, w32 = (t.detach().clone().requires_grad_() for t in (x, raw, w))
    Bn, C, H, W = x.shape
    Ho, Wo = D.out_hw(H, W, stride)
    with torch.enable_grad():
        cols = D._cols(x32, r32, stride).reshape(Bn * Ho * Wo, 9 * C).contiguous()
        wm = w32.reshape(w.shape[0], C, 9).permute(0, 2, 1).reshape(w.shape[0], 9 * C).contiguous()     # k = tap * C + ci
        z = ops.linear_or_torch(cols, wm)
        assert z.grad_fn is not None and "_LinearFunction" in type(z.grad_fn).__name__, \
            f"the parent's im2col GEMM did not take ops.linear's autograd path ({type(z.grad_fn).__name__})"
        z = z.reshape(Bn, Ho, Wo, -1).permute(0, 3, 1, 2)
        if bn is not None:
            z = B._bn(z, bn)
        gm = g * (y > 0).float() if relu else g
        return torch.autograd.grad((z * gm).sum(), (x32, r32, w32))


def lattice_raw3(shape_bhw, g, half_steps=6):
    """Lattice offsets for the backward: half-integers in [-half_steps / 2, half_steps / 2], logits from {-inf, 0, +64} ->
    (B, 27, Ho, Wo)."""
    Bn, Ho, Wo = shape_bhw
    off = torch.randint(-half_steps, half_steps + 1, (Bn, 18, Ho, Wo), generator=g).float() / 2
    logit = torch.tensor([float("-inf"), 0.0, 64.0])[torch.randint(0, 3, (Bn, 9, Ho, Wo), generator=g)]
    return torch.cat([off, logit], 1)


def positions64(x_shape, raw, stride):
    """(py, px, ok) of every tap in float64: (B, 9, Ho, Wo) each."""
    _, _, H, W = x_shape
    r = _d(raw)
    Ho, Wo = r.shape[2:]
    k = torch.arange(9)
    oy = (torch.arange(Ho, dtype=torch.float64) * stride).view(1, 1, Ho, 1)
    ox = (torch.arange(Wo, dtype=torch.float64) * stride).view(1, 1, 1, Wo)
    py = oy - 1 + (k // 3).double().view(1, 9, 1, 1) + r[:, 0:18:2]
    px = ox - 1 + (k % 3).double().view(1, 9, 1, 1) + r[:, 1:18:2]
    return py, px, (py > -1) & (py < H) & (px > -1) & (px < W)


def position_margin64(x_shape, raw, stride):
    """The smallest distance of any live sample coordinate from an integer (where ``floor`` jumps and a slope with it), and of any
    sample coordinate from the borders -1, H, W (where a tap goes dead), in float64."""
    _, _, H, W = x_shape
    py, px, ok = positions64(x_shape, raw, stride)
    frac = lambda p: torch.minimum(p - p.floor(), p.ceil() - p)     # (an integer gives 0)
    inner = torch.minimum(frac(py), frac(px))[ok]
    m = float(inner.min()) if inner.numel() else float("inf")
    for p, hi in ((py, H), (px, W)):
        p = p[torch.isfinite(p)]
        if p.numel():
            m = min(m, float((p + 1).abs().min()), float((p - hi).abs().min()))
    return m


def exact_sum_bound64(g, x, raw, w, stride):
    """An upper bound, from float64 arithmetic alone, on the absolute value of every partial sum a kernel can form on lattice
    inputs in ANY order of summation — the sums of absolute values of the terms of (a) dcol = sum_co g w, (b) the offset
    gradients' sums over ci of dcol v_c (|v_c| <= max |x|; their final combination has coefficients of absolute sum <= 2),
    (c) dx, over every (pixel, tap) that can add to a row, (d) dW = sum_q g col.  With all terms multiples of 1/16, sums below
    2^24 / 16 are exact in fp32."""
    g64, x64, w64 = _d(g).abs(), _d(x).abs(), _d(w).abs()
    N, C = w.shape[:2]
    dcol_abs_terms = torch.einsum("bohw,ock->bhwkc", g64, w64.reshape(N, C, 9))             # (a), sum of |terms|
    dcol = torch.einsum("bohw,ock->bhwkc", _d(g), _d(w).reshape(N, C, 9)).abs()
    b_offs = 2 * float(dcol.sum(-1).max()) * float(x64.max())                               # (b)
    b_dx = float(dcol.sum((1, 2, 3)).max())                                                 # (c)
    cols_abs = D._cols(x64, _d(raw), stride)
    b_dw = float(torch.einsum("bohw,bhwkc->ock", g64, cols_abs).max())                      # (d)
    return max(float(dcol_abs_terms.max()), b_offs, b_dx, b_dw)


def rows_of_map(t):
    """(B, C, H, W) -> (B H W, C) contiguous rows."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def raw_of_rows(rows, shape_bhw):
    """The kernel's (B Ho Wo, 32) offset-layout matrix -> (B, 27, Ho, Wo)."""
    Bn, Ho, Wo = shape_bhw
    return rows[:, :27].reshape(Bn, Ho, Wo, 27).permute(0, 3, 1, 2)


# ---- a bottleneck whose conv2 is a DCNv2 pack

def block_truth64(block, x, g, need_x=True):
    """(out, dx or None, {name: dW}, raw, draw) of ``sum(g * block.forward_torch(x))`` in float64 autograd on a CPU deep copy;
    ``raw`` is the output of the pack's ``conv_offset`` and ``draw`` the gradient with respect to it."""
    import copy
    b = copy.deepcopy(block).double().cpu()
    keep = {}

    def hook(_m, _i, o):
        if o.requires_grad:
            o.retain_grad()
        keep["raw"] = o
    h = b.conv2.conv_offset.register_forward_hook(hook)
    x64 = _d(x).requires_grad_(need_x)
    with torch.enable_grad():
        out = b.forward_torch(x64)
        (out * _d(g)).sum().backward()
    h.remove()
    gw = {n: p.grad for n, p in b.named_parameters() if p.requires_grad}
    return out.detach(), x64.grad, gw, keep["raw"].detach(), keep["raw"].grad


def parent_dcn_block_diff(block, x):
    """A block with a DCNv2 ``conv2`` and norms in eval mode with the parent's operators, under autograd -> (out, raw): the plain
    convolutions as ``backbone_train_yardstick.parent_conv_diff``, ``conv_offset`` likewise under ``gemm="split"`` (as
    ``dcn_yardstick.parent_pack``), the deformable convolution as ``_cols`` in torch fp32 + ``ops.linear_or_torch`` in the mode in
    force; BatchNorm, add and ReLU in torch fp32."""
    from bevformer_amd import ops
    norm = lambda m, y: B._bn(y, B._norm_of(m))
    conv = lambda c, y: T.parent_conv_diff(y, c.weight, c.stride[0])
    pack = block.conv2
    s2 = pack.stride[0]
    o1 = torch.relu(norm(block.bn1, conv(block.conv1, x)))
    with ops.using(gemm="split"):
        # (27 output channels padded to 32 with zero rows: ``ops.linear``'s kernels want a multiple of 32, and the padding's
        # gradient is dropped by the slice)
        w_off = pack.conv_offset.weight
        w32 = torch.cat([w_off, w_off.new_zeros((5,) + tuple(w_off.shape[1:]))], 0)
        raw = T.parent_conv_diff(o1, w32, s2)[:, :27] + pack.conv_offset.bias.view(1, -1, 1, 1)
    Bn, C, H, W = o1.shape
    Ho, Wo = D.out_hw(H, W, s2)
    cols = D._cols(o1, raw, s2).reshape(Bn * Ho * Wo, 9 * C).contiguous()
    w = pack.weight
    wm = w.reshape(w.shape[0], C, 9).permute(0, 2, 1).reshape(w.shape[0], 9 * C).contiguous()
    z = ops.linear_or_torch(cols, wm)
    assert z.grad_fn is not None and "_LinearFunction" in type(z.grad_fn).__name__, type(z.grad_fn).__name__
    z = z.reshape(Bn, Ho, Wo, -1).permute(0, 3, 1, 2)
    out = torch.relu(norm(block.bn2, z))
    out = norm(block.bn3, conv(block.conv3, out))
    idt = x if block.downsample is None else norm(block.downsample[1], conv(block.downsample[0], x))
    return torch.relu(out + idt), raw


def parent_dcn_block_grads(block, x, g, need_x=True):
    """(out, dx or None, {name: dW}, raw) with the parent's arithmetic on fp32 GPU maps in the GEMM mode in force."""
    x32 = x.detach().clone().requires_grad_(need_x)
    with torch.enable_grad():
        out, raw = parent_dcn_block_diff(block, x32)
        loss = (out * g).sum()
        dx = torch.autograd.grad(loss, x32, retain_graph=True)[0] if need_x else None
        gw = T._grads_of(block, loss)
    return out.detach(), dx, gw, raw.detach()


def lattice_offsets_(pack, seed=0):
    """Lattice parameters for a pack's ``conv_offset`` (in place): per offset channel ONE nonzero weight of +-1/2 and a bias in
    {-1, -1/2, 0, 1/2, 1}; the mask channels have zero weights and a bias drawn per tap from {-inf, 0, 64}.  On integer
    activations the offsets are then half-integers and the logits are ``lattice_raw3``'s."""
    g = torch.Generator().manual_seed(1000 + seed)
    w = pack.conv_offset.weight
    with torch.no_grad():
        flat = torch.zeros(27, w[0].numel())
        for c in range(18):
            i = int(torch.randint(0, flat.shape[1], (1,), generator=g))
            flat[c, i] = 0.5 * (int(torch.randint(0, 2, (1,), generator=g)) * 2 - 1)
        w.copy_(flat.reshape(w.shape))
        b = torch.zeros(27)
        b[:18] = torch.randint(-2, 3, (18,), generator=g).float() / 2
        b[18:] = torch.tensor([float("-inf"), 0.0, 64.0])[torch.randint(0, 3, (9,), generator=g)]
        pack.conv_offset.bias.copy_(b)
    return pack
