"""Yardstick of the backbone fast path (``ops.conv_bn_rows``, ``ops.bottleneck``, ``modes.backbone_fused``): the float64 truth and
the PARENT the error bound is measured from.

The truth of a block or a backbone is the module's own ``forward_torch`` on a ``.double()`` CPU deep copy; of a single convolution
it is ``fpn_yardstick.conv64`` + BatchNorm + residual + ReLU in float64 (``conv_bn64``).  The parent is the same arithmetic with
every plain convolution as ``fpn_yardstick.parent_conv`` (im2col + ``ops.linear`` in the GEMM mode in force), a DCNv2 pack as
``dcn_yardstick.parent_pack``, and BatchNorm / add / ReLU as torch fp32 statements: the arithmetic of the commit before the
kernel, using nothing that came with it.  The bound of every error test: error against float64 <= 3 x the parent's error on the
same inputs in the same mode.

The integer lattice of one convolution is ``fpn_yardstick``'s (x, res in {-4..4}, w in {-2..2}) with a BatchNorm of scale exactly
1 (gamma 1, var 1, eps 0) and integer mean and beta in {-4..4}.  A whole block chains three convolutions — what one writes the
next one reads and rounds to bf16 (``bf16`` mode) or to 16 bits (``split``) — so its lattice weights are SPARSE, in the manner of
``lattice_neck_`` (``lattice_block_``): per output channel two nonzero ``conv1`` weights of magnitude <= 2, three nonzero +-1
``conv2`` weights, two nonzero +-1 ``conv3`` and downsample weights, unit-scale norms (gamma 1, var 1, ``LATTICE_EPS``) with integer beta
and mean in {-2..2}, so integer shifts in {-4..4}.  With x in
{-4..4} every tensor a later convolution reads is then an integer of magnitude <= 256 = exactly a bf16 number: conv1's output
<= 2*2*4 + 4 = 20, conv2's <= 3*20 + 4 = 64, conv3's norm <= 2*64 + 4 = 132, the identity <= 4 (the input) or <= 2*4 + 4 = 12 (a
downsample), the block's output <= 144 (``block64_intermediates`` hands them out; the tests assert the bound on the CPU)."""
import copy

import torch

from dcn_yardstick import parent_pack
from fpn_yardstick import assert_lattice, conv64, lattice, max_err, parent_conv  # noqa: F401  (re-exported for the tests)

BF16_EXACT = 256.0
# the eps of a lattice block's norms: torch's batch_norm refuses eps = 0, and 1 + 1e-30 IS 1 in fp32 and in float64, so the scale
# 1 / sqrt(var + eps) is exactly 1 in the module path and in the kernel alike
LATTICE_EPS = 1e-30


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _bn(y, bn):
    """``bn``: (gamma, beta, mean, var, eps) on a (B, C, H, W) map in its own dtype: torch's inference BatchNorm, statement by statement."""
    ga, be, mu, va, eps = bn
    v = lambda t: t.view(1, -1, 1, 1)
    return (y - v(mu)) / torch.sqrt(v(va) + eps) * v(ga) + v(be)


# ---- one convolution

def conv_bn64(x, w, bn, stride=1, res=None, relu=False):
    """``act(bn(conv(x)) + res)`` in float64 on the CPU: ``x`` (B, C, H, W), ``w`` (C_out, C, k, k) with padding k // 2, ``bn``
    (gamma, beta, mean, var, eps), ``res`` (B, C_out, Ho, Wo) or None."""
    d = lambda t: t.detach().double().cpu()
    y = _bn(conv64(x, w, None, stride), tuple(d(t) for t in bn[:4]) + (bn[4],))
    if res is not None:
        y = y + d(res)
    return torch.relu(y) if relu else y


def parent_conv_bn(x, w, bn, stride=1, res=None, relu=False):
    """``conv_bn64``'s operator on fp32 GPU maps in the GEMM mode in force: ``parent_conv``, then BatchNorm, add, ReLU in torch fp32."""
    y = _bn(parent_conv(x, w, None, stride), bn)
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


# ---- a bottleneck, a backbone

def _is_pack(conv):
    return hasattr(conv, "conv_offset")


def block64(block, x):
    """The block's own module path on a float64 CPU deep copy."""
    with torch.no_grad():
        return copy.deepcopy(block).double().cpu().forward_torch(x.detach().double().cpu())


def block64_intermediates(block, x):
    """(conv1's output after norm + ReLU, conv2's likewise, the identity, the block's output) of a block with a plain conv2 in
    float64 on the CPU: what the lattice tests bound."""
    b = copy.deepcopy(block).double().cpu()
    x = x.detach().double().cpu()
    with torch.no_grad():
        o1 = torch.relu(b.bn1(b.conv1(x)))
        o2 = torch.relu(b.bn2(b.conv2(o1)))
        idt = x if b.downsample is None else b.downsample(x)
        out = torch.relu(b.bn3(b.conv3(o2)) + idt)
    return o1, o2, idt, out


def _norm_of(m):
    return (m.weight, m.bias, m.running_mean, m.running_var, m.eps)


def parent_block(block, x):
    """The block on fp32 GPU maps with the parent's operators: plain convolutions as ``parent_conv``, a pack as ``parent_pack``
    (its norm and ReLU in torch), the norms in the state they are in (``train()``: batch statistics, as the module path), add
    and ReLU in torch fp32."""
    norm = lambda m, y: m(y) if m.training else _bn(y, _norm_of(m))
    conv = lambda c, y: parent_conv(y, c.weight, None, c.stride[0])
    out = torch.relu(norm(block.bn1, conv(block.conv1, x)))
    out = parent_pack(block.conv2, out) if _is_pack(block.conv2) else conv(block.conv2, out)
    out = torch.relu(norm(block.bn2, out))
    out = norm(block.bn3, conv(block.conv3, out))
    idt = x if block.downsample is None else norm(block.downsample[1], conv(block.downsample[0], x))
    return torch.relu(out + idt)


def _resnet(net, x, blockfn):
    x = net.maxpool(net.relu(net.bn1(net.conv1(x))))
    outs = []
    for i, name in enumerate(net.res_layers):
        for blk in getattr(net, name):
            x = blockfn(blk, x)
        if i in net.out_indices:
            outs.append(x)
    return outs


def resnet64(net, x):
    """The backbone's module path (stem, max pooling, every block's ``forward_torch``) on a float64 CPU deep copy, with every
    norm in the state it is in."""
    n64 = copy.deepcopy(net).double().cpu()
    with torch.no_grad():
        return _resnet(n64, x.detach().double().cpu(), lambda b, y: b.forward_torch(y))


def parent_resnet(net, x):
    """The backbone with the stem and the max pooling on torch (as the fast path leaves them) and every block as ``parent_block``."""
    with torch.no_grad():
        return _resnet(net, x, parent_block)


# ---- parameters

def randomize_norms_(module, g, packs=True):
    """Random affine BatchNorms with random running statistics (every ``weight`` in [0.5, 1.5): ``bn3.weight`` is nonzero) and
    random ``conv_offset``s that move the samples, as tests/test_dcn_gpu.py draws them (in place)."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5), m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.2), m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
            if packs and _is_pack(m):
                w = m.conv_offset.weight
                w.copy_(torch.randn(w.shape, generator=g) * (0.8 / (9 * w.shape[1]) ** 0.5))
                m.conv_offset.bias.copy_(torch.randn(27, generator=g) * 0.5)
    return module


def randomize_convs_(module, g):
    """Random convolution weights at the scale that keeps every map O(1): randn / sqrt(fan_in), packs included; ``conv_offset``s are
    ``randomize_norms_``'s (in place)."""
    with torch.no_grad():
        for name, m in module.named_modules():
            w = getattr(m, "weight", None)
            if torch.is_tensor(w) and w.dim() == 4 and not name.endswith("conv_offset"):
                w.copy_(torch.randn(w.shape, generator=g) / w[0].numel() ** 0.5)
    return module


def _sparse_(w, nnz, mag, g):
    flat = torch.zeros(w.shape[0], w[0].numel())
    for co in range(w.shape[0]):
        idx = torch.randperm(flat.shape[1], generator=g)[:nnz]
        flat[co, idx] = torch.randint(1, mag + 1, (nnz,), generator=g).float() * (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1)
    w.copy_(flat.reshape(w.shape))


def lattice_block_(block, seed=0):
    """Sparse lattice parameters for a block with a plain conv2 (in place; module docstring)."""
    g = torch.Generator().manual_seed(seed)
    convs = [(block.conv1, 2, 2), (block.conv2, 3, 1), (block.conv3, 2, 1)]
    norms = [block.bn1, block.bn2, block.bn3]
    if block.downsample is not None:
        convs.append((block.downsample[0], 2, 1))
        norms.append(block.downsample[1])
    with torch.no_grad():
        for conv, nnz, mag in convs:
            _sparse_(conv.weight, nnz, mag, g)
        for n in norms:
            n.eps = LATTICE_EPS
            n.weight.fill_(1.0), n.running_var.fill_(1.0)
            # beta and mean in {-2..2}: the shift beta - mean is an integer in {-4..4}
            n.bias.copy_(lattice(n.bias.shape, -2, 2, g)), n.running_mean.copy_(lattice(n.bias.shape, -2, 2, g))
    return block
