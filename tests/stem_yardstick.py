"""Yardstick of the stem fast path (``ops.stem_rows``, ``ops.stem``, ``modes.stem_fused``): the float64 truth and the PARENT the
error bound is measured from.

The truth is ``max_pool2d(relu(bn(conv2d(x, w, stride 2, padding 3))), 3, 2, 1)`` in float64 on the CPU (``stem64``, which also
hands out the un-pooled map).  The parent is the arithmetic of the commit before the kernel: ``F.unfold(x, 7, padding 3, stride 2)``
into ``ops.linear`` in the GEMM mode in force — the K = 147 columns and the weight zero-padded to 160, since ``ops.linear`` wants
K % 32 = 0 —, then BatchNorm, ReLU and ``max_pool2d`` as torch fp32 statements (``parent_stem``).  The bound of every error test:
error against float64 <= 3 x the parent's error on the same inputs in the same mode.

The integer lattice: x in {-4..4}, w in {-2..2}, a norm of scale exactly +-1 (gamma +-1, var 1, ``LATTICE_EPS``) with integer beta
and mean in {-4..4}: |sum| <= 147 * 8 + 8, every operand a bf16 number, every sum exact in fp32."""
import torch
import torch.nn.functional as F

from backbone_yardstick import LATTICE_EPS, _bn  # noqa: F401  (re-exported for the tests)
from fpn_yardstick import assert_lattice, lattice, max_err  # noqa: F401

K_PAD = 160         # 3 * 7 * 7 = 147 padded to ops.linear's K granularity


def out_hw(H, W):
    """(Hc, Wc), (Hp, Wp) of an H x W image."""
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (Hc, Wc), ((Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1)


def stem64(x, w, bn):
    """-> (pooled map, un-pooled map) in float64 on the CPU; ``bn``: (gamma, beta, mean, var, eps)."""
    d = lambda t: t.detach().double().cpu()
    c = torch.relu(_bn(F.conv2d(d(x), d(w), None, stride=2, padding=3), tuple(d(t) for t in bn[:4]) + (bn[4],)))
    return F.max_pool2d(c, 3, 2, 1), c


def parent_stem(x, w, bn):
    """``stem64``'s operator on fp32 GPU tensors with the parent's operators -> (pooled map, un-pooled map)."""
    from bevformer_amd import ops
    B, C, H, W = x.shape
    (Hc, Wc), _ = out_hw(H, W)
    N = w.shape[0]
    cols = F.unfold(x, 7, padding=3, stride=2).transpose(1, 2).reshape(B * Hc * Wc, C * 49)
    a = torch.zeros(cols.shape[0], K_PAD, device=x.device)
    a[:, :C * 49] = cols
    wp = torch.zeros(N, K_PAD, device=x.device)
    wp[:, :C * 49] = w.reshape(N, -1)
    y = ops.linear(a, wp, None).reshape(B, Hc, Wc, N).permute(0, 3, 1, 2)
    c = torch.relu(_bn(y, bn))
    return F.max_pool2d(c, 3, 2, 1), c


def norm_of(m):
    return (m.weight, m.bias, m.running_mean, m.running_var, m.eps)


def bn_module(bn, training=False, device="cuda"):
    m = torch.nn.BatchNorm2d(bn[0].numel(), eps=bn[4]).to(device).train(training)
    with torch.no_grad():
        m.weight.copy_(bn[0]), m.bias.copy_(bn[1]), m.running_mean.copy_(bn[2]), m.running_var.copy_(bn[3])
    return m


def lattice_case(shape, g, gamma="mixed", beta=None):
    """(x, w, bn) on the lattice for ``shape = (B, H, W)``; ``gamma``: "mixed" (+-1), +1 or -1; ``beta``: a constant or None (drawn)."""
    B, H, W = shape
    x, w = lattice((B, 3, H, W), -4, 4, g), lattice((64, 3, 7, 7), -2, 2, g)
    ga = (torch.randint(0, 2, (64,), generator=g) * 2 - 1).float() if gamma == "mixed" else torch.full((64,), float(gamma))
    be = lattice((64,), -4, 4, g) if beta is None else torch.full((64,), float(beta))
    return x, w, (ga, be, lattice((64,), -4, 4, g), torch.ones(64), LATTICE_EPS)


def random_case(shape, g):
    """N(0, 1) images, Kaiming (fan_out, ReLU) weights, BatchNorm vectors with mixed-sign gamma."""
    B, H, W = shape
    x = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5
    sign = (torch.randint(0, 2, (64,), generator=g) * 2 - 1).float()
    bn = ((torch.rand(64, generator=g) + 0.5) * sign, torch.randn(64, generator=g) * 0.2, torch.randn(64, generator=g) * 0.2,
          torch.rand(64, generator=g) + 0.5, 1e-5)
    return x, w, bn
