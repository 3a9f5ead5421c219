"""Yardstick of the backbone training path (``ops.conv_bn_rows_backward``, ``ops.bottleneck_train``, ``modes.backbone_train``): the
float64 truth of the gradients and the PARENT the error bound is measured from.

One convolution.  The operator is ``backbone_yardstick.conv_bn64``'s: ``y = act(bn(conv(x, w)) + res)`` with an inference BatchNorm.
``conv_bn64`` itself detaches what it is given, so its statements are restated here without the detach (``F.conv2d`` in float64,
``backbone_yardstick._bn``) and differentiated by torch's autograd in float64 on the CPU.  The ReLU's mask is NOT recomputed: it is
taken from the ``y`` the test supplies (``y > 0``, 0 at exactly 0), so a test can put exact zeros into ``y`` and there is no kink
to argue about.  The truth of the input gradient also takes the kernel's two epilogue options, in float64: ``+ add``, then
``* (next_mask > 0) * next_scale``.

The parent is float32 autograd of the same arithmetic with the code of the commit before the kernels: the convolution as an
explicit im2col matrix (``F.unfold``) through ``ops.linear_or_torch`` — ``ops.linear``'s autograd path (``_LinearFunction``: the
projection kernel forward, over the transposed weight for the input gradient, the TN kernel for the weight gradient) in the GEMM
mode in force —, BatchNorm and mask as torch fp32 statements.  ``_LinearFunction`` is differentiable in both ``split`` and
``bf16`` (``parent_conv_grads`` asserts that the im2col GEMM did go through it), so torch's own convolution is never the parent.
The bound of every error test: error against float64 <= 3 x the parent's error on the same inputs in the same mode.

A block, a backbone: the truth is float64 autograd through the module's own ``forward_torch`` on a ``.double()`` CPU deep copy;
the parent is float32 autograd through ``backbone_yardstick.parent_block``'s structure with the differentiable im2col
convolution above."""
import copy

import torch
import torch.nn.functional as F

import backbone_yardstick as Y
from backbone_yardstick import max_err  # noqa: F401  (re-exported for the tests)


def _d(t):
    return None if t is None else t.detach().double().cpu()


def scale_of(bn, dtype=None):
    """gamma / sqrt(var + eps) of ``bn = (gamma, beta, mean, var, eps)`` in the vectors' own dtype (or ``dtype``)."""
    ga, _, _, va, eps = bn
    if dtype is not None:
        ga, va = ga.to(dtype), va.to(dtype)
    return ga / torch.sqrt(va + eps)


def _finish(dx, add, next_mask, next_bn):
    if add is not None:
        dx = dx + add
    if next_mask is not None:
        dx = dx * (next_mask > 0).to(dx.dtype)
        if next_bn is not None:
            dx = dx * scale_of(next_bn).view(1, -1, 1, 1)
    return dx


def conv_bwd64(g, y, x, w, bn, stride=1, relu=False, add=None, next_mask=None, next_bn=None):
    """(dx, dW) in float64 on the CPU of ``sum(g * act(bn(conv(x, w))))`` with the ReLU's mask taken from ``y``: maps ``g``, ``y``
    (B, C_out, Ho, Wo), ``x`` (B, C_in, H, W), ``w`` (C_out, C_in, k, k) with padding k // 2, ``bn`` (gamma, beta, mean, var, eps);
    ``add`` / ``next_mask`` (B, C_in, H, W) and ``next_bn``: the input gradient's epilogue."""
    x64, w64 = _d(x).requires_grad_(), _d(w).requires_grad_()
    bn64 = tuple(_d(t) for t in bn[:4]) + (bn[4],)
    z = Y._bn(F.conv2d(x64, w64, None, stride=stride, padding=w.shape[-1] // 2), bn64)
    gm = _d(g) * (_d(y) > 0).double() if relu else _d(g)
    dx, dw = torch.autograd.grad((z * gm).sum(), (x64, w64))
    nb = None if next_bn is None else tuple(_d(t) for t in next_bn[:4]) + (next_bn[4],)
    return _finish(dx, _d(add), _d(next_mask), nb), dw


def parent_conv_diff(x, w, stride=1):
    """``fpn_yardstick.parent_conv`` under autograd: ``F.unfold`` -> (M, C k k) -> ``ops.linear_or_torch`` (``_LinearFunction``)."""
    from bevformer_amd import ops
    k = w.shape[-1]
    B, C, H, Wd = x.shape
    Ho, Wo = Y.out_hw(H, Wd, stride)
    cols = F.unfold(x.contiguous(), k, padding=k // 2, stride=stride)
    cols = cols.permute(0, 2, 1).reshape(B * Ho * Wo, C * k * k).contiguous()
    y = ops.linear_or_torch(cols, w.reshape(w.shape[0], C * k * k))
    assert y.grad_fn is not None and "_LinearFunction" in type(y.grad_fn).__name__, \
        f"the parent's im2col GEMM did not take ops.linear's autograd path ({type(y.grad_fn).__name__})"
    return y.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)


def parent_conv_grads(g, y, x, w, bn, stride=1, relu=False, add=None, next_mask=None, next_bn=None):
    """``conv_bwd64``'s gradients on fp32 GPU maps with the parent's arithmetic in the GEMM mode in force."""
    x32, w32 = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    with torch.enable_grad():
        z = Y._bn(parent_conv_diff(x32, w32, stride), bn)
        gm = g * (y > 0).float() if relu else g
        dx, dw = torch.autograd.grad((z * gm).sum(), (x32, w32))
    return _finish(dx, add, next_mask, next_bn), dw


# ---- a bottleneck, a backbone

def _grads_of(module, loss):
    names, params = zip(*[(n, p) for n, p in module.named_parameters() if p.requires_grad])
    return dict(zip(names, torch.autograd.grad(loss, params, allow_unused=True)))


def block_grads64(block, x, g, need_x=True):
    """(out, dx or None, {name: dW}) of ``sum(g * block.forward_torch(x))`` in float64 autograd on a CPU deep copy."""
    b = copy.deepcopy(block).double().cpu()
    x64 = _d(x).requires_grad_(need_x)
    with torch.enable_grad():
        out = b.forward_torch(x64)
        loss = (out * _d(g)).sum()
        dx = torch.autograd.grad(loss, x64, retain_graph=True)[0] if need_x else None
        gw = _grads_of(b, loss)
    return out.detach(), dx, gw


def block_gz64(block, x, g):
    """(gz1, gz2, gz3) of a block with a plain conv2 in float64 on the CPU: the gradients of ``sum(g * block(x))`` w.r.t. the
    outputs of conv1, conv2 and conv3 — what the backward kernels read as operands."""
    b = copy.deepcopy(block).double().cpu()
    x = _d(x)
    with torch.enable_grad():
        z1 = b.conv1(x)
        z2 = b.conv2(torch.relu(b.bn1(z1)))
        z3 = b.conv3(torch.relu(b.bn2(z2)))
        idt = x if b.downsample is None else b.downsample(x)
        out = torch.relu(b.bn3(z3) + idt)
        return torch.autograd.grad((out * _d(g)).sum(), (z1, z2, z3))


def parent_block_diff(block, x):
    """``backbone_yardstick.parent_block`` for a block with a plain conv2 and norms in eval mode, under autograd."""
    norm = lambda m, y: Y._bn(y, Y._norm_of(m))
    conv = lambda c, y: parent_conv_diff(y, c.weight, c.stride[0])
    out = torch.relu(norm(block.bn1, conv(block.conv1, x)))
    out = torch.relu(norm(block.bn2, conv(block.conv2, out)))
    out = norm(block.bn3, conv(block.conv3, out))
    idt = x if block.downsample is None else norm(block.downsample[1], conv(block.downsample[0], x))
    return torch.relu(out + idt)


def parent_block_grads(block, x, g, need_x=True):
    """``block_grads64`` with the parent's arithmetic on fp32 GPU maps in the GEMM mode in force."""
    x32 = x.detach().clone().requires_grad_(need_x)
    with torch.enable_grad():
        out = parent_block_diff(block, x32)
        loss = (out * g).sum()
        dx = torch.autograd.grad(loss, x32, retain_graph=True)[0] if need_x else None
        gw = _grads_of(block, loss)
    return out.detach(), dx, gw


def pre_activations64(block, x):
    """The three ReLU inputs of a block with a plain conv2 in float64 on the CPU."""
    b = copy.deepcopy(block).double().cpu()
    x = _d(x)
    with torch.no_grad():
        p1 = b.bn1(b.conv1(x))
        p2 = b.bn2(b.conv2(torch.relu(p1)))
        idt = x if b.downsample is None else b.downsample(x)
        p3 = b.bn3(b.conv3(torch.relu(p2))) + idt
    return p1, p2, p3


class _RecordingReLU(torch.nn.Module):
    def __init__(self, sink):
        super().__init__()
        self.sink = sink

    def forward(self, x):
        self.sink.append(float((x.detach().abs() / x.detach().abs().max()).min()))
        return torch.relu(x)


def relu_margin64(net, x):
    """How close the closest ReLU input of a trainable block comes to its kink, in float64 on a CPU deep copy: the minimum over
    those blocks' ReLU inputs of |p| / max |p| of its tensor.  A forward in lower precision whose relative error stays well below
    this takes the same side of every kink, so its gradients differ from float64's by rounding alone."""
    n64 = copy.deepcopy(net).double().cpu()
    sink = []
    for name in n64.res_layers:
        for b in getattr(n64, name):
            if any(p.requires_grad for p in b.parameters()):
                b.relu = _RecordingReLU(sink)
    with torch.no_grad():
        Y._resnet(n64, _d(x), lambda b, y: b.forward_torch(y))
    return min(sink)


def keep_kinks_away_(net, x, gen, k=10.0):
    """Move every ReLU of ``net``'s trainable blocks away from its data, in place, from float64 arithmetic on the CPU alone.

    A random ResNet-50 has some 400,000 ReLU inputs in its trainable blocks; a forward in split precision (relative error about
    2e-5) lands on the other side of a few of those kinks, and ONE flipped mask moves the gradients below it by a percent — parent
    and fast path then both sit a hundred times above their rounding error and their ratio says nothing.  So each norm of a
    trainable block gets the running statistics of its own input on ``x`` (its normalised output then has zero mean and unit
    variance per channel), keeps its random gamma in [0.5, 1.5), and a beta of +k gamma (the channel passes its ReLU) or
    -(k gamma + the largest identity value of the channel) (it does not), the sign drawn per channel: a ReLU input comes
    close to zero only where the normalised value is k standard deviations out.  The masks still differ from channel to channel,
    and the blocks stay coupled through the identity; per-pixel masks are what the lattice and the operator tests check.  Walks
    the network block by block, so every statistic is the one the finished network produces."""
    n64 = copy.deepcopy(net).double().cpu()

    def calibrate(bn32, bn64, z, extra_max=None):
        m, v = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        on = torch.randint(0, 2, (z.shape[1],), generator=gen).bool()
        gamma = bn32.weight.detach().double()
        beta = torch.where(on, k * gamma, -(k * gamma + (extra_max if extra_max is not None else 0.0)))
        with torch.no_grad():
            bn32.running_mean.copy_(m), bn32.running_var.copy_((v - bn32.eps).clamp_min(1e-6)), bn32.bias.copy_(beta)
            for name in ("running_mean", "running_var", "bias"):            # float64 sees exactly the fp32 values
                getattr(bn64, name).copy_(getattr(bn32, name).double())

    with torch.no_grad():
        y = n64.maxpool(n64.relu(n64.bn1(n64.conv1(_d(x)))))
        for name in net.res_layers:
            for b32, b64 in zip(getattr(net, name), getattr(n64, name)):
                if any(p.requires_grad for p in b32.parameters()):
                    conv2 = b64.conv2.forward_torch if hasattr(b64.conv2, "conv_offset") else b64.conv2
                    z1 = b64.conv1(y)
                    calibrate(b32.bn1, b64.bn1, z1)
                    z2 = conv2(torch.relu(b64.bn1(z1)))
                    calibrate(b32.bn2, b64.bn2, z2)
                    idt = y
                    if b64.downsample is not None:
                        zd = b64.downsample[0](y)
                        calibrate(b32.downsample[1], b64.downsample[1], zd)
                        # (the identity of a block with a downsample has both signs: its ReLU-free norm is only standardised)
                        with torch.no_grad():
                            b32.downsample[1].bias.zero_(), b64.downsample[1].bias.zero_()
                        idt = b64.downsample[1](zd)
                    z3 = b64.conv3(torch.relu(b64.bn2(z2)))
                    hi = idt.amax((0, 2, 3)).clamp_min(0.0) - idt.amin((0, 2, 3)).clamp_max(0.0)
                    calibrate(b32.bn3, b64.bn3, z3, hi)
                    with torch.no_grad():       # an identity with negative values: lift the passing channels over them, too
                        lift = -idt.amin((0, 2, 3)).clamp_max(0.0)
                        b32.bn3.bias.add_(torch.where(b32.bn3.bias > 0, lift.float(), torch.zeros_like(b32.bn3.bias)))
                        b64.bn3.bias.copy_(b32.bn3.bias.double())
                y = b64.forward_torch(y)
    return net


def net_grads(net, x, gs):
    """{name: dW} of ``sum_i sum(gs[i] * net(x)[i])`` through the module's own ``forward`` in the modes in force."""
    with torch.enable_grad():
        outs = net(x)
        loss = sum((o * g).sum() for o, g in zip(outs, gs))
        return [o.detach() for o in outs], _grads_of(net, loss)


def net_grads64(net, x, gs):
    """``net_grads`` in float64 on a CPU deep copy with every block on ``forward_torch`` (norms in the state they are in)."""
    n64 = copy.deepcopy(net).double().cpu()
    with torch.enable_grad():
        outs = Y._resnet(n64, _d(x), lambda b, y: b.forward_torch(y))
        loss = sum((o * _d(g)).sum() for o, g in zip(outs, gs))
        return [o.detach() for o in outs], _grads_of(n64, loss)
