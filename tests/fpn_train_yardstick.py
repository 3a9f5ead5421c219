"""Yardstick of the neck's training path (``ops.fpn_train``, ``modes.fpn_train``, the options of ``ops.conv_bn_rows_backward``): the
float64 truth of the gradients and the PARENT the error bound is measured from.

The truth is float64 autograd on the CPU through the ``forward_torch`` of a ``.double()`` deep copy of the module
(``neck_grads64``).  ``neck_reads64`` restates the same forward on ``fpn_yardstick._fpn``'s structure to get at what the backward
kernels READ: the levels, and the gradients with respect to the summed laterals and to every level (a level's own output gradient
plus what the next extra convolution sends back).

The parent is float32 autograd through ``fpn_yardstick._fpn``'s structure with ``backbone_train_yardstick.parent_conv_diff`` as
the convolution — the differentiable im2col GEMM through ``ops.linear``'s autograd path in the GEMM mode in force, the code of the
commit before the kernels — and the bias, the add, the upsampling and the ReLU as torch fp32 statements.  The bound of every
error test: error against float64 <= 3 x the parent's error on the same inputs in the same mode."""
import copy

import torch
import torch.nn.functional as F

import backbone_train_yardstick as T
import fpn_yardstick as Y
from fpn_yardstick import max_err  # noqa: F401  (re-exported for the tests)


def _d(t):
    return None if t is None else t.detach().double().cpu()


def _named_grads(module, loss):
    names, params = zip(*[(n, p) for n, p in module.named_parameters() if p.requires_grad])
    return dict(zip(names, torch.autograd.grad(loss, params, allow_unused=True)))


def neck_grads64(neck, inputs, gs, need_x=True):
    """(outs, [dx per input or None], {name: gradient}) of ``sum_i sum(gs[i] * neck.forward_torch(inputs)[i])`` in float64 autograd
    on a CPU deep copy."""
    n64 = copy.deepcopy(neck).double().cpu()
    xs = [_d(x).requires_grad_(need_x) for x in inputs]
    with torch.enable_grad():
        outs = n64.forward_torch(xs)
        loss = sum((o * _d(g)).sum() for o, g in zip(outs, gs))
        dxs = list(torch.autograd.grad(loss, xs, retain_graph=True, allow_unused=True)) if need_x else [None] * len(xs)
        gw = _named_grads(n64, loss)
    return [o.detach() for o in outs], dxs, gw


def neck_reads64(neck, inputs, gs):
    """What the backward kernels read, in float64 on the CPU: (levels, gradients w.r.t. the summed laterals, gradients w.r.t.
    every level) — the levels being the summed laterals, the outputs and the extra levels."""
    sd = {k: _d(v) for k, v in neck.state_dict().items()}
    seen = []
    with torch.enable_grad():
        xs = [_d(x).requires_grad_() for x in inputs]
        conv = lambda x, w, b, s, r: F.conv2d(torch.relu(x) if r else x, w, b, stride=s, padding=w.shape[-1] // 2)
        outs = Y._fpn(sd, Y.spec_of(neck), xs, conv, lambda t, size: F.interpolate(t, size=size, mode="nearest"), torch.relu,
                      seen.append)
        n = len(seen) - len(outs)
        loss = sum((o * _d(g)).sum() for o, g in zip(outs, gs))
        grads = torch.autograd.grad(loss, seen)
    return [t.detach() for t in seen], list(grads[:n]), list(grads[n:])


def parent_neck_grads(neck, inputs, gs, need_x=True):
    """``neck_grads64`` with the parent's arithmetic on fp32 GPU maps in the GEMM mode in force."""
    xs = [x.detach().clone().requires_grad_(need_x) for x in inputs]
    sd = dict(neck.named_parameters())

    def conv(x, w, b, stride, relu_in):
        y = T.parent_conv_diff(torch.relu(x) if relu_in else x, w, stride)
        return y if b is None else y + b.view(1, -1, 1, 1)

    with torch.enable_grad():
        outs = Y._fpn(sd, Y.spec_of(neck), xs, conv, lambda t, size: F.interpolate(t, size=size, mode="nearest"), torch.relu)
        loss = sum((o * g).sum() for o, g in zip(outs, gs))
        dxs = list(torch.autograd.grad(loss, xs, retain_graph=True, allow_unused=True)) if need_x else [None] * len(xs)
        gw = _named_grads(neck, loss)
    return [o.detach() for o in outs], dxs, gw


def first_extra_pre_relu64(neck, inputs):
    """The first extra level (the one input a ReLU of the neck reads) in float64 on the CPU, or ``None`` when the neck has no
    ReLU."""
    n = len(neck.lateral_convs)
    if not (neck.relu_before_extra_convs and neck.num_outs > n + 1):
        return None
    outs = Y.fpn64(neck.state_dict(), Y.spec_of(neck), inputs)
    return outs[n]
