"""Yardstick of BatchNorm with batch statistics on rows (``ops.bn_stats_rows``, ``ops.bn_apply_rows``, ``ops.bn_rows_backward``,
``ops.bottleneck_train`` under ``modes.bn_train``): the float64 truth, the PARENT the error bound is measured from, and the bound.

Truth: float64 on the CPU — ``torch.var_mean``, ``F.batch_norm(training=True)`` under autograd, and autograd through
``Bottleneck.forward_torch`` on a ``.double()`` deep copy in train mode.  The ReLU's mask of the operator tests is NOT recomputed: it
is taken from the ``y`` the test supplies (``y > 0``), so a test can place exact zeros (``backbone_train_yardstick.conv_bwd64``'s way).

Parent: what the commit before the kernels runs on the same GPU inputs in fp32 — torch's own ``torch.var_mean`` /
``F.batch_norm(training=True)`` statements and their autograd; for a block ``backbone_train_yardstick.parent_conv_diff``'s im2col
convolution through ``ops.linear_or_torch`` in the GEMM mode in force, with torch fp32 batch-norm, add and ReLU around it.

Bound (``bound``, ``check``): error against float64 <= 3 x the parent's error on the same inputs, the parent's error floored at
one fp32 ulp of the float64 tensor's largest magnitude (errors are maxima over a tensor, so the ulp is taken at the tensor's
scale): where torch lands within an ulp of the truth, three ulps is what fp32 can be held to.

Kinks.  A block in ``bf16`` mode has a forward error of some 1e-3 of its values, and a ReLU input inside that error takes another
side than float64's: one flipped mask moves the gradients below it by far more than rounding.  ``keep_kinks_away_`` therefore sets
every beta from float64 alone.  In train mode a norm's ``xhat`` is standardised by construction (zero mean, unit variance per
channel over the batch, |xhat| <= sqrt(M - 1)), so with gamma in [0.5, 1.5) and beta = +k gamma the channel passes its ReLU and
with beta = -(k gamma + the identity's largest value) it does not: a ReLU input is close to zero only where |xhat| comes
close to k.  The sign is drawn per channel; per-pixel masks are what the operator tests check with supplied ``y``."""
import copy
import functools
import math

import torch
import torch.nn.functional as F

import backbone_train_yardstick as T
import backbone_yardstick as Y
from backbone_yardstick import max_err  # noqa: F401  (re-exported for the tests)

BN = dict(type="BN")
KINK_K = 8.0
# |p| / max |p| of the closest ReLU input of every block case and of the net, from float64 on the CPU (asserted in
# tests/test_bn_train_cpu.py; measured there: the closest is 0.134 for a block, 0.040 for the net)
BLOCK_MARGIN, NET_MARGIN = 0.1, 0.03
# a forward in lower precision whose relative error stays this factor below the margin takes the same side of every kink.  The
# error is measured on the block's OUTPUT; the factor leaves room for a pre-activation whose error is that much larger
MARGIN_FACTOR = 10


def _d(t):
    return None if t is None else t.detach().double().cpu()


def ulp32(want):
    """One fp32 ulp at the largest magnitude of the float64 tensor ``want``."""
    m = float(want.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 and math.isfinite(m) else 2.0 ** -149


def bound(e_parent, want):
    return 3 * max(e_parent, ulp32(want))


def check(tag, got, parent, want, lines=None):
    """Print both errors and the bound of one tensor, then assert ``error <= bound``."""
    e_parent, e = max_err(parent, want), max_err(got, want)
    b = bound(e_parent, want)
    line = f"{tag}: E_parent {e_parent:.3e}  fused {e:.3e}  bound {b:.3e}"
    print(line)
    if lines is not None:
        lines.append(line)
    assert e <= b, line


# ---- one norm

def stats64(z):
    var, mean = torch.var_mean(_d(z), 0, unbiased=False)
    return mean, var


def parent_stats(z):
    var, mean = torch.var_mean(z, 0, unbiased=False)
    return mean, var


def _bn_grads(z, gamma, beta, eps, res, g, y, relu):
    """(out, dz, dgamma, dbeta, gy) of ``sum(g * act(batch_norm(z) + res))`` by autograd in the tensors' own dtype and device, the
    ReLU's mask taken from ``y``: (M, C) rows, normalised over the rows."""
    z, gamma, beta = (t.detach().clone().requires_grad_() for t in (z, gamma, beta))
    with torch.enable_grad():
        p = F.batch_norm(z, None, None, gamma, beta, True, 0.0, eps)
        if res is not None:
            p = p + res
        gy = g * (y > 0).to(g.dtype) if relu else g
        dz, dgamma, dbeta = torch.autograd.grad((p * gy).sum(), (z, gamma, beta))
    out = torch.relu(p.detach()) if relu else p.detach()
    return out, dz, dgamma, dbeta, gy


def bn64(z, bn, res, g, y, relu):
    return _bn_grads(_d(z), _d(bn.weight), _d(bn.bias), bn.eps, _d(res), _d(g), _d(y), relu)


def parent_bn(z, bn, res, g, y, relu):
    return _bn_grads(z, bn.weight, bn.bias, bn.eps, res, g, y, relu)


# ---- blocks

def _downsample(cin, cout, stride, norm_cfg):
    from bevformer_amd.modules.backbone import _build_norm
    return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False), _build_norm(norm_cfg, cout))


BLOCKS = ["plain", "stride2_pytorch", "stride2_caffe", "input_without_grad", "frozen_conv2", "frozen_affine"]
# kernel launches of one forward + backward (tags of the GEMM timer): forward 3 per convolution; backward 4 per convolution
# (reduce, apply, dW, dx) less what nobody asked for — the two input gradients into an input without gradient, the weight gradient
# of a frozen weight
N_LAUNCHES = {"plain": 9 + 12, "stride2_pytorch": 12 + 16, "stride2_caffe": 12 + 16, "input_without_grad": 12 + 14,
              "frozen_conv2": 9 + 11, "frozen_affine": 9 + 12}


def make_block(name):
    from bevformer_amd.modules import Bottleneck
    cfg = dict(type="BN", requires_grad=False) if name == "frozen_affine" else BN
    ds = lambda: _downsample(64, 256, 2, cfg)
    blk = {
        "plain": lambda: Bottleneck(256, 64, style="caffe", norm_cfg=cfg),
        "stride2_pytorch": lambda: Bottleneck(64, 64, stride=2, style="pytorch", downsample=ds(), norm_cfg=cfg),
        "stride2_caffe": lambda: Bottleneck(64, 64, stride=2, style="caffe", downsample=ds(), norm_cfg=cfg),
        "input_without_grad": lambda: Bottleneck(64, 64, stride=2, style="pytorch", downsample=ds(), norm_cfg=cfg),
        "frozen_conv2": lambda: Bottleneck(256, 64, style="caffe", norm_cfg=cfg),
        "frozen_affine": lambda: Bottleneck(256, 64, style="caffe", norm_cfg=cfg),
    }[name]()
    if name == "frozen_conv2":
        blk.conv2.weight.requires_grad = False
    return blk.train()


def randomize_(module, gen):
    """Random convolutions (``backbone_yardstick.randomize_convs_``) and, for every BatchNorm of any class, gamma in [0.5, 1.5) and
    random running statistics (in place)."""
    Y.randomize_convs_(module, gen)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5), m.bias.zero_()
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=gen) + 0.5)
    return module


def _set_beta(bn32, gen, k, extra=None, lift=None):
    on = torch.randint(0, 2, (bn32.num_features,), generator=gen).bool()
    gamma = bn32.weight.detach().double()
    zero = torch.zeros_like(gamma)
    beta = torch.where(on, k * gamma + (lift if lift is not None else zero), -(k * gamma + (extra if extra is not None else zero)))
    with torch.no_grad():
        bn32.bias.copy_(beta)


def _xhat64(bn, z):
    """The norm's standardised input in float64 (batch statistics)."""
    return F.batch_norm(z, None, None, None, None, True, 0.0, bn.eps)


def _kinks_block_(b32, y, gen, k):
    """``keep_kinks_away_`` for one block on its float64 input ``y`` -> the block's float64 output."""
    d = lambda p: p.detach().double()
    act = lambda bn, z: torch.relu(_xhat64(bn, z) * d(bn.weight).view(1, -1, 1, 1) + d(bn.bias).view(1, -1, 1, 1))
    conv = lambda c, t: F.conv2d(t, d(c.weight), None, c.stride, c.padding)
    z1 = conv(b32.conv1, y)
    _set_beta(b32.bn1, gen, k)
    z2 = conv(b32.conv2, act(b32.bn1, z1))
    _set_beta(b32.bn2, gen, k)
    idt = y
    if b32.downsample is not None:
        dn = b32.downsample[1]
        with torch.no_grad():
            dn.bias.zero_()                                 # (the ReLU-free norm of the identity: standardised, both signs)
        idt = _xhat64(dn, conv(b32.downsample[0], y)) * d(dn.weight).view(1, -1, 1, 1)
    z3 = conv(b32.conv3, act(b32.bn2, z2))
    hi = idt.amax((0, 2, 3)).clamp_min(0.0)
    lo = -idt.amin((0, 2, 3)).clamp_max(0.0)
    _set_beta(b32.bn3, gen, k, extra=hi, lift=lo)
    return torch.relu(_xhat64(b32.bn3, z3) * d(b32.bn3.weight).view(1, -1, 1, 1) + d(b32.bn3.bias).view(1, -1, 1, 1) + idt)


def keep_kinks_away_(module, x, gen, k=KINK_K):
    """Set every beta of a block, or of every block of a ResNet, from float64 arithmetic on the CPU alone (module docstring)."""
    with torch.no_grad():
        if hasattr(module, "res_layers"):
            n64 = copy.deepcopy(module).double().cpu()
            y = n64.maxpool(n64.relu(n64.bn1(n64.conv1(_d(x)))))
            for name in module.res_layers:
                for b in getattr(module, name):
                    y = _kinks_block_(b, y, gen, k)
        else:
            _kinks_block_(module, _d(x), gen, k)
    return module


def pre_activations64(block, x):
    """The three ReLU inputs of a block in train mode in float64 on the CPU (a deep copy: no running statistic moves)."""
    return T.pre_activations64(block, x)


def margin_of(tensors):
    return min(float(p.abs().min() / p.abs().max()) for p in tensors)


@functools.lru_cache(maxsize=None)
def block_case(name):
    """(block in train mode on the CPU, x, g) of a block case: random convolutions and gammas, betas that keep the kinks away."""
    gen = torch.Generator().manual_seed(300 + BLOCKS.index(name))
    blk = randomize_(make_block(name), gen)
    cin = blk.conv1.in_channels
    x = torch.randn(2, cin, 6, 10, generator=gen)
    keep_kinks_away_(blk, x, gen)
    s = 2 if blk.downsample is not None else 1
    g = torch.randn(2, 256, (6 - 1) // s + 1, (10 - 1) // s + 1, generator=gen)
    return blk, x, g


def parent_block_diff(block, x):
    """``backbone_train_yardstick.parent_block_diff`` for norms in train mode: the im2col convolution, then torch's fp32
    ``F.batch_norm(training=True)`` with the module's own vectors (its running statistics move as in the module path)."""
    norm = lambda m, y: F.batch_norm(y, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps)
    conv = lambda c, y: T.parent_conv_diff(y, c.weight, c.stride[0])
    out = torch.relu(norm(block.bn1, conv(block.conv1, x)))
    out = torch.relu(norm(block.bn2, conv(block.conv2, out)))
    out = norm(block.bn3, conv(block.conv3, out))
    idt = x if block.downsample is None else norm(block.downsample[1], conv(block.downsample[0], x))
    return torch.relu(out + idt)


def parent_block_grads(block, x, g, need_x=True):
    """(out, dx or None, {name: gradient}, {name: running statistic}) with the parent's arithmetic on a deep copy of ``block`` on
    fp32 GPU maps in the GEMM mode in force."""
    b = copy.deepcopy(block)
    x32 = x.detach().clone().requires_grad_(need_x)
    with torch.enable_grad():
        out = parent_block_diff(b, x32)
        loss = (out * g).sum()
        dx = torch.autograd.grad(loss, x32, retain_graph=True)[0] if need_x else None
        gw = T._grads_of(b, loss)
    return out.detach(), dx, gw, running_of(b)


def running_of(module):
    return {n: t.detach().clone() for n, t in module.named_buffers() if n.endswith(("running_mean", "running_var"))}


def block_grads64(block, x, g, need_x=True):
    """``backbone_train_yardstick.block_grads64`` plus the running statistics of the float64 copy after its forward."""
    b = copy.deepcopy(block).double().cpu()
    x64 = _d(x).requires_grad_(need_x)
    with torch.enable_grad():
        out = b.forward_torch(x64)
        loss = (out * _d(g)).sum()
        dx = torch.autograd.grad(loss, x64, retain_graph=True)[0] if need_x else None
        gw = T._grads_of(b, loss)
    return out.detach(), dx, gw, running_of(b)


# ---- the net

def make_net(norm_type="SyncBN"):
    """A ResNet-50 like tests/test_backbone_train_gpu.py's, nothing frozen, every norm in train mode: the bevformerv2 backbone's
    settings at base_channels=32."""
    from bevformer_amd.modules import ResNet
    gen = torch.Generator().manual_seed(43)
    net = ResNet(depth=50, base_channels=32, stem_channels=64, frozen_stages=-1, norm_eval=False, norm_cfg=dict(type=norm_type, requires_grad=True),
                 style="caffe", out_indices=(1, 2, 3), zero_init_residual=False)
    randomize_(net, gen).train()
    x = torch.randn(2, 3, 64, 64, generator=gen)
    keep_kinks_away_(net, x, gen)
    gs = [torch.randn(2, c, s, s, generator=gen) for c, s in ((256, 8), (512, 4), (1024, 2))]
    return net, x, gs


def parent_net_grads(net, x, gs):
    """The backbone with the parent's operators on a deep copy: the stem on torch, every block as ``parent_block_diff``."""
    n = copy.deepcopy(net)
    with torch.enable_grad():
        outs = Y._resnet(n, x, parent_block_diff)
        loss = sum((o * g).sum() for o, g in zip(outs, gs))
        return [o.detach() for o in outs], T._grads_of(n, loss)


def net_grads64(net, x, gs):
    return T.net_grads64(net, x, gs)


def net_margin64(net, x):
    return T.relu_margin64(net, x)
