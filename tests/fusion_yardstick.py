"""Yardstick of the temporal-fusion fast path (``ops.conv3x3_bn``, ``ops.resnet_fusion``): a float64 CPU restatement of
``ResNetFusion`` taken from a module's ``state_dict`` (``torch.nn.functional.conv2d``, the BatchNorm formula, ReLU, Linear,
LayerNorm), and the PARENT the error bound is measured from — the same convolution written as an explicit im2col matrix
(``unfold``, zero padded, (M, 9 C_in)) put through ``ops.linear``, followed by torch fp32 statements for BatchNorm, residual
and ReLU.  The bound of every test: error against the float64 yardstick <= 3 x the parent's error on the same inputs in the
same GEMM mode."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
LN_EPS = 1e-5


def rows_to_maps(rows, H, W):
    """(bs, H W, C) -> (bs, C, H, W)."""
    return rows.reshape(rows.shape[0], H, W, rows.shape[-1]).permute(0, 3, 1, 2)


def maps_to_rows(maps):
    """(bs, C, H, W) -> (bs, H W, C)."""
    return maps.flatten(2).permute(0, 2, 1)


def _f64(t):
    return t.detach().double().cpu()


# ---- float64 yardstick

def conv_sum64(rows, H, W, weight):
    """The bare 3 x 3 convolution (padding 1) of float64 rows (bs, H W, C) -> (bs, H W, C_out), float64 on the CPU."""
    return maps_to_rows(F.conv2d(rows_to_maps(_f64(rows), H, W), _f64(weight), padding=1))


def bn64(y, gamma, beta, mean, var, eps):
    return (y - _f64(mean)) / torch.sqrt(_f64(var) + eps) * _f64(gamma) + _f64(beta)


def conv_bn64(rows, H, W, weight, gamma, beta, mean, var, eps, relu, res=None, conv=None):
    """act(bn(conv(rows)) + res) in float64; ``conv``: a precomputed ``conv_sum64`` of the same inputs."""
    y = bn64(conv if conv is not None else conv_sum64(rows, H, W, weight), gamma, beta, mean, var, eps)
    if res is not None:
        y = y + _f64(res)
    return y.clamp_min(0) if relu else y


def _bn_of(sd, prefix):
    return (sd[prefix + ".weight"], sd[prefix + ".bias"], sd[prefix + ".running_mean"], sd[prefix + ".running_var"])


def fusion64(sd, rows, H, W, bn_eps=BN_EPS, ln_eps=LN_EPS):
    """``ResNetFusion`` from its ``state_dict`` on the frames' rows (list of (bs, H W, C)) -> (bs, H W, out) float64."""
    x = torch.cat([_f64(r) for r in rows], -1)
    i = 0
    while f"layers.{i}.conv1.weight" in sd:
        p = f"layers.{i}."
        if p + "downsample.0.weight" in sd:
            identity = conv_bn64(x, H, W, sd[p + "downsample.0.weight"], *_bn_of(sd, p + "downsample.1"), bn_eps, False)
        else:
            identity = x
        out = conv_bn64(x, H, W, sd[p + "conv1.weight"], *_bn_of(sd, p + "bn1"), bn_eps, True)
        x = conv_bn64(out, H, W, sd[p + "conv2.weight"], *_bn_of(sd, p + "bn2"), bn_eps, True, res=identity)
        i += 1
    y = F.linear(x, _f64(sd["layer_norm.0.weight"]), _f64(sd["layer_norm.0.bias"]))
    return F.layer_norm(y, (y.shape[-1],), _f64(sd["layer_norm.1.weight"]), _f64(sd["layer_norm.1.bias"]), ln_eps)


# ---- the parent: im2col + ops.linear + torch fp32 statements (code of the commit before the convolution kernel)

def parent_conv_bn(rows, H, W, weight, gamma, beta, mean, var, eps, relu, res=None):
    """``rows`` (bs, H W, C) fp32 on the GPU (already concatenated) -> (bs, H W, C_out) fp32 in the GEMM mode in force."""
    from bevformer_amd import ops
    bs, HW, C = rows.shape
    cols = F.unfold(rows_to_maps(rows, H, W).contiguous(), 3, padding=1)           # (bs, C * 9, H W), zero padded
    cols = cols.permute(0, 2, 1).reshape(bs * HW, C * 9).contiguous()
    y = ops.linear(cols, weight.reshape(weight.shape[0], C * 9).contiguous())
    assert y is not None, "ops.linear declined the im2col GEMM"
    y = (y - mean) / torch.sqrt(var + eps) * gamma + beta
    y = y.reshape(bs, HW, -1)
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def parent_fusion(sd, rows, H, W, bn_eps=BN_EPS, ln_eps=LN_EPS):
    """``fusion64``'s structure on the parent's convolution, fp32 on the GPU; Linear through ``ops.linear``, LayerNorm torch."""
    from bevformer_amd import ops
    x = torch.cat(list(rows), -1)
    i = 0
    while f"layers.{i}.conv1.weight" in sd:
        p = f"layers.{i}."
        if p + "downsample.0.weight" in sd:
            identity = parent_conv_bn(x, H, W, sd[p + "downsample.0.weight"], *_bn_of(sd, p + "downsample.1"), bn_eps, False)
        else:
            identity = x
        out = parent_conv_bn(x, H, W, sd[p + "conv1.weight"], *_bn_of(sd, p + "bn1"), bn_eps, True)
        x = parent_conv_bn(out, H, W, sd[p + "conv2.weight"], *_bn_of(sd, p + "bn2"), bn_eps, True, res=identity)
        i += 1
    y = ops.linear(x, sd["layer_norm.0.weight"], sd["layer_norm.0.bias"])
    assert y is not None, "ops.linear declined the output projection"
    return F.layer_norm(y, (y.shape[-1],), sd["layer_norm.1.weight"], sd["layer_norm.1.bias"], ln_eps)


def max_err(got, want64):
    return (got.detach().double().cpu() - want64).abs().max().item()


def randomize_bn(module, seed=0):
    """Non-trivial affine parameters and running statistics for every BatchNorm of ``module`` (in place)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                n = m.num_features
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
    return module
