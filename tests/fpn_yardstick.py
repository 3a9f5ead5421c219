"""Yardstick of the image-neck fast path (``ops.conv_rows``, ``ops.fpn``): mmdet's FPN forward restated in float64 torch on
the CPU from a module's ``state_dict`` (``conv2d``, ``interpolate(size=, mode='nearest')``, the extra-level rules), and the
PARENT the error bound is measured from — the same neck with every convolution written as an explicit im2col matrix
(``F.unfold``, stride 1 or 2) put through ``ops.linear`` in the GEMM mode in force, the add and the upsampling in torch fp32:
the arithmetic of the commit before the kernel, using nothing that came with it.  The bound of every test: error against the
float64 yardstick <= 3 x the parent's error on the same inputs in the same mode.

The integer lattice: inputs, biases and residuals in {-4..4}, weights in {-2..2}.  Every product is then exact in bf16 and
every sum exact in fp32 while it stays below 2^24, so a kernel must EQUAL the float64 result; ``assert_lattice`` checks on
the CPU that the float64 sums are such integers, so that a failed comparison blames the kernel and not the inputs.  A whole
neck chains convolutions: what one convolution writes the next one reads and rounds to bf16 (``bf16`` mode) or to 16 bits
(``split``), so for a neck the lattice weights are SPARSE (``lattice_neck_``: two nonzero lateral weights, three nonzero
3 x 3 weights of magnitude 1 and one nonzero stride-2 weight per output channel), which keeps every intermediate an integer
of magnitude <= 256 = exactly a bf16 number: laterals <= 2*2*4 + 4 = 20, three summed levels <= 60, outputs <= 3*60 + 4 = 184,
extra levels <= 184 + 4 + 4 = 192 (``fpn64`` with ``check_lattice`` asserts it)."""
import torch
import torch.nn.functional as F

BF16_EXACT = 256.0


def _f64(t):
    return None if t is None else t.detach().double().cpu()


def max_err(got, want64):
    return (got.detach().double().cpu() - want64).abs().max().item()


def spec_of(neck):
    """The structural arguments of an FPN the restatements need."""
    return dict(n_in=len(neck.in_channels), start=neck.start_level, end=neck.backbone_end_level, num_outs=neck.num_outs,
                extra=neck.add_extra_convs, relu=bool(neck.relu_before_extra_convs))


def assert_lattice(t64, bound=float(1 << 24)):
    assert torch.equal(t64, t64.round()), "the yardstick's sums are not integers: the lattice inputs are wrong"
    assert t64.abs().max().item() <= bound, \
        f"the yardstick's sums reach {t64.abs().max().item()}: not exact in the kernel's number formats"


# ---- float64 yardstick

def conv64(x, w, b, stride=1, relu_in=False, res=None, res_up=False):
    """One convolution of the kernel's family on maps, float64 on the CPU: k x k with padding k // 2, optional input ReLU,
    bias, then ``+ res`` (same shape) or ``+ interpolate(res, size=, mode='nearest')``."""
    x, w, b, res = _f64(x), _f64(w), _f64(b), _f64(res)
    if relu_in:
        x = torch.relu(x)
    y = F.conv2d(x, w, b, stride=stride, padding=w.shape[-1] // 2)
    if res is not None:
        y = y + (F.interpolate(res, size=y.shape[2:], mode="nearest") if res_up else res)
    return y


def _fpn(sd, spec, inputs, conv, up, relu, check=None):
    n = spec["end"] - spec["start"]
    W = lambda pre, i: (sd[f"{pre}.{i}.conv.weight"], sd.get(f"{pre}.{i}.conv.bias"))
    lat = [conv(inputs[spec["start"] + i], *W("lateral_convs", i), 1, False) for i in range(n)]
    for i in range(n - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + up(lat[i], lat[i - 1].shape[2:])
    outs = [conv(lat[i], *W("fpn_convs", i), 1, False) for i in range(n)]
    if spec["num_outs"] > n:
        if not spec["extra"]:
            for _ in range(spec["num_outs"] - n):
                outs.append(F.max_pool2d(outs[-1], 1, stride=2))
        else:
            assert spec["extra"] == "on_output"
            outs.append(conv(outs[-1], *W("fpn_convs", n), 2, False))
            for i in range(n + 1, spec["num_outs"]):
                outs.append(conv(outs[-1], *W("fpn_convs", i), 2, spec["relu"]))
    if check is not None:
        for t in lat + outs:
            check(t)
    return outs


def fpn64(sd, spec, inputs, check_lattice=False):
    """mmdet's FPN forward from a ``state_dict`` in float64 on the CPU -> list of ``num_outs`` maps.  ``check_lattice``: every
    lateral sum and every output must be an integer of magnitude <= 256 (module docstring)."""
    sd = {k: _f64(v) for k, v in sd.items()}
    chk = (lambda t: assert_lattice(t, BF16_EXACT)) if check_lattice else None
    return _fpn(sd, spec, [_f64(x) for x in inputs], lambda x, w, b, s, r: conv64(x, w, b, s, r),
                lambda t, size: F.interpolate(t, size=size, mode="nearest"), torch.relu, chk)


# ---- the parent: im2col + ops.linear + torch fp32 statements (code of the commit before the kernel)

def parent_conv(x, w, b, stride=1, relu_in=False, res=None, res_up=False):
    """``conv64``'s convolution on fp32 GPU maps in the GEMM mode in force: ``F.unfold`` -> (M, C k k) -> ``ops.linear``."""
    from bevformer_amd import ops
    if relu_in:
        x = torch.relu(x)
    k = w.shape[-1]
    B, C, H, Wd = x.shape
    Ho, Wo = (H - 1) // stride + 1, (Wd - 1) // stride + 1
    cols = F.unfold(x.contiguous(), k, padding=k // 2, stride=stride)             # (B, C k k, Ho Wo), zero padded
    cols = cols.permute(0, 2, 1).reshape(B * Ho * Wo, C * k * k).contiguous()
    y = ops.linear(cols, w.reshape(w.shape[0], C * k * k).contiguous(), b)
    assert y is not None, "ops.linear declined the im2col GEMM"
    y = y.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)
    if res is not None:
        y = y + (F.interpolate(res, size=y.shape[2:], mode="nearest") if res_up else res)
    return y


def parent_fpn(sd, spec, inputs):
    """``fpn64``'s structure on the parent's convolution, fp32 on the GPU."""
    return _fpn(sd, spec, list(inputs), lambda x, w, b, s, r: parent_conv(x, w, b, s, r),
                lambda t, size: F.interpolate(t, size=size, mode="nearest"), torch.relu)


# ---- inputs

def lattice(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def lattice_neck_(neck, seed=0):
    """Sparse lattice parameters for every convolution of ``neck`` (in place; module docstring): per output channel two
    nonzero lateral weights in {-2, -1, 1, 2}, three nonzero 3 x 3 weights in {-1, 1}, one nonzero stride-2 weight in
    {-1, 1}; biases in {-4..4}."""
    g = torch.Generator().manual_seed(seed)
    n = len(neck.lateral_convs)
    with torch.no_grad():
        for group, convs, nnz, mag in (("lat", neck.lateral_convs, 2, 2), ("out", list(neck.fpn_convs)[:n], 3, 1),
                                       ("extra", list(neck.fpn_convs)[n:], 1, 1)):
            for cm in convs:
                w = cm.conv.weight
                flat = torch.zeros(w.shape[0], w[0].numel())
                for co in range(w.shape[0]):
                    idx = torch.randperm(flat.shape[1], generator=g)[:nnz]
                    val = torch.randint(1, mag + 1, (nnz,), generator=g).float() * (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1)
                    flat[co, idx] = val
                w.copy_(flat.reshape(w.shape))
                cm.conv.bias.copy_(lattice(cm.conv.bias.shape, -4, 4, g))
    return neck


def randomize_neck_(neck, seed=0):
    """Random weights at the scale that keeps every level O(1), random biases (in place)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight[0].numel() ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return neck
