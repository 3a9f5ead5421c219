"""BatchNorm with BATCH statistics over channel-last rows (csrc/batchnorm_rows.h), for a backbone whose norms are in ``train()`` mode
(the bevformerv2 configs: ``norm_eval=False``, ``SyncBN``): ``bn_stats_rows`` (the per-channel mean and biased variance of (M, C)
rows, the module's running statistics and ``num_batches_tracked`` updated by the same call), ``bn_apply_rows``
(``act(xhat * gamma + beta + res)``), ``bn_rows_backward`` (``dz``, ``dgamma``, ``dbeta`` and the masked gradient ``gy``: two
launches) and ``conv_raw_rows`` (the bare convolution ``z = conv(x)`` from the row convolution + BatchNorm kernel with an identity
norm).  All statistics arithmetic is fp32 whatever the GEMM mode, and deterministic: no atomics, two calls give the same bits.

With ``modes.bn_train`` (together with ``modes.backbone_train``) ``ops.bottleneck_train`` covers a block whose norms are all in
``train()`` mode as ONE autograd Function on these kernels (``_BottleneckTrainBN``): per convolution three launches forward —
the raw convolution, the statistics, the apply — and four backward — the reduce, the apply, the weight gradient, the input
gradient."""
import torch
import torch.nn as nn

from .. import _lib
from ..ext import _ptr
from ._base import _forward_modes, _gemm_ctx, _launch, _m, _optr
from .backbone import _block_convs, _need, _out_hw, _pair
from .conv import CONV_GRAN, CONV_MAX_ROWS, _norm_reject
from .gemm import _pkg, _rows2d
from .neck import map_of_rows, rows_of_map


def _f32_cuda(*tensors):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _vec_ok(v, C):
    return torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == C \
        and v.data_ptr() % 16 == 0


def _bn_rows(t, C):
    """``t`` (..., C) as the kernels' (M, C) operand -> (2-D view, row stride), or ``None`` when M is outside 2 .. 2^24."""
    t2, ld = _rows2d(t, C)
    return (t2, ld) if 2 <= t2.shape[0] <= CONV_MAX_ROWS else None


def _bn_workspace(device, M, C):
    """The slab the two reductions merge their per-workgroup partials through (``bevmsda_bn_rows_workspace_bytes``): fresh per
    call from torch's allocator, so that a captured graph owns its own."""
    nbytes = int(_lib.load().bevmsda_bn_rows_workspace_bytes(M, C))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _out_rows(out, M, C, device):
    if out is None:
        return torch.empty((M, C), dtype=torch.float32, device=device)
    if out.dim() != 2 or tuple(out.shape) != (M, C) or out.stride(1) != 1:
        return None
    return out


def bn_stats_rows(z, bn=None, *, update_running=True, tag="bn_stats_rows"):
    """``(mean, var)`` of the (M, C) rows ``z`` per channel — ``var`` the BIASED variance, as ``F.batch_norm`` normalises with — in
    one C call (``bevmsda_bn_stats_rows_f32``; Chan's merge, no ``E[z^2] - E[z]^2``, bit-reproducible).  With a BatchNorm module
    ``bn`` and ``update_running`` the same call updates ``bn.running_mean`` / ``bn.running_var`` (unbiased, ``bn.momentum``) and
    ``bn.num_batches_tracked`` in place, as one training forward of the module does.  Returns two (C) vectors (views of one
    (2, C) tensor), or ``None`` when the call is not covered: not CUDA fp32, grad mode on, C no multiple of 32, M outside 2 .. 2^24,
    ``momentum=None``."""
    if torch.is_grad_enabled() or not _f32_cuda(z) or z.dim() < 2:
        return None
    C = int(z.shape[-1])
    if C == 0 or C % CONV_GRAN:
        return None
    zz = _bn_rows(z, C)
    if zz is None:
        return None
    z2, ldz = zz
    M = z2.shape[0]
    rm = rv = nbt = None
    momentum = 0.0
    if bn is not None and update_running:
        if _norm_reject(bn) is not None or bn.num_features != C or bn.momentum is None:
            return None
        rm, rv, nbt, momentum = bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.momentum)
        if not (_vec_ok(rm, C) and _vec_ok(rv, C)):
            return None
        if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64 and nbt.numel() == 1):
            return None
    ws = _bn_workspace(z.device, M, C)
    if ws is None:
        return None
    mv = torch.empty((2, C), dtype=torch.float32, device=z.device)
    # algorithmic bytes: the rows once, the two vectors (the running pair read and written)
    timer = _gemm_ctx(tag, 4.0 * M * C, 4.0 * (M * C + 2 * C + (4 * C if rm is not None else 0)))
    ok = _launch(z.device, "bn_stats_rows", lambda lib, stream: lib.bevmsda_bn_stats_rows_f32(
        _ptr(z2), ldz, M, C, _ptr(mv[0]), _ptr(mv[1]), _optr(rm), _optr(rv), _optr(nbt), momentum, _ptr(ws), stream), timer=timer)
    return (mv[0], mv[1]) if ok else None


def _affine_ok(bn, C):
    return _norm_reject(bn) is None and bn.num_features == C and _vec_ok(bn.weight, C) and _vec_ok(bn.bias, C)


def bn_apply_rows(z, mean, var, bn, *, relu=False, res=None, out=None, tag="bn_apply_rows"):
    """``act((z - mean) / sqrt(var + bn.eps) * bn.weight + bn.bias + res)`` over (M, C) rows in one launch
    (``bevmsda_bn_apply_rows_f32``): ``mean`` / ``var`` the (C) batch statistics of ``bn_stats_rows`` (the kernel forms the inverse
    standard deviation: nothing is derived on the host), ``res`` optional (M, C) rows, ReLU when ``relu`` (a NaN stays NaN).
    ``out``: an optional (M, C) destination with unit column stride, which may be ``z`` itself.  Returns the rows, or ``None`` when
    the call is not covered."""
    tensors = [z, mean, var] + [t for t in (res, out) if t is not None]
    if torch.is_grad_enabled() or not _f32_cuda(*tensors) or z.dim() < 2:
        return None
    C = int(z.shape[-1])
    if C == 0 or C % CONV_GRAN or not _affine_ok(bn, C) or not (_vec_ok(mean, C) and _vec_ok(var, C)):
        return None
    zz = _bn_rows(z, C)
    if zz is None:
        return None
    z2, ldz = zz
    M = z2.shape[0]
    if res is not None and (res.shape[-1] != C or res.numel() != M * C):
        return None
    y = _out_rows(out, M, C, z.device)
    if y is None or y.stride(0) % 4 or y.data_ptr() % 16:
        return None
    r2, ldres = _rows2d(res, C) if res is not None else (None, 0)
    timer = _gemm_ctx(tag, 4.0 * M * C, 4.0 * (M * C * (3 if res is not None else 2) + 4 * C))
    return y if _launch(z.device, "bn_apply_rows", lambda lib, stream: lib.bevmsda_bn_apply_rows_f32(
        _ptr(z2), ldz, _ptr(mean), _ptr(var), _ptr(bn.weight), _ptr(bn.bias), float(bn.eps), _optr(r2), ldres, int(bool(relu)), M, C,
        _ptr(y), y.stride(0), stream), timer=timer) else None


def bn_rows_backward(g, y, z, mean, var, bn, *, relu=False, gy_out=None, dz_out=None, tag="bn_rows_backward"):
    """The backward of ``bn_apply_rows`` THROUGH the batch statistics, two launches: ``g`` (M, C) the gradient w.r.t. the output
    ``y`` of ``act(bn(z) + res)``; with ``gy = g * (y > 0)`` (``relu=False`` or ``y=None``: ``gy = g``)

    * ``bevmsda_bn_bwd_reduce_rows_f32`` (tag + "_reduce"): ``dbeta = sum gy`` and ``dgamma = sum gy * xhat`` — deterministic;
    * ``bevmsda_bn_bwd_apply_rows_f32`` (tag + "_apply"): ``dz = gamma * invstd * (gy - dbeta / M - xhat * dgamma / M)``, and
      ``gy`` itself — the gradient of the residual branch — into ``gy_out`` (a destination with unit column stride, or ``True``
      for fresh rows).

    ``dz_out``: an optional destination with unit column stride (its row stride may exceed C).  Returns ``(dz, dgamma, dbeta)``,
    with ``gy_out`` ``(dz, dgamma, dbeta, gy)``, or ``None`` when the call is not covered."""
    mask = y if relu else None
    want_gy = gy_out is not None and gy_out is not False
    tensors = [g, z, mean, var] + [t for t in (mask, dz_out, gy_out if torch.is_tensor(gy_out) else None) if t is not None]
    if torch.is_grad_enabled() or not _f32_cuda(*tensors) or z.dim() < 2:
        return None
    C = int(z.shape[-1])
    if C == 0 or C % CONV_GRAN or _norm_reject(bn) is not None or bn.num_features != C or not _vec_ok(bn.weight, C) \
            or not (_vec_ok(mean, C) and _vec_ok(var, C)):
        return None
    zz = _bn_rows(z, C)
    if zz is None:
        return None
    z2, ldz = zz
    M = z2.shape[0]
    for t in (g, mask):
        if t is not None and (t.shape[-1] != C or t.numel() != M * C):
            return None
    g2, ldg = _rows2d(g, C)
    y2, ldy = _rows2d(mask, C) if mask is not None else (None, 0)
    dz = _out_rows(dz_out, M, C, z.device)
    gy = _out_rows(gy_out if torch.is_tensor(gy_out) else None, M, C, z.device) if want_gy else None
    if dz is None or (want_gy and gy is None) or any(t is not None and (t.stride(0) % 4 or t.data_ptr() % 16) for t in (dz, gy)):
        return None
    ws = _bn_workspace(z.device, M, C)
    if ws is None:
        return None
    sums = torch.empty((2, C), dtype=torch.float32, device=z.device)
    eps = float(bn.eps)
    nmask = 1 if mask is not None else 0
    timer = _gemm_ctx(tag + "_reduce", 6.0 * M * C, 4.0 * (M * C * (2 + nmask) + 4 * C))
    if not _launch(z.device, "bn_bwd_reduce_rows", lambda lib, stream: lib.bevmsda_bn_bwd_reduce_rows_f32(
            _ptr(g2), ldg, _optr(y2), ldy, _ptr(z2), ldz, _ptr(mean), _ptr(var), eps, M, C, _ptr(sums), _ptr(ws), stream), timer=timer):
        return None
    timer = _gemm_ctx(tag + "_apply", 8.0 * M * C, 4.0 * (M * C * (3 + nmask + (1 if want_gy else 0)) + 5 * C))
    if not _launch(z.device, "bn_bwd_apply_rows", lambda lib, stream: lib.bevmsda_bn_bwd_apply_rows_f32(
            _ptr(g2), ldg, _optr(y2), ldy, _ptr(z2), ldz, _ptr(mean), _ptr(var), _ptr(bn.weight), eps, _ptr(sums), M, C,
            _ptr(dz), dz.stride(0), _optr(gy), gy.stride(0) if gy is not None else 0, stream), timer=timer):
        return None
    return (dz, sums[1], sums[0], gy) if want_gy else (dz, sums[1], sums[0])


# ---- the bare convolution z = conv(x): the row convolution + BatchNorm kernel with an identity norm

_IDENTITY_NORMS = {}


def _identity_norm(device, C):
    """A BatchNorm in eval mode with gamma = 1, beta = 0, mean = 0, var = 1 and eps = 0, cached per (device, C):
    ``bevmsda_conv_bn_rows_f32`` then computes ``acc * (1 / sqrt(1 + 0)) + (0 - 0 * 1)`` — the accumulator itself."""
    key = (torch.device(device), int(C))
    bn = _IDENTITY_NORMS.get(key)
    if bn is None:
        bn = nn.BatchNorm2d(int(C), eps=0.0).to(device).eval()
        for p in bn.parameters():
            p.requires_grad = False
        _IDENTITY_NORMS[key] = bn
    return bn


def conv_raw_rows(rows, n_img, hw, weight, *, stride=1, out=None, tag="conv_raw_rows"):
    """``conv(x)`` over channel-last rows without a norm, on ``conv_bn_rows``'s kernel, shape rules, strides and weight images:
    that call with a cached identity norm (``_identity_norm``).  Returns (n_img Ho Wo, C_out) rows, or ``None`` when the call is
    not covered."""
    if not torch.is_tensor(weight) or weight.dim() != 4:
        return None
    return _pkg().conv_bn_rows(rows, n_img, hw, weight, _identity_norm(rows.device, weight.shape[0]), stride=stride, out=out, tag=tag)


# ---- a bottleneck whose norms run on batch statistics, as one autograd Function

class _BottleneckTrainBN(torch.autograd.Function):
    """A whole bottleneck with norms in ``train()`` mode as one node (``bottleneck_train`` with ``modes.bn_train``).  ``params``: the
    block's convolution weights in ``_block_convs``'s order, then each norm's ``weight`` and ``bias`` in the same order."""

    @staticmethod
    def forward(ctx, x, block, *params):
        ops = _pkg()
        B, _, H, W = x.shape
        hw = (int(H), int(W))
        rows = rows_of_map(x)
        convs = _block_convs(block)

        def cbn(r, hw_in, c, n, relu, name, res=None):
            s = _pair(c.stride)[0]
            z = _need(ops.conv_raw_rows(r, B, hw_in, c.weight, stride=s, tag=f"bottleneck_{name}"))
            mean, var = _need(ops.bn_stats_rows(z, n, tag=f"bottleneck_{name}_stats"))
            o = _need(ops.bn_apply_rows(z, mean, var, n, relu=relu, res=res, tag=f"bottleneck_{name}_apply"))
            return z, mean, var, o, _out_hw(hw_in, s)

        z1, m1, v1, o1, hw1 = cbn(rows, hw, *convs[0], True, "conv1")
        z2, m2, v2, o2, hw2 = cbn(o1, hw1, *convs[1], True, "conv2")
        extra = ()
        idt = rows
        if len(convs) == 4:
            zd, md, vd, idt, _ = cbn(rows, hw, *convs[3], False, "downsample")
            extra = (zd, md, vd)
        z3, m3, v3, o3, hw3 = cbn(o2, hw2, *convs[2], True, "conv3", res=idt)
        out = map_of_rows(o3, B, hw3)
        ctx.block, ctx.modes, ctx.geom = block, _m().snapshot(), (B, hw, hw1, hw2)
        ctx.save_for_backward(rows, out, z1, m1, v1, o1, z2, m2, v2, o2, z3, m3, v3, *extra, *params)
        return out

    @staticmethod
    @_forward_modes
    def backward(ctx, g):
        ops, block = _pkg(), ctx.block
        B, hw, hw1, hw2 = ctx.geom
        saved = ctx.saved_tensors
        rows, out = saved[0], rows_of_map(saved[1])
        z1, m1, v1, o1, z2, m2, v2, o2, z3, m3, v3 = saved[2:13]
        convs = _block_convs(block)
        (c1, n1), (c2, n2), (c3, n3) = convs[:3]
        ds = convs[3] if len(convs) == 4 else None
        nc = len(convs)
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[2:2 + nc]
        need_a = ctx.needs_input_grad[2 + nc:2 + 3 * nc]              # (gamma, beta) per norm
        affine = lambda i: need_a[2 * i] or need_a[2 * i + 1]
        need1 = need_x or need_w[0] or affine(0)                      # does anything at or ahead of bn1 want a gradient?
        need_d = ds is not None and (need_x or need_w[3] or affine(3))
        sizes = [c.weight.numel() if nw else 0 for (c, _), nw in zip(convs, need_w)]
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=rows.device) if sum(sizes) else None     # one zero fill
        dws, o = [], 0
        for (c, _), n in zip(convs, sizes):
            dws.append(flat[o:o + n].view(c.weight.shape) if n else None)
            o += n
        bn_bwd = lambda *a, **k: _need(ops.bn_rows_backward(*a, **k))
        conv_bwd = lambda *a, **k: _need(ops.conv_bn_rows_backward(*a, **k))
        dgs = [None] * (2 * nc)

        def keep(i, dgamma, dbeta):
            dgs[2 * i], dgs[2 * i + 1] = (dgamma if need_a[2 * i] else None), (dbeta if need_a[2 * i + 1] else None)

        # conv3: its norm's backward also writes gy = g * (out > 0), the gradient of the identity branch
        want_gy = need_x if ds is None else need_d
        r = bn_bwd(rows_of_map(g), out, z3, m3, v3, n3, relu=True, gy_out=True if want_gy else None, tag="bottleneck_conv3_bn")
        dz3, gy = r[0], (r[3] if want_gy else None)
        keep(2, r[1], r[2])
        g2, _ = conv_bwd(dz3, None, o2, B, hw2, c3.weight, None, need_dw=need_w[2], dw_out=dws[2], tag="bottleneck_conv3")
        r = bn_bwd(g2, o2, z2, m2, v2, n2, relu=True, tag="bottleneck_conv2_bn")
        keep(1, r[1], r[2])
        g1, _ = conv_bwd(r[0], None, o1, B, hw1, c2.weight, None, stride=_pair(c2.stride)[0], need_dx=need1, need_dw=need_w[1],
                         dw_out=dws[1], tag="bottleneck_conv2")
        dx = None
        if need1:
            r = bn_bwd(g1, o1, z1, m1, v1, n1, relu=True, tag="bottleneck_conv1_bn")
            keep(0, r[1], r[2])
            if need_x or need_w[0]:
                dx, _ = conv_bwd(r[0], None, rows, B, hw, c1.weight, None, stride=c1.stride[0], need_dx=need_x, need_dw=need_w[0],
                                 dw_out=dws[0], add=gy if ds is None else None, tag="bottleneck_conv1")
        if need_d:
            zd, md, vd = saved[13:16]
            r = bn_bwd(gy, None, zd, md, vd, ds[1], relu=False, tag="bottleneck_downsample_bn")
            keep(3, r[1], r[2])
            if need_x or need_w[3]:
                dx, _ = conv_bwd(r[0], None, rows, B, hw, ds[0].weight, None, stride=ds[0].stride[0], need_dx=need_x, need_dw=need_w[3],
                                 dw_out=dws[3], add=dx, dx_out=dx, tag="bottleneck_downsample")
        return (map_of_rows(dx, B, hw) if need_x else None, None, *dws, *dgs)


def _bottleneck_train_bn(block, x):
    convs = _block_convs(block)
    return _BottleneckTrainBN.apply(x, block, *(c.weight for c, _ in convs), *(p for _, n in convs for p in (n.weight, n.bias)))
