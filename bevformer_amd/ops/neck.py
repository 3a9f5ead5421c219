"""The image neck on the channel-last row convolution kernel (csrc/conv_rows.h): ``conv_rows`` (1 x 1 / 3 x 3 / 3 x 3 stride-2
convolution over (n_img H W, C) rows with bias, input ReLU and a same-shape or 2 x nearest upsampled residual in the
epilogue), ``fpn`` (the schedule of an FPN: mmdet's class, or ``modules.neck.FPN``) and ``fpn_reject`` (why a module or call is
not covered).  ``fpn_train`` (the neck as one autograd Function on the backward kernels of csrc/conv_bwd_rows.h) and
``fpn_train_reject`` are the training path; the rest is inference only.

Layout: the kernel computes in rows, so a level's output IS ``(B, h, w, C)`` memory; ``fpn`` hands it out as the NCHW-shaped
view ``rows.view(B, h, w, C).permute(0, 3, 1, 2)`` (what ``torch.channels_last`` calls dense), ``flatten_feats`` reads such
views without ``contiguous()`` and without a transpose, and an input level that is dense in ``torch.channels_last`` is read in
place — a backbone run in channels-last makes the whole path copy-free; any other layout costs one
``x.contiguous(memory_format=torch.channels_last)`` per level."""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from .. import modes as _modes
from ..ext import _ptr
from ._base import _forward_modes, _gemm_ctx, _launch, _m, _optr, _precision
from .conv import CONV_GRAN, CONV_MAX_ROWS
from .gemm import _pkg, _rows2d
from .images import conv1x1_weight, conv3x3_weight


def rows_of_map(x):
    """(B, C, H, W) -> its (B H W, C) channel-last rows: a view when ``x`` is dense in ``torch.channels_last``, else of one
    channels-last copy."""
    nhwc = x.permute(0, 2, 3, 1)
    if not nhwc.is_contiguous():
        nhwc = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        if not nhwc.is_contiguous():        # (a size-1 dimension: the memory format is ambiguous there)
            nhwc = nhwc.contiguous()
    return nhwc.reshape(-1, x.shape[1])


def map_of_rows(rows, n_img, hw):
    """(n_img H W, C) contiguous rows -> the (n_img, C, H, W)-shaped view of the same memory."""
    return rows.view(n_img, int(hw[0]), int(hw[1]), rows.shape[-1]).permute(0, 3, 1, 2)


def conv_rows(rows, n_img, hw, weight, bias, *, stride=1, relu_in=False, res=None, res_up=False, out=None, tag="conv_rows"):
    """A convolution over channel-last rows (``bevmsda_conv_rows_f32``): ``rows`` (n_img H W, C_in), ``hw = (H, W)``,
    ``weight`` (C_out, C_in, 1, 1) — padding 0, stride 1 — or (C_out, C_in, 3, 3) — padding 1, ``stride`` 1 or 2 —, ``bias``
    (C_out) or ``None``, ``relu_in``: ReLU on the input first, ``res``: added to the result, (n_img Ho Wo, C_out) rows or,
    with ``res_up``, the rows of the (Ho / 2, Wo / 2) map that is upsampled by 2 (nearest).  ``out``: an optional
    (n_img Ho Wo, C_out) destination with unit column stride (its row stride may exceed its width).  Returns
    (n_img Ho Wo, C_out) rows with Ho = (H - 1) // stride + 1, or ``None`` when the call is not covered."""
    mode = _m().gemm
    tensors = [rows, weight] + [t for t in (bias, res, out) if t is not None]
    if mode not in ("split", "bf16") or torch.is_grad_enabled() \
            or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return None
    H, W, n_img = int(hw[0]), int(hw[1]), int(n_img)
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (1, 3) or stride not in (1, 2):
        return None
    taps = int(weight.shape[2]) ** 2
    N, C = int(weight.shape[0]), int(weight.shape[1])
    if (taps == 1 and stride != 1) or C % CONV_GRAN or N % CONV_GRAN or rows.shape[-1] != C \
            or rows.numel() != n_img * H * W * C or n_img * H * W > CONV_MAX_ROWS:
        return None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = n_img * Ho * Wo
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        return None
    if res is not None:
        if res_up and (Ho % 2 or Wo % 2):
            return None
        if res.shape[-1] != N or res.numel() != (M // 4 if res_up else M) * N:
            return None
    if out is None:
        y = torch.empty((M, N), dtype=torch.float32, device=rows.device)
    else:
        y = out
        if y.dim() != 2 or tuple(y.shape) != (M, N) or y.stride(1) != 1:
            return None
    if M == 0 or N == 0:
        return y
    blob = conv3x3_weight(weight) if taps == 9 else conv1x1_weight(weight)
    if blob is None:
        return None
    x2, ldx = _rows2d(rows, C)
    desc = _lib.ConvRowsDesc(x=_ptr(x2), ld_x=ldx, n_img=n_img, H=H, W=W, c_in=C, c_out=N, taps=taps, stride=stride,
                             relu_in=int(bool(relu_in)), precision=_precision(), bias=_optr(bias))
    keep = [x2]
    if res is not None:
        r2, ldres = _rows2d(res, N)
        keep.append(r2)
        desc.res, desc.ld_res, desc.res_mode = _ptr(r2), ldres, (_lib.CONV_RES_UP2 if res_up else _lib.CONV_RES_SAME)
    K = taps * C
    ld_y = y.stride(0) if M > 1 else N
    timer = _gemm_ctx(tag, 2.0 * M * N * K, 4.0 * (n_img * H * W * C + N * K + M * N + (res.numel() if res is not None else 0)))
    return y if _launch(y.device, "conv_rows", lambda lib, stream: lib.bevmsda_conv_rows_f32(
        ctypes.byref(desc), _ptr(blob), _ptr(y), ld_y, stream), timer=timer) else None


# ---- recognition of an FPN by its attributes (mmdet's class qualifies where mmdet exists)

def _conv_of(cm, k, stride, pad):
    """The ``nn.Conv2d`` of a ConvModule-like ``cm`` when it is a bare k x k convolution of that stride and padding, else a
    reason (str)."""
    conv = getattr(cm, "conv", None)
    if not isinstance(conv, nn.Conv2d):
        return "a level is not a ConvModule around a Conv2d"
    if any(child is not conv for child in cm.children()) or getattr(cm, "with_norm", False) \
            or getattr(cm, "with_activation", False):
        return "a ConvModule has a norm or an activation"
    if tuple(conv.kernel_size) != (k, k) or tuple(conv.stride) != (stride, stride) \
            or conv.padding not in ((pad, pad), pad) or getattr(conv, "padding_mode", "zeros") != "zeros" \
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1:
        return f"a convolution is not {k} x {k}, stride {stride}, padding {pad}"
    if conv.in_channels % CONV_GRAN or conv.out_channels % CONV_GRAN:
        return f"channel counts are not multiples of {CONV_GRAN}"
    return conv


def _plan(neck):
    """(laterals, outputs, extras, start_level, end_level) — lists of ``nn.Conv2d`` — or a reason (str)."""
    try:
        lat, fpn_convs = list(neck.lateral_convs), list(neck.fpn_convs)
        start, end = int(neck.start_level), int(neck.backbone_end_level)
        num_outs, num_ins = int(neck.num_outs), len(neck.in_channels)
        extra_mode = neck.add_extra_convs
        up = dict(neck.upsample_cfg)
    except (AttributeError, TypeError):
        return "not an FPN"
    used = end - start
    if used < 1 or len(lat) != used or end > num_ins or num_outs < used:
        return "not an FPN"
    if extra_mode not in (False, "on_output"):
        return f"add_extra_convs={extra_mode!r}"
    if up.get("mode", "nearest") != "nearest" or "scale_factor" in up or set(up) - {"mode"}:
        return "upsample_cfg is not nearest by size"
    n_extra = num_outs - used if extra_mode else 0
    if len(fpn_convs) != used + n_extra:
        return "not an FPN"
    convs = []
    for mods, k, s, p in ((lat, 1, 1, 0), (fpn_convs[:used], 3, 1, 1), (fpn_convs[used:], 3, 2, 1)):
        got = [_conv_of(m, k, s, p) for m in mods]
        why = next((g for g in got if isinstance(g, str)), None)
        if why is not None:
            return why
        convs.append(got)
    out_c = convs[0][0].out_channels
    if any(c.out_channels != out_c for grp in convs for c in grp) or any(c.in_channels != out_c for grp in convs[1:] for c in grp):
        return "the convolutions do not chain"
    return convs[0], convs[1], convs[2], start, end


def _fpn_structure(neck, inputs=None):
    """``_plan(neck)`` after ``fpn_reject``'s structural and shape rules, or the reason (str) one of them gives."""
    plan = _plan(neck)
    if isinstance(plan, str):
        return plan
    lat, outs, extras, start, end = plan
    if inputs is not None:
        inputs = list(inputs)
        if len(inputs) != len(neck.in_channels) or not all(torch.is_tensor(x) and x.dim() == 4 for x in inputs):
            return "not one (B, C, H, W) tensor per input level"
        used = inputs[start:end]
        if any(x.shape[0] != used[0].shape[0] for x in used) or any(x.shape[1] != c.in_channels for x, c in zip(used, lat)):
            return "the inputs do not match the lateral convolutions"
        for fine, coarse in zip(used, used[1:]):
            if fine.shape[2] != 2 * coarse.shape[2] or fine.shape[3] != 2 * coarse.shape[3]:
                return "adjacent levels are not exact 2x of each other"
        if max(x.shape[0] * x.shape[2] * x.shape[3] for x in used) > CONV_MAX_ROWS:
            return "more than 2^24 rows"
    return plan


def _fpn_modes_reject(neck, inputs, start, end):
    """``fpn_reject``'s rules on the GEMM mode, then devices and dtypes."""
    if _m().gemm not in ("split", "bf16"):
        return f"GEMM mode {_m().gemm}"
    if not all(p.is_cuda and p.dtype == torch.float32 for p in neck.parameters()):
        return "not CUDA fp32 parameters"
    if inputs is not None and not all(x.is_cuda and x.dtype == torch.float32 for x in list(inputs)[start:end]):
        return "not CUDA fp32 inputs"
    return None


def fpn_reject(neck, inputs=None):
    """Why ``fpn`` does not cover ``neck`` on ``inputs`` (the backbone levels, a list of (B, C_i, H_i, W_i); ``None``: the
    module alone is judged) — a short reason — or ``None`` when it does.  The switch itself (``modes.fpn_fused``) is the
    caller's to test.  The module's structure first, then the inputs' shapes, then modes, then devices and dtypes."""
    plan = _fpn_structure(neck, inputs)
    if isinstance(plan, str):
        return plan
    if torch.is_grad_enabled():
        return "grad mode is on"
    return _fpn_modes_reject(neck, inputs, plan[3], plan[4])


def _fpn_rows(ops, neck, used, what="fpn", reject="fpn_reject"):
    """``fpn``'s launches on the used input levels -> (input rows, laterals, level rows, level sizes), the levels being the
    outputs and then the extra levels."""
    lat, outs, extras, _, _ = _plan(neck)
    B = used[0].shape[0]
    hws = [(int(x.shape[2]), int(x.shape[3])) for x in used]

    def conv(x, hw, c, tag, **kw):
        y = ops.conv_rows(x, B, hw, c.weight, c.bias, tag=tag, **kw)
        if y is None:
            raise RuntimeError(f"bevmsda: {what}: conv_rows declined a call {reject} had accepted")
        return y

    n = len(used)
    xrows = [rows_of_map(x) for x in used]
    laterals = [None] * n
    laterals[n - 1] = conv(xrows[n - 1], hws[n - 1], lat[n - 1], "fpn_lateral")
    for i in range(n - 2, -1, -1):
        laterals[i] = conv(xrows[i], hws[i], lat[i], "fpn_lateral", res=laterals[i + 1], res_up=True)
    rows = [conv(laterals[i], hws[i], outs[i], "fpn_out") for i in range(n)]
    for j, c in enumerate(extras):
        rows.append(conv(rows[-1], hws[-1], c, "fpn_extra", stride=2, relu_in=bool(j > 0 and neck.relu_before_extra_convs)))
        hws.append(((hws[-1][0] - 1) // 2 + 1, (hws[-1][1] - 1) // 2 + 1))
    return xrows, laterals, rows, hws


def fpn(neck, inputs):
    """An FPN on the row convolution kernel -> the list of its ``num_outs`` level outputs, NCHW-shaped views of channel-last
    storage with the module path's shapes and values, or ``None`` when the call is not covered (``fpn_reject``).

    Schedule: the top lateral; each lower lateral as ONE launch (1 x 1 + bias + the upsampled coarser lateral); one 3 x 3
    launch per output level; the extra levels as stride-2 launches on the previous output, with the ReLU on the input from
    the second extra level on when ``relu_before_extra_convs`` (mmdet's order).  Without extra convolutions the additional
    outputs are the ``max_pool2d(1, stride=2)`` subsamples.  A convolution the kernel declines after ``fpn_reject`` has
    accepted the call is an error, not a detour."""
    if fpn_reject(neck, inputs) is not None:
        return None
    _, _, _, start, end = _plan(neck)
    used = list(inputs)[start:end]
    B = used[0].shape[0]
    _, _, rows, hws = _fpn_rows(_pkg(), neck, used)
    result = [map_of_rows(r, B, hw) for r, hw in zip(rows, hws)]
    while len(result) < int(neck.num_outs):         # add_extra_convs=False: max_pool2d(x, 1, stride=2) is this subsample
        result.append(result[-1][:, :, ::2, ::2].contiguous(memory_format=torch.channels_last))
    return result


# ---- training the neck: one autograd Function on the backward kernels of the row convolution (csrc/conv_bwd_rows.h)

def fpn_train_reject(neck, inputs=None):
    """Why ``fpn_train`` does not cover ``neck`` on ``inputs`` — a short reason — or ``None`` when it does: ``fpn_reject``'s rules
    on the module's structure and the inputs' shapes, then, in this order: additional outputs that are subsamples
    (``add_extra_convs=False`` with ``num_outs`` above the used levels), the GEMM mode, devices and dtypes.  Grad mode is NOT a
    reason.  The switch itself (``modes.fpn_train``) is the caller's to test."""
    plan = _fpn_structure(neck, inputs)
    if isinstance(plan, str):
        return plan
    lat, outs, extras, start, end = plan
    if int(neck.num_outs) > len(lat) + len(extras):
        return "subsampled extra levels (no backward yet)"
    return _fpn_modes_reject(neck, inputs, start, end)


def _fpn_need(y):
    if y is None:
        raise RuntimeError("bevmsda: fpn_train: a kernel declined a call fpn_train_reject had accepted")
    return y


class _FpnTrain(torch.autograd.Function):
    """A whole FPN as one node: ``fpn``'s launches forward; backward, per convolution, one weight-gradient launch that also sums
    the bias gradient and one input-gradient launch whose epilogue adds the other branch's gradient (``fpn_train``).
    ``tensors``: the used input levels, then the weights of the laterals, the output and the extra convolutions, then their
    biases (``None`` for a convolution without one)."""

    @staticmethod
    def forward(ctx, neck, n_used, *tensors):
        ops = _pkg()
        used = list(tensors[:n_used])
        ctx.modes = _m().snapshot()
        ctx.modes.fpn_train = True            # (a captured step rebuilds the images of trainable weights: images._cache_ok)
        with _modes.activate(ctx.modes):
            xrows, laterals, rows, hws = _fpn_rows(ops, neck, used, "fpn_train", "fpn_train_reject")
        B = used[0].shape[0]
        ctx.neck, ctx.geom = neck, (B, hws, n_used)
        ctx.n_saved = (len(xrows), len(laterals), len(rows) - n_used)
        # the extra convolutions read the top output and every extra level but the last
        ctx.save_for_backward(*xrows, *laterals, *rows[n_used - 1:len(rows) - 1], *(t for t in tensors[n_used:] if t is not None))
        return tuple(map_of_rows(r, B, hw) for r, hw in zip(rows, hws))

    @staticmethod
    @_forward_modes
    def backward(ctx, *gouts):
        ops, neck = _pkg(), ctx.neck
        B, hws, n = ctx.geom
        lat, outs, extras, _, _ = _plan(neck)
        ne = len(extras)
        saved = ctx.saved_tensors
        xrows, laterals, chain = saved[:n], saved[n:2 * n], saved[2 * n:2 * n + ne]     # chain[j]: the input of extra j
        convs = lat + outs + extras
        nc = len(convs)
        need_x = ctx.needs_input_grad[2:2 + n]
        need_w = ctx.needs_input_grad[2 + n:2 + n + nc]
        need_b = [c.bias is not None and nb for c, nb in zip(convs, ctx.needs_input_grad[2 + n + nc:])]
        # one zero fill for every weight and bias gradient of the neck; a weight-gradient launch fills both, so a convolution
        # with one of the two frozen still gets both destinations
        launch = [nw or nb for nw, nb in zip(need_w, need_b)]
        sizes = [(c.weight.numel(), c.bias.numel() if c.bias is not None else 0) if go else (0, 0) for c, go in zip(convs, launch)]
        total = sum(a + b for a, b in sizes)
        flat = torch.zeros(total, dtype=torch.float32, device=xrows[0].device) if total else None
        dws, dbs, o = [], [], 0
        for c, (a, b) in zip(convs, sizes):
            dws.append(flat[o:o + a].view(c.weight.shape) if a else None)
            dbs.append(flat[o + a:o + a + b] if b else None)
            o += a + b
        g = [rows_of_map(t) for t in gouts]

        def bwd(k, gz, x, hw, tag, **kw):
            return _fpn_need(ops.conv_bn_rows_backward(gz, None, x, B, hw, convs[k].weight, None, need_dw=launch[k], dw_out=dws[k],
                                                   db_out=dbs[k], tag=tag, **kw))[0]

        # the extra levels, last to first: a level's gradient is its own output gradient plus the input gradient of the next
        # extra convolution, masked where that convolution read relu(level)
        top = g[n - 1 + ne]
        for j in range(ne - 1, -1, -1):
            relu_in = bool(j > 0 and neck.relu_before_extra_convs)
            mask = dict(next_mask=chain[j], add_after_mask=True) if relu_in else {}
            top = bwd(2 * n + j, top, chain[j], hws[n - 1 + j], "fpn_extra", stride=2, relu_x=relu_in, add=g[n - 1 + j], **mask)
        # the output convolutions, finest to coarsest: a lateral's gradient is its output convolution's input gradient plus the
        # 2 x 2 sums of the finer lateral's gradient (the transpose of the forward's upsampled residual)
        glat = []
        for i in range(n):
            fine = dict(add=glat[i - 1], add_pool2=True) if i else {}
            glat.append(bwd(n + i, top if i == n - 1 else g[i], laterals[i], hws[i], "fpn_out", **fine))
        gx = [None] * n
        for i in range(n):
            if need_x[i] or launch[i]:
                gx[i] = bwd(i, glat[i], xrows[i], hws[i], "fpn_lateral", need_dx=need_x[i])
        grads_w = [dw if nw else None for dw, nw in zip(dws, need_w)]
        grads_b = [db if nb else None for db, nb in zip(dbs, need_b)]
        return (None, None, *(map_of_rows(d, B, hw) if d is not None else None for d, hw in zip(gx, hws)), *grads_w, *grads_b)


def fpn_train(neck, inputs):
    """``fpn`` under autograd: ONE autograd Function for the whole neck -> the tuple of its ``num_outs`` level outputs, NCHW-shaped
    views of channel-last rows, bit-equal to ``fpn``'s, or ``None`` when the call is not covered (``fpn_train_reject``).

    Forward: ``fpn``'s launches; the used inputs' rows, the laterals, the top output and the extra levels that feed another are
    saved.  Backward, under the modes the forward saw, with one zero fill for every weight and bias gradient: the extra
    convolutions, last to first — a weight gradient with the bias gradient in it (and ``relu_x`` where the forward had the input
    ReLU) and a stride-2 input gradient whose epilogue adds that level's own output gradient, after the ReLU mask where there is
    one —; the output convolutions, finest to coarsest — a weight gradient and an input gradient whose epilogue adds the 2 x 2
    sums of the finer lateral's gradient —; the laterals — a weight gradient, and an input gradient only for an input that needs
    one.  Two launches per convolution (16 at three levels and two extras), no mask or bias launch, no torch add or interpolate;
    a convolution whose weight and bias are both frozen skips its weight gradient.  The input gradients are NCHW-shaped views of
    channel-last rows; the incoming output gradients are read in place when they are dense channel-last (``rows_of_map``).  A
    launch the kernels decline after ``fpn_train_reject`` has accepted the call is an error, not a detour."""
    if fpn_train_reject(neck, inputs) is not None:
        return None
    lat, outs, extras, start, end = _plan(neck)
    convs = lat + outs + extras
    used = list(inputs)[start:end]
    return _FpnTrain.apply(neck, len(used), *used, *(c.weight for c in convs), *(c.bias for c in convs))
