"""Dense softmax attention: the core of the decoder's ``nn.MultiheadAttention`` (csrc/mha_d32.h)."""
import math

import torch

from .. import _lib
from ..ext import _ptr
from ._base import _gemm_ctx, _launch
from .sampling import fused_wanted

MHA_HEAD_DIM = 32


def _seq_rows(t):
    """``t`` (seq, bs, E) as rows ``s * bs + b`` of one matrix, in place where its strides allow (a column block of a wider
    projection output does): returns (tensor, row stride)."""
    S, bs, E = t.shape
    ld = E if S == 1 and bs == 1 else (t.stride(0) if bs == 1 else t.stride(1))
    if t.stride(2) != 1 or ld % 4 or ld < E or t.data_ptr() % 16 or (bs > 1 and S > 1 and t.stride(0) != bs * ld):
        return t.contiguous(), E
    return t, ld


def mha(q, k, v, num_heads, *, scale=None, tag="dec_mha"):
    """``softmax(q k^T * scale) v`` per (batch, head) through ``bevmsda_mha_d32_f32`` (include/bevmsda.h): q (nq, bs, E),
    k / v (nk, bs, E) fp32 GPU tensors in ``nn.MultiheadAttention``'s ``batch_first=False`` layout, already projected; E =
    ``num_heads`` * 32; ``scale`` defaults to 1 / sqrt(32).  No masks, no dropout.  Column-block views of a merged projection
    are read in place.  Exact-fp32 MFMA in every GEMM mode.  Returns (nq, bs, E), or ``None`` when the call is not covered
    (head width other than 32, CPU or non-fp32 tensors, a gradient wanted) and the caller runs its own attention."""
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or not q.is_cuda or not k.is_cuda or not v.is_cuda \
            or q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32 \
            or not fused_wanted(q, k, v):
        return None
    nq, bs, E = q.shape
    nk = k.shape[0]
    if num_heads <= 0 or E != num_heads * MHA_HEAD_DIM or tuple(k.shape) != (nk, bs, E) or tuple(v.shape) != (nk, bs, E) \
            or nk == 0:
        return None
    out = torch.empty((nq, bs, E), dtype=torch.float32, device=q.device)
    if nq == 0 or bs == 0:
        return out
    q2, ldq = _seq_rows(q)
    k2, ldk = _seq_rows(k)
    v2, ldv = _seq_rows(v)
    scale = 1.0 / math.sqrt(MHA_HEAD_DIM) if scale is None else float(scale)
    # algorithmic: both products, and every operand once
    timer = _gemm_ctx(tag, 4.0 * bs * num_heads * nq * nk * MHA_HEAD_DIM, 4.0 * bs * E * (2 * nq + 2 * nk))
    if not _launch(q.device, "mha", lambda lib, stream: lib.bevmsda_mha_d32_f32(
            _ptr(q2), ldq, _ptr(k2), ldk, _ptr(v2), ldv, nq, nk, bs, num_heads, MHA_HEAD_DIM, scale, _ptr(out), E, stream),
            timer=timer, also_declined=(_lib.ERR_TOO_LARGE,)):
        return None
    return out
