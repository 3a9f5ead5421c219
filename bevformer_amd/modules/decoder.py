"""Decoder-side users of the deformable-attention operator.

``CustomMSDeformableAttention`` and ``DetectionTransformerDecoder`` with the registry names,
constructor arguments, parameters and forward contracts of
projects/mmdet3d_plugin/bevformer/modules/decoder.py:53-129 and :133-345.  The attention runs
on the same kernels as the encoder: one merged GEMM for sampling offsets + attention logits, and
softmax / ``reference + offset / (W, H)`` / sampling / aggregation in the fused D = 32 kernel
(one BEV level, 4 points, 900 object queries at base), the unfused operator under autograd
or for box-shaped (4-d) reference points.

The decoder *layer* type of the reference configs (``DetrTransformerDecoderLayer`` with
mmcv's ``MultiheadAttention`` self-attention) is third-party and comes from mmcv / mmdet when
they are installed; the layer sequence here accepts any registered layer type (the tests build
it from this package's ``MyCustomBaseTransformerLayer``).
"""
import warnings

import torch
import torch.nn as nn

from .. import ops
from ..registry import (ATTENTION, HAVE_MMCV, TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE, BaseModule,
                        constant_, xavier_uniform_)
from .custom_base_transformer_layer import MyCustomBaseTransformerLayer
from .encoder import TransformerLayerSequence
from .temporal_self_attention import _direction_grid, _is_power_of_2


def inverse_sigmoid(x, eps=1e-5):
    """decoder.py:34-50."""
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


@TRANSFORMER_LAYER_SEQUENCE.register_module(force=True)
class DetectionTransformerDecoder(TransformerLayerSequence):
    """Layer loop with iterative reference-point refinement (decoder.py:53-129)."""

    def __init__(self, *args, return_intermediate=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.return_intermediate = return_intermediate
        self.fp16_enabled = False

    def forward(self, query, *args, reference_points=None, reg_branches=None, key_padding_mask=None,
                **kwargs):
        """query (num_query, bs, C); reference_points (bs, num_query, 3) -> (output,
        reference_points), stacked over layers with ``return_intermediate``."""
        fused_values = None
        if ops.modes().decoder_fused and self.fused_reject(query, *args, reference_points=reference_points,
                                                           key_padding_mask=key_padding_mask, **kwargs) is None:
            fused_values = self.hoisted_value_projection(kwargs["value"])
        output = query
        intermediate, intermediate_reference_points = [], []
        for lid, layer in enumerate(self.layers):
            fused = None
            if fused_values is not None:
                fused = self._fused_layer(layer, output, kwargs.get("query_pos"), reference_points[..., :2], fused_values[lid],
                                          kwargs["spatial_shapes"], kwargs["level_start_index"])
            refined = None
            if fused is not None:
                output = fused
                if reg_branches is not None and ops.modes().head_fused:
                    # the refinement below as one launch (csrc/head_branch.h); None: not the stock branch, the statements run
                    refined = ops.reg_refine(output, reference_points, reg_branches[lid])
            else:
                reference_points_input = reference_points[..., :2].unsqueeze(2)   # (bs, nq, 1 level, 2)
                output = layer(output, *args, reference_points=reference_points_input,
                               key_padding_mask=key_padding_mask, **kwargs)
            output = output.permute(1, 0, 2)
            if refined is not None:
                reference_points = refined
            elif reg_branches is not None:
                tmp = reg_branches[lid](output)
                assert reference_points.shape[-1] == 3
                new_reference_points = torch.zeros_like(reference_points)
                new_reference_points[..., :2] = tmp[..., :2] + inverse_sigmoid(reference_points[..., :2])
                new_reference_points[..., 2:3] = tmp[..., 4:5] + inverse_sigmoid(reference_points[..., 2:3])
                reference_points = new_reference_points.sigmoid().detach()
            output = output.permute(1, 0, 2)
            if self.return_intermediate:
                intermediate.append(output)
                intermediate_reference_points.append(reference_points)
        if self.return_intermediate:
            return torch.stack(intermediate), torch.stack(intermediate_reference_points)
        return output, reference_points

    # ------------------------------------------------------------------------------------------------------------
    # Inference fast path of the stock six-op layer (``modes.decoder_fused``, opt-in): per layer
    #   q = k = (x + pos) W_qk^T, v = x W_v^T          ops.linear over views of in_proj_weight
    #   softmax(q k^T / sqrt(32)) v                     ops.mha (csrc/mha_d32.h)
    #   norm0(out_proj(.) + x)                          ops.linear_layernorm
    #   merged offset / weight projection of (. + pos)  ops.linear
    #   sampling from the layer's slice of the BEV values projected ONCE for all layers   ops.msda_fused
    #   norm2(ffn(norm1(output_proj(.) + .)))           ops.proj_ffn_chain
    #   with ``modes.head_fused``: sigmoid(reg_branch(.)[{0, 1, 4}] + inverse_sigmoid(ref))   ops.reg_refine
    # Rows stay in the decoder's (num_query, bs) order throughout.  No step reads a device value on the host.
    # ------------------------------------------------------------------------------------------------------------
    def fused_reject(self, query, *args, reference_points=None, key_padding_mask=None, attn_masks=None,
                     query_key_padding_mask=None, value=None, query_pos=None, spatial_shapes=None, level_start_index=None,
                     **kwargs):
        """Why this call does NOT take the fast path (a short reason), or ``None`` when it does: the arguments are those of
        ``forward``.  The switch itself (``modes.decoder_fused``) is the caller's to test.  Structure first, then modes and
        arguments, the tensors' device last — so that everything but the last is decided the same on a CPU-built module."""
        for layer in self.layers:
            why = fused_layer_reject(layer)
            if why is not None:
                return why
        if torch.is_grad_enabled():
            return "gradient mode is on"
        if self.training or any(layer.training for layer in self.layers):
            return "train() mode"
        if ops.gemm_mode() not in ("split", "bf16"):
            return "GEMM mode is not split / bf16"
        if args:
            return "positional key / value"
        if key_padding_mask is not None or query_key_padding_mask is not None:
            return "key-padding mask"
        if attn_masks is not None and (torch.is_tensor(attn_masks) or any(m is not None for m in attn_masks)):
            return "attention mask"
        if not torch.is_tensor(reference_points) or reference_points.dim() != 3 or reference_points.shape[-1] != 3:
            return "reference points are not (bs, num_query, 3)"
        if not torch.is_tensor(query) or query.dim() != 3 or query.shape[-1] != 256 or not torch.is_tensor(value) \
                or value.dim() != 3 or value.shape[-1] != 256 or value.shape[1] != query.shape[1] \
                or (query_pos is not None and query_pos.shape != query.shape) \
                or tuple(reference_points.shape[:2]) != (query.shape[1], query.shape[0]):
            return "operand shapes"
        if not torch.is_tensor(spatial_shapes) or tuple(spatial_shapes.shape) != (1, 2) or spatial_shapes.dtype != torch.long \
                or not torch.is_tensor(level_start_index) or level_start_index.numel() != 1 \
                or level_start_index.dtype != torch.long:
            return "not one BEV level"
        for t in (query, value, query_pos, reference_points):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32):
                return "not CUDA fp32 tensors"
        if not spatial_shapes.is_cuda or not level_start_index.is_cuda:
            return "not CUDA fp32 tensors"
        return None

    def hoisted_value_projection(self, value):
        """Every layer's ``CustomMSDeformableAttention.value_proj`` of the BEV (``value`` (Q, bs, C), the same for all layers)
        in ONE grouped GEMM: a list of contiguous (bs, Q, 8, 32) value tensors, or ``None`` when the GEMM declines."""
        cross = [layer.attentions[1] for layer in self.layers]
        w, b = ops.merged_linear_params(self, *[m.value_proj for m in cross], slot="_merged_dec_value")
        y = ops.linear(value.permute(1, 0, 2), w, b, groups=len(cross), tag="dec_value_proj_hoisted")
        if y is None:
            return None
        if len(cross) == 1:
            y = y[None]
        bs, Q = value.shape[1], value.shape[0]
        return [y[i].view(bs, Q, cross[i].num_heads, -1) for i in range(len(cross))]

    def _fused_layer(self, layer, x, pos, ref2d, value, spatial_shapes, level_start_index):
        """One layer of the fast path: x / pos (num_query, bs, 256), ref2d (bs, num_query, 2), value (bs, Q, 8, 32) ->
        (num_query, bs, 256), or ``None`` when a kernel declines (the caller then runs the layer's modules)."""
        self_attn, cross = layer.attentions
        mha = self_attn.attn
        nq, bs, C = x.shape
        w_qk, b_qk, w_v, b_v = _in_proj_views(mha)
        qk = ops.linear(x, w_qk, b_qk, x_add=pos, tag="dec_qk_proj")
        v = ops.linear(x, w_v, b_v, tag="dec_v_proj")
        if qk is None or v is None:
            return None
        att = ops.mha(qk[..., :C], qk[..., C:], v, mha.num_heads, tag="dec_mha")
        if att is None:
            return None
        x = ops.linear_layernorm(att, mha.out_proj.weight, mha.out_proj.bias, x, layer.norms[0], tag="dec_attn_out_proj")
        if x is None:
            return None
        M, L, P = cross.num_heads, cross.num_levels, cross.num_points
        n_off = cross.sampling_offsets.out_features
        w, b = ops.merged_linear_params(cross, cross.sampling_offsets, cross.attention_weights)
        proj = ops.linear(x, w, b, x_add=pos, tag="dec_offs_attn")
        if proj is None or not ops.fused_wanted(proj, value):
            return None
        # rows q * bs + b: their value batch entry is b, their reference point ref2d[b, q]
        row_batch = self._row_batch(nq, bs, x.device) if bs > 1 else None
        ref = ref2d.permute(1, 0, 2).reshape(nq * bs, 1, L, 2)
        out = ops.msda_fused(value, spatial_shapes, level_start_index, proj.view(nq * bs, -1), n_off, ref, row_batch, M=M, L=L,
                             P=P, K=1, off_head=L * P * 2, off_k=0, lg_head=L * P, lg_k=0, ref_mode=1, vmul=1, vadd=0,
                             Q=nq, tag="dec_fwd")
        if out is None:
            return None
        if out.dtype != torch.float32:
            out = out.float()
        ffn = layer.ffns[0]
        y = ops.proj_ffn_chain(out, cross.output_proj.weight, cross.output_proj.bias, x, layer.norms[1], ffn.layers[0][0],
                               ffn.layers[1], layer.norms[2], tag="dec_out_ffn_chain")
        return None if y is None else y.view(nq, bs, C)

    def _row_batch(self, nq, bs, device):
        if torch.cuda.is_current_stream_capturing():     # (a capture's allocation is the graph's: not kept)
            return (torch.arange(nq * bs, device=device, dtype=torch.int32) % bs).contiguous()
        hit = self.__dict__.get("_fused_row_batch")
        if hit is None or hit[0] != (nq, bs, device):
            hit = self.__dict__["_fused_row_batch"] = (
                (nq, bs, device), (torch.arange(nq * bs, device=device, dtype=torch.int32) % bs).contiguous())
        return hit[1]


_FUSED_ORDER = ("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")


def _linear_is(m, n_out, n_in):
    return isinstance(m, nn.Linear) and tuple(m.weight.shape) == (n_out, n_in) and m.bias is not None


def fused_layer_reject(layer):
    """Why ``layer`` is not the stock decoder layer the fast path covers (a short reason), or ``None`` when it is.  By
    attributes, not by class: with mmcv / mmdet installed the layer, its self-attention wrapper and its FFN are theirs."""
    if tuple(getattr(layer, "operation_order", None) or ()) != _FUSED_ORDER:
        return "operation order"
    att, ffns, norms = (getattr(layer, n, None) for n in ("attentions", "ffns", "norms"))
    if att is None or ffns is None or norms is None or len(att) != 2 or len(ffns) != 1 or len(norms) != 3:
        return "layer structure"
    mha = getattr(att[0], "attn", None)
    if not isinstance(mha, nn.MultiheadAttention):
        return "self-attention does not wrap nn.MultiheadAttention"
    if mha.embed_dim != 256 or mha.num_heads != 8 or getattr(mha, "batch_first", False) \
            or getattr(att[0], "batch_first", False) or mha.in_proj_weight is None or mha.in_proj_bias is None \
            or mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn or not _linear_is(mha.out_proj, 256, 256):
        return "self-attention is not 256 dims / 8 heads / batch_first=False"
    cross = att[1]
    if not isinstance(cross, CustomMSDeformableAttention) or cross.num_levels != 1 or cross.embed_dims != 256 \
            or cross.num_heads != 8 or cross.batch_first or not _linear_is(cross.value_proj, 256, 256) \
            or not _linear_is(cross.output_proj, 256, 256):
        return "cross-attention is not a one-level CustomMSDeformableAttention"
    fcs = getattr(ffns[0], "layers", None)
    if fcs is None or len(fcs) != 3 or not isinstance(fcs[0], nn.Sequential) or len(fcs[0]) < 2 \
            or not _linear_is(fcs[0][0], 512, 256) or not isinstance(fcs[0][1], nn.ReLU) or not _linear_is(fcs[1], 256, 512) \
            or not getattr(ffns[0], "add_identity", True):
        return "FFN is not two-layer 256 -> 512 -> 256 ReLU"
    for norm in norms:
        if not isinstance(norm, nn.LayerNorm) or tuple(norm.normalized_shape) != (256,) or norm.weight is None \
                or norm.bias is None:
            return "norms are not nn.LayerNorm(256)"
    return None


def _in_proj_views(mha):
    """(W_qk (512, 256), b_qk, W_v (256, 256), b_v): views of ``in_proj_weight`` / ``in_proj_bias``, kept on the module while
    the parameters stay where they are — the weight images of the GEMM kernels are cached on the tensor objects."""
    w, b = mha.in_proj_weight, mha.in_proj_bias
    key = (w.data_ptr(), b.data_ptr(), w.device)
    hit = mha.__dict__.get("_bevmsda_in_proj_views")
    if hit is None or hit[0] != key:
        E = mha.embed_dim
        wd, bd = w.detach(), b.detach()
        hit = mha.__dict__["_bevmsda_in_proj_views"] = (key, (wd[:2 * E], bd[:2 * E], wd[2 * E:], bd[2 * E:]))
    return hit[1]


@ATTENTION.register_module(force=True)
class CustomMSDeformableAttention(BaseModule):
    """Object queries attend to the BEV grid (decoder.py:133-345)."""

    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64,
                 dropout=0.1, batch_first=False, norm_cfg=None, init_cfg=None):
        super().__init__(init_cfg)
        if embed_dims % num_heads != 0:
            raise ValueError(f"embed_dims must be divisible by num_heads, "
                             f"but got {embed_dims} and {num_heads}")
        if not _is_power_of_2(embed_dims // num_heads):
            warnings.warn("You'd better set embed_dims in MultiScaleDeformAttention to make the "
                          "dimension of each attention head a power of 2 (the HIP kernel's "
                          "16-byte lane-group path needs a multiple of 4).")
        self.norm_cfg = norm_cfg
        self.dropout = nn.Dropout(dropout)
        self.batch_first = batch_first
        self.fp16_enabled = False
        self.im2col_step = im2col_step
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.init_weights()

    def init_weights(self):
        constant_(self.sampling_offsets, 0.0)
        self.sampling_offsets.bias.data = _direction_grid(self.num_heads, self.num_levels,
                                                          self.num_points)
        constant_(self.attention_weights, 0.0, 0.0)
        xavier_uniform_(self.value_proj)
        xavier_uniform_(self.output_proj)
        self._is_init = True

    def forward(self, query, key=None, value=None, identity=None, query_pos=None,
                key_padding_mask=None, reference_points=None, spatial_shapes=None,
                level_start_index=None, flag="decoder", **kwargs):
        """query (num_query, bs, C) [(bs, num_query, C) with batch_first]; value (num_value,
        bs, C); reference_points (bs, num_query, num_levels, 2 | 4) -> same layout as query."""
        if value is None:
            value = query
        if identity is None:
            identity = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query = query.permute(1, 0, 2)
            value = value.permute(1, 0, 2)
        bs, num_query, C = query.shape
        num_value = value.shape[1]
        M, L, P = self.num_heads, self.num_levels, self.num_points

        v = ops.linear_or_torch(value, self.value_proj.weight, self.value_proj.bias,
                                tag="dec_value_proj")
        if key_padding_mask is not None:
            v = v.masked_fill(key_padding_mask[..., None], 0.0)
        v = v.reshape(bs, num_value, M, -1)

        n_off = self.sampling_offsets.out_features
        w, b = ops.merged_linear_params(self, self.sampling_offsets, self.attention_weights)
        proj = ops.linear_or_torch(query.reshape(bs * num_query, C), w, b, tag="dec_offs_attn")
        out = None
        if reference_points.shape[-1] == 2 and ops.fused_wanted(proj, v):
            ref = reference_points.reshape(bs * num_query, 1, L, 2)
            out = ops.msda_fused(v, spatial_shapes, level_start_index, proj, n_off, ref, None, M=M,
                                 L=L, P=P, K=1, off_head=L * P * 2, off_k=0, lg_head=L * P, lg_k=0,
                                 ref_mode=1, vmul=1, vadd=0, Q=num_query, tag="dec_fwd")
            if out is not None:
                out = out.to(query.dtype).view(bs, num_query, C)
        if out is None:
            off = proj[:, :n_off].view(bs, num_query, M, L, P, 2)
            att = proj[:, n_off:].view(bs, num_query, M, L * P).softmax(-1).view(bs, num_query, M, L, P)
            if reference_points.shape[-1] == 2:
                normalizer = torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1)
                loc = reference_points[:, :, None, :, None, :] \
                    + off / normalizer[None, None, None, :, None, :]
            elif reference_points.shape[-1] == 4:
                loc = reference_points[:, :, None, :, None, :2] \
                    + off / P * reference_points[:, :, None, :, None, 2:] * 0.5
            else:
                raise ValueError(f"Last dim of reference_points must be 2 or 4, "
                                 f"but get {reference_points.shape[-1]} instead.")
            out = ops.msda(v, spatial_shapes, level_start_index, loc.contiguous(), att.contiguous(),
                           self.im2col_step, tag="dec_fwd")
        out = ops.linear_or_torch(out, self.output_proj.weight, self.output_proj.bias,
                                  tag="dec_output_proj")
        if not self.batch_first:
            out = out.permute(1, 0, 2)
        return self.dropout(out) + identity


# ---------------------------------------------------------------------------
# The two third-party classes the reference's decoder config names
# (bevformer_base.py:110-127): mmcv's ``MultiheadAttention`` wrapper and mmdet's
# ``DetrTransformerDecoderLayer``.  Neither lives in the reference tree (mmcv-full 1.4.0 /
# mmdet 2.14.0, docs/install.md:27,33); when those packages are installed their own classes are
# used and nothing below is registered.  Without them, these restatements — from the published
# behaviour of the two classes, NOT pinned against their source (third-party, absent) — let the
# reference's decoder config build and ``PerceptionTransformer.forward`` run stand-alone.
# ---------------------------------------------------------------------------

class MultiheadAttention(BaseModule):
    """``identity + dropout(proj_drop(nn.MultiheadAttention(q + q_pos, k + k_pos, v)))`` with
    mmcv's defaults: key = query, value = key, identity = query, key_pos = query_pos when the
    shapes agree; parameters under ``attn.*`` (``in_proj_weight``, ``in_proj_bias``,
    ``out_proj.{weight,bias}``)."""

    def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0,
                 dropout_layer=dict(type="Dropout", drop_prob=0.0), init_cfg=None, batch_first=False,
                 **kwargs):
        super().__init__(init_cfg)
        dropout_layer = dict(dropout_layer) if dropout_layer else None
        if "dropout" in kwargs:             # deprecated spelling used by the BEVFormer configs
            attn_drop = kwargs["dropout"]
            if dropout_layer is not None:
                dropout_layer["drop_prob"] = kwargs.pop("dropout")
            else:
                kwargs.pop("dropout")
        self.embed_dims = embed_dims
        self.num_heads = num_heads
        self.batch_first = batch_first
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop, **kwargs)
        self.proj_drop = nn.Dropout(proj_drop)
        p = dropout_layer.get("drop_prob", 0.0) if dropout_layer else 0.0
        self.dropout_layer = nn.Dropout(p) if dropout_layer else nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None,
                attn_mask=None, key_padding_mask=None, **kwargs):
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None and query_pos is not None:
            if query_pos.shape == key.shape:
                key_pos = query_pos
            else:
                warnings.warn(f"position encoding of key is missing in {self.__class__.__name__}.")
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if self.batch_first:
            query, key, value = query.transpose(0, 1), key.transpose(0, 1), value.transpose(0, 1)
        out = self.attn(query=query, key=key, value=value, attn_mask=attn_mask,
                        key_padding_mask=key_padding_mask)[0]
        if self.batch_first:
            out = out.transpose(0, 1)
        return identity + self.dropout_layer(self.proj_drop(out))


@ATTENTION.register_module(force=True)      # (the plugin's own name, as CustomMSDeformableAttention)
class GroupMultiheadAttention(MultiheadAttention):
    """projects/mmdet3d_plugin/bevformer/modules/group_attention.py:18-162, the self-attention of the Group-DETR decoders
    (``group=11`` in the bevformerv2 configs): the wrapper above, except that in ``train()`` mode the ``num_query`` rows are
    split into ``group`` blocks of ``num_query // group`` rows which attend among themselves only — the blocks are stacked on
    the batch axis for ``nn.MultiheadAttention`` and unstacked after.  In ``eval()`` mode (one group of queries is run,
    ``BEVFormerHead_GroupDETR.forward``) it IS the wrapper above.  Parameters under ``attn.*``.  The training path is torch."""

    def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0, group=1,
                 dropout_layer=dict(type="Dropout", drop_prob=0.0), init_cfg=None, batch_first=False, **kwargs):
        super().__init__(embed_dims, num_heads, attn_drop=attn_drop, proj_drop=proj_drop, dropout_layer=dropout_layer,
                         init_cfg=init_cfg, batch_first=batch_first, **kwargs)
        self.group = group

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None,
                attn_mask=None, key_padding_mask=None, **kwargs):
        if not self.training:
            return super().forward(query, key=key, value=value, identity=identity, query_pos=query_pos, key_pos=key_pos,
                                   attn_mask=attn_mask, key_padding_mask=key_padding_mask, **kwargs)
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None and query_pos is not None:
            if query_pos.shape == key.shape:
                key_pos = query_pos
            else:
                warnings.warn(f"position encoding of key is missing in {self.__class__.__name__}.")
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if self.batch_first:
            query, key, value = query.transpose(0, 1), key.transpose(0, 1), value.transpose(0, 1)
        # group_attention.py:147-157
        num_queries = query.shape[0]
        bs = query.shape[1]
        query = torch.cat(query.split(num_queries // self.group, dim=0), dim=1)
        key = torch.cat(key.split(num_queries // self.group, dim=0), dim=1)
        value = torch.cat(value.split(num_queries // self.group, dim=0), dim=1)
        out = self.attn(query=query, key=key, value=value, attn_mask=attn_mask, key_padding_mask=key_padding_mask)[0]
        out = torch.cat(out.split(bs, dim=1), dim=0)
        if self.batch_first:
            out = out.transpose(0, 1)
        return identity + self.dropout_layer(self.proj_drop(out))


class DetrTransformerDecoderLayer(MyCustomBaseTransformerLayer):
    """mmdet's decoder layer: the generic op-order layer with ``batch_first=False`` and the
    six-operation order (self_attn, norm, cross_attn, norm, ffn, norm)."""

    def __init__(self, attn_cfgs, feedforward_channels, ffn_dropout=0.0, operation_order=None,
                 act_cfg=dict(type="ReLU", inplace=True), norm_cfg=dict(type="LN"), ffn_num_fcs=2,
                 **kwargs):
        kwargs.setdefault("batch_first", False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            super().__init__(attn_cfgs=attn_cfgs, feedforward_channels=feedforward_channels,
                             ffn_dropout=ffn_dropout, operation_order=operation_order, act_cfg=act_cfg,
                             norm_cfg=norm_cfg, ffn_num_fcs=ffn_num_fcs, **kwargs)
        assert len(operation_order) == 6
        assert set(operation_order) == set(["self_attn", "norm", "cross_attn", "ffn"])


if not HAVE_MMCV:
    ATTENTION.register_module(name="MultiheadAttention", module=MultiheadAttention)
    TRANSFORMER_LAYER.register_module(name="DetrTransformerDecoderLayer", module=DetrTransformerDecoderLayer)
