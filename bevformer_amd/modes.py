"""Execution modes of the host layer (``ops``): which kernel family, arithmetic and storage a call uses.

One ``Modes`` object holds every switch.  ``current()`` is what a call sees: the innermost ``using(...)`` block of
the CALLING THREAD, else the process-wide defaults (initialised from ``BEVMSDA_*`` environment variables once, at
import; the ``ops.set_*`` functions edit those defaults).  The autograd Functions of ``ops`` snapshot ``current()``
in ``forward`` and re-activate it in ``backward`` — the autograd engine runs backward on its own thread, which
would otherwise see the process defaults instead of the caller's modes.  The C library keeps no state: every
switch travels in a descriptor field of the call (include/bevmsda.h)."""
import contextlib
import copy
import os
import threading

import torch

GEMM_MODES = ("split", "bf16", "native")
# panelr*: the role-split 64-row panels (csrc/linear_roles.h) where they apply; r1 MFMA wavefronts at priority 0, r2 non-temporal
# stores, r3 both, r4 neither
GEMM_KERNELS = (None, "first", "first64", "pipe", "panel", "panel64", "panel128",
                "panelr", "panelr1", "panelr2", "panelr3", "panelr4")
FUSED_SPECS = (0, 1)


class Modes:
    __slots__ = ("value_storage", "fused", "fused_train", "gemm", "gemm_variant", "gemm_pack", "train_forward_mfma",
                 "gemm_kernel", "ln_fuse", "wgrad", "bf16_lanes8", "chain_shape", "grad_thread", "train_chain", "wgrad_workgroups", "wgrad_variant", "stack_free", "weight_views", "flatten_params", "fused_save", "chain_backward", "grad_arena", "overlap_value_proj", "use_grad_arena", "fused_spec", "fused_capacity_launch", "graph_repack", "tsa_seam", "chain_gather_all", "plan_on_side", "tile_halo", "decoder_fused", "head_fused", "loss_fused", "bevfusion_fused", "fpn_fused", "dcn_fused", "backbone_fused", "stem_fused", "backbone_train", "dcn_train", "fpn_train", "bn_train")

    def __init__(self):
        env = os.environ.get
        self.value_storage = torch.float32      # storage of the projected value tensors sampled by the kernels
        self.fused = True                        # fused softmax + location + sampling kernel on the no-grad path
        self.fused_train = env("BEVMSDA_FUSED_TRAIN", "1") == "1"   # ... and under autograd (three-step backward)
        self.gemm = env("BEVMSDA_GEMM", "split")                    # split | bf16 | native
        self.gemm_variant = int(env("BEVMSDA_GEMM_VARIANT")) if env("BEVMSDA_GEMM_VARIANT") else None  # None, 0, 12
        self.gemm_pack = env("BEVMSDA_GEMM_PACK", "1") == "1"       # pre-split weight images
        self.train_forward_mfma = env("BEVMSDA_TRAIN_FWD_MFMA", "1") == "1"
        k = env("BEVMSDA_GEMM_KERNEL", "")
        self.gemm_kernel = k if k in GEMM_KERNELS[1:] else None     # None = by measurement (ops._panel_covers)
        self.ln_fuse = env("BEVMSDA_FUSE_LN", "1") == "1"           # residual + LayerNorm in the projection's epilogue
        self.wgrad = env("BEVMSDA_WGRAD", "1") == "1"               # weight gradients on the TN MFMA kernel
        self.bf16_lanes8 = env("BEVMSDA_BF16_LANES8") is not None   # benchmark knob: 8-byte-lane bf16 kernels
        # fused sampling bodies (msda_d32.h LC / MC), the library's reserved[5]: 0 = default (TemporalSelfAttention's shape on the
        # body with compile-time head / level counts), 1 = generic bodies only.  The other values are retired
        # (tools/experimental/): they fail here and in ops.msda_fused instead of silently running the default
        self.fused_spec = int(env("BEVMSDA_FUSED_SPEC", "0"))
        if self.fused_spec not in FUSED_SPECS:
            raise ValueError(f"BEVMSDA_FUSED_SPEC must be one of {FUSED_SPECS}, not {self.fused_spec}")
        # sampling launches over a device-side row count: True = ONE launch sized by the row CAPACITY (surplus workgroups return
        # on their first instruction), False = a launch sized by the host's hint + a small strided tail launch for rows beyond
        # it, "auto" (default) = the capacity launch when it has at most FUSED_CAPACITY_AUTO_ROWS surplus rows (tiles of the BEV
        # grid, small grids: the surplus workgroups cost less than the tail launch's 5 us; at the base grid's 190,000 surplus
        # rows the two are level — profiles/r6z/r6zz_capacity_launch_ab.txt)
        self.fused_capacity_launch = {"0": False, "1": True}.get(env("BEVMSDA_FUSED_CAPACITY", "auto"), "auto")
        # A/B knob: re-pack the weight images of trainable parameters inside EVERY captured graph (round 4's behaviour; the
        # default re-packs only in graphs captured with grad mode on: ops.images._cache_ok)
        self.graph_repack = env("BEVMSDA_GRAPH_REPACK", "0") == "1"
        self.stack_free = env("BEVMSDA_STACK_FREE", "1") == "1"      # inference: TSA's [history ; queries] value projected without forming the stack
        self.weight_views = env("BEVMSDA_WEIGHT_VIEWS", "1") == "1"  # training: W^T images packed from W (no transposed copies)
        self.flatten_params = env("BEVMSDA_FLATTEN_PARAMS", "1") == "1"  # training: merged projections' parameters back to back (views, no cat)
        # training: what SCA's forward kernel writes for its backward — 1 = locations and weights (round 5, the default), 2 = the
        # attention weights only (round 6: the backward kernels recompute the locations from the projection rows,
        # bevmsda_backward_rows_offs_*: 564 MB less kept per base step, bit-equal gradients, the same step time — the forward kernel's
        # 32 us come back in the backward kernels' row_src -> offset indirection, profiles/r6/r6t_fused_save_ab.txt), 0 = nothing
        # (a bevmsda_frontend_expand_rows_f32 pass in the backward recomputes both)
        self.fused_save = int(env("BEVMSDA_FUSED_SAVE", "1"))
        self.chain_backward = env("BEVMSDA_CHAIN_BWD", "1") == "1"   # training: the row-local backward of the SCA seam in one kernel
        self.chain_shape = int(env("BEVMSDA_CHAIN_SHAPE", "0"))     # benchmark knob: workgroup shape of the row-chain kernels
        self.grad_thread = env("BEVMSDA_GRAD_THREAD", "1") == "1"   # training: value-projection input gradients summed in the GEMMs
        # autograd path of the encoder layer on the inference kernels (train_ops.py): chain kernels that save what their
        # backward needs, hoisted value projections, device-side row count through forward and backward
        self.train_chain = env("BEVMSDA_TRAIN_CHAIN", "1") == "1"
        self.wgrad_workgroups = int(env("BEVMSDA_WGRAD_WGS", "0"))  # benchmark knob: workgroup target of the multi-problem weight gradient
        self.wgrad_variant = int(env("BEVMSDA_WGRAD_VARIANT", "2"))  # 2 (default, round 6): 256 x 128 tiles on 8 wavefronts with 2 LDS stages where its one-workgroup-per-CU grid fills the chip, else 0; 0: 128 x 128, bf16 planes + transposing LDS reads; 1: gathered fragments
        # training: the parameter-gradient arena of the encoder call being recorded (train_ops.GradArena; set by
        # BEVFormerEncoder.forward for the duration of its call, carried to the backward pass by the Functions' snapshots)
        self.grad_arena = None
        self.use_grad_arena = env("BEVMSDA_GRAD_ARENA", "1") == "1"   # one zero fill for all parameter-gradient accumulators of a pass
        # inference: a layer's last kernel also makes the NEXT layer's TemporalSelfAttention offset / weight projection of
        # the rows it produces (csrc/linear_chain.h TP, BEVFormerEncoder.tsa_seam; round 6)
        self.tsa_seam = env("BEVMSDA_TSA_SEAM", "1") == "1"
        # BEV tiling: a rank projects only the BEV rows within this many cells of its tile (bev_tiling.enable_bev_tiling(halo=...),
        # exactness kept by a device-side flag + fallback); 0 = off, every rank projects the whole grid
        self.tile_halo = max(0, int(env("BEVMSDA_TILE_HALO", "0") or 0))
        # inference: SpatialCrossAttention's chain kernel walks every camera's row of a slot (idx = q_rows_all) instead of two
        # rows after a stand-alone fold launch (a no-op on most frames, 5 us per layer in a replayed graph)
        self.chain_gather_all = env("BEVMSDA_CHAIN_GATHER_ALL", "1") == "1"
        # inference with overlap_value_proj: the frame-plan kernels are issued on the side stream too, ahead of the camera-value
        # projection (nothing on the main stream reads the plan before the first SpatialCrossAttention joins that stream)
        self.plan_on_side = env("BEVMSDA_PLAN_SIDE", "1") == "1"
        self.overlap_value_proj = env("BEVMSDA_OVERLAP", "1") == "1"  # inference: hoisted SCA value projection on a side stream (its tail rounds and the TSA chain's fill each other: -2 % of the base frame, round 6)
        # inference: the stock six-op detection decoder (self_attn, norm, cross_attn, norm, ffn, norm) on the HIP self-attention
        # core, one hoisted BEV value projection for all layers and the seam kernels (DetectionTransformerDecoder; opt-in)
        self.decoder_fused = env("BEVMSDA_DECODER_FUSED", "0") == "1"
        # inference: the detection head's branch chains for all decoder layers in one launch, the decoder's reference-point
        # refinement as one launch per layer and the NMS-free decode as one kernel (csrc/head_branch.h, head_decode.h; opt-in)
        self.head_fused = env("BEVMSDA_HEAD_FUSED", "0") == "1"
        # training: BEVFormerHead.loss on the device — match costs, the batched assignment solver and the focal + L1 loss with
        # its unit gradients in three launches, no host read (csrc/det_cost.h, match_lsap.h, det_loss.h; opt-in)
        self.loss_fused = env("BEVMSDA_LOSS_FUSED", "0") == "1"
        # inference: PerceptionTransformerV2's temporal fusion (ResNetFusion) on the channel-last 3 x 3 convolution kernel — the
        # frames' BEV rows read in place, BatchNorm / residual / ReLU in the epilogue (csrc/conv3x3.h, ops.resnet_fusion; opt-in)
        self.bevfusion_fused = env("BEVMSDA_BEVFUSION_FUSED", "0") == "1"
        # inference: the image neck (FPN) on the channel-last row convolution kernel — laterals with bias and the upsampled
        # top-down residual in one launch each, outputs as NCHW views of channel-last rows that flatten_feats reads without a
        # transpose (csrc/conv_rows.h, ops.fpn; opt-in)
        self.fpn_fused = env("BEVMSDA_FPN_FUSED", "0") == "1"
        # inference: the backbone's modulated deformable convolutions (DCNv2) on the channel-last deformable kernel — the offset
        # matrix as one row convolution (always in split precision), then the bilinear-gather 3 x 3 with the block's BatchNorm
        # and ReLU in the epilogue (csrc/deform_conv.h, ops.dcn; opt-in)
        self.dcn_fused = env("BEVMSDA_DCN_FUSED", "0") == "1"
        # inference: the backbone's bottlenecks on channel-last rows — conv1, the plain conv2, conv3 and the downsample on the row
        # convolution kernel with BatchNorm, the residual sum and the ReLU in the epilogue, a DCNv2 conv2 on the deformable
        # kernel; a block, and so a stage, stays in rows (csrc/conv_bn_rows.h, ops.bottleneck; opt-in)
        self.backbone_fused = env("BEVMSDA_BACKBONE_FUSED", "0") == "1"
        # inference: the backbone's stem — 7 x 7 stride-2 convolution, BatchNorm, ReLU and the 3 x 3 max pooling — as ONE launch
        # that reads the NCHW image batch in place and writes the channel-last rows the first bottleneck reads; independent of
        # backbone_fused (csrc/stem_conv.h, ops.stem; opt-in)
        self.stem_fused = env("BEVMSDA_STEM_FUSED", "0") == "1"
        # training: a backbone with frozen BatchNorms (norm_eval=True, requires_grad=False norms) on channel-last rows — a covered
        # bottleneck as ONE autograd Function whose backward is the row input-gradient and weight-gradient kernels, frozen
        # blocks and a frozen stem on the inference kernels under no_grad (csrc/conv_bwd_rows.h, ops.bottleneck_train; opt-in)
        self.backbone_train = env("BEVMSDA_BACKBONE_TRAIN", "0") == "1"
        # training, together with backbone_train only: a bottleneck whose conv2 is a DCNv2 pack as the same one-node Function — the
        # deformable input, offset / mask and weight gradients on the kernels of csrc/deform_conv_bwd.h, conv_offset's gradients
        # on the row kernels (ops.deform_conv_rows_backward; opt-in)
        self.dcn_train = env("BEVMSDA_DCN_TRAIN", "0") == "1"
        # training: the image neck (FPN) as ONE autograd Function on channel-last rows — ops.fpn's launches forward; backward the
        # row weight-gradient kernel with the bias gradient in it and the row input-gradient kernel with the 2 x 2 sum of the
        # finer lateral's gradient in its epilogue; independent of fpn_fused (csrc/conv_bwd_rows.h, ops.fpn_train; opt-in)
        self.fpn_train = env("BEVMSDA_FPN_TRAIN", "0") == "1"
        # training, together with backbone_train only: a bottleneck whose norms are all in train() mode (batch statistics, the
        # bevformerv2 configs' norm_eval=False) as one Function — per convolution the raw row convolution, the per-channel
        # statistics (running statistics updated in the same call) and the apply; backward through the statistics, dgamma /
        # dbeta returned (csrc/batchnorm_rows.h, ops.norm; opt-in)
        self.bn_train = env("BEVMSDA_BN_TRAIN", "0") == "1"
        assert self.gemm in GEMM_MODES, f"BEVMSDA_GEMM must be one of {GEMM_MODES}"

    def snapshot(self):
        return copy.copy(self)


_PROCESS = Modes()
_TLS = threading.local()


def process_defaults():
    """The process-wide defaults (what ``ops.set_*`` edit)."""
    return _PROCESS


def current():
    stack = getattr(_TLS, "stack", None)
    return stack[-1] if stack else _PROCESS


@contextlib.contextmanager
def activate(modes):
    """Make ``modes`` (a snapshot) the calling thread's modes for the block."""
    stack = getattr(_TLS, "stack", None)
    if stack is None:
        stack = _TLS.stack = []
    stack.append(modes)
    try:
        yield modes
    finally:
        stack.pop()


@contextlib.contextmanager
def using(**overrides):
    """``with modes.using(gemm="bf16", value_storage=torch.bfloat16): ...`` — thread-local overrides."""
    m = current().snapshot()
    for k, v in overrides.items():
        if k not in Modes.__slots__:
            raise AttributeError(f"unknown mode {k!r}")
        setattr(m, k, v)
    with activate(m):
        yield m
