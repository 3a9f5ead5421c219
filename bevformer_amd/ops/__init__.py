"""Thin functional front of the HIP operator for the modules of this package.

``msda`` is the reference's operator call (``MultiScaleDeformableAttnFunction_fp32
.apply`` at spatial_cross_attention.py:390-392 / temporal_self_attention.py:247-249);
``msda_ragged`` is the same math over a ragged batch (row -> value-batch table),
which is how this package runs SpatialCrossAttention without zero-padded rows.
Neither has a CPU implementation: CPU tensors raise ``RuntimeError``.

Round 5: the module is a package — ``_base`` (modes, cache keys, the kernel and GEMM timers, the launch tail ``_launch`` every operator ends in with its operand idioms), ``sampling`` (the operators and the row kernels
around them), ``images`` (weight images of the MFMA kernels, their caches, merged / flattened parameters), ``gemm`` (the dense
projections behind ``linear``, ``KERNEL_SELECTION``, the autograd Function), ``chains`` (projection + LayerNorm and the seam
kernels of an encoder layer; round 6 took ``images`` and ``chains`` out of ``gemm``), ``prologue`` (rotation, flattening), ``attention`` (the decoder's dense self-attention core), ``head`` (the detection head's branch chains and box decode), ``loss`` (the detection loss: match costs, assignment solver, focal + L1 loss), ``optim`` (the optimizer step: gradient norm + AdamW over a job table), ``conv`` (the channel-last 3 x 3 convolution + BatchNorm of BEVFormerV2's temporal fusion), ``neck`` (the image neck: row convolutions with bias / upsampled residual, the FPN schedule), ``backbone`` (the backbone's DCNv2: the offset matrix and the deformable 3 x 3 convolution over channel-last rows; the bottlenecks on rows: convolution + BatchNorm + residual + ReLU per launch, the schedule of a block; the stem — 7 x 7 convolution + BatchNorm + ReLU + max pooling of an NCHW image batch — as one launch; training with frozen norms: the backward of the row convolutions and of the deformable convolution, a bottleneck as one autograd Function), ``norm`` (BatchNorm with batch statistics over channel-last rows: statistics, apply and the backward through the statistics; a bottleneck whose norms are in ``train()`` mode as one autograd Function) —
re-exported here name for name: ``ops.linear``, ``ops.msda_fused`` ... are what the modules call and what the tests
substitute; calls BETWEEN operators go through this namespace too (``_pkg()`` in the submodules).
"""
from . import _base, sampling, images, gemm, chains, prologue, attention, head, loss, optim, conv, neck, backbone, norm

for _mod in (_base, sampling, images, gemm, chains, prologue, attention, head, loss, optim, conv, neck, backbone, norm):
    for _k, _v in vars(_mod).items():
        if not _k.startswith("__") and _k != "_pkg":
            globals()[_k] = _v
del _mod, _k, _v
