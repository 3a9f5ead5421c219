"""Shared helpers of the ``ops`` modules: the modes of the calling thread, cache keys, the kernel and GEMM timers, the launch
tail every operator ends in (``_launch``) and the operand idioms around it."""
import torch

from .. import _lib
from ..ext import _ptr
from .. import modes as _modes


def _forward_modes(backward):
    """Decorator of an autograd Function's ``backward``: runs it under the modes its ``forward`` saw (``ctx.modes``) —
    the autograd engine calls backward on its own thread, outside any ``using`` block of the caller."""
    import functools

    @functools.wraps(backward)
    def wrapped(ctx, *grads):
        with _modes.activate(ctx.modes):
            return backward(ctx, *grads)
    return wrapped


def _ver(t):
    """Version counter of a tensor for cache keys; inference tensors (``torch.inference_mode``) track none — and cannot
    be written to outside inference mode — so their address alone keys the cache."""
    return 0 if t.is_inference() else t._version


def _m():
    """The modes of this call (bevformer_amd/modes.py): the calling thread's ``using`` block or the process defaults."""
    return _modes.current()


_TIMER = {"cb": None}


def set_kernel_timer(cb):
    """``cb(tag, algorithmic_bytes)`` must return a context manager; it brackets
    every sampling-kernel launch (bench.py records HIP events on the launch
    stream with it).  ``None`` removes the hook."""
    _TIMER["cb"] = cb


class _NoTimer:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_TIMER = _NoTimer()


def _timed(tag, value, loc, attn, out_elems):
    cb = _TIMER["cb"]
    if cb is None:
        return _NoTimer()
    alg = value.numel() * value.element_size() + loc.numel() * 4 + attn.numel() * 4 \
        + out_elems * value.element_size()
    return cb(tag, alg)


_GEMM_TIMER = {"cb": None}          # ``set_gemm_timer`` (ops/gemm.py): ``cb(tag, flops, bytes)`` -> context manager


def _gemm_ctx(tag, flops, nbytes):
    """The GEMM timer's context for one launch (``_launch(timer=...)``), or ``None`` when no timer is registered."""
    cb = _GEMM_TIMER["cb"]
    return cb(tag, flops, nbytes) if cb is not None else None


def _declined(rc, what, also_declined=(), required=False):
    """Classify a launch's return code: 0 -> ``False``; unsupported / misaligned / a code of ``also_declined`` -> ``True`` (the
    library declines the call and the caller takes its other path) unless the call is ``required``; anything else raises with
    ``what`` in the message."""
    if not required and (rc in (_lib.ERR_UNSUPPORTED, _lib.ERR_MISALIGNED) or rc in also_declined):
        return True
    _lib.check(rc, what)
    return False


def _launch(device, what, call, *, timer=None, also_declined=(), required=False):
    """The tail every launch shares: ``rc = call(lib, stream)`` on ``device``'s current stream, bracketed by ``timer`` (an
    already-built context: ``_gemm_ctx(...)``, ``_timed(...)``; ``None`` = untimed) -> ``True``, or ``False`` where the library
    declines the call (``_declined``).  ``required``: a call that has no other path — every non-zero code raises."""
    with torch.cuda.device(device), (timer if timer is not None else _NO_TIMER):
        rc = call(_lib.load(), torch.cuda.current_stream().cuda_stream)
    return rc == 0 or not _declined(rc, what, also_declined, required)


def _aligned(w):
    """``w`` as a weight operand of the kernels: itself when its columns are contiguous, its row stride a multiple of four floats
    and its address of 16 bytes, else a contiguous copy."""
    return w if (w.stride(-1) == 1 and w.stride(0) % 4 == 0 and w.data_ptr() % 16 == 0) else w.contiguous()


def _precision():
    """``precision`` of the descriptors: 0 = every fp32 operand split into two bf16 terms, 1 = operands rounded to bf16."""
    return 0 if _m().gemm == "split" else 1


def _optr(t):
    """Device pointer of an optional tensor (``None`` stays ``None``)."""
    return _ptr(t) if t is not None else None


def value_storage():
    return _m().value_storage


def modes():
    """The modes of this call (read-only use; edit through ``using`` or the ``set_*`` functions)."""
    return _m()


def using(**overrides):
    """``with ops.using(gemm="bf16", value_storage=torch.bfloat16): ...`` — modes for the calling thread only
    (``bevformer_amd.modes.using``); the ``set_*`` functions below edit the process-wide defaults instead."""
    return _modes.using(**overrides)


def set_value_storage(dtype):
    """fp32 (reference semantics, default) or bf16 storage of the projected
    value tensor inside the sampling kernels (fp32 arithmetic either way)."""
    assert dtype in (torch.float32, torch.bfloat16)
    _modes.process_defaults().value_storage = dtype


_ZERO_SCALARS = {}


def _zero_scalar(dtype, device):
    """A 0-d zero per (dtype, device), made once (outside any stream capture): the zero-stride placeholder gradients of
    tensors whose real gradient travels through a sink."""
    key = (dtype, torch.device(device))
    z = _ZERO_SCALARS.get(key)
    if z is None:
        if torch.cuda.is_current_stream_capturing():
            return torch.zeros((), dtype=dtype, device=device)
        z = _ZERO_SCALARS[key] = torch.zeros((), dtype=dtype, device=device)
    return z
