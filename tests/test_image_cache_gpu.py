"""GPU: every weight image of ``ops/images.py`` is cached on its tensor until the tensor is written to, and the launches of an
encoder frame — their count, order, tags and the FLOP / byte figures they report to the timers — are the recorded ones
(tests/golden/host_launch_tiny.json, recorded by ``_launch_record`` below before the host layer's launch tails were merged)."""
import contextlib
import json
import os

import pytest
import torch

from bevformer_amd import ops
from bevformer_amd import synthetic as S

from helpers import build_pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_launch_tiny.json")


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def test_panel_weight_is_cached_until_written():
    x, w = _rand(64, 256, seed=1), _rand(64, 256, seed=2)
    with torch.no_grad(), ops.using(gemm="split", gemm_kernel="panel64"):
        y1 = ops.linear(x, w)
        blob = w._bevmsda_panel[1]
        ops.linear(x, w)
        assert w._bevmsda_panel[1] is blob
        w.mul_(2.0)                                   # in-place write bumps the version
        y2 = ops.linear(x, w)
        assert w._bevmsda_panel[1] is not blob
    torch.testing.assert_close(y2, 2 * y1, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("image,attr,shape", [("conv3x3_weight", "_bevmsda_conv3", (32, 32, 3, 3)),
                                              ("conv1x1_weight", "_bevmsda_conv1", (32, 32, 1, 1))])
def test_conv_weight_is_cached_until_written(image, attr, shape):
    w = _rand(*shape, seed=3)
    fn = getattr(ops, image)
    with torch.no_grad():
        blob = fn(w)
        assert blob is not None and getattr(w, attr)[1] is blob
        assert fn(w) is blob
        w.mul_(2.0)
        again = fn(w)
        assert again is not blob and getattr(w, attr)[1] is again
    assert not torch.equal(again, blob)               # (packed from the new values: a factor of two moves every exponent)


def test_dcn_offset_weight_is_cached_until_weight_or_bias_is_written():
    w, b = _rand(27, 32, 3, 3, seed=4), _rand(27, seed=5)
    with torch.no_grad():
        blob, b32 = ops.dcn_offset_weight(w, b)
        assert w._bevmsda_dcnoff[1][0] is blob and w._bevmsda_dcnoff[1][1] is b32
        assert torch.equal(b32[:27], b) and not b32[27:].any()
        again = ops.dcn_offset_weight(w, b)
        assert again[0] is blob and again[1] is b32
        w.mul_(2.0)
        second = ops.dcn_offset_weight(w, b)
        assert second[0] is not blob and w._bevmsda_dcnoff[1][0] is second[0] and not torch.equal(second[0], blob)
        b.add_(1.0)                                   # a write to the bias alone rebuilds it too
        third = ops.dcn_offset_weight(w, b)
        assert third[0] is not second[0] and third[1] is not second[1] and w._bevmsda_dcnoff[1][0] is third[0]
        assert torch.equal(third[1][:27], b) and torch.equal(third[0], second[0])


def test_transposed_weight_copy_is_cached_until_written():
    w = _rand(40, 64, seed=6)
    with torch.no_grad(), ops.using(weight_views=False):
        wt = ops.transposed_weight(w)
        assert wt.is_contiguous() and torch.equal(wt, w.t()) and w._bevmsda_wt[1] is wt
        assert ops.transposed_weight(w) is wt
        w.mul_(2.0)
        again = ops.transposed_weight(w)
        assert again is not wt and torch.equal(again, w.t())


@contextlib.contextmanager
def _timers(seen):
    @contextlib.contextmanager
    def gemm_cb(tag, flops, nbytes):
        seen.append(["gemm", tag, flops, nbytes])
        yield

    @contextlib.contextmanager
    def kernel_cb(tag, nbytes):
        seen.append(["kernel", tag, nbytes])
        yield

    ops.set_gemm_timer(gemm_cb)
    ops.set_kernel_timer(kernel_cb)
    try:
        yield
    finally:
        ops.set_gemm_timer(None)
        ops.set_kernel_timer(None)


def _launch_record():
    """What the timers see of the ``tiny`` encoder with history: {"frame": one no-grad frame, "step": one differentiable forward
    + backward}, each the list of ["gemm", tag, flops, bytes] / ["kernel", tag, bytes] in launch order."""
    enc, _ = build_pair("tiny", device=DEV)
    q, f, kw = S.make_inputs("tiny", seed=0, temporal=True, device=DEV)
    gout = torch.randn(1, q.shape[0], 256, generator=torch.Generator().manual_seed(2)).to(DEV)
    frame, step = [], []
    with _timers(frame), torch.no_grad():
        enc(q, f, f, **kw)
    with _timers(step):
        qd, fd = q.clone().requires_grad_(True), f.clone().requires_grad_(True)
        enc(qd, fd, fd, **kw).backward(gout)
    torch.cuda.synchronize()
    return json.loads(json.dumps({"frame": frame, "step": step}))


def test_launches_and_timer_figures_of_a_tiny_frame_are_the_recorded_ones():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = _launch_record()
    for part in ("frame", "step"):
        assert len(got[part]) == len(want[part]), f"{part}: {len(got[part])} launches, recorded {len(want[part])}"
        for i, (a, b) in enumerate(zip(got[part], want[part])):
            assert a == b, f"{part}: launch {i} reports {a}, recorded {b}"
