"""The sampling kernels ON the pixel lattice and the map borders, bit for bit.

Every other test of the sampling kernels draws its locations from a continuous distribution: no point lands on a pixel
centre, on a pixel edge or at x = -1, W - 1, W — where the operator's definition branches (the point-level range test, the
four per-tap tests, the half-weight band -1 < x < 0), and where those branches are written out by hand in every kernel
(``make_tap``, ``point_params_xy``, ``grad_point_params``, the LDS-sort grad_value kernel, the two-taps-per-request bf16
forward).  The cases here (tests/helpers.py: ``make_lattice_case``) put every point on the quarter-pixel lattice from -1.25 to
side + 0.25 of power-of-two levels, with small-integer values and weights k / 64: every product and partial sum is a dyadic
number of few bits (certified from the reference alone by tests/test_msda_lattice_cpu.py), so the kernels must reproduce the
C oracle EXACTLY — ``torch.equal``, no tolerance, no point excluded — whatever their summation order, FMA contraction or
atomic order.  grad_loc follows the operator's convention at the kinks (the slope of the floor cell; nothing outside
(-1, W) x (-1, H)), which is the C oracle's, not autograd's through ``grid_sample``.

The fused front end's softmax and division are not exact: compared at the tolerances of tests/test_msda_gpu.py, nothing
excluded — and exactly where the softmax is (logits in {0, -200}: weights 0 or 1 / 2^k)."""
import ctypes
import os
import sys

import pytest
import torch

from bevformer_amd import _lib
from bevformer_amd import ext
from bevformer_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import helpers as H                                                             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D32 = ["d32_p8", "d32_p4", "d32_grid"]
OPERANDS = ("value", "shapes", "start", "loc", "attn")


def _gpu(ref, *keys):
    return [ref[k].to(DEV) for k in keys]


def _backward(ref, value_dtype=torch.float32, tuning=None):
    """The operator's backward into NaN-filled grad_loc / grad_attn (overwritten by contract) and a zeroed grad_value."""
    v, sh, st, loc, attn = _gpu(ref, *OPERANDS)
    v = v.to(value_dtype)
    g = ref["grad_out"].to(DEV).to(value_dtype)
    gv = torch.zeros(v.shape, device=DEV)
    gl = torch.full_like(loc, float("nan"))
    ga = torch.full_like(attn, float("nan"))
    ext.ms_deform_attn_backward(v, sh, st, loc, attn, g, gv, gl, ga, tuning=ctypes.byref(tuning) if tuning is not None else None)
    return gv.cpu(), gl.cpu(), ga.cpu()


def _assert_gradients_equal(got, ref):
    gv, gl, ga = got
    assert torch.equal(ga, ref["grad_attn"])
    assert torch.equal(gl, ref["grad_loc"])
    assert torch.equal(gv, ref["grad_value"])


@pytest.mark.parametrize("name", sorted(H.LATTICE_CASES))
def test_forward_fp32_is_the_oracle_bit_for_bit(name):
    ref = H.lattice_reference(name)
    got = ext.ms_deform_attn_forward(*_gpu(ref, *OPERANDS)).cpu()
    assert torch.equal(got, ref["out"])


@pytest.mark.parametrize("name", sorted(H.LATTICE_CASES))
def test_backward_fp32_is_the_oracle_bit_for_bit(name):
    ref = H.lattice_reference(name)
    _assert_gradients_equal(_backward(ref), ref)


@pytest.mark.parametrize("rows", [64, 128, 256])
@pytest.mark.parametrize("name", D32)
def test_backward_at_every_workgroup_shape_of_the_sort_kernel(name, rows):
    ref = H.lattice_reference(name)
    t = _lib.Tuning()
    t.reserved[0] = rows
    _assert_gradients_equal(_backward(ref, tuning=t), ref)


@pytest.mark.parametrize("variant", [1, 3])
@pytest.mark.parametrize("name", D32)
def test_backward_first_generation_and_generic_kernels_at_d32(name, variant):
    """``bevmsda_tuning.variant`` 3: the first-generation D = 32 backward (one atomic per tap), 1: the generic lane-group kernels."""
    ref = H.lattice_reference(name)
    t = _lib.Tuning(variant=variant)
    got = ext.ms_deform_attn_forward(*_gpu(ref, *OPERANDS), tuning=ctypes.byref(t)).cpu()
    assert torch.equal(got, ref["out"])
    _assert_gradients_equal(_backward(ref, tuning=t), ref)


@pytest.mark.parametrize("name", D32)
def test_ragged_entry_point_with_row_batch(name):
    """Rows of batch entry 1 first, then entry 0's: the ragged forward and backward (``row_batch``) on the permuted rows."""
    ref = H.lattice_reference(name)
    N, Q = ref["loc"].shape[:2]
    R = N * Q
    perm = torch.cat([torch.arange(Q, R), torch.arange(Q)])
    v, sh, st = _gpu(ref, "value", "shapes", "start")
    loc = ref["loc"].flatten(0, 1)[perm].contiguous().to(DEV)
    attn = ref["attn"].flatten(0, 1)[perm].contiguous().to(DEV)
    rb = (perm // Q).to(torch.int32).to(DEV)
    with torch.no_grad():
        out = ops.msda_ragged(v, sh, st, loc, attn, rb)
    assert torch.equal(out.cpu(), ref["out"].flatten(0, 1)[perm])
    g = ref["grad_out"].flatten(0, 1)[perm].contiguous().to(DEV)
    gv = torch.zeros_like(v)
    gl = torch.full_like(loc, float("nan"))
    ga = torch.full_like(attn, float("nan"))
    S, M, D = v.shape[1:]
    L, P = loc.shape[2:4]
    _lib.check(_lib.load().bevmsda_backward_ragged_f32(
        v.data_ptr(), sh.data_ptr(), st.data_ptr(), loc.data_ptr(), attn.data_ptr(), rb.data_ptr(), g.data_ptr(),
        N, S, M, D, L, R, P, gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), torch.cuda.current_stream().cuda_stream), "ragged backward")
    assert torch.equal(ga.cpu(), ref["grad_attn"].flatten(0, 1)[perm])
    assert torch.equal(gl.cpu(), ref["grad_loc"].flatten(0, 1)[perm])
    assert torch.equal(gv.cpu(), ref["grad_value"])


# ----------------------------------------------------------------- bf16 value storage
@pytest.mark.parametrize("lanes8", [False, True])
@pytest.mark.parametrize("name", D32)
def test_bf16_storage_is_exact_too(name, lanes8):
    """value and grad_out are exact in bf16: the fp32 gradients are the oracle's bit for bit with the 16-byte-lane gather kernel
    and with the 8-byte-lane one, the bf16 output is the oracle's rounded ONCE."""
    ref = H.lattice_reference(name)
    v, sh, st, loc, attn = _gpu(ref, *OPERANDS)
    out = ext.ms_deform_attn_forward(v.bfloat16(), sh, st, loc, attn)
    assert out.dtype == torch.bfloat16 and torch.equal(out.cpu(), ref["out"].bfloat16())
    t = _lib.Tuning()
    t.reserved[3] = int(lanes8)
    _assert_gradients_equal(_backward(ref, torch.bfloat16, tuning=t), ref)
    # and as the modules reach them (ops.using -> MultiScaleDeformableAttnFunction_bf16)
    v, loc, attn = v.requires_grad_(True), loc.requires_grad_(True), attn.requires_grad_(True)
    with ops.using(value_storage=torch.bfloat16, bf16_lanes8=lanes8):
        out = ops.msda(v, sh, st, loc, attn)
        out.backward(ref["grad_out"].to(DEV))
    assert torch.equal(out.detach().cpu(), ref["out"].bfloat16().float())
    _assert_gradients_equal((v.grad.cpu(), loc.grad.cpu(), attn.grad.cpu()), ref)


# ----------------------------------------------------------------- non-finite and far locations
@pytest.mark.parametrize("store", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", H.NONFINITE_CASES)
def test_nonfinite_and_far_locations_contribute_nothing(name, store):
    """NaN, +inf, -inf, 1e30, -1e30 in x, in y, in both: the point fails the range test — no contribution, zero grad_loc and
    grad_attn, like the oracle and the reference operator (input validation of finite kernels: nothing faults)."""
    ref = H.nonfinite_reference(name)
    v, sh, st, loc, attn = _gpu(ref, *OPERANDS)
    out = ext.ms_deform_attn_forward(v.to(store), sh, st, loc, attn).cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref["out"].to(store))
    gv, gl, ga = _backward(ref, store)
    bad = ref["bad"]
    print("grad_attn at the points:", ga.view(-1)[bad].tolist())
    print("grad_loc at the points:", gl.view(-1, 2)[bad].tolist())
    assert torch.isfinite(gv).all()
    assert torch.count_nonzero(ga.view(-1)[bad]) == 0 and torch.count_nonzero(gl.view(-1, 2)[bad]) == 0
    _assert_gradients_equal((gv, gl, ga), ref)


@pytest.mark.parametrize("lanes8", [False, True])
def test_nonfinite_locations_bf16_gather_kernels(lanes8):
    ref = H.nonfinite_reference("d32_p8")
    t = _lib.Tuning()
    t.reserved[3] = int(lanes8)
    _assert_gradients_equal(_backward(ref, torch.bfloat16, tuning=t), ref)


# ----------------------------------------------------------------- fused front end
def _fused(ref, value=None, proj=None, fn=ops.msda_fused):
    kw = dict(ref["kw"])
    rs, rb = kw.pop("row_src", None), ref["row_batch"]
    return fn(ref["value"].to(DEV) if value is None else value, ref["shapes"].to(DEV), ref["start"].to(DEV),
              ref["proj"].to(DEV) if proj is None else proj, ref["n_off"], ref["ref"].to(DEV),
              rb.to(DEV) if rb is not None else None, row_src=rs.to(DEV) if rs is not None else None, **kw)


@pytest.mark.parametrize("fused_spec", [0, 1])
@pytest.mark.parametrize("kind", ["sca", "tsa"])
def test_fused_front_end_on_the_lattice(kind, fused_spec):
    """SCA (ref_mode 0, shared projection rows) and TSA (two queue entries) with every location on the lattice, both body
    selections.  Softmax and division are not exact: the tolerances of test_fused_front_end_matches_unfused_oracle, nothing
    excluded; rows whose points are all outside their maps are EXACTLY zero."""
    ref = H.fused_lattice_reference(kind, False)
    with ops.using(fused_spec=fused_spec):
        got = _fused(ref)
    assert got is not None
    got = got.cpu()
    torch.testing.assert_close(got, ref["out"], rtol=1e-4, atol=2e-5)
    assert ref["zero_rows"].numel() >= 3 and torch.count_nonzero(got[ref["zero_rows"]]) == 0


@pytest.mark.parametrize("path", ["fp32_spec0", "fp32_spec1", "bf16_lanes16", "bf16_lanes8"])
@pytest.mark.parametrize("kind", ["sca", "tsa"])
def test_fused_front_end_is_exact_where_its_softmax_is(kind, path):
    """Logits in {0, -200} with a power-of-two count of zeros: exp(0) = 1, exp(-200) = 0, 1 / 2^k — the fused kernels are then
    exact as well: fp32 bodies, the bf16 16-byte-lane kernel (two x-adjacent taps per request, fp32 output rows) bit for
    bit, the bf16 8-byte-lane kernel (bf16 output) after ONE rounding."""
    ref = H.fused_lattice_reference(kind, True)
    modes = dict(fp32_spec0=dict(fused_spec=0), fp32_spec1=dict(fused_spec=1),
                 bf16_lanes16=dict(value_storage=torch.bfloat16, bf16_lanes8=False),
                 bf16_lanes8=dict(value_storage=torch.bfloat16, bf16_lanes8=True))[path]
    with ops.using(**modes):
        got = _fused(ref)
    assert got is not None
    if path == "bf16_lanes8":
        assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), ref["out"].bfloat16())
    else:
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), ref["out"])


@pytest.mark.parametrize("store", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("exact_softmax", [False, True])
@pytest.mark.parametrize("kind", ["sca", "tsa"])
def test_fused_autograd_on_the_lattice(kind, exact_softmax, store):
    """``ops.msda_fused_autograd`` against the contract's statement differentiated through the C oracle's backward (the
    operator's own grad_loc convention at the kinks): the tolerances of test_fused_autograd_function_matches_unfused_autograd;
    with an exact softmax the output, grad_value and the offset columns of the projection gradient are exact."""
    ref = H.fused_lattice_reference(kind, exact_softmax)
    value = ref["value"].to(DEV).requires_grad_(True)
    proj = ref["proj"].to(DEV).requires_grad_(True)
    with ops.using(value_storage=store):
        out = _fused(ref, value, proj, fn=ops.msda_fused_autograd)
        out.backward(ref["grad_out"].to(DEV))
    out, gv, gp = out.detach().float().cpu(), value.grad.cpu(), proj.grad.cpu()
    n_off = ref["n_off"]
    torch.testing.assert_close(out, ref["out"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(gv, ref["grad_value"], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(gp, ref["grad_proj"], rtol=1e-3, atol=2e-4)
    assert torch.count_nonzero(out[ref["zero_rows"]]) == 0
    if exact_softmax:
        assert torch.equal(out, ref["out"])
        assert torch.equal(gv, ref["grad_value"])
        assert torch.equal(gp[:, :n_off], ref["grad_proj"][:, :n_off])
