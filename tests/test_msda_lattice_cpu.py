"""Exactness certificate of the lattice cases (tests/helpers.py: ``make_lattice_case``, ``make_lattice_fused_case``), from the
reference alone — no kernel involved.  tests/test_msda_lattice_gpu.py compares the HIP kernels with the C oracle by
``torch.equal`` on these cases; that is legitimate only if every result is exactly representable whatever the order of the
operations, which is what is asserted here:

  * the pixel coordinates ``loc * (W, H) - 0.5`` are the same numbers in fp32 (the kernels) and in double (the oracle) and lie
    on the quarter-pixel lattice, every lattice point of every level from -1.25 to side + 0.25 occurring — so ``floor`` and
    every range / tap predicate see the same operands on both sides;
  * every expected tensor is an integral multiple of its quantum (``LATTICE_QUANTA``);
  * the oracle on |value|, |grad_out| (same locations and weights) — an upper bound of every partial sum of the terms of an
    output element in any order — stays below 2^22 quanta, so no partial sum needs more than fp32's 24 bits."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import helpers as H                                                             # noqa: E402
from oracle import bevformer_cpu as O                                           # noqa: E402
from oracle import msda_c                                                       # noqa: E402

RESULTS = ("out", "grad_value", "grad_loc", "grad_attn")


def _assert_on_lattice(sh, loc, finite_only=False):
    """fp32 and double pixel coordinates agree, are multiples of 1/4 and cover the whole lattice of every level."""
    p32, p64 = H.pixel_coordinates(sh, loc, torch.float32), H.pixel_coordinates(sh, loc, torch.float64)
    ok = torch.isfinite(loc).all(-1, keepdim=True).expand_as(p32) & (loc.abs() < 1e29).all(-1, keepdim=True) if finite_only \
        else torch.ones_like(p32, dtype=torch.bool)
    assert torch.equal(p32.double()[ok], p64[ok])
    assert torch.equal((p64 * 4)[ok], (p64 * 4).round()[ok])
    for l, (Hh, W) in enumerate(sh.tolist()):
        pts, keep = p64[:, :, :, l].reshape(-1, 2), ok[:, :, :, l].reshape(-1, 2).all(-1)
        seen = set(map(tuple, (pts[keep] * 4).long().tolist()))
        assert set(map(tuple, (H.lattice_points(Hh, W) * 4).long().tolist())) <= seen, f"level {l}: lattice points missing"
    return p32, p64, ok


def _assert_quanta(ref):
    for k in RESULTS:
        q = ref[k].double() / H.LATTICE_QUANTA[k]
        assert torch.equal(q, q.round()), k
    bound = H._with_oracle(ref["value"].abs(), ref["shapes"], ref["start"], ref["loc"], ref["attn"], ref["grad_out"].abs())
    for k in RESULTS:
        assert (bound[k].double().abs() / H.LATTICE_QUANTA[k]).max() < 2 ** 22, k
        assert (ref[k].abs() <= bound[k].abs()).all() or k == "grad_loc"       # (differences of taps: not monotone in |value|)


@pytest.mark.parametrize("name", sorted(H.LATTICE_CASES))
def test_lattice_case_is_exact(name):
    ref = H.lattice_reference(name)
    _assert_on_lattice(ref["shapes"], ref["loc"])
    _assert_quanta(ref)
    for k, lo, hi, scale in (("value", -4, 4, 1), ("grad_out", -2, 2, 1), ("attn", 0, 8, 64)):
        t = ref[k] * scale
        assert torch.equal(t, t.round()) and t.min() == lo and t.max() == hi
        assert torch.equal(ref[k].bfloat16().float(), ref[k]) or k == "attn"    # exact in bf16 storage
    assert (ref["attn"] == 0).any()
    # the grid_sample statement in fp32 is the same function on these inputs, bit for bit, and so is any order of the points
    assert torch.equal(O.msda_gridsample(ref["value"], ref["shapes"], ref["loc"], ref["attn"]), ref["out"])
    perm = torch.randperm(ref["loc"].shape[4], generator=torch.Generator().manual_seed(0))
    assert torch.equal(msda_c.forward(ref["value"], ref["shapes"], ref["start"], ref["loc"][:, :, :, :, perm].contiguous(),
                                      ref["attn"][:, :, :, :, perm].contiguous()), ref["out"])


@pytest.mark.parametrize("name", H.NONFINITE_CASES)
def test_nonfinite_case_is_exact_and_the_oracle_skips_the_points(name):
    ref = H.nonfinite_reference(name)
    _, p64, ok = _assert_on_lattice(ref["shapes"], ref["loc"], finite_only=True)
    bad = ref["bad"]
    assert bad.numel() == 15 and int((~ok.view(-1, 2).all(-1)).sum()) == 15
    # NaN, +inf, -inf, 1e30, -1e30 each in x only, y only, both
    flat = ref["loc"].view(-1, 2)[bad]
    assert int(torch.isnan(flat).any(-1).sum()) == 3 and int(torch.isinf(flat).any(-1).sum()) == 6
    _assert_quanta(ref)
    for k in RESULTS:
        assert torch.isfinite(ref[k]).all()
    assert torch.count_nonzero(ref["grad_loc"].view(-1, 2)[bad]) == 0 and torch.count_nonzero(ref["grad_attn"].view(-1)[bad]) == 0
    # ... and they do carry weight in some of these points: the zero is the range test's, not the weight's
    assert torch.count_nonzero(ref["attn"].view(-1)[bad]) > 0


@pytest.mark.parametrize("exact_softmax", [False, True])
@pytest.mark.parametrize("kind", ["sca", "tsa"])
def test_fused_lattice_case(kind, exact_softmax):
    ref = H.fused_lattice_reference(kind, exact_softmax)
    sh, kw = ref["shapes"], ref["kw"]
    loc = ref["loc"]                                                            # (R, K, M, L, P, 2), formed in fp32
    _assert_on_lattice(sh, loc)
    # the same locations in double from the double operands: the fp32 sum ref + off / (W, H) was exact
    loc64 = H.fused_lattice_locations(sh, ref["proj"].double(), ref["n_off"], ref["ref"].double(), **kw)
    assert torch.equal(loc.double(), loc64.double())
    assert ref["zero_rows"].numel() >= 3 and torch.count_nonzero(ref["out"][ref["zero_rows"]]) == 0
    assert torch.count_nonzero(ref["out"]) > 0 and torch.isfinite(ref["grad_proj"]).all()
    if exact_softmax:
        # weights are 0 or 1 / 2^k: out is a multiple of 2^-4 (bilinear) * 2^-5 (weight) * 2^-1 (queue mean) * integers
        proj = ref["proj"] if kw.get("row_src") is None else ref["proj"][kw["row_src"].long()]
        att = proj[:, ref["n_off"]:].reshape(proj.shape[0], kw["M"], kw["K"], -1).softmax(-1)
        inv = 1 / att[att > 0]
        assert torch.equal(inv, inv.round()) and ((inv.long() & (inv.long() - 1)) == 0).all() and (att == 0).any()
        # likewise grad_value, and the offset columns of grad_proj (grad_loc / (W, H), summed over the rows that share the
        # projection row); the logit columns go through aw * (ga - sum aw * ga), whose intermediates are not certified here
        for k, t in (("out", ref["out"]), ("grad_value", ref["grad_value"]), ("grad_offsets", ref["grad_proj"][:, :ref["n_off"]])):
            q = t.double() * 2 ** 10
            assert torch.equal(q, q.round()) and q.abs().max() < 2 ** 22, k
