"""GPU: the row helpers of csrc/rowops.h against float64 statements on the CPU and on exact cases (inputs, references and
the yardstick E32: tests/rowops_yardstick.py; their premises: tests/test_rowops_yardstick_cpu.py).  Toleranced checks:
max abs error <= 4 x E32 with E32 torch's own float32 CPU evaluation against float64 on the same inputs; every figure is
printed (``pytest -s``)."""
import pytest
import torch

import rowops_yardstick as Y
from bevformer_amd import _lib, ops
from bevformer_amd.ext import _ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _d(t):
    return None if t is None else t.to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ratio(err, e32):
    return err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))


# ---------------------------------------------------------------------------------------------------------------------
# add_layernorm, forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", Y.LN_WIDTHS)
@pytest.mark.parametrize("family", Y.LN_FAMILIES)
def test_add_layernorm_matches_float64(family, C):
    """Rows with a large common offset (a one-pass variance fails these: test_rowops_yardstick_cpu.py), cancelling addends,
    a variance far below eps, eps = 0; rows 1, 2, 3, 5, 9, with and without ``res``.  Bound: 4 x max(E32, E_mean) — E_mean, the
    cost of rounding a row's mean to float32, and the two cases that miss 4 x E32 alone: ``Y.ln_forward_case``.  The case
    with the largest error / E32 per (family, C) on an MI355X:
      offset_1000   C=256  rows=9 res=True:  max abs error 9.023e-05, E32 9.028e-05 (ratio 1.00), E_mean 7.718e-05 (ratio 1.17)
      offset_1000   C=512  rows=9 res=False: max abs error 1.480e-04, E32 1.097e-04 (ratio 1.35), E_mean 1.398e-04 (ratio 1.06)
      offset_1000   C=1024 rows=9 res=False: max abs error 8.178e-05, E32 6.978e-05 (ratio 1.17), E_mean 1.318e-04 (ratio 0.62)
      offset_1      C=256  rows=3 res=False: max abs error 5.152e-05, E32 1.923e-05 (ratio 2.68), E_mean 3.546e-05 (ratio 1.45)
      offset_1      C=512  rows=1 res=True:  max abs error 6.441e-05, E32 6.371e-06 (ratio 10.11), E_mean 3.539e-05 (ratio 1.82)
      offset_1      C=1024 rows=9 res=True:  max abs error 4.315e-05, E32 3.781e-05 (ratio 1.14), E_mean 3.604e-05 (ratio 1.20)
      cancelling    C=256  rows=1 res=True:  max abs error 1.351e-07, E32 1.111e-07 (ratio 1.22), E_mean 4.404e-10
      cancelling    C=512  rows=1 res=True:  max abs error 1.278e-07, E32 1.106e-07 (ratio 1.16), E_mean 2.091e-10
      cancelling    C=1024 rows=3 res=True:  max abs error 1.478e-07, E32 1.401e-07 (ratio 1.06), E_mean 1.353e-09
      tiny_variance C=256  rows=1 res=False: max abs error 5.095e-06, E32 3.432e-06 (ratio 1.48), E_mean 8.530e-06 (ratio 0.60)
      tiny_variance C=512  rows=1 res=False: max abs error 9.341e-06, E32 4.527e-07 (ratio 20.63), E_mean 8.890e-06 (ratio 1.05)
      tiny_variance C=1024 rows=5 res=True:  max abs error 1.698e-05, E32 8.161e-06 (ratio 2.08), E_mean 8.987e-06 (ratio 1.89)
      eps_zero      C=256  rows=2 res=False: max abs error 3.368e-07, E32 2.115e-07 (ratio 1.59), E_mean 5.310e-09
      eps_zero      C=512  rows=2 res=True:  max abs error 4.573e-07, E32 3.817e-07 (ratio 1.20), E_mean 2.651e-09
      eps_zero      C=1024 rows=3 res=True:  max abs error 5.918e-07, E32 3.937e-07 (ratio 1.50), E_mean 3.301e-09
    """
    worst = (-1.0, None)
    fails = []
    for rows in Y.LN_ROWS:
        for with_res in (False, True):
            c = Y.ln_forward_case(family, rows, C, with_res)
            if c is None:
                continue
            got = ops.add_layernorm(_d(c["x"]), _d(c["res"]), _d(c["gamma"]), _d(c["beta"]), c["eps"])
            assert got is not None and got.shape == (rows, C)
            err = (got.cpu().double() - c["want"]).abs().max().item()
            r = _ratio(err, c["e32"])
            line = f"rows={rows} res={with_res}: max abs error {err:.3e}, E32 {c['e32']:.3e} (ratio {r:.2f}), " \
                   f"E_mean {c['e_mean']:.3e} (ratio {_ratio(err, c['e_mean']):.2f})"
            if r > worst[0]:
                worst = (r, line)
            if not err <= Y.FACTOR * c["yard"]:
                fails.append(line)
    print(f"\nadd_layernorm {family} C={C}: {worst[1]}")
    assert not fails, "above 4 x max(E32, E_mean): " + "; ".join(fails)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("C", Y.LN_WIDTHS)
def test_add_layernorm_of_a_constant_row_is_beta(C, with_res):
    """Rows equal to 0, 1, -3, 2^-20: sum and mean are exact, z - mean is 0, the output EQUALS beta."""
    x, res, gamma, beta = Y.ln_constant_case(C, with_res)
    got = ops.add_layernorm(_d(x), _d(res), _d(gamma), _d(beta), 1e-5).cpu()
    assert torch.equal(got, beta[None].expand_as(got))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("C", Y.LN_WIDTHS)
def test_add_layernorm_rows_are_independent(C, bad):
    """One non-finite entry in one row (through ``x``, then through ``res``): exactly that row is NaN, every other row is
    equal to the clean run's.  A 3-D input keeps its shape."""
    rows = 9
    c = Y.ln_forward_case("offset_1", rows, C, True)
    x, res, gamma, beta = (_d(c[k]) for k in ("x", "res", "gamma", "beta"))
    clean = ops.add_layernorm(x, res, gamma, beta, c["eps"])
    assert torch.isfinite(clean).all()
    for r, col, through_res in [(0, 0, False), (4, C - 1, True), (rows - 1, C // 2 + 1, False)]:
        xb, rb = x.clone(), res.clone()
        (rb if through_res else xb)[r, col] = bad
        got = ops.add_layernorm(xb.view(3, 3, C), rb.view(3, 3, C), gamma, beta, c["eps"])
        assert got.shape == (3, 3, C)
        got = got.view(rows, C)
        want_nan = torch.zeros(rows, C, dtype=torch.bool, device=DEV)
        want_nan[r] = True
        assert torch.equal(torch.isnan(got), want_nan)
        assert torch.equal(got[~want_nan], clean[~want_nan])


# ---------------------------------------------------------------------------------------------------------------------
# add_layernorm, backward
# ---------------------------------------------------------------------------------------------------------------------
def _backward(x, res, gamma, g, g2=None, two=False, eps=Y.BWD_EPS):
    """``bevmsda_add_layernorm_backward_f32`` (``two``: ``..._backward2_f32`` with the second addend ``g2``, which may be
    None) on device tensors -> (gx, dgamma, dbeta); the outputs are pre-filled with NaN."""
    rows, C = x.shape
    lib = _lib.load()
    parts = int(lib.bevmsda_add_layernorm_backward_partials(rows))
    scratch = torch.full((max(parts, 1) * 2 * C,), float("nan"), device=DEV)
    gwb = torch.full((2, C), float("nan"), device=DEV)
    gx = torch.full_like(x, float("nan"))
    opt = lambda t: None if t is None else _ptr(t)
    with torch.cuda.device(DEV):
        if two:
            rc = lib.bevmsda_add_layernorm_backward2_f32(_ptr(x), opt(res), _ptr(gamma), _ptr(g), opt(g2), eps, rows, C, _ptr(gx),
                                                         _ptr(scratch), _ptr(gwb), _stream())
        else:
            rc = lib.bevmsda_add_layernorm_backward_f32(_ptr(x), opt(res), _ptr(gamma), _ptr(g), eps, rows, C, _ptr(gx),
                                                        _ptr(scratch), _ptr(gwb), _stream())
    _lib.check(rc, "add_layernorm backward")
    return gx, gwb[0], gwb[1]


def _check_bwd(got, want, e32, what, names=("gx", "dgamma", "dbeta")):
    msgs = []
    for name, a, b in zip(("gx", "dgamma", "dbeta"), got, want):
        if name not in names:
            continue
        err = (a.cpu().double() - b).abs().max().item()
        print(f"\nln backward {what} {name}: max abs error {err:.3e}, E32 {e32[name]:.3e}, ratio {_ratio(err, e32[name]):.2f}")
        if not err <= Y.FACTOR * e32[name]:
            msgs.append(f"{name}: max abs error {err:.3e} > 4 x E32 = {Y.FACTOR * e32[name]:.3e}")
    assert not msgs, f"{what}: " + "; ".join(msgs)


@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
@pytest.mark.parametrize("rows", Y.BWD_ROWS)
def test_add_layernorm_autograd_matches_float64_autograd(rows, C):
    """``ops.add_layernorm_autograd``: gx, dgamma, dbeta within 4 x E32 of float64 autograd (E32 per output; at rows = 1 grad
    beta is g itself in any precision, E32 = 0, and equality is what the bound asks); the gradients of x and of res are the
    same tensor.  8192 rows: the last count at which every wavefront of the backward has one row.  The factor holds; measured
    on an MI355X, max abs error / E32 = ratio (E32 of the column sums depends on the host's thread count):
      rows      C    gx                          dgamma                      dbeta
      1         256  1.372e-07/1.349e-07=1.02    2.508e-07/2.321e-07=1.08    0/0
      1         512  1.959e-07/2.810e-07=0.70    2.520e-07/3.113e-07=0.81    0/0
      3         256  1.730e-07/2.151e-07=0.80    7.971e-07/4.810e-07=1.66    3.576e-07/3.576e-07=1.00
      3         512  1.607e-07/2.743e-07=0.59    6.172e-07/1.158e-06=0.53    2.906e-07/2.906e-07=1.00
      5         256  1.502e-07/1.836e-07=0.82    5.291e-07/4.821e-07=1.10    2.980e-07/4.321e-07=0.69
      5         512  1.972e-07/2.801e-07=0.70    9.028e-07/9.028e-07=1.00    5.662e-07/5.662e-07=1.00
      8192      256  3.829e-07/6.680e-07=0.57    4.321e-05/1.206e-04=0.36    3.657e-05/1.241e-04=0.29
      8192      512  4.199e-07/5.240e-07=0.80    4.950e-05/1.307e-04=0.38    4.541e-05/1.264e-04=0.36
      8193      256  4.910e-07/4.767e-07=1.03    3.723e-05/1.180e-04=0.32    4.541e-05/1.076e-04=0.42
      8193      512  4.134e-07/5.523e-07=0.75    5.208e-05/1.025e-04=0.51    4.352e-05/1.252e-04=0.35
      8197      256  3.947e-07/5.206e-07=0.76    3.772e-05/1.011e-04=0.37    3.644e-05/1.181e-04=0.31
      8197      512  4.195e-07/5.933e-07=0.71    5.883e-05/1.244e-04=0.47    3.742e-05/1.260e-04=0.30
      16389     256  4.325e-07/5.726e-07=0.76    6.485e-05/2.329e-04=0.28    6.623e-05/2.507e-04=0.26
      16389     512  4.587e-07/5.137e-07=0.89    7.138e-05/2.278e-04=0.31    7.751e-05/2.842e-04=0.27
    (the column sums come through atomics in no fixed order: their errors vary from run to run by about a third)
    """
    c = Y.bwd_case(rows, C)
    norm = torch.nn.LayerNorm(C, eps=Y.BWD_EPS).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(c["gamma"])
        norm.bias.copy_(c["beta"])
    x, res = _d(c["x"]).requires_grad_(True), _d(c["res"]).requires_grad_(True)
    y = ops.add_layernorm_autograd(x, res, norm)
    assert y is not None
    assert torch.equal(y.detach(), ops.add_layernorm(x.detach(), res.detach(), norm.weight.detach(), norm.bias.detach(), norm.eps))
    y.backward(_d(c["g"]))
    assert torch.equal(x.grad, res.grad)
    _check_bwd((x.grad, norm.weight.grad, norm.bias.grad), c["want"], c["e32"], f"rows={rows} C={C}")
    # the C entry point itself gives the same bits for gx (row-local arithmetic)
    gx, dg, db = _backward(_d(c["x"]), _d(c["res"]), _d(c["gamma"]), _d(c["g"]))
    assert torch.equal(gx, x.grad)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
def test_add_layernorm_backward_column_sums_are_exact_on_integers(C, two):
    """g integers in {-2..2}: grad beta EQUALS the float64 column sum at every row count — the strided row loop, the per-block
    partials and colsum_partials, whatever the order of the atomics (grad gamma walks the same loop)."""
    for rows in Y.BWD_ROWS:
        x, res, gamma, g, want = Y.bwd_lattice_case(rows, C)
        gx, dg, db = _backward(_d(x), _d(res), _d(gamma), _d(g), None, two)
        assert torch.equal(db.cpu().double(), want), f"rows={rows}"
        assert torch.isfinite(gx).all() and torch.isfinite(dg).all()


@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
@pytest.mark.parametrize("r", Y.live_rows())
def test_add_layernorm_backward_one_live_row(r, C):
    """g zero except row r of 8197 (r = 8192: the first row a wavefront reaches on its second step): gx is exactly 0 in every
    other row, grad beta EQUALS g[r], grad gamma is within the bound of g[r] * xhat64[r].  Measured on an MI355X, the largest
    error / E32 of the eight cases: gx 2.411e-07/1.389e-07=1.74 (r=8192 C=256), dgamma 2.481e-07/1.613e-07=1.54 (r=0 C=256)."""
    c = Y.bwd_live_row_case(C, r)
    gx, dg, db = _backward(_d(c["x"]), _d(c["res"]), _d(c["gamma"]), _d(c["g"]))
    gx = gx.cpu()
    other = torch.ones(Y.BWD_LIVE_ROWS, dtype=torch.bool)
    other[r] = False
    assert (gx[other] == 0).all()
    assert torch.equal(db.cpu(), c["g"][r])
    want_dg = c["g"][r].double() * c["xhat_r"]
    _check_bwd((gx, dg, db), (c["want"][0], want_dg, c["want"][2]), c["e32"], f"live row {r} C={C}", names=("gx", "dgamma"))


@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
@pytest.mark.parametrize("rows", [5, 8197])
def test_add_layernorm_backward2_forms_the_sum_in_the_kernel(rows, C):
    """backward2(g, g2): gx is equal to backward(g + g2) with the sum formed in float32 by torch, grad gamma / grad beta
    match float64 within the bound (their final atomics have no fixed order: no equality); with g2 = None — and with
    res = None, train_ops._ln_backward's call — it is backward(g).  Measured on an MI355X, the largest error / E32 over all
    forms: gx 0.88, dgamma 1.10 (5.291e-07/4.821e-07, rows=5 C=256, g2=None), dbeta 1.00; at 8197 rows the column sums stay
    below 0.53."""
    c = Y.bwd_case(rows, C, "two")
    x, res, gamma, g, g2 = (_d(c[k]) for k in ("x", "res", "gamma", "g", "g2"))
    gsum = g + g2
    assert torch.equal(gsum.cpu(), c["gsum"])
    one = _backward(x, res, gamma, gsum)
    two = _backward(x, res, gamma, g, g2, two=True)
    assert torch.equal(two[0], one[0])
    _check_bwd(two, c["want"], c["e32"], f"backward2 rows={rows} C={C}")
    _check_bwd(one, c["want"], c["e32"], f"backward(g + g2) rows={rows} C={C}")
    plain = _backward(x, res, gamma, g)
    none = _backward(x, res, gamma, g, None, two=True)
    assert torch.equal(none[0], plain[0])
    z = x + res
    zn = _backward(z, None, gamma, g, None, two=True)
    assert torch.equal(zn[0], plain[0])
    want = Y.ln_backward64(c["x"] + c["res"], c["gamma"], c["g"], Y.BWD_EPS)[:3]
    e32 = Y.bwd_errors32(c["x"], c["res"], c["gamma"], c["beta"], c["g"], Y.BWD_EPS, want)
    _check_bwd(none, want, e32, f"backward2 g2=None rows={rows} C={C}")
    _check_bwd(zn, want, e32, f"backward2 g2=None res=None rows={rows} C={C}")


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("C", Y.BWD_WIDTHS)
def test_add_layernorm_backward_of_no_rows_zeroes_the_column_sums(C, two):
    lib = _lib.load()
    gwb = torch.full((2, C), float("nan"), device=DEV)
    with torch.cuda.device(DEV):
        if two:
            rc = lib.bevmsda_add_layernorm_backward2_f32(None, None, None, None, None, Y.BWD_EPS, 0, C, None, None, _ptr(gwb), _stream())
        else:
            rc = lib.bevmsda_add_layernorm_backward_f32(None, None, None, None, Y.BWD_EPS, 0, C, None, None, _ptr(gwb), _stream())
    _lib.check(rc, "add_layernorm backward, no rows")
    assert int(lib.bevmsda_add_layernorm_backward_partials(0)) == 0
    assert (gwb == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# gather_mean, rows_from_slots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("Q,J,R,C", Y.GATHER_SHAPES)
def test_gather_mean_is_the_float32_loop(Q, J, R, C, seed):
    """The J rows added in ascending j, one multiply: equal to that float32 loop on the CPU on randn rows, EQUAL to float64 on
    integer rows with power-of-two scales; all-empty queries give exact zeros; a -1 between two live ids and a row taken
    twice are in every table they fit in."""
    for exact in (False, True):
        rows, idx, scale = Y.gather_case(Q, J, R, C, exact, seed)
        got = ops.gather_mean(_d(rows), _d(idx), _d(scale)).cpu()
        assert got.shape == (Q, C)
        assert torch.equal(got, Y.gather_mean32(rows, idx, scale))
        if exact:
            assert torch.equal(got.double(), Y.gather_mean32(rows.double(), idx, scale.double()))
        empty = (idx < 0).all(1)
        assert (got[empty] == 0).all()
    none = torch.full((Q, J), -1, dtype=torch.int32)
    assert (ops.gather_mean(_d(rows), _d(none), _d(scale)) == 0).all()


@pytest.mark.parametrize("Q,J,R,C", Y.GATHER_SHAPES[1:])
def test_gather_mean_autograd(Q, J, R, C):
    """Forward equal to ``ops.gather_mean``; the gradient of ``rows`` EQUALS (g * scale[:, None])[row_slot]."""
    rows, idx, scale = Y.gather_case(Q, J, R, C, exact=False)
    gen = torch.Generator().manual_seed(Q)
    row_slot = torch.randint(0, Q, (R,), generator=gen)
    g = torch.randn(Q, C, generator=gen)
    rd = _d(rows).requires_grad_(True)
    out = ops.gather_mean_autograd(rd, _d(idx), _d(scale), _d(row_slot))
    assert torch.equal(out.detach(), ops.gather_mean(_d(rows), _d(idx), _d(scale)))
    out.backward(_d(g))
    assert torch.equal(rd.grad.cpu(), (g * scale[:, None])[row_slot])


SENTINEL = -12345.0


@pytest.mark.parametrize("C", [4, 256])
def test_rows_from_slots(C):
    """rows[r] EQUALS slots[row_slot[r]] * scale[row_slot[r]] (one float32 multiply) from a slot matrix with a padded row
    stride; rows at and beyond a device-side count keep what was there; a count above R is R, a negative count writes nothing."""
    R, S, ld = 70, 23, C + 32
    gen = torch.Generator().manual_seed(C)
    slots = torch.randn(S, ld, generator=gen)
    scale = torch.rand(S, generator=gen) + 0.1
    row_slot = torch.randint(0, S, (R,), generator=gen, dtype=torch.int32)
    row_slot[0], row_slot[-1] = S - 1, 0
    want = slots[row_slot.long(), :C] * scale[row_slot.long()][:, None]
    sd, cd, rsd = _d(slots), _d(scale), _d(row_slot)
    lib = _lib.load()
    for count in Y.device_counts(R):
        out = torch.full((R, C), SENTINEL, device=DEV)
        n_dev = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
        with torch.cuda.device(DEV):
            rc = lib.bevmsda_rows_from_slots_f32(_ptr(sd), ld, _ptr(cd), _ptr(rsd), None if n_dev is None else n_dev.data_ptr(),
                                                 R, C, _ptr(out), _stream())
        _lib.check(rc, "rows_from_slots")
        n = Y.rows_written(count, R)
        out = out.cpu()
        assert torch.equal(out[:n], want[:n]), f"count={count}"
        assert (out[n:] == SENTINEL).all(), f"count={count}"


# ---------------------------------------------------------------------------------------------------------------------
# cast_rows_bf16
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL_BITS = 0x7B7B


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("C", [8, 264])
def test_cast_rows_bf16(C, scale):
    """Round to nearest even, bit for bit the CPU's ``(a * scale).to(torch.bfloat16)`` on ties both ways, a carry into the
    exponent, overflow to inf, zeros, infinities and denormals; a NaN stays a NaN; the device-side row count as above."""
    R = 33
    a, nan = Y.cast_case(R, C)
    want = (a * scale).to(torch.bfloat16).view(torch.int16)
    ad = _d(a)
    lib = _lib.load()
    for count in Y.device_counts(R):
        out = torch.full((R, C), SENTINEL_BITS, dtype=torch.int16, device=DEV)
        n_dev = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
        with torch.cuda.device(DEV):
            rc = lib.bevmsda_cast_rows_bf16(_ptr(ad), None if n_dev is None else n_dev.data_ptr(), R, C, scale, _ptr(out), _stream())
        _lib.check(rc, "cast_rows_bf16")
        n = Y.rows_written(count, R)
        out = out.cpu()
        got, ref, isnan = out[:n], want[:n], nan[:n]
        assert torch.equal(got[~isnan], ref[~isnan]), f"count={count}"
        assert torch.isnan(got.view(torch.bfloat16)[isnan]).all(), f"count={count}"
        assert (out[n:] == SENTINEL_BITS).all(), f"count={count}"
