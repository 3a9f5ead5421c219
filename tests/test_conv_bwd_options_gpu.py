"""GPU: the options of ``ops.conv_bn_rows_backward`` that the neck's backward needs (csrc/conv_bwd_rows.h), each alone, against
float64 (tests/backbone_train_yardstick.py's ``conv_bwd64`` plus the option's own statement in float64):

* ``add_pool2`` — ``add`` is the rows of the (2H, 2W) map and its 2 x 2 sums are added: the transpose of a nearest 2 x upsampling;
* ``add_after_mask`` — ``conv_transpose * (next_mask > 0) + add`` in place of ``(conv_transpose + add) * (next_mask > 0)``;
* ``relu_x`` — the weight gradient of a convolution that read ``relu(x)``;
* ``db_out`` — the bias gradient ``gz.sum(0)`` from the weight-gradient launch.

On the integer lattice of ``fpn_yardstick`` (g in {-2..2}, x and add in {-4..4}, w in {-2..2}, scales exactly 1 or 2) every operand
is a bf16 number and every sum stays far below 2^24: the results EQUAL float64 in ``split`` and in ``bf16``.  One random case per
option in ``split``: error <= 3 x the error of the parent — the same kernel with the option off plus the torch fp32 statement that
replaces it (``4 * avg_pool2d``, the reordered add, ``relu(x)``, ``gz.sum(0)``).

Shapes, the smallest at which each mechanism can go wrong: two images (the fine rows of the second start at 4 H W); coarse 3 x 5
(one partial 128-row tile) and 9 x 15 (270 rows: two full tiles and a partial one; for the weight gradient three row slices, so
more than one workgroup adds to a column of ``dbias``); an ``add`` whose row stride exceeds its width; stride 2 from 3 x 5 to 2 x 3
(odd sizes); ``c_out`` 160 (a second, partial 128-column tile)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import backbone_train_yardstick as T
import backbone_yardstick as Y

pytestmark = pytest.mark.gpu

MODES = ["split", "bf16"]
N_IMG = 2


def _unit_bn(co):
    return (torch.ones(co), torch.zeros(co), torch.zeros(co), torch.ones(co), 0.0)


def _bn_of(vecs, eps):
    bn = torch.nn.BatchNorm2d(vecs[0].numel(), eps=eps).eval()
    with torch.no_grad():
        for p, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), vecs):
            p.copy_(v)
    for p in bn.parameters():
        p.requires_grad = False
    return bn.cuda()


def _zeros_in(t, g, every=4):
    return t * (torch.randint(0, every, t.shape, generator=g) != 0).to(t.dtype)


@functools.lru_cache(maxsize=None)
def _inputs(hw, ci, co, taps, stride, lattice, seed=0):
    """CPU tensors of one geometry, made once and shared; nobody writes to them."""
    H, W = hw
    g = torch.Generator().manual_seed(7000 + 100 * H + 10 * taps + stride + ci + co + 1000 * int(lattice) + seed)
    Ho, Wo = Y.out_hw(H, W, stride)
    k = 3 if taps == 9 else 1
    if lattice:
        L = lambda shape, m: Y.lattice(shape, -m, m, g)
        t = dict(g=L((N_IMG, co, Ho, Wo), 2), y=L((N_IMG, co, Ho, Wo), 1), x=L((N_IMG, ci, H, W), 4), w=L((co, ci, k, k), 2),
                 add=L((N_IMG, ci, H, W), 4), fine=L((N_IMG, ci, 2 * H, 2 * W), 4), next_mask=L((N_IMG, ci, H, W), 1))
        t["bn"] = (torch.randint(1, 3, (co,), generator=g).float(), L((co,), 2), L((co,), 2), torch.ones(co), 0.0)
    else:
        R = lambda shape: torch.randn(shape, generator=g)
        t = dict(g=R((N_IMG, co, Ho, Wo)), y=_zeros_in(R((N_IMG, co, Ho, Wo)), g), x=_zeros_in(R((N_IMG, ci, H, W)), g),
                 w=R((co, ci, k, k)) / (ci * k * k) ** 0.5, add=R((N_IMG, ci, H, W)), fine=R((N_IMG, ci, 2 * H, 2 * W)),
                 next_mask=_zeros_in(R((N_IMG, ci, H, W)), g))
        t["bn"] = (torch.rand(co, generator=g) + 0.5, R((co,)) * 0.2, R((co,)) * 0.2, torch.rand(co, generator=g) + 0.5, 1e-5)
    return t


def _kernel(t, hw, stride, **kw):
    """``ops.conv_bn_rows_backward`` on the maps of ``t`` in the GEMM mode in force -> what it returns, ``dx`` as a map."""
    from bevformer_amd import ops
    rows = lambda m: ops.rows_of_map(m.cuda())
    scaled = kw.pop("scaled", False)
    bn = _bn_of(t["bn"][:4], t["bn"][4]) if scaled else None
    x = kw.pop("x", t["x"])
    for name in ("add", "next_mask"):
        if torch.is_tensor(kw.get(name)) and kw[name].dim() == 4:
            kw[name] = rows(kw[name])
    with torch.no_grad():
        got = ops.conv_bn_rows_backward(rows(t["g"]), rows(t["y"]) if scaled else None, rows(x), N_IMG, hw, t["w"].cuda(), bn,
                                        stride=stride, relu=scaled, **kw)
    assert got is not None, "ops.conv_bn_rows_backward declined a covered call"
    dx = got[0]
    return (None if dx is None else ops.map_of_rows(dx.contiguous(), N_IMG, hw),) + tuple(got[1:])


def _truth(t, stride, scaled=False, x=None, **kw):
    return T.conv_bwd64(t["g"], t["y"], t["x"] if x is None else x, t["w"], t["bn"] if scaled else _unit_bn(t["w"].shape[0]),
                        stride=stride, relu=scaled, **kw)


def _pool64(fine):
    f = fine.double()
    return (f[:, :, 0::2, 0::2] + f[:, :, 0::2, 1::2]) + (f[:, :, 1::2, 0::2] + f[:, :, 1::2, 1::2])


def _gz(t, scaled, dtype):
    g = t["g"].to(dtype)
    if scaled:
        g = g * (t["y"] > 0).to(dtype) * T.scale_of(t["bn"], dtype).view(1, -1, 1, 1)
    return g


def _check(tag, got, parent, want):
    e_parent, e = T.max_err(parent, want), T.max_err(got, want)
    print(f"{tag}: E_parent {e_parent:.3e}  kernel {e:.3e}  bound {3 * e_parent:.3e}")
    assert float(want.abs().max()) > 0.1 and e <= 3 * e_parent, tag


# ---- add_pool2

POOL_CASES = [((3, 5), 9, False), ((3, 5), 1, False), ((9, 15), 9, False), ((9, 15), 1, False), ((3, 5), 9, True)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw,taps,wide", POOL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_pool2_equals_float64_on_the_lattice(hw, taps, wide, mode):
    from bevformer_amd import ops
    t = _inputs(hw, 64, 32, taps, 1, True)
    want = _truth(t, 1)[0] + _pool64(t["fine"])
    Y.assert_lattice(want)
    fine = ops.rows_of_map(t["fine"].cuda())
    if wide:                                # an add whose row stride exceeds its width
        buf = torch.full((fine.shape[0], 64 + 32), 1e6, device="cuda")
        buf[:, :64] = fine
        fine = buf[:, :64]
    before = fine.clone()
    with ops.using(gemm=mode):
        dx, _ = _kernel(t, hw, 1, add=fine, add_pool2=True, need_dw=False)
        plain, _ = _kernel(t, hw, 1, need_dw=False)
    assert torch.equal(dx.double().cpu(), want)
    assert torch.equal(fine, before)                                            # add is only read
    assert not torch.equal(dx, plain) and float(_pool64(t["fine"]).abs().max()) > 0


def test_pool2_declines_what_it_cannot_add():
    from bevformer_amd import ops
    t = _inputs((3, 5), 64, 32, 9, 1, True)
    rows = lambda m: ops.rows_of_map(m.cuda())
    call = lambda **kw: ops.conv_bn_rows_backward(rows(t["g"]), None, None, N_IMG, (3, 5), t["w"].cuda(), None, need_dw=False, **kw)
    with ops.using(gemm="split"), torch.no_grad():
        assert call(add=rows(t["fine"]), add_pool2=True) is not None
        assert call(add=rows(t["add"]), add_pool2=True) is None                 # the coarse map's rows
        assert call(add_pool2=True) is None and call(add_after_mask=True, next_mask=rows(t["next_mask"])) is None
        assert call(add=rows(t["add"]), add_after_mask=True) is None            # no mask to come after


def test_pool2_random_within_three_parent_errors():
    from bevformer_amd import ops
    hw = (9, 15)
    t = _inputs(hw, 64, 32, 9, 1, False)
    want = _truth(t, 1)[0] + _pool64(t["fine"])
    with ops.using(gemm="split"):
        dx, _ = _kernel(t, hw, 1, add=t["fine"], add_pool2=True, need_dw=False)
        parent, _ = _kernel(t, hw, 1, add=(4 * F.avg_pool2d(t["fine"].cuda(), 2)).contiguous(), need_dw=False)
    _check("pool2", dx, parent, want)


# ---- add_after_mask

@pytest.mark.parametrize("mode", MODES)
def test_add_after_mask_equals_float64_and_differs_from_the_other_order(mode):
    from bevformer_amd import ops
    hw = (3, 5)
    t = _inputs(hw, 64, 32, 9, 2, True)
    assert tuple(t["g"].shape[2:]) == (2, 3)
    conv = _truth(t, 2)[0]
    mask = (t["next_mask"] > 0).double()
    after, before = conv * mask + t["add"].double(), (conv + t["add"].double()) * mask
    assert bool((t["next_mask"] == 0).any()) and not torch.equal(after, before)         # the two orders differ on this input
    Y.assert_lattice(after)
    with ops.using(gemm=mode):
        dx_after, _ = _kernel(t, hw, 2, add=t["add"], next_mask=t["next_mask"], add_after_mask=True, need_dw=False)
        dx_before, _ = _kernel(t, hw, 2, add=t["add"], next_mask=t["next_mask"], need_dw=False)
    assert torch.equal(dx_after.double().cpu(), after)
    assert torch.equal(dx_before.double().cpu(), before)


def test_add_after_mask_random_within_three_parent_errors():
    from bevformer_amd import ops
    hw = (3, 5)
    t = _inputs(hw, 64, 32, 9, 2, False)
    want = _truth(t, 2, next_mask=t["next_mask"])[0] + t["add"].double()
    with ops.using(gemm="split"):
        dx, _ = _kernel(t, hw, 2, add=t["add"], next_mask=t["next_mask"], add_after_mask=True, need_dw=False)
        parent = _kernel(t, hw, 2, next_mask=t["next_mask"], need_dw=False)[0] + t["add"].cuda()
    _check("add_after_mask", dx, parent, want)


# ---- relu_x

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stride", [1, 2])
def test_relu_x_equals_float64_on_the_lattice(stride, mode):
    from bevformer_amd import ops
    hw = (3, 5)
    t = _inputs(hw, 64, 32, 9, stride, True)
    assert bool((t["x"] < 0).any()) and bool((t["x"] == 0).any())
    want, without = _truth(t, stride, x=torch.relu(t["x"]))[1], _truth(t, stride)[1]
    Y.assert_lattice(want)
    assert not torch.equal(want, without)
    with ops.using(gemm=mode):
        _, dw = _kernel(t, hw, stride, relu_x=True, need_dx=False)
        _, dw_plain = _kernel(t, hw, stride, need_dx=False)
    assert torch.equal(dw.double().cpu(), want) and torch.equal(dw_plain.double().cpu(), without)


def test_relu_x_random_within_three_parent_errors():
    from bevformer_amd import ops
    hw = (3, 5)
    t = _inputs(hw, 64, 32, 9, 2, False)
    want = _truth(t, 2, x=torch.relu(t["x"]))[1]
    with ops.using(gemm="split"):
        _, dw = _kernel(t, hw, 2, relu_x=True, need_dx=False)
        _, parent = _kernel(t, hw, 2, x=torch.relu(t["x"]), need_dx=False)
    _check("relu_x", dw, parent, want)


# ---- dbias

# (hw, c_out, taps, stride): 9 x 15 at two images is 270 output rows = three row slices
DBIAS_CASES = [((3, 5), 32, 1, 1), ((3, 5), 32, 9, 1), ((3, 5), 32, 9, 2), ((3, 5), 160, 9, 1), ((9, 15), 32, 9, 1), ((9, 15), 160, 1, 1)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scaled", [False, True], ids=["gz", "g_y_norm"])
@pytest.mark.parametrize("hw,co,taps,stride", DBIAS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dbias_equals_float64_on_the_lattice(hw, co, taps, stride, scaled, mode):
    from bevformer_amd import ops
    t = _inputs(hw, 64, co, taps, stride, True)
    dw64 = _truth(t, stride, scaled=scaled)[1]
    db64 = _gz(t, scaled, torch.float64).sum((0, 2, 3))
    Y.assert_lattice(dw64), Y.assert_lattice(db64)
    assert float(db64.abs().max()) > 0
    db = torch.zeros(co, device="cuda")
    with ops.using(gemm=mode):
        got = _kernel(t, hw, stride, scaled=scaled, need_dx=False, db_out=db)
        _, dw_plain = _kernel(t, hw, stride, scaled=scaled, need_dx=False)
    assert len(got) == 3 and got[2] is db
    assert torch.equal(db.double().cpu(), db64)
    assert torch.equal(got[1].double().cpu(), dw64) and torch.equal(dw_plain.double().cpu(), dw64)      # dW is what it was


def test_dbias_accumulates_into_what_it_is_given():
    from bevformer_amd import ops
    hw = (9, 15)
    t = _inputs(hw, 64, 32, 9, 1, True)
    db64 = _gz(t, False, torch.float64).sum((0, 2, 3))
    db = torch.full((32,), 3.0, device="cuda")
    with ops.using(gemm="split"):
        _kernel(t, hw, 1, need_dx=False, db_out=db)
    assert torch.equal(db.double().cpu(), db64 + 3.0)


def test_dbias_random_within_three_parent_errors():
    from bevformer_amd import ops
    hw = (9, 15)
    t = _inputs(hw, 64, 160, 9, 1, False)
    want = _gz(t, True, torch.float64).sum((0, 2, 3))
    db = torch.zeros(160, device="cuda")
    with ops.using(gemm="split"):
        _kernel(t, hw, 1, scaled=True, need_dx=False, db_out=db)
    tc = {k: (tuple(u.cuda() if torch.is_tensor(u) else u for u in v) if isinstance(v, tuple) else v.cuda()) for k, v in t.items()}
    parent = ops.rows_of_map(_gz(tc, True, torch.float32)).sum(0)
    _check("dbias", db, parent, want)
