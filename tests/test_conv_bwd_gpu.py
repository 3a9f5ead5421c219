"""GPU: the backward of ``ops.conv_bn_rows`` with a frozen norm (``ops.conv_bn_rows_backward``, csrc/conv_bwd_rows.h) against float64
autograd (tests/backbone_train_yardstick.py).  The test chooses the saved output ``y`` the mask is taken from and draws it with
exact zeros, so there is no kink to argue about.  On the integer lattice — g in {-2..2}, x, add in {-4..4}, w in {-2..2}, scales
exactly 1 or 2 — every operand is a bf16 number and every sum stays far below 2^24: ``dx`` and ``dW`` EQUAL the float64 result in
``split`` and in ``bf16``.  On random inputs: error <= 3 x the error of the parent (im2col + ``ops.linear``'s autograd path in the
same GEMM mode) on the same inputs.

Shapes, the smallest at which each mechanism can go wrong: two images (a tap must not cross into the next one); 5 x 7 and 6 x 8
(odd and even sizes at stride 2: Ho = (H - 1) // 2 + 1, the last row and column); 9 x 11 = 198 rows at two images (one full and
one partial 128-row tile); (C_in, C_out) = (32, 64), (160, 32), (64, 160) (a partial and a second 128-column tile on either side);
1 and 9 taps; stride 1 and 2; every epilogue option, an aliased ``add`` and a destination wider than its rows."""
import functools
import itertools

import pytest
import torch

import backbone_train_yardstick as T
import backbone_yardstick as Y

pytestmark = pytest.mark.gpu

MODES = ["split", "bf16"]
HWS = [(5, 7), (6, 8), (9, 11)]
CHANNELS = [(32, 64), (160, 32), (64, 160)]
GEOMS = list(itertools.product(HWS, CHANNELS, (1, 9), (1, 2)))
N_IMG = 2
# option sets: (relu, scale, add, alias add with a wide destination, next_mask, next_bn, need_dx, need_dw)
OPTIONS = {
    "plain": dict(relu=True, scale=True),
    "all": dict(relu=True, scale=True, add=True, next_mask=True, next_bn=True),
    "alias_wide": dict(relu=False, scale=False, add=True, alias=True),
    "mask_only": dict(relu=True, scale=False, next_mask=True, need_dw=False),
    "dw_only": dict(relu=False, scale=True, need_dx=False),
}


def _id(geom):
    (H, W), (ci, co), taps, stride = geom
    return f"{H}x{W}-{ci}to{co}-t{taps}-s{stride}"


def _zeros_in(t, g, every=5):
    """Exact zeros in a fifth of the entries."""
    return t * (torch.randint(0, every, t.shape, generator=g) != 0).to(t.dtype)


def _bn_of(vecs, eps):
    bn = torch.nn.BatchNorm2d(vecs[0].numel(), eps=eps).eval()
    with torch.no_grad():
        for p, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), vecs):
            p.copy_(v)
    for p in bn.parameters():
        p.requires_grad = False
    return bn.cuda()


@functools.lru_cache(maxsize=None)
def _inputs(geom, lattice):
    """CPU tensors of one geometry, made once and shared; nobody writes to them."""
    (H, W), (ci, co), taps, stride = geom
    g = torch.Generator().manual_seed(1000 * GEOMS.index(geom) + int(lattice))
    Ho, Wo = Y.out_hw(H, W, stride)
    k = 3 if taps == 9 else 1
    if lattice:
        L = lambda shape, m: Y.lattice(shape, -m, m, g)
        t = dict(g=L((N_IMG, co, Ho, Wo), 2), y=L((N_IMG, co, Ho, Wo), 1), x=L((N_IMG, ci, H, W), 4), w=L((co, ci, k, k), 2),
                 add=L((N_IMG, ci, H, W), 4), next_mask=L((N_IMG, ci, H, W), 1))
        pow2 = lambda n: torch.randint(1, 3, (n,), generator=g).float()
        # scale = gamma / sqrt(1 + 0) exactly 1 or 2; beta and mean take no part in a gradient
        t["bn"] = (pow2(co), L((co,), 2), L((co,), 2), torch.ones(co), 0.0)
        t["next_bn"] = (pow2(ci), L((ci,), 2), L((ci,), 2), torch.ones(ci), 0.0)
    else:
        R = lambda shape: torch.randn(shape, generator=g)
        t = dict(g=R((N_IMG, co, Ho, Wo)), y=_zeros_in(R((N_IMG, co, Ho, Wo)), g), x=R((N_IMG, ci, H, W)),
                 w=R((co, ci, k, k)) / (ci * k * k) ** 0.5, add=R((N_IMG, ci, H, W)), next_mask=_zeros_in(R((N_IMG, ci, H, W)), g))
        U = lambda n: torch.rand(n, generator=g) + 0.5
        t["bn"] = (U(co), R((co,)) * 0.2, R((co,)) * 0.2, U(co), 1e-5)
        t["next_bn"] = (U(ci), R((ci,)) * 0.2, R((ci,)) * 0.2, U(ci), 1e-5)
    return t


def _args(t, opt):
    """The yardstick's keyword arguments of one option set."""
    unit = lambda bn: (torch.ones_like(bn[0]), bn[1], bn[2], torch.ones_like(bn[3]), 0.0)
    return dict(bn=t["bn"] if opt.get("scale") else unit(t["bn"]), relu=bool(opt.get("relu")), add=t["add"] if opt.get("add") else None,
                next_mask=t["next_mask"] if opt.get("next_mask") else None, next_bn=t["next_bn"] if opt.get("next_bn") else None)


@functools.lru_cache(maxsize=None)
def _truth(geom, lattice, name):
    t, stride = _inputs(geom, lattice), geom[3]
    return T.conv_bwd64(t["g"], t["y"], t["x"], t["w"], stride=stride, **_args(t, OPTIONS[name]))


def _run(geom, lattice, name):
    """(dx map or None, dW or None) of the kernels for one geometry and option set, in the GEMM mode in force."""
    from bevformer_amd import ops
    (H, W), (ci, co), taps, stride = geom
    t, opt = _inputs(geom, lattice), OPTIONS[name]
    rows = lambda m: ops.rows_of_map(m.cuda())
    kw = dict(stride=stride, relu=bool(opt.get("relu")), need_dx=opt.get("need_dx", True), need_dw=opt.get("need_dw", True))
    if opt.get("next_mask"):
        kw["next_mask"] = rows(t["next_mask"])
    if opt.get("next_bn"):
        kw["next_bn"] = _bn_of(t["next_bn"][:4], t["next_bn"][4])
    if opt.get("alias"):                     # add IS the destination, whose row stride exceeds its width
        wide = torch.full((N_IMG * H * W, ci + 32), 7.0, device="cuda")
        wide[:, :ci] = rows(t["add"])
        kw["add"] = kw["dx_out"] = wide[:, :ci]
    elif opt.get("add"):
        kw["add"] = rows(t["add"])
    bn = _bn_of(t["bn"][:4], t["bn"][4]) if opt.get("scale") else None
    add_before = kw["add"].clone() if "add" in kw and not opt.get("alias") else None
    with torch.no_grad():
        got = ops.conv_bn_rows_backward(rows(t["g"]), rows(t["y"]), rows(t["x"]), N_IMG, (H, W), t["w"].cuda(), bn, **kw)
    assert got is not None, "ops.conv_bn_rows_backward declined a covered call"
    dx, dw = got
    assert (dx is None) == (not kw["need_dx"]) and (dw is None) == (not kw["need_dw"])
    if opt.get("alias"):
        assert dx.data_ptr() == wide.data_ptr() and bool((wide[:, ci:] == 7.0).all())      # columns beyond the width untouched
    if add_before is not None:
        assert torch.equal(kw["add"], add_before)                                          # a separate add is only read
    return (None if dx is None else ops.map_of_rows(dx.contiguous(), N_IMG, (H, W))), dw


# ---- 1. lattice: bit-equal to float64

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", GEOMS, ids=_id)
def test_gradients_equal_float64_on_the_lattice(geom, mode):
    from bevformer_amd import ops
    for name in OPTIONS:
        dx64, dw64 = _truth(geom, True, name)
        Y.assert_lattice(dx64), Y.assert_lattice(dw64)          # the truth's sums are integers below 2^24: blame the kernel
        with ops.using(gemm=mode):
            dx, dw = _run(geom, True, name)
        if dx is not None:
            assert torch.equal(dx.double().cpu(), dx64), (name, "dx")
            assert float(dx64.abs().max()) > 0
        if dw is not None:
            assert torch.equal(dw.double().cpu(), dw64), (name, "dW")
            assert float(dw64.abs().max()) > 0


# ---- 2. random inputs: within three parent errors

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", GEOMS, ids=_id)
def test_gradients_within_three_parent_errors(geom, mode):
    from bevformer_amd import ops
    t, stride = _inputs(geom, False), geom[3]
    cuda = lambda v: v.cuda() if torch.is_tensor(v) else v
    for name in ("plain", "all"):
        dx64, dw64 = _truth(geom, False, name)
        a = {k: (tuple(cuda(u) for u in v) if isinstance(v, tuple) else cuda(v)) for k, v in _args(t, OPTIONS[name]).items()}
        with ops.using(gemm=mode):
            dx, dw = _run(geom, False, name)
            pdx, pdw = T.parent_conv_grads(t["g"].cuda(), t["y"].cuda(), t["x"].cuda(), t["w"].cuda(), stride=stride, **a)
        for what, got, parent, want in (("dx", dx, pdx, dx64), ("dW", dw, pdw, dw64)):
            e_parent, e = T.max_err(parent, want), T.max_err(got, want)
            print(f"{_id(geom)} {name} {mode} {what}: E_parent {e_parent:.3e}  kernel {e:.3e}  bound {3 * e_parent:.3e}")
            assert float(want.abs().max()) > 0.1 and e <= 3 * e_parent, (name, what)


# ---- 3. 1 x 1 at stride 2: odd input pixels receive exactly add, or 0

@pytest.mark.parametrize("mode", MODES)
def test_odd_pixels_of_a_strided_1x1_receive_exactly_add(mode):
    from bevformer_amd import ops
    geom = ((5, 7), (64, 160), 1, 2)
    t = _inputs(geom, False)
    odd = torch.ones(5, 7, dtype=torch.bool)
    odd[0::2, 0::2] = False
    with ops.using(gemm=mode):
        with_add, _ = _run(geom, False, "alias_wide")
        without, _ = _run(geom, False, "plain")
    assert torch.equal(with_add[:, :, odd].cpu(), t["add"][:, :, odd])
    assert float(without[:, :, odd].abs().max()) == 0.0 and float(without[:, :, ~odd].abs().max()) > 0.1
    assert not torch.equal(with_add[:, :, ~odd].cpu(), t["add"][:, :, ~odd])


# ---- 4. what is not covered is declined, not computed some other way

def test_uncovered_calls_are_declined():
    from bevformer_amd import ops
    geom = ((5, 7), (32, 64), 9, 1)
    t = _inputs(geom, True)
    rows = lambda m: ops.rows_of_map(m.cuda())
    bn = _bn_of(t["bn"][:4], 0.0)
    call = lambda **kw: ops.conv_bn_rows_backward(rows(t["g"]), rows(t["y"]), rows(t["x"]), N_IMG, (5, 7), t["w"].cuda(), bn, **kw)
    with ops.using(gemm="split"):
        assert call() is None                                   # grad mode is on: the op has no double backward
        with torch.no_grad():
            assert call() is not None
            assert call(stride=3) is None
            assert ops.conv_bn_rows_backward(rows(t["g"]), None, rows(t["x"]), N_IMG, (5, 7), t["w"].cuda()[:, :, :2, :2], bn) is None
            bn.train()
            assert call() is None                               # batch statistics: not this operator
            bn.eval()
    with ops.using(gemm="native"), torch.no_grad():
        assert call() is None
