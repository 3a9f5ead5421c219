"""GPU: ``ops.deform_conv_rows_backward`` (csrc/deform_conv_bwd.h) against the float64 yardstick of tests/dcn_train_yardstick.py.
On the lattice every gradient must EQUAL float64 (no element excluded); on random inputs its error against float64 is at most
3 x the parent's — float32 autograd through the deformable im2col and ``ops.linear`` — per gradient, in the same GEMM mode.
Shapes are ``tests/test_dcn_gpu.py``'s; ``gz`` is given directly (cases with a BatchNorm + ReLU epilogue also give ``y`` and the
norm, so the kernels form ``gz`` on the way)."""
import functools

import pytest
import torch

import dcn_train_yardstick as Y
import dcn_yardstick as D

pytestmark = pytest.mark.gpu

# (n_img, H, W, C_in, C_out, stride, epilogue)
CASES = {
    "1x1px": (1, 1, 1, 32, 128, 1, "none"),
    "6x10_96to160": (2, 6, 10, 96, 160, 1, "none"),
    "5x7_s2": (2, 5, 7, 64, 128, 2, "none"),
    "3x130": (1, 3, 130, 32, 128, 1, "bn+relu"),
    "6x10_256": (2, 6, 10, 256, 256, 1, "bn+relu"),
    "4x5_512": (1, 4, 5, 512, 512, 1, "bn+relu"),
}
IDS = list(CASES)
# lattice only: 32 row tiles (the XCD tile map wraps four times, the weight gradient runs several row slices), stride 2
CASES["40x50_s2_many_tiles"] = (2, 80, 100, 64, 96, 2, "bn+relu")
MODES = ["split", "bf16"]
POSITION_MARGIN = 1e-3


def _lattice_inputs(name, seed):
    n_img, H, W, C, N, stride, ep = CASES[name]
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = D.out_hw(H, W, stride)
    x, w = D.lattice((n_img, C, H, W), -4, 4, g), D.lattice((N, C, 3, 3), -2, 2, g)
    gr = D.lattice((n_img, N, Ho, Wo), -2, 2, g)
    # (a single pixel: [-3, 3] offsets leave the image almost always and every gradient is zero — {-1/2, 0, 1/2} there)
    raw = Y.lattice_raw3((n_img, Ho, Wo), g, half_steps=1 if H * W == 1 else 6)
    y = bn = None
    if ep == "bn+relu":       # scale exactly 1 (gamma 1, var 1, eps 0); y has exact zeros, negatives and positives
        y = D.lattice((n_img, N, Ho, Wo), -2, 2, g)
        bn = (torch.ones(N), D.lattice((N,), -4, 4, g), D.lattice((N,), -4, 4, g), torch.ones(N), 0.0)
    return x, raw, w, gr, y, bn


def _nudged(x_shape, raw, stride):
    """Random offsets moved so that no live coordinate lies within POSITION_MARGIN of an integer or a border: a slope jumps
    there, and arms that floor differently would measure nothing."""
    raw = raw.clone()
    for _ in range(50):
        py, px, _ = Y.positions64(x_shape, raw, stride)
        H, W = x_shape[2:]
        near = lambda p, hi: ((p - p.round()).abs() < 2 * POSITION_MARGIN) | ((p + 1).abs() < 2 * POSITION_MARGIN) \
            | ((p - hi).abs() < 2 * POSITION_MARGIN)
        by, bx = near(py, H), near(px, W)
        if not (by.any() or bx.any()):
            break
        raw[:, 0:18:2] += by.float() * 0.01
        raw[:, 1:18:2] += bx.float() * 0.01
    assert Y.position_margin64(x_shape, raw, stride) >= POSITION_MARGIN
    return raw


@functools.lru_cache(maxsize=None)
def _case(name, kind="random"):
    """Inputs of a case (CPU fp32) and the float64 gradients, made once and shared: (x, raw, w, g, y, bn, (dx, draw, dW))."""
    n_img, H, W, C, N, stride, ep = CASES[name]
    relu = ep == "bn+relu"
    if kind == "lattice":
        for seed in range(8):           # the seed is chosen here, from float64 arithmetic on the CPU alone
            x, raw, w, gr, y, bn = _lattice_inputs(name, seed)
            want = Y.dcn_bwd64(gr, y, x, raw, w, bn, stride, relu)
            gm = gr * (y > 0).float() if relu else gr
            dx, draw, dw = want
            parts = (dx, dw, draw[:, :18], draw[:, 18:])
            if all(torch.isfinite(t).all() and torch.equal(16 * t, (16 * t).round()) for t in parts) \
                    and all((t != 0).any() for t in parts) \
                    and 16 * Y.exact_sum_bound64(gm, x, raw, w, stride) < 2 ** 24 \
                    and 16 * max(float(t.abs().max()) for t in Y.dcn_bwd64(gm.abs(), None, x.abs(), raw, w.abs(), None, stride)) < 2 ** 24:
                return x, raw, w, gr, y, bn, want
        raise AssertionError(f"{name}: no lattice seed meets the exactness conditions")
    g = torch.Generator().manual_seed(100 + IDS.index(name))
    Ho, Wo = D.out_hw(H, W, stride)
    x, w = torch.randn(n_img, C, H, W, generator=g), torch.randn(N, C, 3, 3, generator=g) / (9 * C) ** 0.5
    gr = torch.randn(n_img, N, Ho, Wo, generator=g)
    # (a single pixel: offsets of scale 1.5 leave the image for most taps)
    raw = _nudged(x.shape, D.random_raw((n_img, Ho, Wo), g, scale=0.4 if H * W == 1 else 1.5), stride)
    y = bn = None
    if relu:
        y = torch.randn(n_img, N, Ho, Wo, generator=g)
        bn = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2, torch.randn(N, generator=g) * 0.2,
              torch.rand(N, generator=g) + 0.5, 1e-5)
    want = Y.dcn_bwd64(gr, y, x, raw, w, bn, stride, relu)
    for t in want:
        assert float(t.abs().max()) > 1e-3
    return x, raw, w, gr, y, bn, want


def _bn_module(bn):
    N = bn[0].numel()
    m = torch.nn.BatchNorm2d(N, eps=bn[4]).cuda().eval()
    with torch.no_grad():
        m.weight.copy_(bn[0]), m.bias.copy_(bn[1]), m.running_mean.copy_(bn[2]), m.running_var.copy_(bn[3])
    return m


def _run(name, mode, kind="random", raw=None, **kw):
    """-> ``ops.deform_conv_rows_backward``'s (dx rows, doffs rows, dW) for the case's inputs (``_maps`` turns them into maps)."""
    from bevformer_amd import ops
    n_img, H, W, C, N, stride, ep = CASES[name]
    x, raw0, w, gr, y, bn, _ = _case(name, kind)
    dev = torch.device("cuda")
    rawd = (raw0 if raw is None else raw).to(dev)
    with torch.no_grad(), ops.using(gemm=mode):
        res = ops.deform_conv_rows_backward(Y.rows_of_map(gr.to(dev)), None if y is None else Y.rows_of_map(y.to(dev)),
                                            Y.rows_of_map(x.to(dev)), n_img, (H, W), D.rows_of_raw(rawd), w.to(dev),
                                            None if bn is None else _bn_module(bn), stride=stride, relu=ep == "bn+relu", **kw)
    assert res is not None
    return res


def _maps(name, res):
    n_img, H, W, C, N, stride, ep = CASES[name]
    Ho, Wo = D.out_hw(H, W, stride)
    dx, doffs, dw = res
    assert tuple(dx.shape) == (n_img * H * W, C) and tuple(doffs.shape) == (n_img * Ho * Wo, 32) and tuple(dw.shape) == (N, C, 3, 3)
    assert (doffs[:, 27:] == 0).all()                               # columns 27 .. 31 are never written
    return dx.reshape(n_img, H, W, C).permute(0, 3, 1, 2), Y.raw_of_rows(doffs, (n_img, Ho, Wo)), dw


# ---- 1. lattice exactness

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IDS + ["40x50_s2_many_tiles"])
def test_gradients_equal_float64_on_the_lattice(name, mode):
    """x in {-4..4}, w and g in {-2..2}, half-integer offsets, m in {0, 1/2, 1}: every gradient is a multiple of 1/16 and every
    partial sum is exact in any order (``_case`` checks both on the float64 truth), so dx, doffs and dW EQUAL float64 — a corner
    added to the wrong row, a slope from the wrong cell or a dead tap that leaks cannot hide in a tolerance."""
    want = _case(name, "lattice")[6]
    got = _maps(name, _run(name, mode, kind="lattice"))
    for what, a, b in zip(("dx", "draw", "dW"), got, want):
        assert torch.equal(a.double().cpu(), b), f"{what}: {Y.max_err(a, b):.3e}"


# ---- 2. the error bound

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IDS)
def test_gradients_within_three_parent_errors(name, mode):
    from bevformer_amd import ops
    n_img, H, W, C, N, stride, ep = CASES[name]
    x, raw, w, gr, y, bn, want = _case(name)
    dev = torch.device("cuda")
    got = _maps(name, _run(name, mode))
    bnd = None if bn is None else tuple(t.to(dev) for t in bn[:4]) + (bn[4],)
    with ops.using(gemm=mode):
        parent = Y.parent_dcn_grads(gr.to(dev), None if y is None else y.to(dev), x.to(dev), raw.to(dev), w.to(dev), bnd, stride,
                                    ep == "bn+relu")
    errs = []
    for what, a, p, b in zip(("dx", "draw", "dW"), got, parent, want):
        e_parent, e_fused = Y.max_err(p, b), Y.max_err(a, b)
        print(f"{name} {mode} {what}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        errs.append((what, e_fused, e_parent))
    for what, e_fused, e_parent in errs:
        assert e_fused <= 3 * e_parent, what


# ---- 3. dead taps

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["6x10_96to160", "5x7_s2"])
def test_non_finite_positions_are_dead_taps(name, mode):
    """NaN, +-inf and +-1e30 offsets on chosen taps (the forward test's own inputs) against the same taps switched off by their
    mask (logit -inf, offset 0), on lattice inputs: dx and dW are equal, those taps' three doffs entries are exactly 0 and
    everything is finite — such a position is range-checked before it is converted and addresses nothing."""
    raw = _case(name, "lattice")[1]
    bad, off = raw.clone(), raw.clone()
    vals = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]
    g = torch.Generator().manual_seed(7)
    B, _, Ho, Wo = raw.shape
    hit = torch.rand(B, 9, Ho, Wo, generator=g) < 0.3
    which = torch.randint(0, len(vals), (B, 9, Ho, Wo), generator=g)
    on_x = torch.rand(B, 9, Ho, Wo, generator=g) < 0.5              # the bad value sits on dx, else on dy
    v = torch.tensor(vals)[which]
    for k in range(9):
        h = hit[:, k]
        bad[:, 2 * k] = torch.where(h & ~on_x[:, k], v[:, k], bad[:, 2 * k])
        bad[:, 2 * k + 1] = torch.where(h & on_x[:, k], v[:, k], bad[:, 2 * k + 1])
        off[:, 2 * k] = torch.where(h, torch.zeros(()), off[:, 2 * k])
        off[:, 2 * k + 1] = torch.where(h, torch.zeros(()), off[:, 2 * k + 1])
        off[:, 18 + k] = torch.where(h, torch.full((), float("-inf")), off[:, 18 + k])
    assert hit.any() and not torch.isfinite(bad).all()
    a = _maps(name, _run(name, mode, kind="lattice", raw=bad))
    b = _maps(name, _run(name, mode, kind="lattice", raw=off))
    for t in a:
        assert torch.isfinite(t).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    hit3 = torch.cat([hit.repeat_interleave(2, 1), hit], 1).cuda()  # channels 2 k, 2 k + 1 and 18 + k of a hit tap
    assert (a[1][hit3] == 0).all() and (b[1][hit3] == 0).all()
    assert torch.equal(a[1], b[1])
    assert (a[1] != 0).any() and (a[0] != 0).any()


# ---- 4. what can be left out, and accumulation

def test_each_gradient_can_be_left_out_and_outputs_accumulate():
    name, mode = "6x10_96to160", "split"
    n_img, H, W, C, N, stride, ep = CASES[name]
    Ho, Wo = D.out_hw(H, W, stride)
    full = _run(name, mode, kind="lattice")
    dev = torch.device("cuda")
    mk = lambda: (torch.full((n_img * H * W, C), 3.0, device=dev), torch.full((n_img * Ho * Wo, 32), -2.0, device=dev),
                  torch.full((N, C, 3, 3), 5.0, device=dev))
    for skip in range(3):
        need = [i != skip for i in range(3)]
        dxo, doo, dwo = mk()
        res = _run(name, mode, kind="lattice", need_dx=need[0], need_doffs=need[1], need_dw=need[2], dx_out=dxo, doffs_out=doo,
                   dw_out=dwo)
        assert res[skip] is None
        # a left-out output is untouched; the others accumulated onto their non-zero contents (lattice: exact sums)
        for i, (buf, fill) in enumerate(zip((dxo, doo, dwo), (3.0, -2.0, 5.0))):
            if i == skip:
                assert (buf == fill).all()
            elif i == 1:
                assert res[i] is buf and torch.equal(buf[:, :27], full[i][:, :27] + fill) and (buf[:, 27:] == fill).all()
            else:
                assert res[i] is buf and torch.equal(buf, full[i] + fill)


# ---- 5. the same GEMMs as the plain convolution's backward

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["6x10_96to160", "5x7_s2"])
def test_zero_offsets_are_the_plain_convolutions_backward(name, mode):
    from bevformer_amd import ops
    n_img, H, W, C, N, stride, ep = CASES[name]
    x, raw, w, gr, y, bn, _ = _case(name, "lattice")
    Ho, Wo = D.out_hw(H, W, stride)
    plain_raw = torch.cat([torch.zeros(n_img, 18, Ho, Wo), torch.full((n_img, 9, Ho, Wo), 64.0)], 1)
    dx, _, dw = _run(name, mode, kind="lattice", raw=plain_raw)
    dev = torch.device("cuda")
    with torch.no_grad(), ops.using(gemm=mode):
        pdx, pdw = ops.conv_bn_rows_backward(Y.rows_of_map(gr.to(dev)), None, Y.rows_of_map(x.to(dev)), n_img, (H, W), w.to(dev),
                                             None, stride=stride)
    assert float(pdx.abs().max()) > 0 and float(pdw.abs().max()) > 0
    assert torch.equal(dx, pdx) and torch.equal(dw, pdw)


# ---- 6. what is not covered

def test_uncovered_calls_return_none():
    from bevformer_amd import ops
    name = "6x10_96to160"
    n_img, H, W, C, N, stride, ep = CASES[name]
    x, raw, w, gr, _, _, _ = _case(name, "lattice")
    dev = torch.device("cuda")
    args = lambda d, c=C: (Y.rows_of_map(gr.to(d)), None, Y.rows_of_map(x[:, :c].to(d)), n_img, (H, W), D.rows_of_raw(raw.to(d)),
                           w[:, :c].contiguous().to(d), None)
    with torch.no_grad():
        assert ops.deform_conv_rows_backward(*args(dev)) is not None
        assert ops.deform_conv_rows_backward(*args("cpu")) is None
        with ops.using(gemm="native"):
            assert ops.deform_conv_rows_backward(*args(dev)) is None
        assert ops.deform_conv_rows_backward(*args(dev, 48)) is None
    with torch.enable_grad():
        assert ops.deform_conv_rows_backward(*args(dev)) is None
