"""GPU: ``ops.conv3x3_bn`` (csrc/conv3x3.h) against the float64 yardstick of tests/fusion_yardstick.py.  Bound: error <= 3 x the
error of the parent — the same convolution as an im2col matrix through ``ops.linear`` plus torch fp32 BatchNorm / residual /
ReLU — on the same inputs in the same GEMM mode.  Shapes are the smallest at which the kernel can go wrong: a single pixel, a
grid below one 128-pixel tile, tiles that straddle image rows and the boundary between two images, rows longer than a tile,
the real row width with a repeated segment."""
import functools

import pytest
import torch

import fusion_yardstick as Y

pytestmark = pytest.mark.gpu

# (bs, H, W, segment widths, C_out); a segment list entry may name an earlier segment: see _case
CASES = [
    (1, 1, 1, (32,), 128),                  # only the centre tap is live
    (1, 5, 7, (32,), 128),                  # below one tile, every pixel on or next to a border
    (1, 13, 21, (64,), 128),                # two tiles and a tail, tiles straddle image rows, two K chunks per tap
    (2, 6, 11, (32, 32), 256),              # the boundary between the images inside a tile, two segments, two column tiles
    (1, 3, 130, (32,), 128),                # a row longer than a tile: the dy taps reach +-130 rows
    (1, 4, 200, (32, 32, 32, 32), 128),     # the real row width, one segment passed twice
]
IDS = ["x".join(map(str, c[:3])) + "_" + "+".join(map(str, c[3])) + f"_{c[4]}" for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(case, lattice=False):
    """Inputs of a case (CPU fp32) and the float64 convolution sums, made once and shared by every variant."""
    bs, H, W, segs, N = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    draw = (lambda *s: torch.randint(-4, 5, s, generator=g).float()) if lattice else (lambda *s: torch.randn(*s, generator=g))
    rows = [draw(bs, H * W, c) for c in segs]
    if len(rows) == 4:
        rows[2] = rows[0]                   # the same tensor twice (fuse_frames repeats a neighbour for a missing frame)
    C = sum(segs)
    w = draw(N, C, 3, 3) if lattice else draw(N, C, 3, 3) / (9 * C) ** 0.5
    if lattice:
        bn = (torch.ones(N), torch.zeros(N), torch.zeros(N), torch.ones(N))
    else:
        bn = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g) * 0.2,
              torch.rand(N, generator=g) + 0.5)
    res = draw(bs, H * W, N)
    conv = Y.conv_sum64(torch.cat(rows, -1), H, W, w)
    return rows, w, bn, res, conv


def _bn_module(bn, eps, dev):
    m = torch.nn.BatchNorm2d(bn[0].numel(), eps=eps).to(dev).eval()
    with torch.no_grad():
        for dst, src in zip((m.weight, m.bias, m.running_mean, m.running_var), bn):
            dst.copy_(src)
    return m


def _gpu(case, lattice=False):
    rows, w, bn, res, conv = _case(case, lattice)
    dev = torch.device("cuda")
    uniq = {}
    rows_d = [uniq.setdefault(id(r), r.to(dev)) for r in rows]      # a repeated segment stays ONE device tensor
    return rows_d, w.to(dev), bn, res.to(dev), conv


@pytest.mark.parametrize("res_on", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv3x3_bn_within_three_parent_errors(case, mode, relu, res_on):
    from bevformer_amd import ops
    bs, H, W, segs, N = case
    rows, w, bn, res, conv = _gpu(case)
    eps = 1e-5
    bnm = _bn_module(bn, eps, w.device)
    r = res if res_on else None
    want = Y.conv_bn64(None, H, W, None, *bn, eps, relu, res=r, conv=conv)
    with torch.no_grad(), ops.using(gemm=mode):
        got = ops.conv3x3_bn(rows if len(rows) > 1 else rows[0], (H, W), w, bnm, relu=relu, res=r)
        parent = Y.parent_conv_bn(torch.cat(rows, -1), H, W, w, *(t.to(w.device) for t in bn), eps, relu, res=r)
    assert got is not None and got.shape == (bs, H * W, N)
    e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
    print(f"{case} {mode} relu={relu} res={res_on}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
    assert e_fused <= 3 * e_parent


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("case", [CASES[3], CASES[2]], ids=[IDS[3], IDS[2]])
def test_conv3x3_bn_exact_on_the_integer_lattice(case, mode):
    """Integers in [-4, 4], identity BatchNorm with eps = 0: every product and sum is exact in both modes, so the result
    EQUALS the yardstick — a tap leaking across a row end or an image boundary cannot hide in a tolerance."""
    from bevformer_amd import ops
    bs, H, W, segs, N = case
    rows, w, bn, res, conv = _gpu(case, lattice=True)
    bnm = _bn_module(bn, 0.0, w.device)
    for relu, r in ((False, None), (True, res)):
        want = Y.conv_bn64(None, H, W, None, *bn, 0.0, relu, res=r, conv=conv)
        with torch.no_grad(), ops.using(gemm=mode):
            got = ops.conv3x3_bn(rows, (H, W), w, bnm, relu=relu, res=r)
        assert got is not None
        assert torch.equal(got.double().cpu(), want)


def test_conv3x3_bn_two_runs_are_bit_equal():
    from bevformer_amd import ops
    case = CASES[3]
    rows, w, bn, res, _ = _gpu(case)
    bnm = _bn_module(bn, 1e-5, w.device)
    with torch.no_grad():
        a = ops.conv3x3_bn(rows, case[1:3], w, bnm, relu=True, res=res)
        b = ops.conv3x3_bn(rows, case[1:3], w, bnm, relu=True, res=res)
    assert a is not None and torch.equal(a, b)


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_conv3x3_bn_follows_in_place_updates(mode):
    """The weight image is cached per weight VERSION, and nothing derived from the running statistics is cached at all: an
    in-place update of either is seen by the next call."""
    from bevformer_amd import ops
    case = CASES[2]
    bs, H, W, segs, N = case
    rows, w, bn, res, conv = _gpu(case)
    w = w.clone()
    eps = 1e-5
    bnm = _bn_module(bn, eps, w.device)
    dev_bn = [t.to(w.device) for t in bn]
    with torch.no_grad(), ops.using(gemm=mode):
        first = ops.conv3x3_bn(rows, (H, W), w, bnm, relu=False)
        assert first is not None
        w.mul_(-2.0)                                           # in place: same address, next version
        want = Y.conv_bn64(None, H, W, None, *bn, eps, False, conv=-2.0 * conv)
        got = ops.conv3x3_bn(rows, (H, W), w, bnm, relu=False)
        parent = Y.parent_conv_bn(rows[0], H, W, w, *dev_bn, eps, False)
        e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got, want)
        print(f"weight update {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        assert e_fused <= 3 * e_parent
        assert Y.max_err(first, want) > 1.0                     # (the stale image would have given `first` again)

        bnm.running_mean.add_(0.75)
        bnm.running_var.mul_(2.0)
        stats = (bn[0], bn[1], bn[2] + 0.75, bn[3] * 2.0)
        want = Y.conv_bn64(None, H, W, None, *stats, eps, False, conv=-2.0 * conv)
        got2 = ops.conv3x3_bn(rows, (H, W), w, bnm, relu=False)
        parent = Y.parent_conv_bn(rows[0], H, W, w, *(t.to(w.device) for t in stats), eps, False)
        e_parent, e_fused = Y.max_err(parent, want), Y.max_err(got2, want)
        print(f"statistics update {mode}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        assert e_fused <= 3 * e_parent
        assert Y.max_err(got, want) > 0.25
