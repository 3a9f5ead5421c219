"""GPU: parity ON the configurations BASELINE.json benches — bevformer_base (200x200 queries,
6 cameras, 4 levels, 6 layers) and the "small, 4 levels" shape set (150x150, 3 layers) — not only
on the unit-test sized rigs.

Tolerances (one per level, the same numbers as DESIGN.md §2 and bench.py):
  * encoder forward, fp32 storage, split / native GEMMs:   rtol = atol = 5e-4
  * bf16 value storage and / or bf16 GEMM operands:        3 x E_ref in max abs and 1 - cos, E_ref = the oracle with the
    bf16 roundings emulated against the plain oracle (tests/helpers.py::oracle_bf16: nothing of the product in it), and
    the worst 64-row block's mean row error <= 3 x the mean over all rows; outer bound, as before: max abs < 0.1,
    cosine > 0.999 on the O(1) LayerNorm-ed output (bf16 has 8 mantissa bits; six layers)
  * fused sampling kernels at the full row count:          rtol 1e-4, atol 1e-5 (operator level)
  * gradients (small4 fwd + bwd):                          per tensor, relative L2 error < 1e-2 and max error
    < 0.1 of the tensor's largest entry (bilinear slopes flip at pixel boundaries: see the test)
  * gradients under bf16 GEMM operands (the bench's fwd_bwd_small4_bf16, eval and train() mode): 3 x E_ref of the worst
    tensor in the same two metrics, output 3 x E_ref; each case proves by launch tags that the chain forward / backward
    kernels and the multi-problem weight-gradient launches ran in bf16 mode and nothing fell back to the library GEMM
The oracle runs of a workload are shared by the tests of this module (10 s per base frame)."""
import functools

import pytest
import torch

from bevformer_amd import ops, train_ops
from bevformer_amd import synthetic as S
from oracle import bevformer_cpu as O

from helpers import (E_ref, EdgeRecorder, _oracle_msda_fused, build_pair, camera_rows, oracle_encoder_rows, oracle_forward,
                     oracle_training_step, output_errors, row_block_ratio)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENC_TOL = dict(rtol=5e-4, atol=5e-4)


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, temporal):
    torch.set_num_threads(16)
    _, sd = build_pair(name)
    q, f, kw = S.make_inputs(name, seed=0, temporal=temporal)
    with torch.no_grad():
        return O.encoder_forward(sd, q, f, pc_range=S.PC_RANGE, **kw)


def _gpu_frame(name, temporal):
    enc, _ = build_pair(name, device=DEV)
    q, f, kw = S.make_inputs(name, seed=0, temporal=temporal, device=DEV)
    with torch.no_grad():
        return enc(q, f, f, **kw).cpu()


@pytest.fixture
def modes():
    saved = (ops.gemm_mode(), ops.value_storage())
    yield
    ops.set_gemm_mode(saved[0])
    ops.set_value_storage(saved[1])


# "small" = the reference-true bevformer_small (projects/configs/bevformer/bevformer_small.py:41-43,88: ONE feature level
# (23, 40), 3 layers, 150 x 150 queries); "small4" = BASELINE configs[2]'s synthetic 4-level shape set of the same grid;
# "tiny" = BASELINE configs[1] (bevformer_tiny.py:45-47,90: 50 x 50 queries, one level (15, 25), 3 layers)
@pytest.mark.parametrize("name", ["base", "small4", "small", "tiny"])
@pytest.mark.parametrize("temporal", [True, False])
@pytest.mark.parametrize("gemm", ["split", "native"])
def test_encoder_forward_on_the_benched_configs(name, temporal, gemm, modes):
    ops.set_gemm_mode(gemm)
    got = _gpu_frame(name, temporal)
    want = _oracle_frame(name, temporal)
    torch.testing.assert_close(got, want, **ENC_TOL)


@functools.lru_cache(maxsize=None)
def _forward_yardstick(name, gemm, storage):
    """``E_ref`` of a forward frame with history: the emulated oracle (tests/helpers.py::oracle_bf16) against the plain one."""
    return E_ref(oracle_forward(name, gemm == "bf16", storage == torch.bfloat16), _oracle_frame(name, True))


# E_ref of the forward frame, (max abs, 1 - cos), as computed on the CPU from the oracle alone (the emulated oracle against
# the plain one); the bound of a configuration is 3 x the yardstick the test computes, and a yardstick more than 2 x away
# from its entry here means the emulation changed, not that the bound moved.  3 x an entry is tighter than the
# 0.1 / 1 - 0.999 the test asserted before everywhere but for base's max abs under bf16 GEMMs (0.100 and 0.097: six layers),
# where the old number, kept as the outer assertion, is the bound that binds.  Product (MI355X, profiles/bf16_bounds.log):
# max abs 8.42e-3 / 3.38e-2 / 3.31e-2 (base), 5.81e-3 / 2.23e-2 / 2.24e-2 (small4), 6.76e-3 / 2.40e-2 / 2.78e-2 (small); 1 - cos
# equal to the yardstick's to three digits; block ratios 1.05 .. 1.09.
BF16_FWD_E_REF = {
    ("base", "split", torch.bfloat16): (8.43e-3, 9.28e-7), ("base", "bf16", torch.bfloat16): (3.34e-2, 1.47e-5),
    ("base", "bf16", torch.float32): (3.24e-2, 1.38e-5),
    ("small4", "split", torch.bfloat16): (5.85e-3, 5.22e-7), ("small4", "bf16", torch.bfloat16): (2.27e-2, 8.19e-6),
    ("small4", "bf16", torch.float32): (2.34e-2, 7.67e-6),
    ("small", "split", torch.bfloat16): (6.90e-3, 6.78e-7), ("small", "bf16", torch.bfloat16): (2.47e-2, 8.88e-6),
    ("small", "bf16", torch.float32): (2.67e-2, 8.22e-6)}
# the worst 64-row-aligned block of rows may not have a mean row error above this multiple of the mean over all rows;
# the reference alone (emulated against plain oracle) gives 1.05 .. 1.08 over the nine configurations (under 3: no power of two needed)
BLOCK_RATIO = 3.0


@pytest.mark.parametrize("name", ["base", "small4", "small"])
@pytest.mark.parametrize("gemm,storage", [("split", torch.bfloat16), ("bf16", torch.bfloat16), ("bf16", torch.float32)])
def test_encoder_forward_bf16_configurations(name, gemm, storage, modes):
    ops.set_gemm_mode(gemm)
    ops.set_value_storage(storage)
    got = _gpu_frame(name, True)
    want = _oracle_frame(name, True)
    assert (got - want).abs().max().item() < 0.1
    cos = torch.nn.functional.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    assert cos > 0.999, cos
    # ... and against the reference-only yardstick
    ref = _forward_yardstick(name, gemm, storage)
    tab = BF16_FWD_E_REF[(name, gemm, storage)]
    assert tab[0] / 2 < ref["max_abs"] < tab[0] * 2 and tab[1] / 2 < ref["one_minus_cos"] < tab[1] * 2, (ref, tab)
    tol = (min(3 * ref["max_abs"], 0.1), min(3 * ref["one_minus_cos"], 1e-3))
    err, omc = output_errors(got, want)
    rows = (got - want).abs().amax(-1).flatten()                  # per-row max abs error over the BEV rows
    ratio = row_block_ratio(got, want)
    print(f"{name} gemm={gemm} storage={str(storage).split('.')[-1]} forward: E_ref max abs {ref['max_abs']:.3e}, 1 - cos "
          f"{ref['one_minus_cos']:.3e}, block ratio {ref['block_ratio']:.3f}; product max abs {err:.3e} (bound {tol[0]:.3e}), "
          f"1 - cos {omc:.3e} (bound {tol[1]:.3e}), block ratio {ratio:.3f} (bound {BLOCK_RATIO})")
    assert err <= tol[0] and omc <= tol[1], (err, omc, tol)
    assert rows.numel() == want.shape[1] and int((rows > tol[0]).sum()) == 0
    assert ref["block_ratio"] <= BLOCK_RATIO and ratio <= BLOCK_RATIO, (ref["block_ratio"], ratio)


@pytest.mark.parametrize("row_order", ["polar", "image"])
def test_fused_sca_kernel_at_the_full_base_row_count(row_order):
    """The launch the bench times — fused SCA sampling over all R ~ 46 k ragged rows with the
    shared projection rows (row_src), the device-side row count and 32-bit byte offsets into the
    189 MB value tensor — against the oracle's statement of the fused contract on row slices
    spread over the whole row range (first / middle / last rows of every camera)."""
    from bevformer_amd.modules import geometry as G
    name = "base"
    w = S.WORKLOADS[name]
    Q = w["bev_h"] * w["bev_w"]
    M, L, P, D = 8, 4, 8, 32
    g = torch.Generator().manual_seed(0)
    shapes, start = S.level_tensors(name)
    Sv = int(shapes.prod(1).sum())
    value = torch.randn(S.NUM_CAMS, Sv, M, D, generator=g)
    proj = torch.randn(Q, M * L * P * 3, generator=g)
    n_off = M * L * P * 2
    proj[:, :n_off] *= 4.0                                            # offsets of a few pixels
    # ("image" = the calibrated order the bench runs; "polar" = the order that needs no calibration)
    pl = G.DevicePlanner(w["bev_h"], w["bev_w"], 1, S.PC_RANGE, 4, S.NUM_CAMS, DEV, row_order=row_order)
    plan = pl.plan(S.make_img_metas(name))
    host = plan.materialize()
    R = host.row_batch.numel()
    assert 40000 < R < 60000
    kw = dict(M=M, L=L, P=P, K=1, off_head=L * P * 2, off_k=0, lg_head=L * P, lg_k=0, ref_mode=0, vmul=1, vadd=0)
    static = ops.msda_fused(value.to(DEV), shapes.to(DEV), start.to(DEV), proj.to(DEV), n_off,
                            host.row_ref.reshape(-1, 1, 4, 2), host.row_batch, row_src=host.row_query32, **kw)
    assert R < plan.launch_rows <= plan.row_batch.numel()
    # the hint only sizes the launches: right, too small (the strided tail launch covers the rest),
    # absent, larger than the count — all must equal the fixed-count launch
    for hint in (plan.launch_rows, R // 2, 1000, 0, plan.row_batch.numel()):
        out = ops.msda_fused(value.to(DEV), shapes.to(DEV), start.to(DEV), proj.to(DEV), n_off,
                             plan.row_ref.reshape(-1, 1, 4, 2), plan.row_batch, row_src=plan.row_query32,
                             nrows=plan.nrows_dev, launch_rows=hint, **kw)
        assert out is not None and out.shape[0] == plan.row_batch.numel() >= R
        assert torch.equal(out[:R], static), hint
    rows = torch.cat([torch.arange(0, 300), torch.arange(R // 2 - 150, R // 2 + 150), torch.arange(R - 300, R)]
                     + [torch.arange(s - 20, s + 20).clamp(0, R - 1) for s in host.cam_start.cpu().tolist()[1:-1]])
    rows = rows.unique()
    want = _oracle_msda_fused(value, shapes, start, proj, n_off, host.row_ref.cpu()[rows].reshape(-1, 1, 4, 2),
                              host.row_batch.cpu()[rows], row_src=host.row_query32.cpu()[rows], **kw)
    torch.testing.assert_close(out.cpu()[rows], want, rtol=1e-4, atol=1e-5)


def test_fused_tsa_kernel_at_the_full_base_grid():
    name = "base"
    w = S.WORKLOADS[name]
    Q = w["bev_h"] * w["bev_w"]
    M, L, P, D, K = 8, 1, 4, 32, 2
    g = torch.Generator().manual_seed(1)
    shapes = torch.tensor([[w["bev_h"], w["bev_w"]]])
    start = torch.zeros(1, dtype=torch.long)
    value = torch.randn(2, Q, M, D, generator=g)
    n_off = M * K * L * P * 2
    proj = torch.randn(Q, n_off + M * K * L * P, generator=g)
    proj[:, :n_off] *= 3.0
    ref = torch.rand(Q, K, L, 2, generator=g)
    kw = dict(M=M, L=L, P=P, K=K, off_head=K * L * P * 2, off_k=L * P * 2, lg_head=K * L * P, lg_k=L * P,
              ref_mode=1, vmul=2, vadd=1, Q=Q)
    out = ops.msda_fused(value.to(DEV), shapes.to(DEV), start.to(DEV), proj.to(DEV), n_off, ref.to(DEV), None, **kw)
    rows = torch.cat([torch.arange(0, 400), torch.arange(Q // 2, Q // 2 + 400), torch.arange(Q - 400, Q)])
    # the oracle statement takes whole-row slices: evaluate it on the slice with the slice's own base rows
    want = _oracle_msda_fused(value, shapes, start, proj[rows], n_off, ref[rows], torch.zeros(len(rows), dtype=torch.int32),
                              **{**kw, "Q": 0})
    torch.testing.assert_close(out.cpu()[rows], want, rtol=1e-4, atol=1e-5)
    # the generic kernel (bevmsda_fused_desc.reserved[5] = 1, modes.fused_spec = 1) computes the same sums within round-off
    with ops.using(fused_spec=1):
        alt = ops.msda_fused(value.to(DEV), shapes.to(DEV), start.to(DEV), proj.to(DEV), n_off, ref.to(DEV), None, **kw)
    torch.testing.assert_close(alt, out, rtol=1e-5, atol=1e-6)


@functools.lru_cache(maxsize=None)
def _oracle_step(name, gemm=False, storage=False):
    """(output, gradients) of a training step of ``name`` through autograd of the oracle — plain fp32, or with the bf16
    roundings of ``helpers.oracle_bf16`` (the yardstick) — shared by the gradient cases of this module."""
    return oracle_training_step(name, gemm, storage)


@functools.lru_cache(maxsize=None)
def _grad_yardstick(name, gemm, storage):
    return E_ref(_oracle_step(name, gemm == "bf16", storage == torch.bfloat16), _oracle_step(name))


class _SeenLaunches:
    """``ops.set_gemm_timer`` hook for one step: the tag of every projection / chain / weight-gradient launch and the GEMM
    mode it ran under, and every call of the library GEMM (``torch.nn.functional.linear``) on a device tensor."""
    CHAINS = ("sca_out_ffn_chain", "tsa_out_sca_proj_chain")

    def __init__(self):
        self.tags, self.modes, self.library = [], set(), []

    def __call__(self, tag, flops, nbytes):
        self.tags.append(tag)
        self.modes.add(ops.gemm_mode())
        return ops._NoTimer()

    def __enter__(self):
        self.real = torch.nn.functional.linear

        def spy(x, *a, **k):
            if x.is_cuda:
                self.library.append(tuple(x.shape))
            return self.real(x, *a, **k)
        torch.nn.functional.linear = spy
        ops.set_gemm_timer(self)
        return self

    def __exit__(self, *exc):
        torch.nn.functional.linear = self.real
        ops.set_gemm_timer(None)

    def check(self, gemm, layers, tsa_chain_backward=True):
        """The step ran what the case claims: the chain forward kernels, the chain backward kernels and the multi-problem
        weight-gradient launches of every layer, all under GEMM mode ``gemm``, and no projection on the library GEMM.
        ``tsa_chain_backward`` False: the TSA seam's projection is not a multiple of 256 columns wide (one feature level:
        192), which its backward chain kernel does not take — its two input-gradient GEMMs must have run instead."""
        want = {c + sfx for c in self.CHAINS for sfx in ("", "_bwd", "_dw")}
        if not tsa_chain_backward:
            want = want - {self.CHAINS[1] + "_bwd"} | {self.CHAINS[1] + "_dx1", self.CHAINS[1] + "_dx0"}
        print("launch tags of the step:", {t: self.tags.count(t) for t in sorted(set(self.tags))})
        for tag in sorted(want):
            assert self.tags.count(tag) == layers, (tag, self.tags.count(tag), layers)
        assert tsa_chain_backward or self.CHAINS[1] + "_bwd" not in self.tags
        assert self.modes == {gemm}, self.modes
        assert not self.library, f"projections on torch.nn.functional.linear: {self.library}"


def _gradient_case(name, storage, l2_tol, max_tol, gemm="split", train=False, out_tol=None):
    """Output and the gradients w.r.t. BEV queries, camera features and every parameter of workload ``name`` against
    autograd through the plain fp32 oracle; prints the per-tensor errors (pytest -s / the log shows what the bounds rest
    on).  ``train``: the encoder in train() mode, dropout at its configured probabilities, the oracle fed the scale
    tensors the step drew.  ``out_tol`` = (max abs, 1 - cos) bound of the output (bf16 arithmetic)."""
    ops.set_gemm_mode(gemm)
    ops.set_value_storage(storage)
    torch.set_num_threads(16)
    enc, sd = build_pair(name, device=DEV)
    q, f, kw = S.make_inputs(name, seed=0, temporal=True)
    gout = torch.randn(1, q.shape[0], 256, generator=torch.Generator().manual_seed(5))
    qd, fd = q.to(DEV).requires_grad_(True), f.to(DEV).requires_grad_(True)
    kwd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
    for p in enc.parameters():
        p.requires_grad_(True)
    drawn, real_scale = [], train_ops.dropout_scale

    def recording(shape, p, device):
        drawn.append(real_scale(shape, p, device))
        return drawn[-1]
    if train:
        enc.train()
        train_ops.dropout_scale = recording
        torch.manual_seed(11)
    try:
        with _SeenLaunches() as seen:
            got = enc(qd, fd, fd, **kwd)
            got.backward(gout.to(DEV))
    finally:
        train_ops.dropout_scale = real_scale
    if gemm != "split" or train:
        seen.check(gemm, len(enc.layers), tsa_chain_backward=len(S.WORKLOADS[name]["shapes"]) * 8 * 8 * 3 % 256 == 0)
    tag = f"{name} gemm={gemm} storage={str(storage).split('.')[-1]}" + (" train()" if train else "")
    if train:
        assert len(drawn) == 4 * len(enc.layers), len(drawn)
        scales = [t.cpu() for t in drawn]
        want, want_g = oracle_training_step(name, dropout_scales=scales)
        ref = E_ref(oracle_training_step(name, gemm == "bf16", storage == torch.bfloat16, dropout_scales=scales),
                    (want, want_g))
        l2_tol, max_tol, out_tol = 3 * ref["l2"], 3 * ref["max_ratio"], (3 * ref["max_abs"], 3 * ref["one_minus_cos"])
        print(f"{tag}: E_ref output max abs {ref['max_abs']:.3e}, 1 - cos {ref['one_minus_cos']:.3e}; gradients worst rel L2 "
              f"{ref['l2']:.3e}, worst max ratio {ref['max_ratio']:.3e}")
    else:
        want, want_g = _oracle_step(name)
    bf = storage == torch.bfloat16 or gemm == "bf16"
    if bf:
        err, omc = output_errors(got, want)
        assert err < 0.1                                                # (the bound of every bf16 case before the yardstick)
        if out_tol is not None:
            print(f"{tag} output: max abs {err:.3e} (bound {out_tol[0]:.3e}), 1 - cos {omc:.3e} (bound {out_tol[1]:.3e})")
            assert err <= out_tol[0] and omc <= out_tol[1], (err, omc, out_tol)
    else:
        torch.testing.assert_close(got.detach().cpu(), want.detach(), **ENC_TOL)
    # Bilinear sampling is piecewise linear in the location: a sampling point that sits within round-off
    # of a pixel boundary takes the slope of one side on the CPU and of the other on the GPU, so single
    # elements of a gradient may differ by a whole tap difference.  Two bounds per tensor: the relative
    # L2 error (the tensor as a whole) and the max error relative to the tensor's largest entry.
    bad, worst = {}, (0.0, 0.0)
    pairs = [("bev_query", qd.grad), ("feat", fd.grad)] + [(k, p.grad) for k, p in enc.named_parameters()]
    for k, a in pairs:
        b = want_g.get(k)
        assert a is not None and b is not None, k
        a = a.cpu().double()
        b = b.double()
        l2 = ((a - b).norm() / (b.norm() + 1e-30)).item()
        mx = ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()
        print(f"{tag} grad {k}: rel L2 {l2:.2e}, max err / max |grad| {mx:.2e}")
        worst = (max(worst[0], l2), max(worst[1], mx))
        if l2 > l2_tol or mx > max_tol:
            bad[k] = (l2, mx)
    print(f"{tag}: worst rel L2 {worst[0]:.2e} (bound {l2_tol:.3g}), worst max ratio {worst[1]:.2e} (bound {max_tol:.3g})")
    assert not bad, bad


# fp32 rows: bounds = 3 x the worst per-tensor error measured on the GPU box (profiles/r3/r3c_gradient_errors.log); the float32 CPU
# oracle is itself 2e-3 (d query) / 6e-3 (worst parameter) away from a float64 evaluation (profiles/r2/train_fwd_table.txt)
# measured (r3c): small4 fp32 5.1e-3 / 4.6e-2, small4 bf16 3.1e-2 / 9.0e-2, base1 fp32 2.0e-3 / 2.9e-2, base1 bf16 2.0e-2 / 5.0e-2
# bf16 rows: OUTER bounds only (they were measured on the product).  What a bf16 case is held to is ``_bf16_bounds``.
GRAD_TOL = {("small4", torch.float32): (1e-2, 0.1), ("small4", torch.bfloat16): (5e-2, 0.27),
            ("base1", torch.float32): (6e-3, 0.09), ("base1", torch.bfloat16): (5e-2, 0.15),
            # reference-true small (one level): the same three layers over a 920-pixel map — small4's bounds
            ("small", torch.float32): (1e-2, 0.1), ("small", torch.bfloat16): (5e-2, 0.27)}


def _bf16_bounds(name, gemm, storage):
    """Bounds of a bf16 gradient case: 3 x ``E_ref`` (the emulated oracle against the plain one: tests/helpers.py), the 3
    being this table's margin for a measured bound (different summation order in the product, one more rounding of an
    intermediate activation in the chain kernels).  The yardstick is the worst tensor's: a slope flip at a pixel
    boundary is a chance event for a single tensor, the worst of 80 tensors is a stable statistic.  For the storage-only
    cases the ``GRAD_TOL`` row stays where it is the tighter of the two.  -> (l2, max ratio, (output max abs, 1 - cos))
    E_ref on the CPU, worst tensor (rel L2 / max ratio; output max abs / 1 - cos); the product's: profiles/bf16_bounds.log
      small4 bf16 GEMM + bf16 storage 7.07e-2 / 9.31e-2; 2.27e-2 / 8.19e-6      small4 bf16 GEMM 7.08e-2 / 8.89e-2; 2.34e-2 / 7.67e-6
      base1  bf16 GEMM + bf16 storage 5.95e-2 / 1.12e-1; 1.38e-2 / 2.99e-6      small  bf16 GEMM + bf16 storage 6.93e-2 / 9.76e-2; 2.47e-2 / 8.88e-6
      storage only: small4 3.19e-2 / 9.02e-2, base1 1.97e-2 / 4.69e-2, small 3.13e-2 / 7.05e-2 (x 3 = 9.6e-2 / 0.27, 5.9e-2 / 0.14,
      9.4e-2 / 0.21: tighter than ``GRAD_TOL`` for base1's and small's max ratio only)
    the product on an MI355X, worst tensor: small4 bf16 + bf16 6.98e-2 / 9.01e-2, small4 bf16 GEMM 6.98e-2 / 8.93e-2, base1 5.95e-2 /
    1.11e-1, small 6.71e-2 / 1.01e-1, small4 train() 7.66e-2 / 1.04e-1 (its yardstick, same dropout scales: 7.56e-2 / 1.00e-1)"""
    ref = _grad_yardstick(name, gemm, storage)
    print(f"{name} gemm={gemm} storage={str(storage).split('.')[-1]}: E_ref output max abs {ref['max_abs']:.3e}, 1 - cos "
          f"{ref['one_minus_cos']:.3e}; gradients worst rel L2 {ref['l2']:.3e}, worst max ratio {ref['max_ratio']:.3e}")
    l2, mx = 3 * ref["l2"], 3 * ref["max_ratio"]
    if gemm == "split":
        l2, mx = min(l2, GRAD_TOL[(name, storage)][0]), min(mx, GRAD_TOL[(name, storage)][1])
    return l2, mx, (3 * ref["max_abs"], 3 * ref["one_minus_cos"])


def _bounds(name, storage):
    if storage == torch.bfloat16:
        l2, mx, out = _bf16_bounds(name, "split", storage)
        return dict(l2_tol=l2, max_tol=mx, out_tol=out)
    return dict(zip(("l2_tol", "max_tol"), GRAD_TOL[(name, storage)]))


@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16])
def test_small_reference_true_forward_backward_gradients(storage, modes):
    """The reference's own bevformer_small shape set (1 level (23, 40), 3 layers, 150 x 150 queries;
    projects/configs/bevformer/bevformer_small.py:41-43,88), forward + backward."""
    _gradient_case("small", storage, **_bounds("small", storage))


@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16])
def test_small4_forward_backward_gradients(storage, modes):
    """BASELINE configs[2] (150x150 BEV, 4 levels, 3 layers, fwd + bwd)."""
    _gradient_case("small4", storage, **_bounds("small4", storage))


@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16])
def test_base_geometry_one_layer_forward_backward_gradients(storage, modes):
    """One encoder layer at the base geometry (200x200 queries, 45,960 image-ordered SCA rows, 128-row sort
    workgroups, 16x16 TSA tiles): what ``fwd_bwd_base`` of the bench runs six times."""
    _gradient_case("base1", storage, **_bounds("base1", storage))


@pytest.mark.parametrize("name,storage", [("small4", torch.bfloat16), ("small4", torch.float32), ("base1", torch.bfloat16),
                                          ("small", torch.bfloat16)],
                         ids=["small4-bf16", "small4-fp32", "base1-bf16", "small-bf16"])
def test_bf16_gemm_forward_backward_gradients(name, storage, modes):
    """The arithmetic ``fwd_bwd_small4_bf16`` of the bench times — bf16 GEMM operands (chain forward and backward
    kernels, bf16 weight-gradient kernels, the input-gradient GEMMs over the transposed weight images) with bf16 or fp32
    value storage — against autograd through the PLAIN fp32 oracle: output and every gradient within 3 x E_ref."""
    l2, mx, out = _bf16_bounds(name, "bf16", storage)
    _gradient_case(name, storage, l2, mx, gemm="bf16", out_tol=out)


def test_small4_bf16_train_mode_forward_backward_gradients(modes):
    """``fwd_bwd_small4_bf16`` with the encoder in train(): dropout active at its configured probabilities (what selects
    the chain kernels' dropout operands in a training step), the oracle fed the scale tensors the step drew; the
    yardstick is the emulated oracle against the plain one under the SAME scale tensors."""
    _gradient_case("small4", torch.bfloat16, None, None, gemm="bf16", train=True)


def _masked_gradient_case(name, n_rows, l2_tol, max_tol, eps=1e-4, relu_eps=1e-4):
    """Gradients of a training step of workload ``name`` against autograd through the oracle in FLOAT64, with the loss
    restricted to BEV queries that sit on no KINK of the encoder: no sampling point (any layer, TSA or SCA) within
    ``eps`` pixels of a pixel boundary, no FFN pre-activation within ``relu_eps`` of zero.  Bilinear sampling is piecewise
    linear in the location and ReLU in its input, so on the other queries a float32 evaluation may take the
    neighbouring piece's slope — the reason ``_gradient_case`` needs a per-element bound of 10 % (measured on the base
    shape: with the sampling kinks masked but not ReLU's, 13 flipped pre-activations of 1.3 M still put 3.6e-3 rel L2 on
    d bev_query; profiles/r5/r5k_masked_gradients.log) —; with those queries given a zero output gradient (their rows then
    receive none, in either implementation) the comparison is between smooth functions and the bound is float32
    rounding: measured worst tensor 2.9e-5 rel L2, worst element 2.6e-5 of its tensor's largest (base, six layers).  ``n_rows``: evaluate the oracle on that
    many randomly chosen queries only (0 = all) — the output gradient is zero elsewhere, so the product's FULL step has
    the same gradients."""
    ops.set_value_storage(torch.float32)
    torch.set_num_threads(16)
    enc, sd = build_pair(name, device=DEV)
    q, f, kw = S.make_inputs(name, seed=0, temporal=True)
    Q = q.shape[0]
    rows = (torch.randperm(Q, generator=torch.Generator().manual_seed(3))[:n_rows].sort().values if n_rows
            else torch.arange(Q))
    rec = EdgeRecorder(Q, camera_rows(name, rows), eps=eps, query_ids=rows, relu_eps=relu_eps)
    d = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    qc, fc = q.double().requires_grad_(True), f.double().requires_grad_(True)
    want = oracle_encoder_rows(leaves, qc, fc, rows, pc_range=S.PC_RANGE, msda=rec, **{k: d(v) for k, v in kw.items()})
    keep = rows[~rec.fragile[rows]]
    assert len(keep) > len(rows) // 8, (len(keep), len(rows))
    gout = torch.zeros(1, Q, 256)
    gout[:, keep] = torch.randn(1, len(keep), 256, generator=torch.Generator().manual_seed(5))
    want.backward(gout[:, rows].double())
    qd, fd = q.to(DEV).requires_grad_(True), f.to(DEV).requires_grad_(True)
    kwd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
    for p in enc.parameters():
        p.requires_grad_(True)
    got = enc(qd, fd, fd, **kwd)
    got.backward(gout.to(DEV))
    torch.testing.assert_close(got.detach().cpu()[:, rows].double(), want.detach(), rtol=2e-4, atol=2e-4)
    bad, worst = {}, (0.0, 0.0)
    pairs = [("bev_query", qd.grad, qc.grad), ("feat", fd.grad, fc.grad)]
    pairs += [(k, p.grad, leaves[k].grad) for k, p in enc.named_parameters()]
    for k, a, b in pairs:
        assert a is not None and b is not None, k
        a = a.cpu().double()
        l2 = ((a - b).norm() / (b.norm() + 1e-30)).item()
        mx = ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()
        print(f"{name} masked ({len(keep)} of {len(rows)} queries) grad {k}: rel L2 {l2:.2e}, max err / max |grad| {mx:.2e}")
        worst = (max(worst[0], l2), max(worst[1], mx))
        if l2 > l2_tol or mx > max_tol:
            bad[k] = (l2, mx)
    print(f"{name} masked: worst rel L2 {worst[0]:.2e} (bound {l2_tol}), worst max ratio {worst[1]:.2e} (bound {max_tol})")
    assert not bad, bad


def test_small4_gradients_away_from_pixel_boundaries_at_float32_rounding(modes):
    """BASELINE configs[2] again, every query, against float64, the loss on the queries with no edge-adjacent sampling
    point and no near-zero FFN pre-activation: rel L2 <= 2e-4 per tensor, every element within 2e-4 of the tensor's largest."""
    _masked_gradient_case("small4", 0, 2e-4, 2e-4)


def test_base_six_layer_gradients_on_a_query_subsample_against_float64(modes):
    """BASELINE configs[1]'s shape set (200 x 200 queries, 4 levels, SIX layers) forward + backward — what ``fwd_bwd_base``
    of the bench times — against a float64 oracle evaluated on 6,000 of the 40,000 queries."""
    _masked_gradient_case("base", 6000, 2e-4, 2e-4)


def _rank_cells(w, world, rank, layout):
    from bevformer_amd import bev_tiling
    if layout == "rows":
        h0, h1 = bev_tiling.row_blocks(w["bev_h"], world)[rank]
        return torch.arange(h0 * w["bev_w"], h1 * w["bev_w"], device=DEV)
    q0, q1 = bev_tiling.query_blocks(w["bev_h"] * w["bev_w"], world)[rank]
    return bev_tiling.sector_order(w["bev_h"], w["bev_w"], S.PC_RANGE, DEV)[1][q0:q1]


@pytest.mark.parametrize("layout", ["rows", "sectors"])
def test_base_size_tiled_ranks_equal_the_untiled_rows(layout):
    """SURVEY.md §8e at the size BASELINE configs[3] names: rank r of an 8-GPU BEV-tiled job (simulated in this process:
    the rank's device-side tile plan at 200 x 200 / 4 levels, camera-segment skipping of the replicated value projection,
    the sector gather / scatter, every kernel at tile size) must produce the untiled base frame's rows — against the
    untiled GPU frame (tight: the same kernels over other row partitions) and against the CPU oracle (``ENC_TOL``)."""
    from bevformer_amd import bev_tiling
    name, world = "base", 8
    w = S.WORKLOADS[name]
    enc, _ = build_pair(name, device=DEV)
    q, f, kw = S.make_inputs(name, seed=0, temporal=True, device=DEV)
    want_cpu = _oracle_frame(name, True)
    with torch.no_grad():
        want = enc(q, f, f, **kw)
        for rank in (0, 3, 7):
            bev_tiling.enable_bev_tiling(enc, simulate=(rank, world), layout=layout)
            got = enc(q, f, f, **kw)
            bev_tiling.disable_bev_tiling(enc)
            mine = _rank_cells(w, world, rank, layout)
            assert mine.numel() == w["bev_h"] * w["bev_w"] // world
            torch.testing.assert_close(got[:, mine], want[:, mine], rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(got[:, mine].cpu(), want_cpu[:, mine.cpu()], **ENC_TOL)


@pytest.mark.parametrize("name", ["micro4", "small4"])
def test_fp16_enabled_encoder_with_half_inputs_on_the_gpu(name):
    """The reference's fp16 mode (``@auto_fp16()`` at encoder.py:151, ``wrap_fp16_model`` in tools/fp16/train.py:224-226,
    config bevformer_fp16/bevformer_tiny_fp16.py:270): ``fp16_enabled`` set on every module that has it, half
    ``bev_query`` / camera features (cast by the decorator) and half ``bev_pos`` / ``prev_bev`` (as ``get_bev_features``
    hands them over).  The product widens the ROUNDED inputs and computes in fp32, so the result is held to the fp32
    tolerance against the oracle on the rounded inputs (the reference's own fp16 arithmetic is coarser than that)."""
    from bevformer_amd import registry
    enc, sd = build_pair(name, device=DEV)
    registry.wrap_fp16_model(enc)
    q, f, kw = S.make_inputs(name, seed=0, temporal=True)

    def r(t):
        return t.half().float()
    kwr = dict(kw, bev_pos=r(kw["bev_pos"]), prev_bev=r(kw["prev_bev"]))
    torch.set_num_threads(16)
    with torch.no_grad():
        want = O.encoder_forward(sd, r(q), r(f), pc_range=S.PC_RANGE, **kwr)
        kwd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
        kwd["bev_pos"], kwd["prev_bev"] = kwd["bev_pos"].half(), kwd["prev_bev"].half()
        got = enc(q.to(DEV), f.to(DEV), f.to(DEV), **kwd)                 # fp32 in: the decorator rounds to half
        also = enc(q.to(DEV).half(), f.to(DEV).half(), f.to(DEV).half(), **kwd)
    assert got.dtype == torch.float32 and torch.equal(got, also)
    torch.testing.assert_close(got.cpu(), want, **ENC_TOL)
    # ... and under autograd (the widening is differentiable; the per-op / chain path decides on the fp32 tensors)
    qd = q.to(DEV).requires_grad_(True)
    out = enc(qd, f.to(DEV), f.to(DEV), **kwd)
    out.sum().backward()
    assert out.dtype == torch.float32 and torch.isfinite(qd.grad).all()
    torch.testing.assert_close(out.detach().cpu(), want, **ENC_TOL)
