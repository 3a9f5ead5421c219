"""The role-split row-panel projection (csrc/linear_roles.h, ``desc.reserved[2] = 3``): bit-identical to the 64- and
128-row panel shapes of linear_panel.h over the forms it takes — plain, two row blocks, row segments, fp32 / bf16 out,
grouped — and to them inside the encoder, eagerly and in a replayed graph."""
import pytest
import torch

from bevformer_amd import ops
from helpers import build_pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _run(kernel, fn):
    with torch.no_grad(), ops.using(gemm_kernel=kernel):
        return fn()


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("out", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,groups", [(184950, 1536, 6), (5000, 1536, 6), (64 * 37 + 17, 1536, 6), (5000, 256, 1),
                                        (64 * 37 + 17, 256, 1), (1, 256, 1)])
def test_roles_equal_the_panel_shapes(mode, out, M, N, groups):
    x, w, b = _rand(M, 256, seed=1), _rand(N, 256, seed=2) * 0.05, _rand(N, seed=3)
    with ops.using(gemm=mode):
        fn = lambda: ops.linear(x, w, b, groups=groups, out_dtype=out)
        got = _run("panelr", fn)
        want = _run("panel64", fn)
        assert got is not None and torch.equal(got, want)
        if M > 100000:
            for knob in ("panelr1", "panelr2", "panelr3", "panelr4"):
                assert torch.equal(_run(knob, fn), want), knob
            assert torch.equal(_run("panel128", fn), want)


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("out", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("m0,m1", [(40000, 40000), (1000, 37), (33, 5000)])
def test_roles_two_row_blocks(mode, out, m0, m1):
    lo, hi = _rand(m0, 256, seed=4), _rand(m1, 256, seed=5)
    w, b = _rand(1536, 256, seed=6) * 0.05, _rand(1536, seed=7)
    with ops.using(gemm=mode):
        fn = lambda: ops.linear_rows2(lo, hi, w, b, groups=6, out_dtype=out)
        got = _run("panelr", fn)
        want = _run("panel64", fn)
        stacked = _run("panel128", lambda: ops.linear(torch.cat([lo, hi], 0), w, b, groups=6, out_dtype=out))
    assert got is not None and torch.equal(got, want)
    assert torch.equal(got, stacked)


@pytest.mark.parametrize("seg_len,nseg,empty", [(375, 12, (0, 3, 4, 11)), (37, 40, tuple(range(5, 31))), (1000, 3, (0, 1, 2))])
def test_roles_skip_unused_row_segments(seg_len, nseg, empty):
    """Rows of used segments equal the full launch; every row a 64-row workgroup skipped keeps its NaN prefill."""
    M, N, L = seg_len * nseg, 1536, 6
    x, w, b = _rand(M, 256, seed=8), _rand(N, 256, seed=9) * 0.05, _rand(N, seed=10)
    counts = torch.tensor([0 if i in empty else 1 + i % 3 for i in range(nseg)])
    start = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).to(torch.int32).to(DEV)
    ops._SEGMENT_POISON["on"] = True
    try:
        full = _run("panelr", lambda: ops.linear(x, w, b, groups=L))
        part = _run("panelr", lambda: ops.linear(x, w, b, groups=L, segments=(start, seg_len)))
        ref = _run("panel64", lambda: ops.linear(x, w, b, groups=L, segments=(start, seg_len)))
    finally:
        ops._SEGMENT_POISON["on"] = False
    assert torch.equal(full, _run("panel64", lambda: ops.linear(x, w, b, groups=L)))
    # same workgroups skipped as the 64-row panel kernel: NaN exactly where it left NaN, equal elsewhere
    assert torch.equal(torch.isnan(part), torch.isnan(ref))
    fin = ~torch.isnan(part)
    assert torch.equal(part[fin], full[fin])
    rows_used = torch.zeros(M, dtype=torch.bool)
    for i in range(nseg):
        if i not in empty:
            rows_used[i * seg_len:(i + 1) * seg_len] = True
    assert fin.all(-1).all(0).cpu()[rows_used].all()
    if len(empty) and seg_len >= 128:
        assert torch.isnan(part).any()


@pytest.mark.parametrize("graph", [False, True])
def test_encoder_equal_with_roles_forced_on_and_off(graph):
    enc, _ = build_pair("tiny", device=DEV)
    from bevformer_amd import synthetic as S
    q, f, kw = S.make_inputs("tiny", seed=0, temporal=True, device=DEV)
    outs = {}
    for kernel in ("panelr", "panel64"):
        with torch.no_grad(), ops.using(gemm_kernel=kernel):
            if not graph:
                outs[kernel] = enc(q, f, f, **kw)
                continue
            enc(q, f, f, **kw)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = enc(q, f, f, **kw)
            for _ in range(2):
                g.replay()
            torch.cuda.synchronize()
            outs[kernel] = out.clone()
    assert torch.isfinite(outs["panelr"]).all()
    assert torch.equal(outs["panelr"], outs["panel64"])
