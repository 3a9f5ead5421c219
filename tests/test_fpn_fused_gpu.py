"""GPU: the image neck on the row convolution kernel (``ops.fpn``, ``modes.fpn_fused``) against the float64 restatement of
mmdet's FPN forward (tests/fpn_yardstick.py).  Bound per level: error <= 3 x the error of the parent arm (every convolution as
im2col + ``ops.linear``, adds and upsampling in torch fp32) on the same inputs in the same GEMM mode; on the sparse integer
lattice of the yardstick every level EQUALS it.  Then the seams: the module switch, the weight image cache, graph capture,
``flatten_feats`` on the neck's channel-last views, and neck -> ``get_bev_features`` at micro size."""
import functools

import pytest
import torch

import bevformer_amd
from bevformer_amd import synthetic as S

import fpn_yardstick as Y
from helpers import build_transformer_pair

pytestmark = pytest.mark.gpu

# name -> (in_channels, out_channels, num_outs, finest (H, W)); n_img = 2 everywhere
NECKS = {
    "base_toy": ((64, 96, 128), 160, 4, (12, 20)),        # 12x20, 6x10, 3x5 -> + a 2x3 extra level
    "tiny": ((2048,), 160, 1, (3, 5)),                    # one lateral of the deepest K, one output
    "extra2": ((64, 96, 128), 160, 5, (12, 20)),          # ReLU in front of the second extra level (2x3 -> 1x2)
}
FLAT = "flat"                                             # for flatten_feats, whose transposing kernel takes C % 64 == 0
NECKS_FLAT = {FLAT: ((64, 96, 128), 192, 4, (12, 20))}
N_IMG = 2


def _build(name, **kw):
    in_c, out_c, num_outs, _ = {**NECKS, **NECKS_FLAT}[name]
    cfg = dict(type="FPN", in_channels=list(in_c), out_channels=out_c, start_level=0, add_extra_convs="on_output",
               num_outs=num_outs, relu_before_extra_convs=True)
    cfg.update(kw)
    return bevformer_amd.build_neck(cfg)


@functools.lru_cache(maxsize=None)
def _case(name, lattice=False):
    """(neck on the GPU, inputs on the GPU, float64 outputs): made once per case and shared; nobody writes to it."""
    in_c, out_c, num_outs, (H, W) = {**NECKS, **NECKS_FLAT}[name]
    neck = (Y.lattice_neck_ if lattice else Y.randomize_neck_)(_build(name), seed=11)
    g = torch.Generator().manual_seed(12)
    draw = (lambda *s: Y.lattice(s, -4, 4, g)) if lattice else (lambda *s: torch.randn(*s, generator=g))
    xs = [draw(N_IMG, c, H >> i, W >> i) for i, c in enumerate(in_c)]
    want = Y.fpn64(neck.state_dict(), Y.spec_of(neck), xs, check_lattice=lattice)
    return neck.cuda().eval(), [x.cuda() for x in xs], want


def _shapes(name):
    _, out_c, num_outs, (H, W) = NECKS[name]
    n = len(NECKS[name][0])
    hw = [(H >> i, W >> i) for i in range(n)]
    while len(hw) < num_outs:
        hw.append(((hw[-1][0] - 1) // 2 + 1, (hw[-1][1] - 1) // 2 + 1))
    return [(N_IMG, out_c, h, w) for h, w in hw]


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("name", list(NECKS))
def test_fpn_within_three_parent_errors_per_level(name, mode):
    from bevformer_amd import ops
    neck, xs, want = _case(name)
    with torch.no_grad(), ops.using(gemm=mode):
        assert ops.fpn_reject(neck, xs) is None
        got = ops.fpn(neck, xs)
        parent = Y.parent_fpn(neck.state_dict(), Y.spec_of(neck), xs)
    assert got is not None and [tuple(g.shape) for g in got] == _shapes(name)
    for lvl, (g, p, w) in enumerate(zip(got, parent, want)):
        assert g.permute(0, 2, 3, 1).is_contiguous()                    # an NCHW-shaped view of channel-last rows
        e_parent, e_fused = Y.max_err(p, w), Y.max_err(g, w)
        print(f"{name} {mode} level {lvl}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        assert e_fused <= 3 * e_parent


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("name", list(NECKS))
def test_fpn_exact_on_the_lattice(name, mode):
    from bevformer_amd import ops
    neck, xs, want = _case(name, lattice=True)
    with torch.no_grad(), ops.using(gemm=mode):
        got = ops.fpn(neck, xs)
    assert got is not None and len(got) == len(want)
    for g, w in zip(got, want):
        assert torch.equal(g.double().cpu(), w)


def test_fpn_without_extra_convs_subsamples():
    from bevformer_amd import ops
    neck = Y.lattice_neck_(_build("base_toy", add_extra_convs=False), seed=13)
    _, xs, _ = _case("base_toy", lattice=True)
    want = Y.fpn64(neck.state_dict(), Y.spec_of(neck), xs, check_lattice=True)
    neck = neck.cuda()
    with torch.no_grad(), ops.using(gemm="split"):
        got = ops.fpn(neck, xs)
    assert [tuple(g.shape) for g in got] == _shapes("base_toy")
    assert all(torch.equal(g.double().cpu(), w) for g, w in zip(got, want))


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_the_module_takes_the_fast_path_only_with_the_switch(mode):
    from bevformer_amd import ops
    neck, xs, _ = _case("base_toy")
    # (MIOpen's default forward convolution is not reproducible run to run, so both module-path arms ask for its
    # deterministic algorithms; the comparison stays bit for bit)
    with torch.no_grad(), ops.using(gemm=mode), torch.backends.cudnn.flags(deterministic=True):
        torch_path = neck.forward_torch(xs)
        off = neck(xs)
        fused = ops.fpn(neck, xs)
        with ops.using(fpn_fused=True):
            on = neck(xs)
    assert isinstance(on, tuple) and isinstance(off, tuple) and len(on) == len(off) == 4
    assert all(torch.equal(a, b) for a, b in zip(off, torch_path))
    assert all(torch.equal(a, b) for a, b in zip(on, fused))
    assert not any(torch.equal(a, b) for a, b in zip(on, off))         # (different arithmetic: they cannot be the same bits)


def test_the_module_with_the_switch_but_a_rejected_call_runs_the_module_path():
    from bevformer_amd import ops
    neck, xs, _ = _case("base_toy")
    with torch.no_grad(), ops.using(gemm="native", fpn_fused=True), torch.backends.cudnn.flags(deterministic=True):
        assert ops.fpn_reject(neck, xs) == "GEMM mode native" and ops.fpn(neck, xs) is None
        on = neck(xs)
        want = neck.forward_torch(xs)
    assert all(torch.equal(a, b) for a, b in zip(on, want))
    uneven = [xs[0], xs[1][:, :, :, :9].contiguous(), xs[2]]
    with torch.no_grad(), ops.using(gemm="split", fpn_fused=True):
        assert ops.fpn_reject(neck, uneven) == "adjacent levels are not exact 2x of each other"


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_an_in_place_weight_update_is_seen_by_the_next_call(mode):
    """The weight images (1 x 1 and 3 x 3) are cached per weight VERSION."""
    from bevformer_amd import ops
    neck = Y.randomize_neck_(_build("base_toy"), seed=14).cuda().eval()
    _, xs, _ = _case("base_toy")
    with torch.no_grad(), ops.using(gemm=mode):
        first = ops.fpn(neck, xs)
        again = ops.fpn(neck, xs)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        neck.lateral_convs[2].conv.weight.mul_(-2.0)                    # in place: same address, next version
        neck.fpn_convs[0].conv.weight.mul_(0.5)
        neck.fpn_convs[3].conv.bias.add_(1.0)
        want = Y.fpn64(neck.state_dict(), Y.spec_of(neck), xs)
        got = ops.fpn(neck, xs)
        parent = Y.parent_fpn(neck.state_dict(), Y.spec_of(neck), xs)
    for lvl, (g, p, w, f) in enumerate(zip(got, parent, want, first)):
        e_parent, e_fused = Y.max_err(p, w), Y.max_err(g, w)
        print(f"weight update {mode} level {lvl}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  bound {3 * e_parent:.3e}")
        assert e_fused <= 3 * e_parent
        assert Y.max_err(f, w) > 0.1                                    # (the stale images would have given `first` again)


def test_captured_graph_replays_bit_equal():
    from bevformer_amd import ops
    neck, xs, _ = _case("extra2")
    second = [torch.randn(x.shape, generator=torch.Generator().manual_seed(20 + i)).cuda() for i, x in enumerate(xs)]
    static = [x.clone() for x in xs]
    with torch.no_grad(), ops.using(gemm="split", fpn_fused=True):
        eager = [[o.clone() for o in neck(src)] for src in (xs, second)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            neck(static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = neck(static)
        for src, want in ((xs, eager[0]), (second, eager[1]), (xs, eager[0])):
            for s, r in zip(static, src):
                s.copy_(r)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(o, w) for o, w in zip(out, want))


@pytest.mark.parametrize("bs,nc", [(1, 2), (2, 1)])
@pytest.mark.parametrize("cams", [True, False], ids=["cams", "nocams"])
def test_flatten_feats_reads_the_necks_views_without_a_transpose(bs, nc, cams):
    """With the switch on and the neck's channel-last views as input, ``flatten_feats`` goes through ``bevmsda_flatten_rows_f32``
    and writes the bits the transposing kernel writes from the same values as contiguous NCHW with the switch off."""
    from bevformer_amd import ops
    neck, xs, _ = _case(FLAT)
    g = torch.Generator().manual_seed(30)
    C = NECKS_FLAT[FLAT][1]
    cams_embeds = torch.randn(nc, C, generator=g).cuda() if cams else None
    level_embeds = torch.randn(4, C, generator=g).cuda()
    with torch.no_grad(), ops.using(gemm="split"):
        outs = ops.fpn(neck, xs)
        views = [o.view(bs, nc, *o.shape[1:]) for o in outs]
        assert all(v.data_ptr() == o.data_ptr() and not v.is_contiguous() for v, o in zip(views[:3], outs))
        dense = [v.contiguous() for v in views]
        want, shapes_w, starts_w = ops.flatten_feats(dense, cams_embeds, level_embeds)
        with ops.using(fpn_fused=True):
            got, shapes_g, starts_g = ops.flatten_feats(views, cams_embeds, level_embeds)
            mixed, _, _ = ops.flatten_feats(dense, cams_embeds, level_embeds)       # NCHW levels with the switch on: as before
    assert got.shape == want.shape == (nc, sum(o.shape[2] * o.shape[3] for o in outs), bs, C)
    assert torch.equal(got, want) and torch.equal(mixed, want)
    assert torch.equal(shapes_g, shapes_w) and torch.equal(starts_g, starts_w)


def test_flatten_feats_fast_branch_is_taken(monkeypatch):
    """(the equality above would also hold if the early branch were never entered: count the launches)"""
    from bevformer_amd import _lib, ops
    neck, xs, _ = _case(FLAT)
    lib = _lib.load()
    calls = {"rows": 0, "feats": 0}
    real_rows, real_feats = lib.bevmsda_flatten_rows_f32, lib.bevmsda_flatten_feats_f32
    monkeypatch.setattr(lib, "bevmsda_flatten_rows_f32", lambda *a: (calls.__setitem__("rows", calls["rows"] + 1), real_rows(*a))[1])
    monkeypatch.setattr(lib, "bevmsda_flatten_feats_f32", lambda *a: (calls.__setitem__("feats", calls["feats"] + 1), real_feats(*a))[1])
    level_embeds = torch.randn(4, NECKS_FLAT[FLAT][1]).cuda()
    with torch.no_grad(), ops.using(gemm="split"):
        views = [o.view(1, N_IMG, *o.shape[1:]) for o in ops.fpn(neck, xs)]
        with ops.using(fpn_fused=True):
            ops.flatten_feats(views, None, level_embeds)
        assert calls == {"rows": 4, "feats": 0}
        ops.flatten_feats(views, None, level_embeds)
        assert calls == {"rows": 4, "feats": 4}


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_neck_into_get_bev_features_at_micro_size(mode):
    """Neck -> ``PerceptionTransformer.get_bev_features`` with the switch on against the same chain with it off.  Tolerance:
    3 x the difference the PARENT arm's neck outputs produce at the encoder output against that same module-path chain."""
    from bevformer_amd import ops
    t, _ = build_transformer_pair("micro4", device="cuda")
    _, bq, kw = S.make_transformer_inputs("micro4", seed=0, bs=1, device="cuda")
    neck = Y.randomize_neck_(bevformer_amd.build_neck(dict(
        type="FPN", in_channels=[64, 96, 128], out_channels=S.EMBED_DIMS, start_level=0, add_extra_convs="on_output",
        num_outs=4, relu_before_extra_convs=True)), seed=15).cuda().eval()
    g = torch.Generator().manual_seed(16)
    xs = [torch.randn(S.NUM_CAMS, c, 16 >> i, 24 >> i, generator=g).cuda() for i, c in enumerate((64, 96, 128))]

    def bev(levels):
        mlvl = [o.view(1, S.NUM_CAMS, *o.shape[1:]) for o in levels]
        return t.get_bev_features(mlvl, bq, kw["bev_h"], kw["bev_w"], grid_length=kw["grid_length"], bev_pos=kw["bev_pos"],
                                  prev_bev=None, img_metas=kw["img_metas"])

    with torch.no_grad(), ops.using(gemm=mode), torch.backends.cudnn.flags(deterministic=True):
        off = bev(neck(xs))
        parent = bev(Y.parent_fpn(neck.state_dict(), Y.spec_of(neck), xs))
        with ops.using(fpn_fused=True):
            levels = neck(xs)
            assert all(o.permute(0, 2, 3, 1).is_contiguous() for o in levels)       # the fast path ran
            on = bev(levels)
    d_parent, d_on = (parent - off).abs().max().item(), (on - off).abs().max().item()
    print(f"neck -> encoder {mode}: parent arm vs module path {d_parent:.3e}  switch on vs module path {d_on:.3e}  bound {3 * d_parent:.3e}")
    assert on.shape == off.shape and torch.isfinite(on).all()
    assert d_on <= 3 * d_parent
