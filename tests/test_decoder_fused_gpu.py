"""GPU: the decoder fast path (``modes.decoder_fused``: HIP self-attention core, one hoisted BEV value projection, seam
kernels) of the stock six-op ``DetectionTransformerDecoder``.  Yardstick: the SAME module on the CPU with every kernel
routed through the oracle (``helpers.oracle_ops``), as in ``test_full_transformer_forward_gpu_matches_cpu_path``."""
import contextlib

import pytest
import torch

import bevformer_amd
from bevformer_amd import ops
from bevformer_amd import synthetic as S

from helpers import oracle_ops
from test_decoder_cpu import _Reg, _trained

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEW_TAGS = ("dec_mha", "dec_value_proj_hoisted", "dec_qk_proj", "dec_v_proj", "dec_attn_out_proj", "dec_out_ffn_chain")


def _decoder(num_layers, seed=0):
    torch.manual_seed(seed)
    dec = bevformer_amd.build_transformer_layer_sequence(S.reference_decoder_cfg(num_layers)).eval()
    dec.load_state_dict(_trained(dec.state_dict()))
    return dec


def _inputs(bev, nq, bs, seed=4, **extra):
    q, qp, v, ref, shapes, start = S.make_decoder_inputs(*bev, num_query=nq, bs=bs, seed=seed)
    kw = dict(query=q, key=None, value=v, query_pos=qp, reference_points=ref, spatial_shapes=shapes, level_start_index=start)
    kw.update(extra)
    return kw


def _to(kw, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) or isinstance(v, torch.nn.Module) else v) for k, v in kw.items()}


def _run(dec, kw, fused):
    with torch.no_grad(), ops.using(decoder_fused=fused):
        return dec(**kw)


@contextlib.contextmanager
def _tags():
    seen = []

    @contextlib.contextmanager
    def gemm_cb(tag, flops, nbytes):
        seen.append(tag)
        yield

    @contextlib.contextmanager
    def kernel_cb(tag, nbytes):
        seen.append(tag)
        yield

    ops.set_gemm_timer(gemm_cb)
    ops.set_kernel_timer(kernel_cb)
    try:
        yield seen
    finally:
        ops.set_gemm_timer(None)
        ops.set_kernel_timer(None)


def test_switch_on_runs_the_new_kernels_once_per_layer_and_hoists_the_value_projection():
    dec = _decoder(6).to(DEV)
    kw = _to(_inputs((12, 10), 37, 2), DEV)
    with _tags() as seen:
        _run(dec, kw, fused=True)
    assert seen.count("dec_mha") == 6
    assert seen.count("dec_value_proj_hoisted") == 1
    assert seen.count("dec_value_proj") == 0
    assert seen.count("dec_out_ffn_chain") == 6 and seen.count("dec_fwd") == 6 and seen.count("dec_offs_attn") == 6
    assert seen.count("dec_output_proj") == 0
    with _tags() as seen:
        _run(dec, kw, fused=False)
    assert not [t for t in seen if t in NEW_TAGS]
    assert seen.count("dec_value_proj") == 6 and seen.count("dec_fwd") == 6


@pytest.mark.parametrize("bev,nq,bs", [((12, 10), 37, 2), ((50, 50), 900, 1)])
@pytest.mark.parametrize("with_reg", [False, True])
def test_two_layers_match_the_cpu_path(bev, nq, bs, with_reg):
    dec = _decoder(2)
    kw = _inputs(bev, nq, bs, reg_branches=_Reg(2) if with_reg else None)
    with torch.no_grad(), oracle_ops():
        want = dec(**kw)
    dec = dec.to(DEV)
    with ops.using(gemm="split"), _tags() as seen:
        got = _run(dec, _to(kw, DEV), fused=True)
    assert seen.count("dec_mha") == 2
    torch.testing.assert_close(got[0].cpu(), want[0], rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(got[1].cpu(), want[1], rtol=1e-4, atol=1e-4)


def test_six_layers_at_base_size_within_three_times_the_parent_error():
    """200 x 200 BEV, 900 queries, 6 layers, with reference-point refinement: error of the fused path against the CPU
    yardstick <= 3 x E_parent, E_parent = the error of the switch-off path (the parent commit's code) on the same inputs;
    3 = the project's standing factor for re-associated fp32 sums."""
    dec = _decoder(6)
    kw = _inputs((200, 200), 900, 1, reg_branches=_Reg(6))
    with torch.no_grad(), oracle_ops():
        want = dec(**kw)
    dec = dec.to(DEV)
    kwd = _to(kw, DEV)
    parent = _run(dec, kwd, fused=False)
    with _tags() as seen:
        fused = _run(dec, kwd, fused=True)
    assert seen.count("dec_mha") == 6 and seen.count("dec_value_proj_hoisted") == 1
    err = lambda got, i: (got[i].cpu() - want[i]).abs().max().item()
    e_parent, e_fused = err(parent, 0), err(fused, 0)
    print(f"\ndecoder 6 layers base: states  E_parent {e_parent:.3e}  fused {e_fused:.3e}  (bound 3 x E_parent = {3 * e_parent:.3e})")
    print(f"decoder 6 layers base: references  E_parent {err(parent, 1):.3e}  fused {err(fused, 1):.3e}")
    for i in range(6):          # (figures only: how the two paths' errors grow from layer to layer)
        lay = lambda got: (got[0][i].cpu() - want[0][i]).abs().max().item()
        print(f"    after layer {i + 1}: states  E_parent {lay(parent):.3e}  fused {lay(fused):.3e}")
    assert e_fused <= 3 * e_parent, f"fused error {e_fused:.3e} > 3 x E_parent = {3 * e_parent:.3e}"


@pytest.mark.parametrize("case", ["attn_mask", "train", "native", "box_refs"])
def test_uncovered_calls_fall_back_bit_identically(case):
    dec = _decoder(2).to(DEV)
    kw = _to(_inputs((12, 10), 37, 2), DEV)
    mode = {}
    if case == "attn_mask":
        mask = torch.zeros(37, 37, dtype=torch.bool, device=DEV)
        mask[:, ::3] = True
        kw["attn_masks"] = [mask, None]
    elif case == "train":
        dec.train()
        for m in dec.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if isinstance(m, torch.nn.MultiheadAttention):
                m.dropout = 0.0
    elif case == "native":
        mode = dict(gemm="native")
    elif case == "box_refs":
        ref = kw["reference_points"]
        kw["reference_points"] = torch.cat([ref, ref[..., :1]], -1)
    with ops.using(**mode):
        off = _run(dec, kw, fused=False)
        with _tags() as seen:
            on = _run(dec, kw, fused=True)
    assert not [t for t in seen if t in NEW_TAGS]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_captured_graph_replays_bit_equal_to_the_eager_fused_call():
    dec = _decoder(3).to(DEV)
    reg = _Reg(3).to(DEV)
    first = _to(_inputs((50, 50), 300, 2, seed=4), DEV)
    second = _to(_inputs((50, 50), 300, 2, seed=5), DEV)
    static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in first.items()}
    with torch.no_grad(), ops.using(decoder_fused=True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                dec(reg_branches=reg, **static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = dec(reg_branches=reg, **static)
        for kw in (first, second, first):
            for k, v in kw.items():
                if torch.is_tensor(v):
                    static[k].copy_(v)
            graph.replay()
            torch.cuda.synchronize()
            eager = dec(reg_branches=reg, **kw)
            assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        assert not torch.equal(_run(dec, dict(second, reg_branches=reg), True)[0], _run(dec, dict(first, reg_branches=reg), True)[0])


def test_full_transformer_forward_with_the_switch_on_matches_the_cpu_path():
    """``test_full_transformer_forward_gpu_matches_cpu_path`` with the decoder on its fast path: same tolerances."""
    cfg = S.transformer_cfg("micro")
    cfg["decoder"] = S.reference_decoder_cfg(num_layers=2)
    torch.manual_seed(0)
    t = bevformer_amd.build_transformer(cfg).eval()
    t.init_weights()
    t.load_state_dict(_trained(t.state_dict(), seed=9))
    mlvl, bq, kw = S.make_transformer_inputs("micro", seed=0, bs=1, temporal=True)
    oqe = torch.randn(13, 512, generator=torch.Generator().manual_seed(1))
    reg = _Reg(2)
    with torch.no_grad():
        with oracle_ops():
            want = t(mlvl, bq, oqe, reg_branches=reg, **kw)
        kwd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
        with ops.using(decoder_fused=True), _tags() as seen:
            got = t.to(DEV)([f.to(DEV) for f in mlvl], bq.to(DEV), oqe.to(DEV), reg_branches=reg.to(DEV), **kwd)
    assert seen.count("dec_mha") == 2 and seen.count("dec_value_proj_hoisted") == 1 and "dec_value_proj" not in seen
    for g, w_, tol in zip(got, want, (1e-3, 2e-3, 1e-5, 1e-3)):
        torch.testing.assert_close(g.cpu(), w_, rtol=tol, atol=tol)
