"""GPU: the whole ``BEVFormerHead`` and the decoder's refinement with ``modes.head_fused``.  Yardstick: the SAME modules on
the CPU with every kernel routed through the oracle (``helpers.oracle_ops``); bound 3 x E_parent, E_parent = the error of the
switch-off path on the GPU on the same inputs."""
import contextlib
import functools

import pytest
import torch

import bevformer_amd
from bevformer_amd import ops
from bevformer_amd import synthetic as S

import head_yardstick as Y
from helpers import oracle_ops
from test_decoder_cpu import _Reg, _trained

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEAD_TAGS = ("head_branches", "dec_refine", "head_decode")
MAX_NUM = 100


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


@functools.lru_cache(maxsize=None)
def _head_case():
    """(head on the CPU, inputs, the CPU module path's outputs) at ``tiny``: 2 decoder layers, 37 queries, bs 1."""
    torch.manual_seed(0)
    head = bevformer_amd.build_head(S.head_cfg("tiny", num_query=37, decoder_layers=2, max_num=MAX_NUM)).eval()
    head.init_weights()
    head.transformer.load_state_dict(_trained(head.transformer.state_dict(), seed=9))
    Y.trained_like_head_(head.cls_branches, 4)
    Y.trained_like_head_(head.reg_branches, 5)
    mlvl, _, kw = S.make_transformer_inputs("tiny", seed=0, bs=1, temporal=True)
    with torch.no_grad(), oracle_ops():
        want = head(mlvl, kw["img_metas"], prev_bev=kw["prev_bev"])
    return head, mlvl, kw, want


def _run_head(head, mlvl, kw, **modes):
    with torch.no_grad(), ops.using(**modes):
        return head([f.to(DEV) for f in mlvl], kw["img_metas"], prev_bev=kw["prev_bev"].to(DEV))


def test_whole_head_tags_and_error_within_three_times_the_parent():
    head, mlvl, kw, want = _head_case()
    head = head.to(DEV)
    try:
        with _tags() as seen:
            parent = _run_head(head, mlvl, kw, head_fused=False, decoder_fused=True)
            head.get_bboxes({k: (v.clone() if torch.is_tensor(v) else v) for k, v in parent.items()}, kw["img_metas"])
        assert not [t for t in seen if t in HEAD_TAGS]
        with _tags() as seen:
            fused = _run_head(head, mlvl, kw, head_fused=True, decoder_fused=True)
            with ops.using(head_fused=True):
                boxes = head.get_bboxes(fused, kw["img_metas"])
        assert seen.count("head_branches") == 1 and seen.count("dec_refine") == 2 and seen.count("head_decode") == 1
        with _tags() as seen:               # without the decoder's fast path the head still fuses its own two steps
            _run_head(head, mlvl, kw, head_fused=True, decoder_fused=False)
        assert seen.count("head_branches") == 1 and seen.count("dec_refine") == 0
    finally:
        head.cpu()
    for k in ("all_cls_scores", "all_bbox_preds"):
        e_parent = (parent[k].cpu().double() - want[k].double()).abs().max().item()
        e_fused = (fused[k].cpu().double() - want[k].double()).abs().max().item()
        print(f"\nhead tiny {k}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  (bound 3 x E_parent = {3 * e_parent:.3e})")
        assert e_fused <= 3 * e_parent, f"{k}: fused error {e_fused:.3e} > 3 x E_parent = {3 * e_parent:.3e}"
    # get_bboxes stage-wise: the GPU's own predictions through the yardstick's decode on the CPU
    cls, box = fused["all_cls_scores"][-1][0].cpu(), fused["all_bbox_preds"][-1][0].cpu()
    top = cls.sigmoid().view(-1).topk(MAX_NUM + 1)[0]
    assert top.unique().numel() == top.numel(), "condition: the max_num + 1 largest fp32 scores are pairwise distinct"
    w32 = Y.get_bboxes([Y.decode_single(cls, box, MAX_NUM, 10, S.POST_CENTER_RANGE)])[0]
    w64 = Y.get_bboxes([Y.decode_single(cls.double(), box.double(), MAX_NUM, 10, S.POST_CENTER_RANGE)])[0]
    got = [t.cpu() for t in boxes[0]]
    assert torch.equal(got[2], w32[2]) and got[0].shape == w32[0].shape
    assert torch.equal(got[0][:, [0, 1, 7, 8]], w32[0][:, [0, 1, 7, 8]])          # the selected rows (pass-through columns)
    for i, name in ((0, "bboxes"), (1, "scores")):
        e32 = (w32[i].double() - w64[i]).abs().max().item()
        d = (got[i].double() - w64[i]).abs().max().item()
        print(f"head tiny get_bboxes {name}: E32 {e32:.3e}  got {d:.3e}")
        assert d <= 4 * e32


def _decoder(num_layers, seed=0):
    torch.manual_seed(seed)
    dec = bevformer_amd.build_transformer_layer_sequence(S.reference_decoder_cfg(num_layers)).eval()
    dec.load_state_dict(_trained(dec.state_dict()))
    return dec


def _dec_inputs(reg):
    q, qp, v, ref, shapes, start = S.make_decoder_inputs(12, 10, num_query=37, bs=2, seed=4)
    return dict(query=q, key=None, value=v, query_pos=qp, reference_points=ref, spatial_shapes=shapes, level_start_index=start,
                reg_branches=reg)


def _to(kw, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) or isinstance(v, torch.nn.Module) else v) for k, v in kw.items()}


def test_decoder_refinement_within_three_times_the_parent_error():
    dec = _decoder(2)
    _, reg = Y.make_branches(2, 10, 10, False, seed=7)
    kw = _dec_inputs(reg)
    with torch.no_grad(), oracle_ops():
        want = dec(**kw)
    dec, kwd = dec.to(DEV), _to(kw, DEV)
    with torch.no_grad():
        with ops.using(decoder_fused=True, head_fused=False), _tags() as seen:
            parent = dec(**kwd)
        assert "dec_refine" not in seen
        with ops.using(decoder_fused=True, head_fused=True), _tags() as seen:
            fused = dec(**kwd)
        assert seen.count("dec_refine") == 2
    for i, name in ((0, "states"), (1, "references")):
        e_parent = (parent[i].cpu().double() - want[i].double()).abs().max().item()
        e_fused = (fused[i].cpu().double() - want[i].double()).abs().max().item()
        print(f"\ndecoder 2 layers {name}: E_parent {e_parent:.3e}  fused {e_fused:.3e}  (bound 3 x E_parent = {3 * e_parent:.3e})")
        assert e_fused <= 3 * e_parent, f"{name}: fused error {e_fused:.3e} > 3 x E_parent = {3 * e_parent:.3e}"


def test_a_single_linear_reg_branch_keeps_the_torch_statements():
    dec = _decoder(2).to(DEV)
    kwd = _to(_dec_inputs(_Reg(2)), DEV)
    with torch.no_grad():
        with ops.using(decoder_fused=True, head_fused=False):
            off = dec(**kwd)
        with ops.using(decoder_fused=True, head_fused=True), _tags() as seen:
            on = dec(**kwd)
    assert "dec_refine" not in seen and seen.count("dec_mha") == 2
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
