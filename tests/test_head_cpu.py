"""No GPU: the detection head's modules (``BEVFormerHead``, ``NMSFreeCoder``) and the yardstick they are tested with
(tests/head_yardstick.py), the latter pinned against the reference's own files where those are present."""
import ast
import copy
import sys
import types

import pytest
import torch
import torch.nn as nn

import bevformer_amd
from bevformer_amd import modes, ops
from bevformer_amd import synthetic as S
from bevformer_amd.modules.head import BEVFormerHead, NMSFreeCoder

import head_yardstick as Y
from helpers import oracle_ops

REF = "/root/reference/projects/mmdet3d_plugin"
PCR = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]


def _decode_inputs(nq=37, C=10, code=10, seed=5):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(nq, C, generator=g) * 0.8
    box = torch.randn(nq, code, generator=g) * 0.5
    box[:, 0:2] = torch.randn(nq, 2, generator=g) * 40.0
    return cls, box


# ------------------------------------------------------------------------------------------------ the reference's own files
def _reference_coder_namespace():
    """``nms_free_coder.py`` and ``util.py`` of the reference executed under a test-local stub of the two mmdet names they
    import (``BaseBBoxCoder``, ``BBOX_CODERS``)."""
    class _Reg:
        def register_module(self, *a, **k):
            return lambda cls: cls
    stubs = {"mmdet": types.ModuleType("mmdet"), "mmdet.core": types.ModuleType("mmdet.core"),
             "mmdet.core.bbox": types.ModuleType("mmdet.core.bbox"), "mmdet.core.bbox.builder": types.ModuleType("mmdet.core.bbox.builder"),
             "projects": types.ModuleType("projects"), "projects.mmdet3d_plugin": types.ModuleType("projects.mmdet3d_plugin"),
             "projects.mmdet3d_plugin.core": types.ModuleType("projects.mmdet3d_plugin.core"),
             "projects.mmdet3d_plugin.core.bbox": types.ModuleType("projects.mmdet3d_plugin.core.bbox"),
             "projects.mmdet3d_plugin.core.bbox.util": types.ModuleType("projects.mmdet3d_plugin.core.bbox.util")}
    stubs["mmdet.core.bbox"].BaseBBoxCoder = object
    stubs["mmdet.core.bbox.builder"].BBOX_CODERS = _Reg()
    util = stubs["projects.mmdet3d_plugin.core.bbox.util"]
    exec(compile(open(REF + "/core/bbox/util.py").read(), "<reference util>", "exec"), util.__dict__)
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        ns = {}
        exec(compile(open(REF + "/core/bbox/coders/nms_free_coder.py").read(), "<reference coder>", "exec"), ns)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ns


@pytest.mark.reference
@pytest.mark.parametrize("thr", [None, 0.3, 0.99])
def test_yardstick_decode_equals_the_reference_coder(thr):
    ns = _reference_coder_namespace()
    cls, box = _decode_inputs()
    if thr == 0.3:
        assert (cls.sigmoid() > 0.3).any()
    if thr == 0.99:
        assert not (cls.sigmoid() > 0.99).any()          # the ladder is walked
    ref = ns["NMSFreeCoder"](S.PC_RANGE, post_center_range=list(PCR), max_num=300, score_threshold=thr, num_classes=10)
    want = ref.decode_single(cls.clone(), box.clone())
    got = Y.decode_single(cls, box, 300, 10, PCR, thr)
    ours = NMSFreeCoder(S.PC_RANGE, post_center_range=list(PCR), max_num=300, score_threshold=thr, num_classes=10)
    mine = ours.decode_single(cls.clone(), box.clone())
    for k in ("bboxes", "scores", "labels"):
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(mine[k], want[k]), k
    assert 0 < want["scores"].numel() < 300


def _lifted_head_methods():
    """``_init_layers`` and the ``for lvl`` loop of ``forward`` of the reference's ``BEVFormerHead`` as free functions, lifted
    out of the file with ``ast`` (the class itself needs mmdet's ``DETRHead``)."""
    src = open(REF + "/bevformer/dense_heads/bevformer_head.py").read()
    tree = ast.parse(src)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BEVFormerHead")
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    init = copy.deepcopy(fns["_init_layers"])
    init.decorator_list = []
    loop = next(n for n in fns["forward"].body if isinstance(n, ast.For))
    stacks = [n for n in fns["forward"].body if n.lineno > loop.lineno and isinstance(n, ast.Assign)
              and getattr(n.targets[0], "id", "") in ("outputs_classes", "outputs_coords")]
    assert len(stacks) == 2
    fwd = ast.parse("def head_loop(self, hs, init_reference, inter_references):\n    outputs_classes = []\n"
                    "    outputs_coords = []\n    return outputs_classes, outputs_coords").body[0]
    fwd.body = fwd.body[:2] + [loop] + stacks + fwd.body[2:]
    mod = ast.fix_missing_locations(ast.Module(body=[init, fwd], type_ignores=[]))
    from bevformer_amd.modules.decoder import inverse_sigmoid
    ns = {"torch": torch, "nn": nn, "copy": copy, "Linear": nn.Linear, "inverse_sigmoid": inverse_sigmoid}
    exec(compile(mod, "<reference head>", "exec"), ns)
    return ns["_init_layers"], ns["head_loop"]


@pytest.mark.reference
@pytest.mark.parametrize("refine", [True, False])
def test_yardstick_head_equals_the_reference_head_code(refine):
    init_layers, head_loop = _lifted_head_methods()
    stub = nn.Module()
    stub.num_reg_fcs, stub.embed_dims, stub.cls_out_channels, stub.code_size = 2, 256, 10, 10
    stub.as_two_stage, stub.with_box_refine, stub.bev_h, stub.bev_w, stub.num_query = False, refine, 4, 4, 13
    stub.transformer = types.SimpleNamespace(decoder=types.SimpleNamespace(num_layers=3))
    stub.pc_range = S.PC_RANGE
    torch.manual_seed(0)
    init_layers(stub)
    Y.trained_like_head_(stub, seed=2)
    assert (stub.cls_branches[0] is stub.cls_branches[1]) == (not refine)
    g = torch.Generator().manual_seed(1)
    hs = torch.randn(3, 13, 2, 256, generator=g)
    init_ref = torch.rand(2, 13, 3, generator=g)
    inter = torch.rand(3, 2, 13, 3, generator=g)
    with torch.no_grad():
        want = head_loop(stub, hs.permute(0, 2, 1, 3), init_ref, inter)
        refs = torch.cat([init_ref[None], inter[:-1]], 0)
        got = Y.head_outputs(hs, refs, [Y.branch_params(b, torch.float32) for b in stub.cls_branches],
                             [Y.branch_params(b, torch.float32) for b in stub.reg_branches], S.PC_RANGE)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the product's head builds the same layers under the same keys
    head = _head(refine, layers=3)
    mine = {k: tuple(v.shape) for k, v in head.state_dict().items() if k.startswith(("cls_branches", "reg_branches"))}
    theirs = {k: tuple(v.shape) for k, v in stub.state_dict().items() if k.startswith(("cls_branches", "reg_branches"))}
    assert mine == theirs


# ------------------------------------------------------------------------------------------------ the product's modules
def _head(refine=True, layers=2, nq=13, max_num=20, **kw):
    torch.manual_seed(0)
    head = bevformer_amd.build_head(S.head_cfg("micro", num_query=nq, decoder_layers=layers, max_num=max_num,
                                               with_box_refine=refine, **kw)).eval()
    head.init_weights()
    Y.trained_like_head_(head.cls_branches, 4)
    Y.trained_like_head_(head.reg_branches, 5)
    return head


@pytest.mark.parametrize("refine", [True, False])
def test_state_dict_keys_and_shapes(refine):
    head = _head(refine)
    sd = head.state_dict()
    own = {k for k in sd if not k.startswith("transformer.")}
    want = {"bev_embedding.weight", "query_embedding.weight", "code_weights", "positional_encoding.row_embed.weight",
            "positional_encoding.col_embed.weight"}
    for l in range(2):
        want |= {f"cls_branches.{l}.{i}.{p}" for i in (0, 1, 3, 4, 6) for p in ("weight", "bias")}
        want |= {f"reg_branches.{l}.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")}
    assert own == want
    assert any(k.startswith("transformer.decoder.") for k in sd) and any(k.startswith("transformer.encoder.") for k in sd)
    assert tuple(sd["cls_branches.1.6.weight"].shape) == (10, 256) and tuple(sd["reg_branches.0.4.weight"].shape) == (10, 256)
    assert tuple(sd["cls_branches.0.1.weight"].shape) == (256,) and tuple(sd["bev_embedding.weight"].shape) == (120, 256)
    assert tuple(sd["query_embedding.weight"].shape) == (13, 512) and tuple(sd["code_weights"].shape) == (10,)
    assert tuple(sd["positional_encoding.row_embed.weight"].shape) == (12, 128)
    assert not head.code_weights.requires_grad


def test_branches_are_cloned_with_box_refine_and_shared_without():
    cloned, shared = _head(True), _head(False)
    assert cloned.cls_branches[0] is not cloned.cls_branches[1] and cloned.reg_branches[0] is not cloned.reg_branches[1]
    assert shared.cls_branches[0] is shared.cls_branches[1] and shared.reg_branches[0] is shared.reg_branches[1]


def test_init_weights_sets_the_cls_bias_to_the_prior():
    torch.manual_seed(0)
    head = bevformer_amd.build_head(S.head_cfg("micro", num_query=13, decoder_layers=2, max_num=20))
    head.init_weights()
    for b in head.cls_branches:
        assert torch.allclose(b[-1].bias, torch.full((10,), -4.59511985013459))


def test_as_two_stage_raises_and_loss_names_mmdet():
    cfg = S.head_cfg("micro", num_query=13, decoder_layers=2, max_num=20)
    cfg["as_two_stage"] = True
    with pytest.raises(NotImplementedError):
        bevformer_amd.build_head(cfg)
    with pytest.raises(NotImplementedError, match="mmdet"):
        _head().loss()


def test_head_fused_is_a_mode():
    assert "head_fused" in modes.Modes.__slots__ and modes.process_defaults().head_fused is False
    with ops.using(head_fused=True) as m:
        assert m.head_fused and ops.modes().head_fused
    assert not ops.modes().head_fused


@pytest.mark.parametrize("refine", [True, False])
def test_module_path_equals_the_yardstick_on_the_cpu(refine):
    head = _head(refine)
    mlvl, _, kw = S.make_transformer_inputs("micro", seed=0, bs=1, temporal=True)
    seen = {}
    real = head.predictions

    def spy(hs, init_reference, inter_references):
        seen["args"] = (hs, init_reference, inter_references)
        return real(hs, init_reference, inter_references)
    head.predictions = spy
    with torch.no_grad(), oracle_ops():
        out = head(mlvl, kw["img_metas"], prev_bev=kw["prev_bev"])
        boxes = head.get_bboxes({k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}, kw["img_metas"])
    hs, init_ref, inter = seen["args"]
    refs = torch.cat([init_ref[None], inter[:-1]], 0)
    cls, box = Y.head_outputs(hs, refs, [Y.branch_params(b, torch.float32) for b in head.cls_branches],
                              [Y.branch_params(b, torch.float32) for b in head.reg_branches], S.PC_RANGE)
    assert set(out) == {"bev_embed", "all_cls_scores", "all_bbox_preds", "enc_cls_scores", "enc_bbox_preds"}
    assert out["enc_cls_scores"] is None and out["enc_bbox_preds"] is None
    assert torch.equal(out["all_cls_scores"], cls) and torch.equal(out["all_bbox_preds"], box)
    want = Y.get_bboxes([Y.decode_single(cls[-1][0], box[-1][0], 20, 10, S.POST_CENTER_RANGE)])
    for a, b in zip(boxes[0], want[0]):
        assert torch.equal(a, b)
    assert tuple(boxes[0][0].shape[1:]) == (9,)

    class Box:
        def __init__(self, t, box_dim):
            self.tensor, self.box_dim = t, box_dim
    metas = [dict(kw["img_metas"][0], box_type_3d=Box)]
    with torch.no_grad():
        wrapped = head.get_bboxes({k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}, metas)
    assert isinstance(wrapped[0][0], Box) and wrapped[0][0].box_dim == 9 and torch.equal(wrapped[0][0].tensor, want[0][0])


def test_only_bev_returns_the_bev():
    head = _head()
    mlvl, _, kw = S.make_transformer_inputs("micro", seed=0, bs=1, temporal=True)
    with torch.no_grad(), oracle_ops():
        bev = head(mlvl, kw["img_metas"], prev_bev=kw["prev_bev"], only_bev=True)
    assert tuple(bev.shape) == (1, 120, 256)


def test_stock_shape_predicate():
    cls, reg = Y.make_branches(1, 10, 10, True)
    assert ops.head_branch_reject(cls[0], "cls") is None and ops.head_branch_reject(reg[0], "reg") is None
    no_norm = nn.Sequential(*[m for i, m in enumerate(cls[0]) if i != 1])
    assert ops.head_branch_reject(no_norm, "cls") is not None
    no_affine = copy.deepcopy(cls[0])
    no_affine[4] = nn.LayerNorm(256, elementwise_affine=False)
    assert ops.head_branch_reject(no_affine, "cls") is not None
    wide = nn.Sequential(nn.Linear(256, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 10))
    assert ops.head_branch_reject(wide, "reg") is not None
    assert ops.head_branch_reject(Y.make_branches(1, 10, 33, True)[0][0], "cls") is not None
    assert ops.head_branch_reject(Y.make_branches(1, 7, 10, True)[1][0], "reg") is not None
    assert ops.head_branch_reject(Y.make_branches(1, 8, 1, True)[1][0], "reg") is None
    assert ops.head_branch_reject(nn.Linear(256, 10), "reg") is not None       # the decoder tests' one-Linear stand-in
    assert ops.head_branch_reject(reg[0], "cls") is not None


def test_cpu_calls_are_not_covered_and_the_ladder_is_the_references():
    cls, reg = Y.make_branches(1, 10, 10, True)
    hs, refs = torch.randn(1, 5, 1, 256), torch.rand(1, 1, 5, 3)
    with torch.no_grad():
        assert ops.head_branches(hs, refs, cls, reg, S.PC_RANGE) is None
        assert ops.reg_refine(hs[0], refs[0], reg[0]) is None
        assert ops.nms_free_decode(torch.randn(1, 5, 3), torch.randn(1, 5, 10), max_num=15, post_center_range=PCR,
                                   num_classes=3) is None
    assert ops.threshold_ladder(None) == [] and ops.threshold_ladder(0.0) == []
    lad, t = ops.threshold_ladder(0.3), 0.3
    assert lad[0] == 0.3
    for v in lad[1:]:
        t *= 0.9
        assert v == t and v >= 0.01
    assert t * 0.9 < 0.01
