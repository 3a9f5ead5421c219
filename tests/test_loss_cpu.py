"""No GPU: the module path of ``BEVFormerHead.loss`` (modules/loss.py; plain torch + scipy, the default) against the
yardstick (tests/loss_yardstick.py), its registries, special inputs and error paths."""
import importlib.util
import os

import pytest
import torch

import bevformer_amd
from bevformer_amd import modes, registry, synthetic as S
from bevformer_amd.modules import loss as ML

import loss_yardstick as Y

REF_UTIL = "/root/reference/projects/mmdet3d_plugin/core/bbox/util.py"


def _head(L=2, nq=13, code_size=10, **kw):
    cfg = S.head_cfg("micro", num_query=nq, decoder_layers=L, max_num=20, code_size=code_size, train=True, **kw)
    if code_size == 8:
        cfg["code_weights"] = [1.0] * 8
    torch.manual_seed(0)
    return bevformer_amd.build_head(cfg)


@pytest.fixture(scope="module")
def case():
    head = _head()
    cls, box = Y.make_preds(5, 2, 2, 13)
    gts, labels = S.make_gt(11, (3, 0))
    return head, cls, box, gts, labels


def _module_run(head, cls, box, gts, labels):
    c, b = cls.clone().requires_grad_(True), box.clone().requires_grad_(True)
    d = head.loss(gts, labels, {"all_cls_scores": c, "all_bbox_preds": b, "enc_cls_scores": None, "enc_bbox_preds": None})
    sum(d.values()).backward()
    return d, c.grad, b.grad


@pytest.mark.reference
@pytest.mark.parametrize("width", [7, 9])
def test_normalize_bbox_is_the_reference(width):
    """Bit-exact against the reference's own core/bbox/util.py (it imports only torch): the same torch statements."""
    if not os.path.exists(REF_UTIL):
        pytest.skip("reference tree not present")
    spec = importlib.util.spec_from_file_location("_ref_bbox_util", REF_UTIL)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    gts, _ = S.make_gt(3, (17,), code_size=width + 1)
    want = ref.normalize_bbox(gts[0], S.PC_RANGE)
    got = ML.normalize_bbox(gts[0], S.PC_RANGE)
    assert got.shape == (17, width + 1) and torch.equal(got, want)
    assert torch.equal(Y.normalize_bbox(gts[0]), want)


def test_module_path_matches_the_yardstick(case):
    """L = 2, bs = 2, nq = 13, 10 classes, gt counts (3, 0).  Assignments identical; losses and autograd gradients against the
    float64 yardstick on the same float32 inputs.  Tolerance: the module path is the yardstick's statements in fp32, so its
    error is held to TWICE the error of the yardstick run in fp32 against itself in fp64, measured here in the max norm per
    quantity.  Measured (this fixture): losses 7.2e-06 (loss_cls is a few hundred here), grad cls 3.3e-07, grad box 2.5e-09; the module
    path's own errors were the same three numbers (it is bit-equal to the yardstick in fp32)."""
    head, cls, box, gts, labels = case
    cw = head.code_weights.detach().tolist()
    y64 = Y.loss_with_grads(cls, box, gts, labels, cw, dtype=torch.float64)
    y32 = Y.loss_with_grads(cls, box, gts, labels, cw, dtype=torch.float32)
    d, gc, gb = _module_run(head, cls, box, gts, labels)
    # assignments: the module's assigner on the same inputs
    for l in range(2):
        for b in range(2):
            r = head.assigner.assign(box[l, b], cls[l, b], gts[b], labels[b])
            assert torch.equal(r.gt_inds, y64[3][l][b]), (l, b)
            assert r.num_gts == gts[b].shape[0]
            pos = r.gt_inds > 0
            assert torch.equal(r.labels[pos], labels[b][r.gt_inds[pos] - 1]) and (r.labels[~pos] == -1).all()
    assert all(torch.equal(a, b) for la, lb in zip(y32[3], y64[3]) for a, b in zip(la, lb))
    # (with sync_cls_avg_factor the reference's loss_cls is a one-element tensor: reduce_mean returns one)
    got = torch.stack([d[k].detach().reshape(()) for k in ("d0.loss_cls", "d0.loss_bbox", "loss_cls", "loss_bbox")]).view(2, 2)
    for name, m, a32, a64 in (("losses", got, y32[0], y64[0]), ("grad cls", gc, y32[1], y64[1]), ("grad box", gb, y32[2], y64[2])):
        own = (a32.double() - a64).abs().max().item()
        err = (m.double() - a64).abs().max().item()
        print(f"{name}: yardstick fp32 vs fp64 {own:.3e}, module vs fp64 {err:.3e}")
        assert err <= 2 * own, (name, err, own)
    assert y64[0][:, 1].min() > 0 and gb.abs().sum() > 0            # (the fixture has positives: the box loss is live)


def test_dict_keys_are_the_references():
    head = _head(L=3)
    cls, box = Y.make_preds(6, 3, 1, 13)
    gts, labels = S.make_gt(12, (4,))
    d = head.loss(gts, labels, {"all_cls_scores": cls, "all_bbox_preds": box, "enc_cls_scores": None, "enc_bbox_preds": None})
    assert list(d) == ["loss_cls", "loss_bbox", "d0.loss_cls", "d0.loss_bbox", "d1.loss_cls", "d1.loss_bbox"]
    assert all(v.numel() == 1 and torch.isfinite(v).all() for v in d.values())


def test_no_gt_anywhere_gives_finite_losses_and_a_zero_box_loss(case):
    head, cls, box, _, _ = case
    gts, labels = S.make_gt(1, (0, 0))
    d, gc, gb = _module_run(head, cls, box, gts, labels)
    assert all(torch.isfinite(v) for v in d.values())
    assert d["loss_bbox"].item() == 0.0 and d["d0.loss_bbox"].item() == 0.0 and d["loss_cls"].item() > 0
    assert torch.isfinite(gc).all() and gb.abs().max().item() == 0.0
    r = head.assigner.assign(box[0, 0], cls[0, 0], gts[0], labels[0])
    assert r.num_gts == 0 and (r.gt_inds == 0).all() and (r.labels == -1).all()


class _AssignOn:
    """An assigner that matches against other boxes than the loss sees (the same gt before it was damaged)."""

    def __init__(self, inner, boxes):
        self.inner, self.boxes = inner, boxes

    def assign(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        boxes = next(b for b in self.boxes if b.shape == gt_bboxes.shape and torch.equal(b[:, :3], gt_bboxes[:, :3]))
        return self.inner.assign(bbox_pred, cls_pred, boxes, gt_labels, gt_bboxes_ignore)


def test_a_zero_width_gt_is_dropped_from_the_box_loss(case):
    """log(0) = -inf in the normalised target: the row leaves ``loss_bbox`` (bevformer_head.py:378-385) and nothing becomes
    NaN.  The assignment is made on the undamaged boxes: through the assigner the same gt has an infinite cost against
    every query (the width is one of the eight matched columns) and scipy raises 'infeasible', as it does in the reference."""
    head, cls, box, _, _ = case
    good, labels = S.make_gt(2, (2, 1))
    gts = [g.clone() for g in good]
    gts[0][1, 3] = 0.0
    with pytest.raises(ValueError):
        head.assigner.assign(box[0, 0], cls[0, 0], gts[0], labels[0])
    inner = head.assigner
    head.assigner = _AssignOn(inner, good)
    try:
        d, gc, gb = _module_run(head, cls, box, gts, labels)
        full, _, gb_full = _module_run(head, cls, box, good, labels)
    finally:
        head.assigner = inner
    assert all(torch.isfinite(v).all() for v in d.values()) and torch.isfinite(gb).all() and torch.isfinite(gc).all()
    for l in range(2):      # three positives per layer; the one on the damaged gt has no box gradient
        assert (gb_full[l].abs().sum(-1) > 0).sum().item() == 3 and (gb[l].abs().sum(-1) > 0).sum().item() == 2
    assert d["loss_bbox"].item() < full["loss_bbox"].item()
    inds = [[inner.assign(box[l, b], cls[l, b], good[b], labels[b]).gt_inds for b in range(2)] for l in range(2)]
    y = Y.loss_with_grads(cls, box, gts, labels, head.code_weights.tolist(), gt_inds=inds, dtype=torch.float64)
    torch.testing.assert_close(d["loss_bbox"].double().reshape(()), y[0][-1, 1], rtol=1e-5, atol=1e-7)


def test_a_nan_velocity_gt_is_dropped_through_the_whole_path(case):
    """The case the reference's ``isnotnan`` exists for: the velocity columns are outside the eight matched ones, so the
    assigner is unaffected and the row is dropped from the box loss."""
    head, cls, box, _, _ = case
    gts, labels = S.make_gt(2, (2, 1))
    gts[0][1, 7] = float("nan")
    d, gc, gb = _module_run(head, cls, box, gts, labels)
    assert all(torch.isfinite(v).all() for v in d.values()) and torch.isfinite(gb).all() and torch.isfinite(gc).all()
    assert all((gb[l].abs().sum(-1) > 0).sum().item() == 2 for l in range(2))
    y = Y.loss_with_grads(cls, box, gts, labels, head.code_weights.tolist(), dtype=torch.float64)
    torch.testing.assert_close(d["loss_bbox"].double().reshape(()), y[0][-1, 1], rtol=1e-5, atol=1e-7)


def test_reference_blocks_build_through_the_registries():
    for reg, names in ((registry.BBOX_ASSIGNERS, ["HungarianAssigner3D"]), (registry.MATCH_COST, ["BBox3DL1Cost", "FocalLossCost"]),
                       (registry.LOSSES, ["FocalLoss", "L1Loss"])):
        for n in names:
            assert registry.HAVE_MMDET or reg.get(n) is getattr(ML, n)
    cfg = S.head_cfg("micro", num_query=13, decoder_layers=2, max_num=20, train=True)
    a = registry.build_assigner(cfg["train_cfg"]["assigner"])
    assert a.cls_cost.weight == 2.0 and a.reg_cost.weight == 0.25 and a.pc_range == S.PC_RANGE
    assert a.cls_cost.alpha == 0.25 and a.cls_cost.gamma == 2 and a.cls_cost.eps == 1e-12
    f, l1 = registry.build_loss(cfg["loss_cls"]), registry.build_loss(cfg["loss_bbox"])
    assert (f.gamma, f.alpha, f.loss_weight, l1.loss_weight) == (2.0, 0.25, 2.0, 0.25)
    head = bevformer_amd.build_head(cfg)
    assert head.assigner is not None and head.bg_cls_weight == 0
    assert isinstance(head.loss_cls, dict) and isinstance(head.loss_bbox, dict) and head.loss_cls["type"] == "FocalLoss"
    assert not [k for k in head.state_dict() if "loss" in k or "assigner" in k]


def test_error_paths():
    plain = bevformer_amd.build_head(S.head_cfg("micro", num_query=13, decoder_layers=2, max_num=20))
    assert plain.assigner is None
    with pytest.raises(NotImplementedError, match="mmdet"):
        plain.loss()
    for key, typ in (("loss_cls", "CrossEntropyLoss"), ("loss_bbox", "SmoothL1Loss")):
        cfg = S.head_cfg("micro", num_query=13, decoder_layers=2, max_num=20, train=True)
        cfg[key] = dict(cfg[key], type=typ)
        with pytest.raises(NotImplementedError, match=typ):
            bevformer_amd.build_head(cfg)
    cfg = S.head_cfg("micro", num_query=13, decoder_layers=2, max_num=20, train=True)
    cfg["as_two_stage"] = True
    with pytest.raises(NotImplementedError):
        bevformer_amd.build_head(cfg)


def test_a_non_finite_cost_propagates_scipys_error(case):
    head, cls, box, gts, labels = case
    bad = box.clone()
    bad[0, 0, 3, 0] = float("nan")
    with pytest.raises(ValueError):
        head.assigner.assign(bad[0, 0], cls[0, 0], gts[0], labels[0])


def test_loss_fused_is_a_mode_and_off_by_default(case):
    head = case[0]
    assert "loss_fused" in modes.Modes.__slots__ and modes.process_defaults().loss_fused is False
    with modes.using(loss_fused=True) as m:
        assert m.loss_fused is True
    cls, box = case[1], case[2]
    assert head.loss_fused_reject() is None
    assert head.loss_fused_reject({"all_cls_scores": cls, "all_bbox_preds": box}) == "not CUDA fp32 predictions"


def test_synthetic_gt_is_well_formed():
    gts, labels = S.make_gt(4, (5, 0, 2))
    assert [g.shape for g in gts] == [(5, 9), (0, 9), (2, 9)] and [l.shape for l in labels] == [(5,), (0,), (2,)]
    lo, hi = torch.tensor(S.PC_RANGE[:3]), torch.tensor(S.PC_RANGE[3:])
    for g, l in zip(gts, labels):
        assert (g[:, :3] >= lo).all() and (g[:, :3] <= hi).all() and (g[:, 3:6] > 0).all()
        assert l.dtype == torch.int64 and ((l >= 0) & (l < 10)).all()
    assert S.make_gt(4, (3,), code_size=8)[0][0].shape == (3, 7)
