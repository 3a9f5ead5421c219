"""GPU: the grouped (Group-DETR) detection loss — ``ops.match_cost`` / ``ops.det_loss`` / ``ops.detection_loss`` with
``groups``, ``BEVFormerHead_GroupDETR.loss`` under ``loss_fused`` and the head's inference fast paths — against the float64
yardstick (tests/loss_yardstick.py) on the same float32 inputs.  For G groups of n queries the yardstick is the mean over g
of ``Y.loss_with_grads`` on the contiguous slice ``[:, :, g n:(g + 1) n]``.

Bounds (tests/test_loss_fused_gpu.py has the one-group forms).  A cost or a unit gradient is ONE rounding of an fp64 value:
``|k - y| <= 2^-24 |y| + 1e-12`` (the 1 / G of the gradients is in the fp64 factor).  A group's fp32 loss is within 2^-23 of
its yardstick; a mean of non-negative terms keeps that relative bound, and the mean's own rounding adds 2^-24:
``2^-22 |y| + 1e-12`` covers both.  An assignment is judged by optimality on the kernel's own fp32 matrix."""
import functools

import pytest
import torch

import bevformer_amd
from bevformer_amd import ops, synthetic as S

import loss_yardstick as Y
from test_decoder_cpu import _trained
from test_loss_fused_gpu import _assert_bound, _check_optimal, _fixture_is_robust

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
# (G, n) -> (gt counts, L, bs).  n = 37: a group boundary inside a wavefront and off a multiple of 64, a sample without gt;
# n = 300: more than one 256-wide pass; (11, 900): the shipped bevformerv2 shape
CASES = {(3, 37): ((5, 0), 2, 2), (2, 300): ((40, 17), 2, 2), (11, 900): ((40,), 6, 1)}
SMALL = [(3, 37), (2, 300)]
CW = Y.CODE_WEIGHTS


@functools.lru_cache(maxsize=None)
def _case(G, n):
    counts, L, bs = CASES[(G, n)]
    cls, box = Y.make_preds(100 + n + G, L, bs, G * n, 10, 10, logit_scale=1.5, extremes=False)
    gts, labels = S.make_gt(200 + n + G, counts)
    return cls, box, gts, labels


def _slice(t, g, n):
    return t[:, :, g * n:(g + 1) * n].contiguous()


def _assert_fixture_is_robust(G, n):
    """Per group, as tests/test_loss_fused_gpu.py asks of its fixture: the fp32 and fp64 yardstick costs assign identically and
    the assignment survives 16 relative cost perturbations of 1e-5 — a fragile fixture fails here, as a fixture."""
    cls, box, gts, labels = _case(G, n)
    for g in range(G):
        c, b = _slice(cls, g, n), _slice(box, g, n)
        assert _fixture_is_robust(c, b, gts, labels), f"fixture: group {g}'s assignment is not stable under 1e-5 cost perturbations"
        y32 = Y.loss_with_grads(c, b, gts, labels, CW, dtype=torch.float32)[3]
        y64 = Y.loss_with_grads(c, b, gts, labels, CW, dtype=torch.float64)[3]
        assert all(torch.equal(a, b_) for la, lb in zip(y32, y64) for a, b_ in zip(la, lb)), \
            f"fixture: group {g}'s fp32 and fp64 costs assign differently"


def _yardstick(cls, box, gts, labels, G, inds=None, factors=None, cw=CW):
    """The mean over the groups of the float64 yardstick -> (losses (L, 2), grad cls, grad box, [g][l][b] gt_inds)."""
    n = cls.shape[2] // G
    per = [Y.loss_with_grads(_slice(cls, g, n), _slice(box, g, n), gts, labels, cw, gt_inds=None if inds is None else inds[g],
                             factors=factors) for g in range(G)]
    return (torch.stack([p[0] for p in per]).sum(0) / G, torch.cat([p[1] for p in per], 2) / G,
            torch.cat([p[2] for p in per], 2) / G, [p[3] for p in per])


def _inds_from(assigned, G):
    """``assigned`` (L, bs, G n) int32, -1 background -> [g][l][b] 1-based gt_inds of the yardstick."""
    L, bs, nq = assigned.shape
    n = nq // G
    a = assigned.cpu().long() + 1
    return [[[a[l, b, g * n:(g + 1) * n].clone() for b in range(bs)] for l in range(L)] for g in range(G)]


def _count_rep(count, L, G):
    return count.repeat_interleave(G).repeat(L)


_KERNEL = {}


def _kernel_run(G, n):
    """The three grouped kernels on the shared case, once: packed gt, cost (L, bs, G, Gmax, n) on the CPU (written over a
    sentinel), (match, assigned, status) and the loss triple + group losses with the kernel's own assignment."""
    if (G, n) not in _KERNEL:
        cls, box, gts, labels = _case(G, n)
        counts, L, bs = CASES[(G, n)]
        gt, label, count = ops.pack_gt(gts, labels, DEV)
        out = torch.full((L, bs, G, gt.shape[1], n), SENTINEL, dtype=torch.float32, device=DEV)
        cost = ops.match_cost(cls.to(DEV), box.to(DEV), gt, label, count, out=out, groups=G)
        assert cost.data_ptr() == out.data_ptr()
        match, assigned, status = ops.lsap(cost, _count_rep(count, L, G))
        factors = ops.loss_factors(count, n, bs)
        cw = torch.tensor(CW, dtype=torch.float32, device=DEV)
        loss = ops.det_loss(cls.to(DEV), box.to(DEV), gt, label, count, assigned, cw, factors, groups=G, return_group_losses=True)
        _KERNEL[(G, n)] = dict(packed=(gt, label, count), cost=cost.cpu(), match=match.cpu(), assigned=assigned.cpu(),
                               status=status.cpu(), loss=[t.cpu() for t in loss], factors=tuple(factors.cpu().tolist()))
    return _KERNEL[(G, n)]


# ---- 1, 2: costs

@pytest.mark.parametrize("G,n", SMALL)
def test_grouped_costs_are_one_rounding_of_the_fp64_yardstick(G, n):
    cls, box, gts, labels = _case(G, n)
    counts, L, bs = CASES[(G, n)]
    cost = _kernel_run(G, n)["cost"]
    c64, b64 = cls.double(), box.double()
    for l in range(L):
        for b in range(bs):
            k = gts[b].shape[0]
            for g in range(G):
                rows = slice(g * n, (g + 1) * n)
                if k:
                    want = Y.cost_matrix(b64[l, b, rows], c64[l, b, rows], gts[b].double(), labels[b]).t()
                    _assert_bound(f"cost[{l}, {b}, {g}]", cost[l, b, g, :k], want, 2.0 ** -24)
                assert (cost[l, b, g, k:] == SENTINEL).all(), "a padded gt row was written"


@pytest.mark.parametrize("G,n", SMALL)
def test_a_groups_costs_are_bit_equal_to_the_one_group_kernel_on_its_slice(G, n):
    cls, box, _, _ = _case(G, n)
    run = _kernel_run(G, n)
    gt, label, count = run["packed"]
    for g in range(G):
        out = torch.full(run["cost"][:, :, g].shape, SENTINEL, dtype=torch.float32, device=DEV)
        alone = ops.match_cost(_slice(cls, g, n).to(DEV), _slice(box, g, n).to(DEV), gt, label, count, out=out)
        assert torch.equal(alone.cpu(), run["cost"][:, :, g]), g


@pytest.mark.parametrize("n", [37, 300])
def test_one_group_through_the_grouped_entry_points_is_bit_equal_to_the_existing_ones(n):
    G0 = {37: 3, 300: 2}[n]
    cls, box, gts, labels = _case(G0, n)
    cls, box = _slice(cls, 1, n).to(DEV), _slice(box, 1, n).to(DEV)
    gt, label, count = ops.pack_gt(gts, labels, DEV)
    L, bs = cls.shape[:2]
    old_cost = ops.match_cost(cls, box, gt, label, count, out=torch.full((L, bs, gt.shape[1], n), SENTINEL, device=DEV))
    new_cost = ops.match_cost(cls, box, gt, label, count, out=torch.full((L, bs, 1, gt.shape[1], n), SENTINEL, device=DEV),
                              grouped_entry=True)
    assert tuple(new_cost.shape) == (L, bs, 1, gt.shape[1], n) and torch.equal(new_cost[:, :, 0], old_cost)
    old_match = ops.lsap(old_cost, count.repeat(L))
    new_match = ops.lsap(new_cost, _count_rep(count, L, 1))
    assert all(torch.equal(a, b) for a, b in zip(old_match, new_match)) and (old_match[1] >= 0).any()
    cw = torch.tensor(CW, dtype=torch.float32, device=DEV)
    factors = ops.loss_factors(count, n, bs)
    old = ops.det_loss(cls, box, gt, label, count, old_match[1], cw, factors)
    new = ops.det_loss(cls, box, gt, label, count, new_match[1], cw, factors, grouped_entry=True, return_group_losses=True)
    for name, a, b in zip(("losses", "grad_cls", "grad_box"), old, new):
        assert torch.equal(a, b), name
    assert torch.equal(new[3][:, 0], old[0])
    assert old[2].abs().sum() > 0


# ---- 3: the assignment

@pytest.mark.parametrize("G,n", SMALL)
def test_every_groups_assignment_is_optimal_and_lines_up_with_the_prediction_rows(G, n):
    _, _, gts, _ = _case(G, n)
    counts, L, bs = CASES[(G, n)]
    run = _kernel_run(G, n)
    assert run["status"].tolist() == [0] * (L * bs * G)
    assigned = run["assigned"].view(L, bs, G * n)
    for l in range(L):
        for b in range(bs):
            k = gts[b].shape[0]
            for g in range(G):
                p = (l * bs + b) * G + g
                _check_optimal(run["cost"][l, b, g, :k].numpy(), run["match"][p], run["assigned"][p], f"problem ({l}, {b}, {g})")
                # (L, bs, G n) in the predictions' own row order: query g n + q holds the gt whose match is q
                for i in range(k):
                    assert assigned[l, b, g * n + run["match"][p, i]] == i
                assert (assigned[l, b, g * n:(g + 1) * n] >= 0).sum().item() == k


# ---- 4: loss and gradients

def _assert_loss_bounds(got, y):
    _assert_bound("losses", got[0], y[0], 2.0 ** -22)
    _assert_bound("grad_cls", got[1], y[1], 2.0 ** -24)
    _assert_bound("grad_box", got[2], y[2], 2.0 ** -24)


@pytest.mark.parametrize("G,n", SMALL)
def test_grouped_loss_and_gradients_against_the_fp64_yardstick(G, n):
    """The kernel's own assignment is handed to the yardstick.  (3, 37) has a sample without gt."""
    cls, box, gts, labels = _case(G, n)
    run = _kernel_run(G, n)
    L, bs = cls.shape[:2]
    inds = _inds_from(run["assigned"].view(L, bs, G * n), G)
    y = _yardstick(cls, box, gts, labels, G, inds=inds, factors=run["factors"])
    losses, gc, gb, group_losses = run["loss"]
    _assert_loss_bounds((losses, gc, gb), y)
    assert gb.abs().sum() > 0 and (losses > 0).all()
    # a group's pair is the one-group bound's; the layer's value is the fp64 mean of the fp32 pairs in group order, rounded once
    for g in range(G):
        yg = Y.loss_with_grads(_slice(cls, g, n), _slice(box, g, n), gts, labels, CW, gt_inds=inds[g], factors=run["factors"])[0]
        _assert_bound(f"group {g} losses", group_losses[:, g], yg, 2.0 ** -23)
    mean = torch.zeros(L, 2, dtype=torch.float64)
    for g in range(G):
        mean += group_losses[:, g].double()
    assert torch.equal(losses, (mean / G).float())


def test_grouped_loss_drops_a_zero_width_gt_matched_in_one_group():
    """gt 2 of sample 0 has zero width (log 0: its normalised target is not finite).  It stays matched in group 1 only — the
    other groups' queries that held it are background — so one group's box loss drops a positive and the others do not see it."""
    G, n = 3, 37
    cls, box, good, labels = _case(G, n)
    run = _kernel_run(G, n)
    gts = [g.clone() for g in good]
    gts[0][2, 3] = 0.0
    assigned = run["assigned"].view(2, 2, G * n).clone()
    for g in (0, 2):
        block = assigned[:, 0, g * n:(g + 1) * n]
        block[block == 2] = -1
    gt, label, count = ops.pack_gt(gts, labels, DEV)
    cw = torch.tensor(CW, dtype=torch.float32, device=DEV)
    factors = torch.tensor([5.0, 5.0], device=DEV)
    args = (cls.to(DEV), box.to(DEV), gt, label, count, assigned.to(DEV), cw, factors)
    got = [t.cpu() for t in ops.det_loss(*args, groups=G)]
    again = [t.cpu() for t in ops.det_loss(*args, groups=G)]
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs are not bit-equal"
    y = _yardstick(cls, box, gts, labels, G, inds=_inds_from(assigned, G), factors=(5.0, 5.0))
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all()
    _assert_loss_bounds(got, y)
    for l in range(2):
        live = (got[2][l, 0].abs().sum(-1) > 0).view(G, n).sum(-1).tolist()
        assert live == [4, 4, 4], live           # five gt: groups 0 and 2 lost the match, group 1 dropped the row


# ---- 5: the head

@pytest.mark.parametrize("G,n", SMALL)
def test_group_detr_head_loss_fused_matches_the_module_path(G, n):
    cls, box, gts, labels = _case(G, n)
    counts, L, bs = CASES[(G, n)]
    _assert_fixture_is_robust(G, n)
    torch.manual_seed(0)
    head = bevformer_amd.build_head(S.head_cfg("micro", num_query=n, decoder_layers=L, max_num=20, train=True, group_detr=G)).to(DEV)
    dgts, dlabels = [g.to(DEV) for g in gts], [x.to(DEV) for x in labels]

    def run(fused):
        c, b = cls.to(DEV).requires_grad_(True), box.to(DEV).requires_grad_(True)
        with ops.using(loss_fused=fused):
            d = head.loss(dgts, dlabels, {"all_cls_scores": c, "all_bbox_preds": b, "enc_cls_scores": None, "enc_bbox_preds": None})
        sum(v.sum() for v in d.values()).backward()
        return d, c.grad.cpu(), b.grad.cpu()

    assert head.loss_fused_reject({"all_cls_scores": cls.to(DEV), "all_bbox_preds": box.to(DEV)}, dgts) is None
    calls = []
    real = ops.detection_loss_head
    ops.detection_loss_head = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        fd, fgc, fgb = run(True)
        md, mgc, mgb = run(False)
    finally:
        ops.detection_loss_head = real
    assert calls == [1], "the fused path ran exactly under the switch"
    assert list(fd) == list(md) == ["loss_cls", "loss_bbox", "d0.loss_cls", "d0.loss_bbox"]
    _, assigned, status = ops.detection_loss_head(head, cls.to(DEV), box.to(DEV), dgts, dlabels, return_assigned=True)
    assert tuple(assigned.shape) == (L, bs, G * n) and status.cpu().tolist() == [0] * (L * bs * G)
    for l in range(L):
        for b in range(bs):
            for g in range(G):
                rows = slice(g * n, (g + 1) * n)
                r = head.assigner.assign(box[l, b, rows].to(DEV), cls[l, b, rows].to(DEV), dgts[b], dlabels[b])
                assert torch.equal(assigned[l, b, rows].cpu().long() + 1, r.gt_inds.cpu()), (l, b, g)
    y = _yardstick(cls, box, gts, labels, G, cw=head.code_weights.detach().cpu().tolist())
    keys = ("d0.loss_cls", "d0.loss_bbox", "loss_cls", "loss_bbox")
    got = torch.stack([fd[k].detach().reshape(()).cpu() for k in keys]).view(2, 2)
    _assert_loss_bounds((got, fgc, fgb), y)
    # and the module path agrees at its fp32 accuracy
    want = torch.stack([md[k].detach().reshape(()).cpu() for k in keys]).view(2, 2)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(fgc, mgc, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(fgb, mgb, rtol=1e-3, atol=1e-6)


def test_loss_fused_reject_names_what_a_group_call_exceeds():
    head = bevformer_amd.build_head(S.head_cfg("micro", num_query=2049, decoder_layers=1, max_num=20, train=True, group_detr=2))
    preds = {"all_cls_scores": torch.zeros(1, 1, 4098, 10, device=DEV), "all_bbox_preds": torch.zeros(1, 1, 4098, 10, device=DEV)}
    assert head.loss_fused_reject(preds) == "num_query 2049 per group is over 2048"
    head = bevformer_amd.build_head(S.head_cfg("micro", num_query=1, decoder_layers=1, max_num=20, train=True, group_detr=11))
    preds = {"all_cls_scores": torch.zeros(6, 993, 11, 10, device=DEV), "all_bbox_preds": torch.zeros(6, 993, 11, 10, device=DEV)}
    assert head.loss_fused_reject(preds) == "more than 65535 (layer, sample, group) problems"
    preds = {"all_cls_scores": torch.zeros(6, 2, 12, 10, device=DEV), "all_bbox_preds": torch.zeros(6, 2, 12, 10, device=DEV)}
    assert "do not split" in head.loss_fused_reject(preds)


# ---- 6: the shipped shape

def test_the_shipped_group_detr_shape():
    """bevformerv2: 11 groups of 900 queries, 6 decoder layers, one sample, 40 gt — 66 problems in one call."""
    G, n = 11, 900
    cls, box, gts, labels = _case(G, n)
    run = _kernel_run(G, n)
    assert run["status"].tolist() == [0] * 66
    for l in range(6):
        for g in range(G):
            p = l * G + g
            _check_optimal(run["cost"][l, 0, g, :40].numpy(), run["match"][p], run["assigned"][p], f"problem ({l}, 0, {g})")
    inds = _inds_from(run["assigned"].view(6, 1, G * n), G)
    y = _yardstick(cls, box, gts, labels, G, inds=inds, factors=run["factors"])
    assert run["factors"] == (40.0, 40.0)
    _assert_loss_bounds(run["loss"][:3], y)


# ---- 7: capture

def test_grouped_detection_loss_is_capturable_and_a_replay_follows_the_gt():
    """The four launches, forward and backward, in one ``torch.cuda.graph`` on one stream: a synchronisation inside the path
    would make the capture fail.  The packed gt, label and count buffers are then overwritten with a second gt set of other
    counts; the replay is bit-equal to an eager run on that set, and two eager runs are bit-equal to each other."""
    G, n = 3, 37
    cls, box, gts1, labels1 = _case(G, n)
    gts2, labels2 = S.make_gt(77, (2, 9))
    cw = torch.tensor(CW, dtype=torch.float32, device=DEV)
    c, b = cls.to(DEV).requires_grad_(True), box.to(DEV).requires_grad_(True)
    gt, label, count = ops.pack_gt(gts1, labels1, DEV, gmax=16)
    gt2, label2, count2 = ops.pack_gt(gts2, labels2, DEV, gmax=16)
    assert gt.shape == gt2.shape == (2, 16, 9)

    def step():
        losses, assigned, _ = ops.detection_loss(c, b, gt, label, count, cw, return_assigned=True, groups=G)
        gc, gb = torch.autograd.grad(losses.sum(), (c, b))
        return losses, gc, gb, assigned

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    first = [t.clone() for t in out]
    gt.copy_(gt2), label.copy_(label2), count.copy_(count2)
    graph.replay()
    replayed = [t.clone() for t in out]
    eager = [t.clone() for t in step()]
    again = [t.clone() for t in step()]
    torch.cuda.synchronize()
    assert all(torch.equal(r, e) for r, e in zip(replayed, eager)), "the replay does not follow the overwritten gt"
    assert all(torch.equal(a, e) for a, e in zip(again, eager)), "two eager runs are not bit-equal"
    assert not torch.equal(first[3], replayed[3]) and (replayed[3] >= 0).sum().item() == 2 * G * 11
    assert (first[3] >= 0).sum().item() == 2 * G * 5


# ---- 8: the inference fast paths

def test_a_group_detr_head_in_eval_mode_takes_the_decoder_and_head_fast_paths():
    from bevformer_amd.modules.decoder import fused_layer_reject
    import head_yardstick as HY
    G, n = 3, 37
    torch.manual_seed(0)
    group = bevformer_amd.build_head(S.head_cfg("tiny", num_query=n, decoder_layers=2, max_num=100, group_detr=G)).eval()
    group.init_weights()
    group.transformer.load_state_dict(_trained(group.transformer.state_dict(), seed=9))
    HY.trained_like_head_(group.cls_branches, 4)
    HY.trained_like_head_(group.reg_branches, 5)
    plain = bevformer_amd.build_head(S.head_cfg("tiny", num_query=n, decoder_layers=2, max_num=100)).eval()
    sd = {k: v.clone() for k, v in group.state_dict().items()}
    sd["query_embedding.weight"] = sd["query_embedding.weight"][:n]
    plain.load_state_dict(sd)
    mlvl, _, kw = S.make_transformer_inputs("tiny", seed=0, bs=1, temporal=True)
    group, plain = group.to(DEV), plain.to(DEV)
    seen = []
    real_mha, real_branches = ops.mha, ops.head_branches
    ops.mha = lambda *a, **k: (seen.append("mha"), real_mha(*a, **k))[1]
    ops.head_branches = lambda *a, **k: (seen.append("head_branches"), real_branches(*a, **k))[1]
    try:
        with torch.no_grad(), ops.using(decoder_fused=True, head_fused=True):
            assert all(fused_layer_reject(layer) is None for layer in group.transformer.decoder.layers)
            assert group.head_fused_reject() is None
            got = group([f.to(DEV) for f in mlvl], kw["img_metas"], prev_bev=kw["prev_bev"].to(DEV))
            assert seen == ["mha", "mha", "head_branches"], seen         # both fast paths ran, on one group's queries
            want = plain([f.to(DEV) for f in mlvl], kw["img_metas"], prev_bev=kw["prev_bev"].to(DEV))
    finally:
        ops.mha, ops.head_branches = real_mha, real_branches
    assert tuple(got["all_cls_scores"].shape) == (2, 1, n, 10)
    for k in ("bev_embed", "all_cls_scores", "all_bbox_preds"):
        assert torch.equal(got[k], want[k]), k
