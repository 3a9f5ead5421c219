"""No GPU: the host side of the fused optimizer — the float64 yardstick pinned to torch's own float64 run, the mmcv-style
parameter groups of ``registry.build_optimizer``, the registry entry, every reason of ``ops.fused_reject`` and the job
planner's block arithmetic against the library's."""
import types

import pytest
import torch
import torch.nn as nn

from bevformer_amd import _lib, build, ops, registry

import optim_yardstick as Y


def test_yardstick_equals_torch_in_float64():
    """``clip_grad_norm_`` + ``torch.optim.AdamW(foreach=False)`` in float64 on the CPU against the restated statements, to
    1e-14 relative per tensor: clipping on (norm >> max_norm), on with coefficient 1, and off."""
    prob = Y.make_problem(seed=1, small=40)
    for max_norm in (35.0, 1e9, None):
        want = Y.run_torch(prob["params"], prob["groups"], prob["grads"], max_norm, torch.float64)
        got = Y.run_yardstick(prob["params"], prob["groups"], prob["grads"], max_norm)
        for s, (a, b) in enumerate(zip(got, want)):
            assert a["t"] == b["t"], (max_norm, s)
            if max_norm is not None:
                assert abs(a["norm"] - b["norm"]) <= 1e-14 * b["norm"]
            for key in ("p", "m", "v"):
                for i, (x, y) in enumerate(zip(a[key], b[key])):
                    assert (x is None) == (y is None), (key, i)
                    if x is not None and x.numel():
                        err = float((x - y).abs().max())
                        assert err <= 1e-14 * max(float(y.abs().max()), 1e-300), (max_norm, s, key, i, err)
    sp = prob["special"]
    assert want[-1]["t"][sp["sometimes"]] == 2 and want[-1]["t"][sp["empty"]] == 4      # torch's own semantics, for the record


def test_yardstick_notices_a_dropped_term():
    """The bound of the GPU parity test is only worth something if a wrong formula misses it: dropping the weight decay, eps
    or a bias correction moves torch's fp32 result of the lr 1e-2 / wd 0.1 group far outside ``4 * e_ref + 2^-22 * max|p|``."""
    prob = Y.make_problem(seed=1, small=10)
    ref64 = Y.run_yardstick(prob["params"], prob["groups"], prob["grads"], 35.0)
    ref32 = Y.run_torch(prob["params"], prob["groups"], prob["grads"], 35.0, torch.float32)
    Y.check_snapshot(ref32[-1], ref32[-1], ref64[-1], "torch fp32 against itself")
    for broken in ("weight_decay", "eps"):
        groups = [dict(g, **{broken: 0.0}) for g in prob["groups"]]
        bad = Y.run_torch(prob["params"], groups, prob["grads"], 35.0, torch.float32)
        with pytest.raises(AssertionError):
            Y.check_snapshot(bad[-1], ref32[-1], ref64[-1], f"without {broken}")


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.img_backbone = nn.Sequential(nn.Linear(4, 4), nn.Linear(4, 4))
        self.img_neck = nn.Linear(4, 4)
        self.pts_bbox_head = nn.Linear(4, 2)
        self.frozen = nn.Linear(2, 2)
        for p in self.frozen.parameters():
            p.requires_grad_(False)


def test_param_groups_follow_custom_keys_longest_first():
    net = _Net()
    names = [n for n, _ in net.named_parameters()]
    groups = registry.optimizer_param_groups(net, 2e-4, 0.01, dict(custom_keys={
        "img_backbone": dict(lr_mult=0.1), "img_backbone.1": dict(lr_mult=0.5, decay_mult=0.0), "head": dict(decay_mult=2.0)}))
    assert len(groups) == len(names) and all(len(g["params"]) == 1 for g in groups)      # mmcv: one group per parameter
    by = dict(zip(names, groups))
    assert by["img_backbone.0.weight"]["lr"] == pytest.approx(2e-5) and by["img_backbone.0.weight"]["weight_decay"] == pytest.approx(0.01)
    # the longer key wins although the shorter one matches too
    assert by["img_backbone.1.bias"]["lr"] == pytest.approx(1e-4) and by["img_backbone.1.bias"]["weight_decay"] == 0.0
    assert by["pts_bbox_head.weight"]["lr"] == pytest.approx(2e-4) and by["pts_bbox_head.weight"]["weight_decay"] == pytest.approx(0.02)
    assert set(by["img_neck.weight"]) == {"params"}                                     # no key: the optimizer's defaults
    assert set(by["frozen.weight"]) == {"params"}                                       # no gradient: a bare group
    assert registry.optimizer_param_groups(net, 2e-4, 0.01, None)[0] is next(net.parameters())
    with pytest.raises(NotImplementedError):
        registry.optimizer_param_groups(net, 2e-4, 0.01, dict(bias_lr_mult=2.0))
    with pytest.raises(ValueError):
        registry.optimizer_param_groups(net, 2e-4, None, dict(custom_keys={"head": dict(decay_mult=2.0)}))


def test_adamw2_is_registered_and_built_from_the_reference_config():
    from bevformer_amd import optim
    assert "AdamW2" in registry.OPTIMIZERS and registry.OPTIMIZERS.get("AdamW2") is optim.AdamW2
    assert optim.FusedAdamW is optim.AdamW2 and issubclass(optim.AdamW2, torch.optim.Optimizer)
    cfg = dict(type="AdamW2", lr=2e-4, paramwise_cfg=dict(custom_keys={"img_backbone": dict(lr_mult=0.1)}), weight_decay=0.01)
    # (bevformer_base.py:228-239) a CPU model reaches the optimizer and is refused there, with the reason: no fallback
    with pytest.raises(RuntimeError, match="not on a GPU"):
        registry.build_optimizer(_Net(), cfg, dict(grad_clip=dict(max_norm=35, norm_type=2)))
    assert "paramwise_cfg" in cfg                                                       # the caller's dict is not edited


def _fake(**kw):
    base = dict(is_sparse=False, dtype=torch.float32, is_cuda=True, device=torch.device("cuda", 0), grad=None, contiguous=True)
    base.update(kw)
    c = base.pop("contiguous")
    return types.SimpleNamespace(is_contiguous=lambda: c, **base)


def test_every_fused_reject_reason():
    ok = [_fake(), _fake()]
    assert ops.fused_reject(ok) is None
    assert ops.fused_reject(ok, grad_clip=dict(max_norm=35, norm_type=2)) is None
    assert ops.fused_reject(ok, grad_clip=dict(max_norm=35)) is None
    assert "amsgrad" in ops.fused_reject(ok, amsgrad=True)
    assert "maximize" in ops.fused_reject(ok, maximize=True)
    assert "norm_type" in ops.fused_reject(ok, grad_clip=dict(max_norm=35, norm_type=1))
    assert "norm_type" in ops.fused_reject(ok, grad_clip=dict(max_norm=35, norm_type=float("inf")))
    assert "max_norm" in ops.fused_reject(ok, grad_clip=dict(norm_type=2))
    assert "max_norm" in ops.fused_reject(ok, grad_clip=dict(max_norm=-1.0))
    assert "keys" in ops.fused_reject(ok, grad_clip=dict(max_norm=1.0, error_if_nonfinite=True))
    assert "not on a GPU" in ops.fused_reject([torch.zeros(3)])
    assert "sparse" in ops.fused_reject([_fake(is_sparse=True)])
    assert "float32" in ops.fused_reject([_fake(dtype=torch.bfloat16)])
    assert "float32" in ops.fused_reject([torch.zeros(3, dtype=torch.float64)])
    assert "not contiguous" in ops.fused_reject([_fake(contiguous=False)])
    assert "more than one device" in ops.fused_reject([_fake(), _fake(device=torch.device("cuda", 1))])
    g_ok = _fake()
    assert ops.fused_reject([_fake(grad=_fake(contiguous=False))]) is None               # gradients only on request
    assert "gradient of parameter 0 is not contiguous" in ops.fused_reject([_fake(grad=_fake(contiguous=False))], check_grads=True)
    assert "gradient of parameter 1 is sparse" in ops.fused_reject([_fake(grad=g_ok), _fake(grad=_fake(is_sparse=True))], check_grads=True)
    assert "gradient of parameter 0 is torch.float16" in ops.fused_reject([_fake(grad=_fake(dtype=torch.float16))], check_grads=True)
    from bevformer_amd import optim
    for kw, why in ((dict(amsgrad=True), "amsgrad"), (dict(grad_clip=dict(max_norm=1, norm_type=1)), "norm_type")):
        with pytest.raises(RuntimeError, match=why):
            optim.AdamW2([nn.Parameter(torch.zeros(3))], **kw)
    with pytest.raises(ValueError):
        optim.AdamW2([nn.Parameter(torch.zeros(3))], lr=torch.tensor(1e-3))


def test_job_planner_matches_the_library():
    if build.is_stale():
        build.build_library()
    lib = _lib.load(build.LIB_PATH)
    for n in (0, 1, 4095, 4096, 4097, 8192, 8193, 2 ** 31 + 5):
        assert ops.optim_job_blocks(n) == lib.bevmsda_optim_job_blocks(n), n
    assert lib.bevmsda_optim_job_blocks(-1) == -1
    assert lib.bevmsda_optim_workspace_bytes(0) == 8 and lib.bevmsda_optim_workspace_bytes(5) == 40
    numels = [1, 0, 4096, 4097, 0, 3, 2 * 4096 + 13]
    first, total = ops.optim_plan(numels)
    assert first == [0, 1, 1, 2, 4, 4, 5] and total == 8
    assert total == sum(lib.bevmsda_optim_job_blocks(n) for n in numels)
    rows, blocks = ops.optim_job_rows([(0x1000 * (i + 1), 0x2000, 0x3000, 0x4000, 0x5000 + 4 * i, n, i % 3) for i, n in enumerate(numels)])
    assert blocks == total and len(rows[0]) == ops.OPTIM_JOB_WORDS
    # the rows ARE struct bevmsda_optim_job: read them back through the ctypes mirror
    import ctypes
    buf = (ctypes.c_int64 * (7 * len(rows)))(*[w for r in rows for w in r])
    jobs = ctypes.cast(buf, ctypes.POINTER(_lib.OptimJob))
    for i, n in enumerate(numels):
        assert (jobs[i].p, jobs[i].step, jobs[i].numel, jobs[i].group, jobs[i].first_block) == \
            (0x1000 * (i + 1), 0x5000 + 4 * i, n, i % 3, first[i])
    with pytest.raises(ValueError):
        ops.optim_plan([2 ** 43])
