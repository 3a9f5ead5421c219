"""GPU: ``bevformer_amd.optim.AdamW2`` (csrc/optim.h: the gradient-norm launch and the AdamW launch) against the float64
yardstick of tests/optim_yardstick.py.

Tolerance (self-calibrating): per compared tensor, ``max|hip - fp64| <= 4 * e_ref + 2^-22 * max|tensor|`` with ``e_ref`` the
largest distance of torch's own fp32 CPU AdamW (+ ``clip_grad_norm_``) from the yardstick on the same inputs — absolute per
tensor for the parameters and both states (fp32 ``exp_avg`` cancels; an element-relative bound would fail torch itself); the
factor 4 covers FMA contraction and a different division / square-root order.  ``total_norm``: 1e-5 relative (the kernel sums
<= 16 squares in fp32 before the double stage).  Step counts: exactly.  The measured ratios ``max|hip - fp64| / e_ref`` are
printed (profiles/r10/optim_parity.txt holds a recorded run)."""
import copy

import pytest
import torch

from bevformer_amd import ops
from bevformer_amd.optim import AdamW2

import optim_yardstick as Y

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CLIPS = {"clipped": 35.0, "coef_one": 1e9, "off": None}

_CACHE = {}


def _problem():
    if "problem" not in _CACHE:
        _CACHE["problem"] = Y.make_problem(seed=0)
    return _CACHE["problem"]


def _small_problem():
    """A few tensors of the same size classes, for the tests that are about something other than sizes."""
    if "small" not in _CACHE:
        prob = Y.make_problem(seed=5, small=12)
        _CACHE["small"] = prob
    return _CACHE["small"]


def _refs(prob, max_norm, tag):
    """(torch fp32 CPU, fp64 yardstick) snapshots per step, computed once per (problem, clipping)."""
    key = ("refs", tag, max_norm)
    if key not in _CACHE:
        _CACHE[key] = (Y.run_torch(prob["params"], prob["groups"], prob["grads"], max_norm, torch.float32),
                       Y.run_yardstick(prob["params"], prob["groups"], prob["grads"], max_norm))
    return _CACHE[key]


def _device_params(prob):
    """The problem's parameters on the GPU; the ``view`` one is a view at a 4-byte offset of a flat buffer (as the biases
    ``ops.flatten_linear_params`` hands out): not 16-byte aligned."""
    ps = []
    for i, t in enumerate(prob["params"]):
        if i == prob["special"]["view"]:
            flat = torch.zeros(t.numel() + 5, device=DEV)
            flat[1:1 + t.numel()] = t.to(DEV)
            p = torch.nn.Parameter(flat[1:1 + t.numel()])
            assert p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(t.to(DEV).clone())
        ps.append(p)
    return ps


def _set_grads(ps, grads, prob):
    for i, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
        elif i == prob["special"]["view"]:
            flat = torch.zeros(g.numel() + 7, device=DEV)            # a gradient view off 16 bytes too: the norm kernel's element path
            flat[3:3 + g.numel()] = g.to(DEV)
            p.grad = flat[3:3 + g.numel()]
        else:
            p.grad = g.to(DEV).clone()


def _make(prob, max_norm, **kw):
    ps = _device_params(prob)
    groups = [dict(g, params=[ps[i] for i in g["params"]]) for g in prob["groups"]]
    opt = AdamW2(groups, grad_clip=None if max_norm is None else dict(max_norm=max_norm, norm_type=2), **kw)
    return ps, opt


def _snapshot(ps, opt):
    st = [opt.state.get(p, {}) for p in ps]
    torch.cuda.synchronize()
    return dict(p=[p.detach().clone() for p in ps], m=[s["exp_avg"].clone() if "exp_avg" in s else None for s in st],
                v=[s["exp_avg_sq"].clone() if "exp_avg_sq" in s else None for s in st],
                t=[int(s["step"].item()) if "step" in s else 0 for s in st], norm=float(opt.grad_norm.item()))


def _run(prob, max_norm, **kw):
    ps, opt = _make(prob, max_norm, **kw)
    out = []
    for grads in prob["grads"]:
        _set_grads(ps, grads, prob)
        kept = [None if p.grad is None else p.grad.clone() for p in ps]
        opt.step()
        for p, k in zip(ps, kept):
            assert k is None or torch.equal(p.grad, k), "step() changed a gradient"
        out.append(_snapshot(ps, opt))
    return out, ps, opt


@pytest.mark.parametrize("clip", list(CLIPS))
def test_parity_with_the_float64_yardstick(clip):
    """Every size class (1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 13 elements, a 256 x 256 matrix, a bias view at a 4-byte
    offset, an empty tensor, 300 parameters of 1 .. 7 elements), three groups (lr 2e-4 / wd 0.01, lr 1e-2 / wd 0.1, wd 0), four
    steps, one parameter without a gradient on steps 2 and 3, one all-zero gradient; clipping on with norm > max_norm, on with
    coefficient exactly 1, and off."""
    prob, max_norm = _problem(), CLIPS[clip]
    ref32, ref64 = _refs(prob, max_norm, "main")
    got, ps, opt = _run(prob, max_norm)
    lines = []
    for s in range(Y.STEPS):
        want = ref64[s]["norm"]
        print(f"{clip} step {s + 1}: total_norm {got[s]['norm']:.6e} (fp64 {want:.6e}, relative {abs(got[s]['norm'] - want) / want:.2e})")
        assert abs(got[s]["norm"] - want) <= 1e-5 * want
        Y.check_snapshot(got[s], ref32[s], ref64[s], f"{clip} step {s + 1}", lines)
    if clip == "clipped":
        assert ref64[0]["norm"] > 10 * max_norm, "the gradients are meant to be clipped hard"
        assert 0 < float(opt.clip_coef.item()) < 0.1
    else:
        assert float(opt.clip_coef.item()) == 1.0
    sp = prob["special"]
    assert got[-1]["t"][sp["sometimes"]] == 2 and got[-1]["t"][sp["empty"]] == 4 and int(opt.skipped_steps.item()) == 0


def test_two_runs_are_bit_equal():
    prob = _problem()
    a, _, _ = _run(prob, 35.0)
    b, _, _ = _run(prob, 35.0)
    for s in range(Y.STEPS):
        assert a[s]["norm"] == b[s]["norm"] and a[s]["t"] == b[s]["t"]
        for key in ("p", "m", "v"):
            for x, y in zip(a[s][key], b[s][key]):
                assert (x is None and y is None) or torch.equal(x, y), (s, key)


def test_guard_floats_and_a_poisoned_workspace():
    """The two entry points on buffers of the test's own: every parameter, gradient and state tensor lies in a flat buffer
    between NaN guard floats (so most are off 16 bytes: the element path; the others take the 16-byte path up to their tail),
    the workspace is NaN-poisoned before every call.  Afterwards: guards untouched, results finite and within the bound,
    gradients bit-unchanged."""
    prob = _problem()
    ref32, ref64 = _refs(prob, 35.0, "main")
    n = len(prob["params"])
    offs, total = [], 1
    for i, t in enumerate(prob["params"]):
        if i % 2 == 0:
            total = (total + 3) // 4 * 4                # every other tensor on a 16-byte boundary (a guard float sits before it anyway)
        offs.append(total)
        total += t.numel() + 1                           # ... and one guard float after each
    poison = torch.full((total + 4,), float("nan"), device=DEV)
    bufs = {k: poison.clone() for k in "pgmv"}
    inside = torch.zeros(total + 4, dtype=torch.bool, device=DEV)
    view = {k: [bufs[k][o:o + t.numel()] for o, t in zip(offs, prob["params"])] for k in "pgmv"}
    for i, t in enumerate(prob["params"]):
        view["p"][i].copy_(t.flatten())
        view["m"][i].zero_()
        view["v"][i].zero_()
        inside[offs[i]:offs[i] + t.numel()] = True
    assert bufs["p"].data_ptr() % 16 == 0 and any(v.data_ptr() % 16 for v in view["p"]) and any(v.data_ptr() % 16 == 0 and v.numel() > 4 for v in view["p"])
    steps = torch.zeros(n, device=DEV)
    scalars = torch.zeros(8, device=DEV)
    group_of = {i: k for k, g in enumerate(prob["groups"]) for i in g["params"]}
    groups = torch.tensor([[g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]] for g in prob["groups"]],
                          dtype=torch.float64, device=DEV)
    for s, grads in enumerate(prob["grads"]):
        live = [i for i in range(n) if grads[i] is not None]
        bufs["g"].copy_(poison)
        for i in live:
            view["g"][i].copy_(grads[i].flatten())
        g_before = bufs["g"].clone()
        rows, blocks = ops.optim_job_rows([(view["p"][i].data_ptr(), view["g"][i].data_ptr(), view["m"][i].data_ptr(),
                                            view["v"][i].data_ptr(), steps.data_ptr() + 4 * i, prob["params"][i].numel(),
                                            group_of[i]) for i in live])
        table = torch.tensor(rows, dtype=torch.int64, device=DEV)
        workspace = torch.full((ops.optim_workspace_elems(blocks) + 2,), float("nan"), dtype=torch.float64, device=DEV)
        ops.optim_grad_norm(table, len(rows), blocks, workspace[1:-1], scalars, max_norm=35.0)
        ops.optim_adamw(table, len(rows), blocks, groups, groups.shape[0], scalars)
        torch.cuda.synchronize()
        assert torch.equal(bufs["g"].view(torch.int32), g_before.view(torch.int32)), "a gradient (or its guards) was written"
        assert bool(torch.isnan(workspace[0])) and bool(torch.isnan(workspace[-1])), "the workspace's guards were written"
        for k in "pmv":
            assert bool(torch.isnan(bufs[k][~inside]).all()), f"step {s + 1}: a guard float of the {k} buffer was written"
            assert bool(torch.isfinite(bufs[k][inside]).all()), f"step {s + 1}: a non-finite result in the {k} buffer"
        got = dict(p=view["p"], m=[view["m"][i] if ref64[s]["m"][i] is not None else None for i in range(n)],
                   v=[view["v"][i] if ref64[s]["v"][i] is not None else None for i in range(n)],
                   t=[int(x) for x in steps.tolist()])
        assert abs(float(scalars[0]) - ref64[s]["norm"]) <= 1e-5 * ref64[s]["norm"]
        Y.check_snapshot(got, ref32[s], ref64[s], f"guarded step {s + 1}")
    assert int(scalars.view(torch.int32)[4]) == 0, "the ticket did not return to 0"


def _with_inf(prob):
    bad = copy.copy(prob)
    bad["grads"] = [list(g) for g in prob["grads"]]
    g = bad["grads"][0][6].clone()                      # the 4097-element tensor
    g[4096] = float("inf")
    bad["grads"][0][6] = g
    return bad


def test_a_nonfinite_norm_skips_the_step_when_asked():
    """One inf in one gradient, ``skip_nonfinite=True``: parameters, states and step counts bitwise unchanged,
    ``skipped_steps`` 1 — and the next, finite, step equals the yardstick's FIRST step."""
    prob = _small_problem()
    bad = _with_inf(prob)
    ps, opt = _make(prob, 35.0, skip_nonfinite=True)
    before = [p.detach().clone() for p in ps]
    _set_grads(ps, bad["grads"][0], prob)
    opt.step()
    snap = _snapshot(ps, opt)
    assert snap["norm"] == float("inf") and int(opt.skipped_steps.item()) == 1
    assert all(torch.equal(a, b) for a, b in zip(snap["p"], before))
    assert all(t == 0 for t in snap["t"])
    assert all(m is None or not bool(m.view(torch.int32).any()) for m in snap["m"] + snap["v"]), "a state moved on a skipped step"
    ref32, ref64 = _refs(prob, 35.0, "small")
    _set_grads(ps, prob["grads"][0], prob)
    opt.step()
    Y.check_snapshot(_snapshot(ps, opt), ref32[0], ref64[0], "the finite step after a skipped one")
    assert int(opt.skipped_steps.item()) == 1


@pytest.mark.parametrize("clip", ["clipped", "off"])
def test_a_nonfinite_gradient_without_skipping_poisons_what_torch_poisons(clip):
    """``skip_nonfinite=False`` (the default, torch's behaviour): the NaN mask of every tensor equals that of torch's fp32 CPU
    run (clipped: coefficient 0, inf * 0 = NaN in one element; unclipped: inf / inf), finite elements within the bound."""
    prob = _small_problem()
    bad = _with_inf(prob)
    bad["grads"] = bad["grads"][:2]
    max_norm = CLIPS[clip]
    ref32 = Y.run_torch(bad["params"], bad["groups"], bad["grads"], max_norm, torch.float32)
    ref64 = Y.run_yardstick(bad["params"], bad["groups"], bad["grads"], max_norm)
    got, _, opt = _run(bad, max_norm)
    assert bool(torch.isnan(ref32[0]["p"][6]).any()) and not bool(torch.isnan(ref32[0]["p"][5]).any())
    for s in range(2):
        Y.check_snapshot(got[s], ref32[s], ref64[s], f"inf gradient, {clip}, step {s + 1}")
    assert int(opt.skipped_steps.item()) == 0


def _twin(prob, max_norm):
    ps, opt = _make(prob, max_norm)
    static = [torch.zeros_like(p) for p in ps]
    for p, g in zip(ps, static):
        p.grad = g
    return ps, opt, static


def _feed(static, grads):
    for s, g in zip(static, grads):
        s.copy_(g.to(DEV) if g is not None else torch.zeros_like(s))


def _equal_state(a, b, what):
    sa, sb = _snapshot(*a), _snapshot(*b)
    assert sa["t"] == sb["t"] and sa["norm"] == sb["norm"], what
    for key in ("p", "m", "v"):
        for x, y in zip(sa[key], sb[key]):
            assert torch.equal(x, y), f"{what}: {key} differs"


def test_captured_step_replays_like_the_eager_twin():
    """``step()`` captured alone over static gradient tensors after an eager warm-up: three replays with the gradients
    rewritten in between are bit-equal to an eager twin fed the same gradients; a changed ``group['lr']`` is honoured after
    ``sync_hyperparameters()`` and NOT without it (the contract of a captured step)."""
    prob = _small_problem()
    (pa, oa, ga), (pb, ob, gb) = _twin(prob, 35.0), _twin(prob, 35.0)
    for static, o in ((ga, oa), (gb, ob)):
        _feed(static, prob["grads"][0])
        o.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    _equal_state((pa, oa), (pb, ob), "after the warm-up")
    for k in (1, 2, 3):
        _feed(ga, prob["grads"][k])
        _feed(gb, prob["grads"][k])
        graph.replay()
        ob.step()
        _equal_state((pa, oa), (pb, ob), f"replay {k}")
    for o in (oa, ob):
        o.param_groups[1]["lr"] = 5e-3
    oa.sync_hyperparameters()
    graph.replay()
    ob.step()
    _equal_state((pa, oa), (pb, ob), "a new lr after sync_hyperparameters()")
    oa.param_groups[1]["lr"] = 1e-4                 # host value only: the replay keeps 5e-3, as the twin does
    graph.replay()
    ob.step()
    _equal_state((pa, oa), (pb, ob), "a new lr without sync_hyperparameters() must not reach the replay")


def _torch_twin(prob, ps):
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    return qs, torch.optim.AdamW([dict(g, params=[qs[i] for i in g["params"]]) for g in prob["groups"]], foreach=False)


def _torch_step(qs, opt, grads, max_norm):
    for q, g in zip(qs, grads):
        q.grad = None if g is None else g.to(DEV).clone()
    torch.nn.utils.clip_grad_norm_([q for q in qs if q.grad is not None], max_norm, norm_type=2, foreach=False)
    opt.step()


def _torch_snapshot(qs, opt):
    st = [opt.state.get(q, {}) for q in qs]
    return dict(p=[q.detach() for q in qs], m=[s.get("exp_avg") for s in st], v=[s.get("exp_avg_sq") for s in st],
                t=[int(s["step"]) if "step" in s else 0 for s in st])


def test_state_dict_round_trip_with_torch_adamw():
    """Two steps here, ``state_dict()`` into ``torch.optim.AdamW(foreach=False)`` on the GPU, two more steps in both: each
    within the bound of the four-step yardstick.  The reverse direction, and torch's state with ``step`` as a Python int (the
    layout of the reference's torch 1.9 checkpoints)."""
    prob = _small_problem()
    ref32, ref64 = _refs(prob, 35.0, "small")
    ps, opt = _make(prob, 35.0)
    for s in (0, 1):
        _set_grads(ps, prob["grads"][s], prob)
        opt.step()
    sd = opt.state_dict()
    some = next(iter(sd["state"].values()))
    assert some["step"].device.type == "cpu" and some["step"].dtype == torch.float32 and some["step"].dim() == 0 and float(some["step"]) == 2.0
    assert sd["param_groups"][1]["lr"] == 1e-2 and sd["param_groups"][1]["decoupled_weight_decay"] is True
    qs, topt = _torch_twin(prob, ps)
    topt.load_state_dict(copy.deepcopy(sd))          # (as a checkpoint would: load_state_dict adopts the tensors it is given)
    for g in topt.param_groups:
        g["foreach"] = False                         # (the loaded groups carry this optimizer's None)
    for s in (2, 3):
        _set_grads(ps, prob["grads"][s], prob)
        opt.step()
        _torch_step(qs, topt, prob["grads"][s], 35.0)
    Y.check_snapshot(_snapshot(ps, opt), ref32[3], ref64[3], "this optimizer, steps 3-4")
    Y.check_snapshot(_torch_snapshot(qs, topt), ref32[3], ref64[3], "torch.optim.AdamW continuing from this optimizer's state_dict")
    # the reverse: torch's first two steps, continued here — from its state_dict as it is, and with int step counts
    ps0 = _device_params(prob)
    qs, topt = _torch_twin(prob, ps0)
    for s in (0, 1):
        _torch_step(qs, topt, prob["grads"][s], 35.0)
    tsd = topt.state_dict()
    as_int = copy.deepcopy(tsd)
    for st in as_int["state"].values():
        st["step"] = int(st["step"])
    as_int["param_groups"] = [{k: v for k, v in g.items() if k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "params")}
                              for g in as_int["param_groups"]]
    for what, state in (("torch's state_dict", tsd), ("a state_dict with int steps and torch 1.9's group keys", as_int)):
        ps = _device_params(prob)
        with torch.no_grad():
            for p, q in zip(ps, qs):
                p.copy_(q)
        opt = AdamW2([dict(g, params=[ps[i] for i in g["params"]]) for g in prob["groups"]], grad_clip=dict(max_norm=35.0))
        opt.load_state_dict(copy.deepcopy(state))
        for s in (2, 3):
            _set_grads(ps, prob["grads"][s], prob)
            opt.step()
        Y.check_snapshot(_snapshot(ps, opt), ref32[3], ref64[3], f"continuing from {what}")


def _encoder():
    from helpers import build_pair
    enc, _ = build_pair("micro4", device=DEV)
    for p in enc.parameters():
        p.requires_grad_(True)
    return enc


def _encoder_inputs():
    from bevformer_amd import synthetic as S
    q, f, kw = S.make_inputs("micro4", seed=7, temporal=True, device=DEV)
    gout = torch.randn(1, q.shape[0], 256, generator=torch.Generator().manual_seed(2)).to(DEV)
    return q, f, kw, gout


def _oracle_eval(enc, q, f, kw):
    from bevformer_amd import synthetic as S
    from oracle import bevformer_cpu as O
    torch.set_num_threads(16)
    sd = {k: v.detach().float().cpu() for k, v in enc.state_dict().items()}
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in kw.items()}
    with torch.no_grad():
        return O.encoder_forward(sd, q.cpu(), f.cpu(), pc_range=S.PC_RANGE, **cpu)


def test_weight_images_follow_an_eager_step():
    """The encoder's packed / panel / transposed weight images are cached per version counter: ``step()`` bumps the counters
    of what it wrote (``torch.autograd.graph.increment_version``), so the next forward rebuilds them — the ``eval()`` output
    after a step here equals that of a twin stepped by ``torch.optim.AdamW`` + ``clip_grad_norm_`` on the same gradients
    (rtol = atol = 5e-4, the repository's fp32 bound) — and an inference graph captured before the step is reported stale."""
    enc, twin = _encoder(), _encoder()
    q, f, kw, gout = _encoder_inputs()
    enc(q, f, f, **kw).backward(gout)                # (grad mode on: a training step of the fast path; no dropout in eval mode)
    with torch.no_grad():
        before = enc(q, f, f, **kw).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(q, f, f, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        ops.release_captured_images()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            enc(q, f, f, **kw)
    assert ops.graph_weights_stale() == []
    for (_, p), (_, t) in zip(enc.named_parameters(), twin.named_parameters()):
        assert p.grad is not None
        t.grad = p.grad.detach().clone()
    # a step large enough to see: lr 1e-2 moves every weight by ~1e-2
    opt = AdamW2(enc.parameters(), lr=1e-2, weight_decay=0.01, grad_clip=dict(max_norm=35, norm_type=2))
    topt = torch.optim.AdamW(twin.parameters(), lr=1e-2, weight_decay=0.01, foreach=False)
    opt.step()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), 35, norm_type=2)
    topt.step()
    stale = ops.graph_weights_stale()
    assert stale and all("written" in why for _, why in stale), stale
    del graph
    ops.release_captured_images()
    with torch.no_grad():
        got, want = enc(q, f, f, **kw), twin(q, f, f, **kw)
    assert (got - before).abs().max().item() > 1e-2, "the step did not reach the forward: stale weight images"
    torch.testing.assert_close(got, want, rtol=5e-4, atol=5e-4)


def test_weight_images_follow_a_captured_step():
    """Forward + backward + ``step()`` captured as ONE graph after a warm-up: every replay moves the parameters, and the
    ``eval()`` output afterwards equals the CPU oracle on the model's current ``state_dict`` (rtol = atol = 5e-4) — the
    replays rebuilt the weight images from the updated weights."""
    enc = _encoder()
    q, f, kw, gout = _encoder_inputs()
    opt = AdamW2(enc.parameters(), lr=2e-3, weight_decay=0.01, grad_clip=dict(max_norm=35, norm_type=2))

    def train_step():
        enc.zero_grad(set_to_none=True)
        enc(q, f, f, **kw).backward(gout)
        opt.step()

    for _ in range(2):
        train_step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        train_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    steps_before = int(next(iter(opt.state.values()))["step"].item())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_step()
    for k in range(2):
        old = [p.detach().clone() for p in enc.parameters()]
        graph.replay()
        torch.cuda.synchronize()
        moved = [not torch.equal(a, b) for a, b in zip(old, enc.parameters())]
        assert all(moved), f"replay {k + 1}: {moved.count(False)} parameters did not move"
    assert int(next(iter(opt.state.values()))["step"].item()) == steps_before + 2
    with torch.no_grad():
        got = enc(q, f, f, **kw).cpu()
    torch.testing.assert_close(got, _oracle_eval(enc, q, f, kw), rtol=5e-4, atol=5e-4)
    # a forward OUTSIDE the graph between further replays: the replay runs no host code, mark_replayed() tells the caches
    graph.replay()
    opt.mark_replayed()
    with torch.no_grad():
        got = enc(q, f, f, **kw).cpu()
    torch.testing.assert_close(got, _oracle_eval(enc, q, f, kw), rtol=5e-4, atol=5e-4)
    del graph
